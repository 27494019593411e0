"""Streaming inference on top of the engine: the forward filter and the fixed-lag smoother of a log batch, and the online best-path
decoder of a tropical batch, run over audio in chunks.

``ForwardFilter`` keeps, per utterance of a batch, the carried state of ``BatchedFSM.filterposteriors`` (mm_filterposteriors_f32:
the one-step prediction behind the last frame seen, normalised by the mass alive there) and the running prefix log-likelihood.
``push`` takes the next chunk of emissions and returns the filtering posteriors P(pdf_n = p | V up to n) and the increments
ln P(V_n | V before n) of its frames: online confidence, keyword / filler spotting, HMM-smoothed activity detection, endpointing.
Chunking is exact -- the chunks' results are those of one call on the whole audio -- and costs no graph compilation: the state is
an argument of the call.  Everything is a launch chain on the caller's stream; nothing synchronises the host.

``FixedLagSmoother`` is its companion on ``BatchedFSM.windowposteriors`` (mm_windowposteriors_f32): every frame waits for ``lag``
frames of its future and is emitted once, with the smoothing posterior given everything pushed by then.

``OnlineViterbi`` is the decoder, on ``BatchedFSM.viterbiwindow`` (mm_viterbiwindow_f32): every frame is emitted once, as soon as
all surviving paths agree on it (the convergence point), or when ``max_pending`` frames wait behind it.
"""
from __future__ import annotations


class ForwardFilter:
    """The forward filter of ``batch`` (a log-semiring ``BatchedFSM``), one stream of audio per utterance.

    ``state``   float32 ``[total_states]`` device tensor, natural log: element (b, s) at ``batch.state_offsets[b] + s``; advanced in
                place by ``push``
    ``loglik``  float64 ``[B]`` device tensor: the running sum of ``incr``, ln P(all frames pushed so far)"""

    def __init__(self, batch):
        import torch

        self.batch = batch
        dev = torch.device("cuda", torch.cuda.current_device())
        B = batch.B
        # the reset vector, once: a call with lens = 0 passes the start vector through (NULL in: ln alpha_hat)
        zeros = torch.zeros((B, 1, batch.P), dtype=torch.float32, device=dev)
        self._reset = batch.filterposteriors(zeros, torch.zeros(B, dtype=torch.int32, device=dev), want_state=True, want_filt=False)[3]
        sizes = torch.as_tensor([int(c.S1) for c in batch.cfsms], device=dev)
        self._utt = torch.repeat_interleave(torch.arange(B, device=dev), sizes)  # state -> utterance
        self._final = torch.as_tensor(batch.state_offsets[1:] - 1, dtype=torch.int64, device=dev)
        self.state = self._reset.clone()
        self.loglik = torch.zeros(B, dtype=torch.float64, device=dev)

    def push(self, V_chunk, lens=None, want_filt=True):
        """The next chunk ``V_chunk[B, n, P]`` (``lens[b]`` of its frames belong to utterance b; 0: the utterance stands still).
        Returns ``(filt[B, n, P], incr[B, n])`` of the chunk's frames (``filt`` None without ``want_filt``): NumPy for a NumPy
        chunk, device tensors for a device chunk."""
        import torch

        filt, incr, _, _ = self.batch.filterposteriors(V_chunk, lens, state=self.state, want_state=self.state, want_filt=want_filt)
        inc = incr if isinstance(incr, torch.Tensor) else torch.as_tensor(incr).to(self.loglik.device)
        self.loglik += inc.sum(dim=1, dtype=torch.float64)
        return filt, incr

    def logz(self):
        """float64 ``[B]`` device tensor: log Z of the frames pushed so far, were the audio to end here -- ``loglik`` + the log of
        the alive mass the final weights accept (the carried state's final entries)."""
        return self.loglik + self.state[self._final].double()

    def reset(self, mask=None):
        """Put the utterances of ``mask`` (bool ``[B]``; None: all) back on their FSMs' initial vectors, ``loglik`` on 0."""
        import torch

        if mask is None:
            self.state.copy_(self._reset)
            self.loglik.zero_()
            return self
        m = torch.as_tensor(mask).to(device=self.state.device, dtype=torch.bool)
        self.state.copy_(torch.where(m[self._utt], self._reset, self.state))
        self.loglik.masked_fill_(m, 0.0)
        return self


class FixedLagSmoother:
    """The fixed-lag smoother of ``batch`` (a log-semiring ``BatchedFSM``), one stream of audio per utterance: the companion of
    ``ForwardFilter`` that lets every frame see ``lag`` frames of its future, P(pdf_n | V up to n + lag), on
    ``BatchedFSM.windowposteriors`` (mm_windowposteriors_f32).

    Every frame is emitted exactly once, by the ``push`` that brings the ``lag``-th frame behind it or by ``finish``.  Its
    posterior is conditioned on EVERYTHING pushed up to the push that emitted it -- at least ``lag`` frames ahead, more for the
    older frames of a long chunk -- or on the whole audio up to its end for the frames ``finish`` emits; it is exactly the
    open-window (``finish``: the closed) smoothing posterior given all frames of the utterance so far, not an approximation by a
    truncated window: the frames before the window are in the carried state.  A push costs one forward-backward over
    ``lag + chunk`` frames (the filter's push: one forward pass over ``chunk`` frames); the utterances advance each by its own
    ``lens``, not in lock step.  Everything is a launch chain on the caller's stream; nothing synchronises the host except what
    ``count`` costs the caller to read.

    ``state``    float32 ``[total_states]`` device tensor: ``filterposteriors``' carried state behind the last emitted frame
    ``loglik``   float64 ``[B]`` device tensor: ln P(the frames emitted so far)
    ``pending``  float32 ``[B, lag, P]`` device tensor, ``npending`` int32 ``[B]``: the frames pushed and not yet emitted"""

    def __init__(self, batch, lag):
        import torch

        if int(lag) < 1:
            raise ValueError("lag must be at least one frame (lag 0 is the forward filter: streaming.ForwardFilter)")
        self.batch, self.lag = batch, int(lag)
        dev = torch.device("cuda", torch.cuda.current_device())
        B = batch.B
        self.pending = torch.zeros((B, self.lag, batch.P), dtype=torch.float32, device=dev)
        self.npending = torch.zeros(B, dtype=torch.int32, device=dev)
        # the reset vector, once: a window with lens = 0 passes the start vector through (NULL in: ln alpha_hat)
        self._reset = batch.windowposteriors(self.pending[:, :1], self.npending, want_state=True)[3]
        sizes = torch.as_tensor([int(c.S1) for c in batch.cfsms], device=dev)
        self._utt = torch.repeat_interleave(torch.arange(B, device=dev), sizes)  # state -> utterance
        self.state = self._reset.clone()
        self.loglik = torch.zeros(B, dtype=torch.float64, device=dev)

    def push(self, V_chunk, lens=None):
        """The next chunk ``V_chunk[B, n, P]`` (``lens[b]`` of its frames belong to utterance b; 0: the utterance stands still).
        Returns ``(gamma[B, n, P], count[B])``: the first ``count[b]`` rows of ``gamma[b]`` are the smoothed posteriors of b's
        oldest pending frames, in order (``count[b]`` = pending + ``lens[b]`` - ``lag``, at least 0 and at most n -- the width
        every count fits without asking the device); the rows behind them are zeros.  NumPy for a NumPy chunk, device tensors
        for a device chunk."""
        import torch

        as_numpy = not isinstance(V_chunk, torch.Tensor)
        dev = self.state.device
        Vc = torch.as_tensor(V_chunk, dtype=torch.float32).to(dev) if as_numpy else V_chunk
        B, n, P = Vc.shape
        L = torch.full((B,), n, dtype=torch.int32, device=dev) if lens is None else torch.as_tensor(lens).to(device=dev, dtype=torch.int32)
        L = L.clamp(0, n)
        W = self.lag + n
        t = torch.arange(W, device=dev)[None, :]  # [1, W]
        npd = self.npending[:, None].long()
        # utterance b's window: its pending frames, then its frames of the chunk
        both = torch.cat([self.pending, Vc], dim=1)
        src = torch.where(t < npd, t, (self.lag + t - npd).clamp(max=W - 1))
        win = torch.gather(both, 1, src[:, :, None].expand(B, W, P)).contiguous()
        wlen = self.npending + L
        commit = (wlen - self.lag).clamp(min=0)
        gamma, _, lcommit, _ = self.batch.windowposteriors(win, wlen, state=self.state, commit=commit, want_state=self.state)
        self.loglik += lcommit.double()
        # the frames behind the commit frame stay pending
        keep = (commit[:, None].long() + t[:, : self.lag]).clamp(max=W - 1)
        self.pending = torch.gather(win, 1, keep[:, :, None].expand(B, self.lag, P)).contiguous()
        self.npending = wlen - commit
        out = gamma[:, :n] * (t[:, :n] < commit[:, None]).unsqueeze(-1)
        return (out.cpu().numpy(), commit.cpu().numpy()) if as_numpy else (out, commit)

    def finish(self, mask=None, as_numpy=False):
        """The audio of the utterances of ``mask`` (bool ``[B]``; None: all) ends here: one closed window over their pending
        frames.  Returns ``(gamma[B, lag, P], count[B], logz[B])``: the first ``count[b]`` rows of ``gamma[b]`` are the posteriors
        of b's remaining frames -- given the whole audio --, ``logz`` (float64) = ``loglik`` + the closed window's ``ttl``, the
        log Z ``pdfposteriors`` gives the whole audio.  The other utterances take no part (count 0, logz -inf) and go on
        afterwards; the masked ones are reset."""
        import torch

        dev = self.state.device
        m = torch.ones(self.batch.B, dtype=torch.bool, device=dev) if mask is None else torch.as_tensor(mask).to(device=dev, dtype=torch.bool)
        count = torch.where(m, self.npending, torch.zeros_like(self.npending))
        gamma, ttl, _ = self.batch.windowposteriors(self.pending, count, state=self.state, closed=m.to(torch.int32))
        logz = self.loglik + ttl.double()
        self.reset(m)
        return (gamma.cpu().numpy(), count.cpu().numpy(), logz.cpu().numpy()) if as_numpy else (gamma, count, logz)

    def reset(self, mask=None):
        """Put the utterances of ``mask`` (bool ``[B]``; None: all) back on their FSMs' initial vectors with nothing pending,
        ``loglik`` on 0."""
        import torch

        if mask is None:
            self.state.copy_(self._reset)
            self.loglik.zero_()
            self.npending.zero_()
            return self
        m = torch.as_tensor(mask).to(device=self.state.device, dtype=torch.bool)
        self.state.copy_(torch.where(m[self._utt], self._reset, self.state))
        self.loglik.masked_fill_(m, 0.0)
        self.npending.masked_fill_(m, 0)
        return self


class OnlineViterbi:
    """The online best-path decoder of ``batch`` (a tropical ``BatchedFSM``), one stream of audio per utterance, on
    ``BatchedFSM.viterbiwindow`` (mm_viterbiwindow_f32): online alignment, keyword spotting, endpointing on the best path, live
    captioning -- without re-running the prefix at every chunk.

    A ``push`` runs one open window over the pending frames and the chunk and emits every frame up to the window's CONVERGENCE
    POINT, the last frame all surviving paths pass: those states are final, they are the best path of the whole audio whatever
    follows.  The frames behind it stay pending, at most ``max_pending`` of them: what would not fit is committed from the
    window's current best path before it is final -- the fixed-lag truncation, an approximation, counted in ``nforced`` (0: the
    output is exactly ``viterbi``'s path of the whole audio).  Every frame is emitted exactly once, by a ``push`` or by
    ``finish``; the utterances advance each by its own ``lens``.  Everything is a launch chain on the caller's stream: the
    data-dependent commit stays in device tensors, nothing synchronises the host except what ``count`` costs the caller to read.

    ``state``    float32 ``[total_states]`` device tensor: ``viterbiwindow``'s carried state behind the last emitted frame
    ``score``    float64 ``[B]`` device tensor: the sum of ``mcommit``, the best score over the frames emitted so far
    ``nforced``  int64 ``[B]`` device tensor: frames emitted before they were final
    ``pending``  float32 ``[B, max_pending, P]`` device tensor, ``npending`` int32 ``[B]``: the frames pushed and not yet emitted"""

    def __init__(self, batch, max_pending):
        import torch

        if int(max_pending) < 1:
            raise ValueError("max_pending must be at least one frame")
        self.batch, self.max_pending = batch, int(max_pending)
        dev = torch.device("cuda", torch.cuda.current_device())
        B = batch.B
        self.pending = torch.zeros((B, self.max_pending, batch.P), dtype=torch.float32, device=dev)
        self.npending = torch.zeros(B, dtype=torch.int32, device=dev)
        # the reset vector, once: a window with lens = 0 passes the start vector through (NULL in: alpha_hat)
        self._reset = batch.viterbiwindow(self.pending[:, :1], self.npending, want_state=True)[5]
        sizes = torch.as_tensor([int(c.S1) for c in batch.cfsms], device=dev)
        self._utt = torch.repeat_interleave(torch.arange(B, device=dev), sizes)  # state -> utterance
        self._final = torch.as_tensor(batch.state_offsets[1:] - 1, dtype=torch.int64, device=dev)
        self.state = self._reset.clone()
        self.score = torch.zeros(B, dtype=torch.float64, device=dev)
        self.nforced = torch.zeros(B, dtype=torch.int64, device=dev)

    def push(self, V_chunk, lens=None):
        """The next chunk ``V_chunk[B, n, P]`` (``lens[b]`` of its frames belong to utterance b; 0: the utterance stands still).
        Returns ``(states[B, max_pending + n], count[B])``: the first ``count[b]`` entries of ``states[b]`` are the newly emitted
        0-based states of b's oldest pending frames, in order, the rest is -1 (as are the states of an utterance without a
        path).  NumPy for a NumPy chunk, device tensors for a device chunk."""
        import torch

        as_numpy = not isinstance(V_chunk, torch.Tensor)
        dev = self.state.device
        Vc = torch.as_tensor(V_chunk, dtype=torch.float32).to(dev) if as_numpy else V_chunk
        B, n, P = Vc.shape
        L = torch.full((B,), n, dtype=torch.int32, device=dev) if lens is None else torch.as_tensor(lens).to(device=dev, dtype=torch.int32)
        L = L.clamp(0, n)
        W = self.max_pending + n
        t = torch.arange(W, device=dev)[None, :]  # [1, W]
        npd = self.npending[:, None].long()
        # utterance b's window: its pending frames, then its frames of the chunk
        both = torch.cat([self.pending, Vc], dim=1)
        src = torch.where(t < npd, t, (self.max_pending + t - npd).clamp(max=W - 1))
        win = torch.gather(both, 1, src[:, :, None].expand(B, W, P)).contiguous()
        wlen = self.npending + L
        forced = (wlen - self.max_pending).clamp(min=0)
        path, _, conv, ncommit, mcommit, _ = self.batch.viterbiwindow(win, wlen, state=self.state, commit=forced, commit_converged=True,
                                                                      want_state=self.state)
        self.score += mcommit.double()
        self.nforced += (ncommit - conv).clamp(min=0).long()
        # the frames behind the commit frame stay pending
        keep = (ncommit[:, None].long() + t[:, : self.max_pending]).clamp(max=W - 1)
        self.pending = torch.gather(win, 1, keep[:, :, None].expand(B, self.max_pending, P)).contiguous()
        self.npending = wlen - ncommit
        out = torch.where(t < ncommit[:, None], path, torch.full_like(path, -1))
        return (out.cpu().numpy(), ncommit.cpu().numpy()) if as_numpy else (out, ncommit)

    def finish(self, mask=None, as_numpy=False):
        """The audio of the utterances of ``mask`` (bool ``[B]``; None: all) ends here: one closed window over their pending
        frames.  Returns ``(states[B, max_pending], count[B], score[B])``: the first ``count[b]`` entries of ``states[b]`` are the
        states of b's remaining frames, ``score`` (float64) = the running ``score`` + the closed window's, the weight ``viterbi``
        gives the best path of the whole audio when ``nforced`` is 0.  An utterance with nothing pending ends on the carried state's
        final entry, the best final weight behind its last frame (a window without a frame has no score of its own).  The other
        utterances take no part (count 0, score -inf) and go on afterwards; the masked ones are reset."""
        import torch

        dev = self.state.device
        m = torch.ones(self.batch.B, dtype=torch.bool, device=dev) if mask is None else torch.as_tensor(mask).to(device=dev, dtype=torch.bool)
        count = torch.where(m, self.npending, torch.zeros_like(self.npending))
        path, sc, _, _, _, _ = self.batch.viterbiwindow(self.pending, count, state=self.state, closed=m.to(torch.int32))
        sc = torch.where(m & (count == 0), self.state[self._final], sc)
        total = self.score + sc.double()
        self.reset(m)
        return (path.cpu().numpy(), count.cpu().numpy(), total.cpu().numpy()) if as_numpy else (path, count, total)

    def reset(self, mask=None):
        """Put the utterances of ``mask`` (bool ``[B]``; None: all) back on their FSMs' initial vectors with nothing pending,
        ``score`` and ``nforced`` on 0."""
        import torch

        if mask is None:
            self.state.copy_(self._reset)
            self.score.zero_()
            self.nforced.zero_()
            self.npending.zero_()
            return self
        m = torch.as_tensor(mask).to(device=self.state.device, dtype=torch.bool)
        self.state.copy_(torch.where(m[self._utt], self._reset, self.state))
        self.score.masked_fill_(m, 0.0)
        self.nforced.masked_fill_(m, 0)
        self.npending.masked_fill_(m, 0)
        return self
