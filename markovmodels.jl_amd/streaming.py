"""Streaming inference on top of the engine: the forward filter of a log batch run over audio in chunks.

``ForwardFilter`` keeps, per utterance of a batch, the carried state of ``BatchedFSM.filterposteriors`` (mm_filterposteriors_f32:
the one-step prediction behind the last frame seen, normalised by the mass alive there) and the running prefix log-likelihood.
``push`` takes the next chunk of emissions and returns the filtering posteriors P(pdf_n = p | V up to n) and the increments
ln P(V_n | V before n) of its frames: online confidence, keyword / filler spotting, HMM-smoothed activity detection, endpointing.
Chunking is exact -- the chunks' results are those of one call on the whole audio -- and costs no graph compilation: the state is
an argument of the call.  Everything is a launch chain on the caller's stream; nothing synchronises the host.
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
