"""Lattice-based sequence objectives on top of the engine: the log-sum of a pruned lattice's paths under the emissions of this step,

    logz_b = ln sum_{path of the lattice of utterance b} exp W(path)

(mm_latticeposteriors_f32: the log-semiring forward-backward over the records of a ``Lattice``, the whole batch in one call), as an
autograd function.  With the lattice of a decoding graph it is the denominator of lattice-based MMI (Valtchev et al., "MMIE training
of large vocabulary recognition systems", Speech Communication 1997; Povey, "Discriminative training for large vocabulary speech
recognition", 2003): the loss is ``logz_den - logz_num`` per utterance, the numerator from the transcript's graph.  A boosting term
per record in ``extra`` -- b times the record's phone or state error against the reference -- makes it boosted MMI (Povey et al.,
"Boosted MMI for model and feature-space discriminative training", ICASSP 2008).

    d logz_b / d V[b, n, p] = gamma[b, n, p]         (the pdf occupancies of the lattice)
    d logz_b / d extra[r]   = exp(post[r])           (the record's posterior; r a record of utterance b)

and the expected cost of its paths,

    risk_b = sum_{path} exp(W(path) - logz_b) A(path),   A(path) = sum of cost[r] over the path's records

(mm_latticecost_f32), the lattice form of ``mbr.expected_cost``: with the cost of a record minus the phone or word accuracy of its arc
it is MPE / MWE (Povey 2003), with minus [pdf of the record's source = the alignment's pdf at that frame] state-level MBR
(``lattice_smbr_loss``; Vesely et al., "Sequence-discriminative training of deep neural networks", Interspeech 2013).

    d risk_b / d V[b, n, p] = grad[b, n, p]       d risk_b / d extra[r] = diff[r]       d risk_b / d cost[r] = exp(post[r])

and the weight of its best path, ``best_b = max_{path} W(path)`` (mm_latticebest_f32; ``lattice_best_score``): the Viterbi score of
perceptron and max-margin losses, whose gradient is the indicator of the best path's records and pdfs.

and, for a cost that does NOT add up along a path (a word error rate, an edit distance), the sampled risk: the mean cost of paths
drawn from the lattice's posterior (mm_latticesample_f32; ``lattice_sampled_risk``) with the score-function gradient.

A launch chain on the caller's stream.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np


def _function():
    import torch

    class _LatticeLoglik(torch.autograd.Function):
        @staticmethod
        def forward(ctx, V, extra, batch, lat, lens):
            post, logz, gamma = batch.latticeposteriors(lat, V.detach(), lens, None if extra is None else extra.detach())
            offsets = lat.offsets if isinstance(lat.offsets, torch.Tensor) else torch.as_tensor(lat.offsets)
            ctx.save_for_backward(post, logz, gamma, offsets.to(V.device))
            ctx.has_extra = extra is not None
            return logz

        @staticmethod
        def backward(ctx, g):
            post, logz, gamma, offsets = ctx.saved_tensors
            B, N = gamma.shape[0], gamma.shape[1]
            w = torch.where(torch.isneginf(logz), torch.zeros_like(g), g)  # (no path: gamma and exp(post) are 0, and g may be anything)
            gV = gamma * w[:, None, None]
            gE = None
            if ctx.has_extra:
                # the utterance of record r: the last b with offsets[b * N] <= r
                r = torch.arange(post.numel(), device=post.device, dtype=offsets.dtype)
                owner = (torch.searchsorted(offsets[::N][:B].contiguous(), r, right=True) - 1).clamp_(0, B - 1)
                gE = torch.exp(post) * w[owner]
            return gV, gE, None, None, None

    return _LatticeLoglik


def lattice_loglik(bf, lat, V, extra=None, lens=None):
    """``logz[B]`` of the lattice ``lat`` (a ``Lattice`` of ``bf.lattice``, or a subset of one) under ``V`` [B, N, P] float32 on the
    HIP device and the optional per-record scores ``extra`` (a float32 tensor of one score per record), both differentiable: backward
    hands ``gamma[b] * g[b]`` to ``V`` and ``exp(post[r]) * g[b(r)]`` to ``extra``.  Utterances without a path have ``logz = -inf``
    and zero gradients; they are the caller's to filter, as in ``lfmmi_loss``.  ``bf``: a tropical ``BatchedFSM``."""
    return _function().apply(V, extra, bf, lat, lens)


def _owner(offsets, nrec, B, N):
    """The utterance of every record: the last b with offsets[b * N] <= r."""
    import torch

    r = torch.arange(nrec, device=offsets.device, dtype=offsets.dtype)
    return (torch.searchsorted(offsets[::N][:B].contiguous(), r, right=True) - 1).clamp_(0, B - 1)


def _risk_function():
    import torch

    class _LatticeRisk(torch.autograd.Function):
        @staticmethod
        def forward(ctx, V, extra, cost, batch, lat, lens):
            res = batch.latticecost(lat, V.detach(), cost.detach(), lens, None if extra is None else extra.detach(), want_grad=True)
            offsets = lat.offsets if isinstance(lat.offsets, torch.Tensor) else torch.as_tensor(lat.offsets)
            ctx.save_for_backward(res.diff, res.post, res.logz, res.grad, offsets.to(V.device))
            ctx.has_extra = extra is not None
            return res.risk

        @staticmethod
        def backward(ctx, g):
            diff, post, logz, grad, offsets = ctx.saved_tensors
            B, N = grad.shape[0], grad.shape[1]
            w = torch.where(torch.isneginf(logz), torch.zeros_like(g), g)  # (no path: every gradient is 0, and g may be anything)
            gV = grad * w[:, None, None] if ctx.needs_input_grad[0] else None
            gE = gC = None
            if (ctx.has_extra and ctx.needs_input_grad[1]) or ctx.needs_input_grad[2]:
                wr = w[_owner(offsets, post.numel(), B, N)]
                if ctx.has_extra and ctx.needs_input_grad[1]:
                    gE = diff * wr
                if ctx.needs_input_grad[2]:
                    gC = torch.exp(post) * wr
            return gV, gE, gC, None, None, None

    return _LatticeRisk


def lattice_risk(bf, lat, V, cost, extra=None, lens=None):
    """``risk[B]``, the expected cost of the paths of the lattice ``lat`` (a ``Lattice`` of ``bf.lattice``, or a subset of one) under
    ``V`` [B, N, P] float32 on the HIP device, the per-record costs ``cost`` and the optional per-record scores ``extra`` (float32
    tensors of one value per record), all three differentiable: backward hands ``grad[b] * g[b]`` to ``V``, ``diff[r] * g[b(r)]`` to
    ``extra`` and ``exp(post[r]) * g[b(r)]`` to ``cost``.  Utterances without a path have risk 0 and zero gradients, as in
    ``lattice_loglik``.  ``bf``: a tropical ``BatchedFSM``."""
    return _risk_function().apply(V, extra, cost, bf, lat, lens)


def _state_pdfs(bf, device):
    """``[B, max S]`` int64 on ``device``: the pdf of every real state of every utterance's FSM (0 in the padding), made once per
    batch and device."""
    import torch

    cache = bf.__dict__.setdefault("_state_pdf_tables", {})
    if device not in cache:
        rows = [np.asarray(c.C_hat.state2pdf, dtype=np.int64).ravel()[: c.S1 - 1] for c in bf.cfsms]
        table = np.zeros((len(rows), max(r.size for r in rows)), dtype=np.int64)
        for b, r in enumerate(rows):
            table[b, : r.size] = r
        cache[device] = torch.as_tensor(table).to(device)
    return cache[device]


def _best_function():
    import torch

    class _LatticeBestScore(torch.autograd.Function):
        @staticmethod
        def forward(ctx, V, extra, batch, lat, lens):
            res = batch.latticebest(lat, V.detach(), lens, None if extra is None else extra.detach())
            ctx.save_for_backward(res.rec, res.path, _state_pdfs(batch, V.device))
            ctx.shape = tuple(V.shape)
            ctx.nrec = res.score.numel()
            ctx.has_extra = extra is not None
            return res.best

        @staticmethod
        def backward(ctx, g):
            rec, path, pdfs = ctx.saved_tensors
            on = path >= 0  # (the frames of the best path; none for an utterance without one, whatever its g)
            w = g[:, None].expand_as(path)[on]
            gV = gE = None
            if ctx.needs_input_grad[0]:
                b, n = torch.nonzero(on, as_tuple=True)
                gV = torch.zeros(ctx.shape, dtype=g.dtype, device=g.device)
                gV.index_put_((b, n, pdfs[b, path[on].long()]), w, accumulate=True)
            if ctx.has_extra and ctx.needs_input_grad[1]:
                gE = torch.zeros(ctx.nrec, dtype=g.dtype, device=g.device)
                gE.index_put_((rec[on],), w, accumulate=True)
            return gV, gE, None, None, None

    return _LatticeBestScore


def lattice_best_score(bf, lat, V, extra=None, lens=None):
    """``best[B]``, the weight of the best path of the lattice ``lat`` under ``V`` [B, N, P] float32 on the HIP device and the
    optional per-record scores ``extra`` (mm_latticebest_f32), both differentiable -- the Viterbi score of perceptron and max-margin
    losses against a lattice.  The maximum is piecewise linear: backward hands ``g[b]`` to ``extra`` at the records of the best
    path (the indicator of ``rec``) and to ``V`` at ``(b, n, pdf(path[b, n]))``, a subgradient where best paths tie.  Utterances
    without a path have ``best = -inf`` and zero gradients.  ``bf``: a tropical ``BatchedFSM``."""
    return _best_function().apply(V, extra, bf, lat, lens)


def _sampled_risk_function():
    import torch

    class _LatticeSampledRisk(torch.autograd.Function):
        @staticmethod
        def forward(ctx, V, extra, costs, rec, path, logz, pdfs):
            K = costs.shape[1]
            c = costs.detach().to(torch.float32)
            # the leave-one-out weights: (c_k - mean of the others) / K; they sum to 0 over k
            w = (c - (c.sum(1, keepdim=True) - c) / (K - 1)) / K
            ctx.save_for_backward(w, rec, path, pdfs)
            ctx.shape = tuple(V.shape)
            ctx.nrec = None if extra is None else extra.numel()
            return torch.where(torch.isneginf(logz), torch.zeros_like(logz), c.mean(1))

        @staticmethod
        def backward(ctx, g):
            w, rec, path, pdfs = ctx.saved_tensors
            on = path >= 0  # (the frames of the samples; none for an utterance without a path, whatever its g)
            v = (g[:, None] * w)[:, :, None].expand_as(path)[on]
            gV = gE = None
            if ctx.needs_input_grad[0]:
                b, _, n = torch.nonzero(on, as_tuple=True)
                gV = torch.zeros(ctx.shape, dtype=g.dtype, device=g.device)
                gV.index_put_((b, n, pdfs[b, path[on].long()]), v, accumulate=True)
            if ctx.nrec is not None and ctx.needs_input_grad[1]:
                gE = torch.zeros(ctx.nrec, dtype=g.dtype, device=g.device)
                gE.index_put_((rec[on],), v, accumulate=True)
            return gV, gE, None, None, None, None, None

    return _LatticeSampledRisk


def lattice_sampled_risk(bf, lat, V, samples, costs, extra=None):
    """``risk[B]``, the sampled risk of the lattice ``lat`` for costs that do NOT add up along a path: ``risk[b] = mean_k costs[b, k]``
    with ``costs`` [B, K] whatever the caller computed from ``samples`` -- the ``LatticeSamples`` of ``bf.latticesample(lat, V, K, ..)``
    with its ``path``, on the same ``V`` and ``extra`` -- such as the edit distance of each sampled word sequence to the transcript
    (Shannon, "Optimizing expected word error rate via sampling for speech recognition", Interspeech 2017; Prabhavalkar et al.,
    "Minimum word error rate training for attention-based sequence-to-sequence models", ICASSP 2018).  K >= 2.  ``costs`` takes no
    gradient.  Differentiable in ``V`` [B, N, P] float32 on the HIP device and in the per-record scores ``extra`` by the
    score-function estimator with the leave-one-out baseline:

        w_k = (c_k - mean_{k' != k} c_k') / K
        d risk[b] / d V[b, n, p] ~ sum_k w_k [pdf(path[b, k, n]) = p]        d risk[b] / d extra[r] ~ sum_k w_k [rec[b, k, n] = r]

    The gradient of a path's log posterior is its indicator minus the posteriors gamma; the weights of an utterance sum to 0, so
    the gamma term drops out and no posterior call is needed.  The estimate is unbiased for the gradient of the expected cost (it is
    K / (K - 1) times the sample covariance of the cost and the indicator).  Utterances without a path have risk 0 and zero
    gradients.  ``lat`` is read for nothing but its place in the call (the samples name its records).  ``bf``: a tropical
    ``BatchedFSM``."""
    import torch

    if samples.path is None:
        raise ValueError("lattice_sampled_risk: the samples need their path (latticesample(.., want_path=True))")
    dev = V.device
    rec, path, logz = (torch.as_tensor(x).to(dev) for x in (samples.rec, samples.path, samples.logz))
    costs = torch.as_tensor(costs).to(dev)
    if costs.dim() != 2 or tuple(costs.shape) != tuple(path.shape[:2]):
        raise ValueError(f"lattice_sampled_risk: costs must be [B, K] = {tuple(path.shape[:2])}, got {tuple(costs.shape)}")
    if costs.shape[1] < 2:
        raise ValueError("lattice_sampled_risk: the leave-one-out baseline needs K >= 2 samples")
    return _sampled_risk_function().apply(V, extra, costs, rec, path, logz, _state_pdfs(bf, dev))


class RecordIndex(NamedTuple):
    """Per record of a lattice, int64 tensors: its utterance ``b``, its transition ``t`` and the pdf of its source state ``pdf``
    (``P``, the phony pdf, for an entry outside the FSM and for records no cell covers); ``P`` itself."""

    b: object
    t: object
    pdf: object
    P: int


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def record_index_host(fsms, state2pdfs, P, offsets, arc):
    """``record_index`` on host arrays: ``fsms[b]`` / ``state2pdfs[b]`` the FSM and the pdf per real state of utterance b; NumPy
    int64 arrays ``(b, t, pdf)``."""
    from .fsm import _entry_ends

    offsets, arc = np.asarray(offsets, dtype=np.int64), np.asarray(arc, dtype=np.int64)
    B = len(fsms)
    N = (offsets.size - 1) // B
    nrec = arc.size
    off = np.maximum.accumulate(np.clip(offsets, 0, nrec))
    cell = np.searchsorted(off, np.arange(nrec), side="right") - 1  # the last cell that starts at or before r
    covered = (cell >= 0) & (cell < B * N)
    cell = np.clip(cell, 0, B * N - 1)
    bi, ti = cell // N, cell % N
    pdf = np.full(nrec, P, dtype=np.int64)
    for b in range(B):
        src, _ = _entry_ends(fsms[b])
        s2p = np.concatenate([np.asarray(state2pdfs[b], dtype=np.int64).ravel()[: fsms[b].S1 - 1], [P]])
        m = covered & (bi == b) & (arc >= 0) & (arc < src.size)
        pdf[m] = s2p[src[arc[m]]]
    return bi.astype(np.int64), ti.astype(np.int64), pdf


def record_index(bf, lat):
    """Per record of ``lat`` its utterance, its transition and the pdf of its source state: a ``RecordIndex`` of int64 tensors on the
    device of ``lat.arc`` (the host for NumPy members), built once per lattice on the host from the FSMs' entry lists as
    ``decode.lattice_arcs`` reads them."""
    import torch

    bi, ti, pdf = record_index_host([c.fsm for c in bf.cfsms], [c.C_hat.state2pdf for c in bf.cfsms], bf.P, _host(lat.offsets), _host(lat.arc))
    dev = lat.arc.device if isinstance(lat.arc, torch.Tensor) else torch.device("cpu")
    return RecordIndex(*(torch.as_tensor(x).to(dev) for x in (bi, ti, pdf)), bf.P)


def pdf_costs(index, D):
    """Frame costs on records: ``D[b, t, pdf]`` [B, N, P] gathered by a ``RecordIndex`` (or a ``(b, t, pdf)`` triple), one gather,
    differentiable in a tensor ``D``; the phony pdf ``P`` costs 0.  It puts ``expected_cost``'s frame costs, such as sMBR's
    ``-[pdf = alignment]``, onto the records of a lattice."""
    bi, ti, pdf = index[0], index[1], index[2]
    if hasattr(D, "detach"):
        import torch

        Dp = torch.nn.functional.pad(D, (0, 1))
        dev = D.device
        return Dp[torch.as_tensor(bi).to(dev), torch.as_tensor(ti).to(dev), torch.as_tensor(pdf).to(dev)]
    D = np.asarray(D)
    Dp = np.concatenate([D, np.zeros(D.shape[:2] + (1,), dtype=D.dtype)], axis=2)
    return Dp[_host(bi), _host(ti), _host(pdf)]


def lattice_smbr_loss(bf, lat, V, ali, lens=None, index=None):
    """State-level MBR on a lattice: ``risk[B]`` with the cost of a record ``-[pdf of its source = ali[b, t]]``, so the risk is minus
    the expected number of frames (of the ``len``) on which the lattice's paths agree with the alignment ``ali`` [B, N] (pdf
    indices), between ``-len`` and 0.  Differentiable in ``V``.  ``index``: ``record_index(bf, lat)`` when the caller keeps it."""
    import torch

    index = record_index(bf, lat) if index is None else index
    a = torch.as_tensor(ali).to(V.device).long()
    D = -torch.nn.functional.one_hot(a.clamp(0, index.P - 1), index.P).to(torch.float32) * (a >= 0)[..., None]
    return lattice_risk(bf, lat, V, pdf_costs(index, D).to(V.device), lens=lens)
