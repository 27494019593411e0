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

A launch chain on the caller's stream.
"""
from __future__ import annotations


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
