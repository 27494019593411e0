"""Long recordings on top of the engine: the log-likelihood of a batch under its graphs,

    log Z_b = ln sum_pi P(pi, V_b),        d log Z_b / d V[b, n, p] = gamma[b, n, p],

with the exact smoothing posteriors computed chunk by chunk (``BatchedFSM.chunkedposteriors``: a forward filtering pass that keeps
no frame, then mm_segmentposteriors_f32 over the chunks in reverse, each ending on the end vector the chunk behind it handed
back).  The alpha~ store is that of one chunk whatever the length of the audio: the denominator term of LF-MMI for recordings
whose store does not fit in one call.

A launch chain on the caller's stream; in a data-parallel job the per-rank sums go through `dist.allreduce_logz`.
"""
from __future__ import annotations

from typing import Optional


def _function():
    import torch

    class _ChunkedLoglik(torch.autograd.Function):
        @staticmethod
        def forward(ctx, V, batch, lens, chunk):
            gamma, ttl = batch.chunkedposteriors(V.detach(), lens, chunk=chunk)
            ctx.save_for_backward(gamma)
            return ttl

        @staticmethod
        def backward(ctx, grad):
            (gamma,) = ctx.saved_tensors
            return grad[:, None, None] * gamma, None, None, None

    return _ChunkedLoglik


def chunked_loglik(V, batch, lens: Optional["torch.Tensor"] = None, chunk: int = 1024):
    """V: [B, N, P] float32 on the HIP device (requires_grad as needed); batch: a BatchedFSM of B utterances (log semiring); chunk:
    the most frames one call of the engine sees.  Returns log Z [B]; backward hands ``grad[:, None, None] * gamma`` to V without a
    call of the engine.  Utterances without an accepting path have log Z = -inf and gamma = 0: they are the caller's to filter, as
    in `lfmmi_loss`."""
    return _function().apply(V, batch, lens, int(chunk))
