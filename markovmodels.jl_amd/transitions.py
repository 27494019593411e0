"""Frame-dependent transition scores: log Z as a differentiable function of the emissions and of per-frame scores on classes of arcs
(``transition_loglik``, one mm_scoredposteriors_f32 call per forward and none in backward), and alignment constraints as such
scores (``constraint_scores``).  The classes are the batch's (``BatchedFSM.set_arc_classes``; ``fsm.loop_exit_classes`` makes
the loop / exit classes of an HMM); the topology and every compiled form stay as they are."""
from __future__ import annotations

from typing import Optional


def _torch():
    import torch

    return torch


def _function():
    import torch

    class _TransitionLogLik(torch.autograd.Function):
        @staticmethod
        def forward(ctx, V, U, batch, lens):
            need_v, need_u = ctx.needs_input_grad[:2]
            gamma, xi, ttl = batch.scoredposteriors(V.detach(), None if U is None else U.detach(), lens, want_gamma=need_v, want_xi=need_u)
            ctx.have = (need_v, need_u)
            ctx.lens = lens
            ctx.save_for_backward(*[t for t in (gamma, xi, ttl) if t is not None])
            return ttl

        @staticmethod
        def backward(ctx, g):
            torch = _torch()
            saved = list(ctx.saved_tensors)
            ttl = saved.pop()
            need_v, need_u = ctx.have
            gamma = saved.pop(0) if need_v else None
            xi = saved.pop(0) if need_u else None
            # (an utterance without a path: ttl = -inf, its gamma and xi are zeros; whatever comes down for it -- an inf or a NaN
            # of a loss over -inf -- must not reach them)
            g = torch.where(torch.isfinite(ttl), g, torch.zeros_like(g))
            gV = gamma * g[:, None, None] if need_v else None
            gU = None
            if need_u:
                gU = xi.permute(0, 2, 1) * g[:, None, None]  # [B, N, C], the layout of U (and of the buffer xi is a view of)
                if ctx.lens is not None:  # (the rows t >= len are not part of Z: the phony loop's 1.0 is no gradient)
                    N = gU.shape[1]
                    live = torch.arange(N, device=gU.device)[None, :] < ctx.lens.to(gU.device)[:, None].clamp(0, N)
                    gU = gU * live[:, :, None]
            return gV, gU, None, None

    return _TransitionLogLik


def transition_loglik(V, U, batch, lens: Optional["torch.Tensor"] = None):
    """ttl[B] = log Z_b(U) of every utterance, differentiable in the emissions and in the scores.

    V: [B, N, P] float32 on the HIP device; U: [B, N, C] float32 on the device, the score of class c at the transition between
    frames t and t + 1 (finite or -inf), or None; batch: a BatchedFSM of B utterances (log semiring) whose classes
    ``set_arc_classes`` has set.  Backward gives ``grad_V = g_b * gamma_b`` and ``grad_U = g_b * xi_b`` with the rows t >= len_b
    zeroed; only what an input that requires a gradient needs is computed.  An utterance without a path has ttl = -inf and zero
    gradients (never NaN)."""
    return _function().apply(V, U, batch, lens)


def constraint_scores(allowed):
    """Scores that enforce a constraint: a bool array or tensor ``[B, N, C]`` -- class c may fire at the transition between frames t
    and t + 1 -- becomes float32 scores of the same shape and kind, 0 where allowed and -inf where not (an alignment window: the
    tolerance around a reference alignment as the frames at which a class's arcs may be taken)."""
    torch = _torch()
    if isinstance(allowed, torch.Tensor):
        if allowed.dtype != torch.bool:
            raise TypeError("allowed must be a bool tensor")
        out = torch.zeros(allowed.shape, dtype=torch.float32, device=allowed.device)
        return out.masked_fill_(~allowed, float("-inf"))
    import numpy as np

    a = np.asarray(allowed)
    if a.dtype != np.bool_:
        raise TypeError("allowed must be a bool array")
    return np.where(a, np.float32(0.0), np.float32(-np.inf)).astype(np.float32)
