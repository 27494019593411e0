"""Learnable graph weights: log Z as a differentiable function of the emissions, the arc log-weights and the initial log-weights
(``graph_loglik``, one mm_weightedposteriors_f32 call per forward and none in backward), and the Baum-Welch M-step on the host
(``reestimate``).  The topology and every compiled form of the batch stay as they are: a training step or an EM iteration
compiles nothing and uploads nothing but its weights."""
from __future__ import annotations

from typing import Optional

import numpy as np


def _function():
    import torch

    class _GraphLogLik(torch.autograd.Function):
        @staticmethod
        def forward(ctx, V, W, W_init, batch, lens):
            need_v, need_w, need_i = ctx.needs_input_grad[:3]
            res = batch.weightedposteriors(V.detach(), None if W is None else W.detach(), None if W_init is None else W_init.detach(),
                                           lens, want_gamma=need_v, want_counts=need_w, want_init=need_i)
            gamma, counts, ttl = res[:3]
            init = res[3] if need_i else None
            ctx.shared = (W is not None and W.dim() == 1, W_init is not None and W_init.dim() == 1)
            ctx.sizes = (None if W is None else W.shape[-1], None if W_init is None else W_init.shape[-1])
            ctx.have = (need_v, need_w, need_i)
            ctx.save_for_backward(*[t for t in (gamma, counts, init, ttl) if t is not None])
            return ttl

        @staticmethod
        def backward(ctx, g):
            torch = _torch()
            saved = list(ctx.saved_tensors)
            ttl = saved.pop()
            need_v, need_w, need_i = ctx.have
            gamma = saved.pop(0) if need_v else None
            counts = saved.pop(0) if need_w else None
            init = saved.pop(0) if need_i else None
            # (an utterance without a path: ttl = -inf, its gamma and counts are zeros; whatever comes down for it -- an inf or a NaN
            # of a loss over -inf -- must not reach them)
            g = torch.where(torch.isfinite(ttl), g, torch.zeros_like(g))
            gV = gamma * g[:, None, None] if need_v else None

            def wgrad(c, shared, n):
                c = c[:, :n] * g[:, None]
                if c.shape[1] < n:  # (a weight tensor wider than the largest FSM: the slack has no gradient)
                    c = torch.nn.functional.pad(c, (0, n - c.shape[1]))
                return c.sum(0) if shared else c

            gW = wgrad(counts, ctx.shared[0], ctx.sizes[0]) if need_w else None
            gI = wgrad(init, ctx.shared[1], ctx.sizes[1]) if need_i else None
            return gV, gW, gI, None, None

    return _GraphLogLik


def _torch():
    import torch

    return torch


def graph_loglik(V, batch, W=None, W_init=None, lens: Optional["torch.Tensor"] = None):
    """ttl[B] = log Z_b of every utterance under the call's weights, differentiable in all three inputs.

    V: [B, N, P] float32 on the HIP device; batch: a BatchedFSM of B utterances (log semiring); W: None (the FSMs' own weights), a
    1-D tensor (one weight vector for the whole batch, which must repeat one FSM) or [B, max nnz] (a vector per utterance), in the
    order of ``FSM.nzval``; W_init likewise in ``FSM.alpha_idx`` order.  Backward gives ``grad_V = g_b * gamma_b``, ``grad_W = g_b *
    counts_b`` and ``grad_W_init = g_b * init_b``, summed over b for a shared vector; only what an input that requires a gradient
    needs is computed.  An utterance without a path has ttl = -inf and zero gradients (never NaN)."""
    return _function().apply(V, W, W_init, batch, lens)


def reestimate(fsm, counts, init_counts=None, floor=1e-30):
    """The Baum-Welch M-step on the host: ``(W, W_init)`` float32, natural log, in the order ``weightedposteriors`` takes them.

    ``fsm`` the FSM the counts belong to; ``counts[nnz]`` the expected arc counts summed over the utterances (``FSM.nzval`` order),
    ``init_counts[n_init]`` the summed initial-state posteriors (None: ``alpha_hat`` stays, W_init comes back as None).  Every
    source state's out-entries, the final column included, are normalised to sum to 1: ``W[k] = log(max(c[k], floor) / max(sum of
    the source's counts, floor))``, so an arc nobody took keeps a (tiny) weight instead of -inf; the phony self-loop stays 0 = log
    one(K).  ``alpha_hat`` is normalised the same way."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1)
    nnz, S1 = fsm.nnz, int(fsm.colptr.shape[0]) - 1
    if c.shape[0] < nnz:
        raise ValueError(f"counts has {c.shape[0]} entries, the FSM has {nnz}")
    c = c[:nnz]
    src = np.asarray(fsm.rowval, dtype=np.int64)
    dst = np.repeat(np.arange(S1, dtype=np.int64), np.diff(fsm.colptr))
    phony = (src == S1 - 1) & (dst == S1 - 1)
    tot = np.bincount(src[~phony], weights=c[~phony], minlength=S1)
    W = np.where(phony, 0.0, np.log(np.maximum(c, floor) / np.maximum(tot[src], floor)))
    W_init = None
    if init_counts is not None:
        ic = np.asarray(init_counts, dtype=np.float64).reshape(-1)[: len(fsm.alpha_idx)]
        W_init = np.log(np.maximum(ic, floor) / max(float(ic.sum()), floor)).astype(np.float32)
    return W.astype(np.float32), W_init
