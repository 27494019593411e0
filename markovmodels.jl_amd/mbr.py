"""Minimum Bayes risk objectives on top of the engine: the expected cost of a path under the path posterior,

    risk_b = E_{pi ~ P(pi | V_b)} [ sum_n cost_b(n, pdf(pi_n)) ],

with its exact gradient (mm_expectedcost_f32: one forward and one backward kernel, a forward-backward in the first-order
expectation semiring).  With cost = -[pdf equals the reference alignment's pdf] over the shared denominator graph it is lattice-free
sMBR (Kanda et al., "Lattice-free state-level minimum Bayes risk training", Interspeech 2018), the usual second stage after LF-MMI
(`lfmmi.lfmmi_loss`) on the same graph and batch shape; with other costs any frame-decomposable Bayes risk, or an exact control
variate for objectives estimated from `samplepaths`.

    d risk_b / d V[b, n, p]    = grad[b, n, p]    (a covariance: Cov(cost of the whole path, [pdf_n = p]))
    d risk_b / d cost[b, n, p] = gamma[b, n, p]   (the pdf posterior)

Costs that sit on an arc rather than on a frame's pdf -- a phone or a word that is right or wrong where its arc is entered
(lattice-free MPE / MWE), insertion and length penalties, an expected number of boundaries -- go through `expected_class_cost`
(mm_classcost_f32): under the arc classes of `BatchedFSM.set_arc_classes`,

    risk_b = E_{pi ~ P(pi | V_b)} [ sum_n D_b(n, pdf(pi_n)) + sum_t A_b(t, class of the arc taken at transition t) ],
    d risk_b / d A[b, t, c] = xi[b, c, t]   (the arc-class posterior of `arcclassposteriors`)

Both are launches on the caller's stream; in a data-parallel job the per-rank sums go through `dist.allreduce_logz`.
"""
from __future__ import annotations

from typing import Optional


def _function():
    import torch

    class _ExpectedCost(torch.autograd.Function):
        @staticmethod
        def forward(ctx, V, cost, batch, lens):
            want_gamma = bool(cost.requires_grad)
            out = batch.expectedcost(V.detach(), cost.detach(), lens, want_gamma=want_gamma)
            risk, grad, ttl = out[:3]
            ctx.want_gamma = want_gamma
            ctx.save_for_backward(grad, *out[3:])
            ctx.mark_non_differentiable(ttl)
            return risk.double().sum().to(V.dtype), risk, ttl

        @staticmethod
        def backward(ctx, g_total, g_risk, _g_ttl):
            grad, *rest = ctx.saved_tensors
            # (the total and the per-utterance risks are both differentiable outputs: d / d V = (g_total + g_risk[b]) grad[b])
            w = g_total if g_risk is None else g_total + g_risk[:, None, None]
            return grad * w, (rest[0] * w) if ctx.want_gamma else None, None, None

    return _ExpectedCost


def expected_cost(V, cost, batch, lens: Optional["torch.Tensor"] = None):
    """V, cost: [B, N, P] float32 on the HIP device (requires_grad as needed); batch: a BatchedFSM of B utterances (log semiring).
    Returns (sum_b risk_b, risk[B], ttl[B]).  Backward hands ``grad * g`` to V and ``gamma * g`` to cost (the posteriors are only
    computed when cost requires a gradient).  Utterances without an accepting path have risk 0, gradient 0 and ttl = -inf."""
    return _function().apply(V, cost, batch, lens)


def smbr_loss(V, ref_pdfs, den_batch, lens: Optional["torch.Tensor"] = None):
    """Lattice-free sMBR: V [B, N, P] float32 log-likelihoods on the HIP device, ref_pdfs int [B, N] the reference alignment's pdf
    of every frame (entries at frames >= len_b are ignored), den_batch the denominator BatchedFSM.  The cost is -onehot(ref_pdfs),
    built on the device.  Returns (loss, accuracy[B], ttl[B]): loss = -(expected number of correct frames), summed over the
    batch; accuracy[b] = the expected number of frames of utterance b whose pdf equals the reference's.  Utterances with
    ttl = -inf contribute nothing and are the caller's to filter, as in `lfmmi_loss`."""
    import torch

    B, N, P = V.shape
    ref = torch.as_tensor(ref_pdfs, device=V.device).long()
    if tuple(ref.shape) != (B, N):
        raise ValueError(f"ref_pdfs must be [B={B}, N={N}], got {tuple(ref.shape)}")
    cost = torch.zeros((B, N, P), dtype=torch.float32, device=V.device)
    cost.scatter_(2, ref.clamp(0, P - 1)[:, :, None], -1.0)
    loss, risk, ttl = expected_cost(V, cost, den_batch, lens)
    return loss, -risk, ttl


def _class_function():
    import torch

    class _ExpectedClassCost(torch.autograd.Function):
        @staticmethod
        def forward(ctx, V, A, D, batch, lens):
            want_gamma = D is not None and bool(D.requires_grad)
            want_xi = bool(A.requires_grad)
            Vd = V.detach()
            out = batch.classcost(Vd, A.detach(), lens, D=None if D is None else D.detach(), want_gamma=want_gamma)
            risk, grad, ttl = out[:3]
            saved = [grad] + list(out[3:])
            if want_xi:  # d risk / d A = xi: one arcclassposteriors call, only when A asks for a gradient
                xi, _ = batch.arcclassposteriors(Vd, lens)
                xi = xi.permute(0, 2, 1).clone()  # [B, N, C]
                if lens is not None:
                    L = torch.as_tensor(lens, device=xi.device).long()
                    xi = xi * (torch.arange(xi.shape[1], device=xi.device)[None, :] < L[:, None])[:, :, None]
                saved.append(xi)
            ctx.want_gamma, ctx.want_xi = want_gamma, want_xi
            ctx.save_for_backward(*saved)
            ctx.mark_non_differentiable(ttl)
            return risk.double().sum().to(V.dtype), risk, ttl

        @staticmethod
        def backward(ctx, g_total, g_risk, _g_ttl):
            saved = list(ctx.saved_tensors)
            grad = saved.pop(0)
            gamma = saved.pop(0) if ctx.want_gamma else None
            xi = saved.pop(0) if ctx.want_xi else None
            w = g_total if g_risk is None else g_total + g_risk[:, None, None]
            return grad * w, (xi * w) if xi is not None else None, (gamma * w) if gamma is not None else None, None, None

    return _ExpectedClassCost


def expected_class_cost(V, A, batch, lens: Optional["torch.Tensor"] = None, D=None):
    """V: [B, N, P], A: [B, N, C], D: [B, N, P] or None, float32 on the HIP device (requires_grad as needed); batch: a BatchedFSM of B
    utterances (log semiring) with its arc classes set (``set_arc_classes``).  Returns (sum_b risk_b, risk[B], ttl[B]).  Backward
    hands ``grad * g`` to V, ``gamma * g`` to D when D requires a gradient (the posteriors are only computed then), and ``xi * g`` to
    A: xi comes from ONE ``arcclassposteriors`` call, made in forward only when A requires a gradient, and is zeroed for t >= len
    (the rows the entry never reads; an utterance without an accepting path has xi = 0 already).  Utterances without an accepting
    path have risk 0, gradient 0 and ttl = -inf."""
    return _class_function().apply(V, A, D, batch, lens)


def mpe_loss(V, ref_classes, batch, lens: Optional["torch.Tensor"] = None):
    """Lattice-free MPE / MWE: V [B, N, P] float32 log-likelihoods on the HIP device, ref_classes int [B, N] the reference's arc
    class at every transition t (the arc from frame t to frame t + 1; t = len - 1: the arc into the final state), batch the
    denominator BatchedFSM with its arc classes set.  The cost is A = -onehot(ref_classes[b, t]), built on the device; entries < 0
    and entries at t >= len_b cost nothing.  Returns (loss, accuracy[B], ttl[B]): loss = -(expected number of transitions whose
    class equals the reference's), summed over the batch; accuracy[b] that expectation for utterance b.  Utterances with
    ttl = -inf contribute nothing and are the caller's to filter, as in `smbr_loss`."""
    import torch

    B, N, P = V.shape
    nc = max(1, batch.info()["arcclass_C"])
    ref = torch.as_tensor(ref_classes, device=V.device).long()
    if tuple(ref.shape) != (B, N):
        raise ValueError(f"ref_classes must be [B={B}, N={N}], got {tuple(ref.shape)}")
    hit = (ref >= 0) & (ref < nc)
    if lens is not None:
        L = torch.as_tensor(lens, device=V.device).long()
        hit = hit & (torch.arange(N, device=V.device)[None, :] < L[:, None])
    A = torch.zeros((B, N, nc), dtype=torch.float32, device=V.device)
    A.scatter_(2, ref.clamp(0, nc - 1)[:, :, None], -hit.to(torch.float32)[:, :, None])
    loss, risk, ttl = expected_class_cost(V, A, batch, lens)
    return loss, -risk, ttl
