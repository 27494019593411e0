"""Minimum Bayes risk objectives on top of the engine: the expected cost of a path under the path posterior,

    risk_b = E_{pi ~ P(pi | V_b)} [ sum_n cost_b(n, pdf(pi_n)) ],

with its exact gradient (mm_expectedcost_f32: one forward and one backward kernel, a forward-backward in the first-order
expectation semiring).  With cost = -[pdf equals the reference alignment's pdf] over the shared denominator graph it is lattice-free
sMBR (Kanda et al., "Lattice-free state-level minimum Bayes risk training", Interspeech 2018), the usual second stage after LF-MMI
(`lfmmi.lfmmi_loss`) on the same graph and batch shape; with other costs any frame-decomposable Bayes risk, or an exact control
variate for objectives estimated from `samplepaths`.

    d risk_b / d V[b, n, p]    = grad[b, n, p]    (a covariance: Cov(cost of the whole path, [pdf_n = p]))
    d risk_b / d cost[b, n, p] = gamma[b, n, p]   (the pdf posterior)

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
