"""Entropy objectives on top of the engine: the entropy of the posterior over complete paths,

    H_b = - sum_pi P(pi | V_b) ln P(pi | V_b)        (nats),

with its exact gradient in the emissions (mm_pathentropy_f32: one forward and one backward kernel, a forward-backward in the
entropy semiring -- Hernando et al., "Efficient computation of the hidden Markov model entropy for a given observation sequence",
IEEE Trans. IT 2005; Li & Eisner, "First- and second-order expectation semirings", EMNLP 2009).  Over the shared denominator graph
of LF-MMI it is the conditional entropy of the state sequence given the audio: the objective of semi-supervised sequence training
on untranscribed audio (Manohar et al., "Semi-supervised maximum mutual information training of deep neural network acoustic
models", Interspeech 2015), an entropy regulariser for LF-MMI / CTC-style losses, and a per-utterance confidence figure.

    d H_b / d V[b, n, p] = grad[b, n, p]    (minus a covariance: -Cov(ln P(pi), [pdf_n = p]))

A launch chain on the caller's stream; in a data-parallel job the per-rank sums go through `dist.allreduce_logz`.
"""
from __future__ import annotations

from typing import Optional


def _function():
    import torch

    class _PathEntropy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, V, batch, lens, want_grad):
            ent, grad, ttl = batch.pathentropy(V.detach(), lens, want_grad=want_grad)
            if want_grad:
                ctx.save_for_backward(grad)
            ctx.mark_non_differentiable(ttl)
            return ent.double().sum().to(V.dtype), ent, ttl

        @staticmethod
        def backward(ctx, g_total, g_ent, _g_ttl):
            (grad,) = ctx.saved_tensors
            # (the total and the per-utterance entropies are both differentiable outputs: d / d V = (g_total + g_ent[b]) grad[b])
            w = g_total if g_ent is None else g_total + g_ent[:, None, None]
            return grad * w, None, None, None

    return _PathEntropy


def path_entropy(V, batch, lens: Optional["torch.Tensor"] = None):
    """V: [B, N, P] float32 on the HIP device (requires_grad as needed); batch: a BatchedFSM of B utterances (log semiring).
    Returns (sum_b H_b, H[B], ttl[B]).  Backward hands ``grad * g`` to V; without a gradient to compute (V does not require one, or under
    ``torch.no_grad()``) only the forward kernel runs.  Utterances without an accepting path have entropy 0, gradient 0 and ttl = -inf."""
    import torch

    # (asked here: inside Function.forward grad mode is always off)
    return _function().apply(V, batch, lens, bool(V.requires_grad and torch.is_grad_enabled()))


def conditional_entropy_loss(V, den_batch, lens: Optional["torch.Tensor"] = None):
    """The semi-supervised sequence objective for untranscribed audio: the conditional entropy of the denominator graph's state
    sequence given the audio, summed over the batch (Manohar et al., Interspeech 2015, who maximise the NEGATIVE conditional
    entropy: this function returns +sum_b H_b, a loss to MINIMISE).  V [B, N, P] float32 log-likelihoods on the HIP device,
    den_batch the denominator BatchedFSM.  Returns (loss, H[B], ttl[B]); utterances with ttl = -inf contribute nothing and are
    the caller's to filter, as in `lfmmi_loss`."""
    return path_entropy(V, den_batch, lens)
