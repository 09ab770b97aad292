"""The tail of a transformer block over a raw slot (csrc/seqffn.hip).

``seq_ffn(x, a, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2, eps=1e-5)`` takes
the block input ``x`` and the attention output ``a`` (both ``(B,
sample_fixed_size, dim+1)`` f16 raw-slot tensors; the mask of ``x`` decides)
and computes, on every valid row,

    u = LayerNorm(x + Wo a + bo; g1, be1)
    y = LayerNorm(u + W2 relu(W1 u + b1) + b2; g2, be2)

-- what follows the attention in a post-norm ``nn.TransformerEncoderLayer``
with ReLU and no dropout -- and returns a raw-slot tensor again (invalid rows
+0, mask channel copied).  With ``seq_self_attn(residual=False)`` in front it
is the whole layer on two kernels per direction; ``models.SeqEncoderLayer``
holds the parameters under ``nn.TransformerEncoderLayer``'s names.

The native path is taken for f16 CUDA ``x`` and ``a`` with f32 CUDA
parameters when the extension is built and ``seq_ffn_feasible(D, F)`` holds
(D in {32, 64}, F a multiple of 32 in 32..256; any L); everything else runs
``ops.reference.seq_ffn_reference``.  ``PA_SEQ_FFN=0`` forces the reference
(A/B); read once at import.
"""
import os

import torch

from persia_amd.ops import native, native_available
from persia_amd.ops.reference import seq_ffn_reference

_ENABLED = os.environ.get("PA_SEQ_FFN", "1") != "0"
_MATRICES = (2, 6, 8)  # Wo, W1, W2 among the twelve tensor arguments


class SeqFfnFn(torch.autograd.Function):
    """Takes the f32 masters of Wo, W1, W2 and rounds them to f16 inside, so
    their f32 gradients pass straight through the rounding."""

    @staticmethod
    def forward(ctx, eps, *tensors):
        ctx.set_materialize_grads(False)
        tensors = [t.half().contiguous() if i in _MATRICES else t.contiguous()
                   for i, t in enumerate(tensors)]
        ctx.save_for_backward(*tensors)
        ctx.eps = eps
        return native().seq_ffn_fwd(*tensors, eps)

    @staticmethod
    def backward(ctx, g_out):
        if g_out is None:
            return (None,) * 13
        g_out = g_out.to(torch.float16).contiguous()
        return (None, *native().seq_ffn_bwd(g_out, *ctx.saved_tensors, ctx.eps))


def _takes_native(x, a, params) -> bool:
    return (
        _ENABLED
        and all(t.is_cuda and t.dtype == torch.float16 for t in (x, a))
        and all(p.is_cuda and p.dtype == torch.float32 for p in params)
        and native_available()
        and native().seq_ffn_feasible(x.shape[2] - 1, params[4].shape[0])
    )


def seq_ffn(x, a, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2, eps=1e-5):
    """x, a [B, L, D+1] (channel D of x the 0/1 mask), Wo [D, D], W1 [F, D],
    W2 [D, F], b1 [F], the other vectors [D] -> out [B, L, D+1], channel D
    copied from x."""
    if x.dim() != 3 or x.shape[2] < 2 or a.shape != x.shape:
        raise ValueError(
            f"seq_ffn: expected x and a [B, L, D+1], got {tuple(x.shape)} and "
            f"{tuple(a.shape)}")
    D = x.shape[2] - 1
    F = W1.shape[0] if W1.dim() == 2 else -1
    params = (Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2)
    want = ((D, D), (D,), (D,), (D,), (F, D), (F,), (D, F), (D,), (D,), (D,))
    if F < 1 or any(tuple(p.shape) != w for p, w in zip(params, want)):
        raise ValueError(
            f"seq_ffn: expected Wo [D, D], W1 [F, D], W2 [D, F], b1 [F] and "
            f"[D] vectors with D = {D}, got {[tuple(p.shape) for p in params]}")
    if not _takes_native(x, a, params):
        return seq_ffn_reference(x, a, *params, eps)
    return SeqFfnFn.apply(float(eps), x, a, *params)
