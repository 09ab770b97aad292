"""Target-attention pooling over a raw (sequence) slot (csrc/seqattn.hip).

``seq_attn_pool(q, seq)`` consumes the ``(B, sample_fixed_size, dim+1)`` f16
tensor ``prepare_features`` builds for a raw slot, mask channel included, and
a ``(B, dim)`` f16 query (typically a sum slot's tensor): one HIP kernel in
forward, one in backward (scores and probabilities are recomputed there,
nothing but ``q`` and ``seq`` is saved).  The eager chain it replaces is
slice / bmm / masked_fill / softmax / bmm and the backward of each.

The native path is taken for f16 CUDA tensors when the extension is built and
``seq_attn_feasible(L, D)`` holds; everything else (CPU, other dtypes, shapes
without a kernel) runs ``ops.reference.seq_attn_pool_reference``.
``PA_SEQ_ATTN=0`` forces the reference (A/B); read once at import.
"""
import os
from typing import Optional

import torch

from persia_amd.ops import native, native_available
from persia_amd.ops.reference import seq_attn_pool_reference

_ENABLED = os.environ.get("PA_SEQ_ATTN", "1") != "0"


class SeqAttnPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, seq, scale: float):
        q, seq = q.contiguous(), seq.contiguous()
        out = native().seq_attn_fwd(q, seq, scale)
        ctx.save_for_backward(q, seq)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, g):
        q, seq = ctx.saved_tensors
        g = g.to(torch.float16).contiguous()
        dq, dseq = native().seq_attn_bwd(g, q, seq, ctx.scale)
        return dq, dseq, None


def _takes_native(q: torch.Tensor, seq: torch.Tensor) -> bool:
    return (
        _ENABLED
        and q.is_cuda
        and seq.is_cuda
        and q.dtype == torch.float16
        and seq.dtype == torch.float16
        and native_available()
        and native().seq_attn_feasible(seq.shape[1], q.shape[1])
    )


def seq_attn_pool(
    q: torch.Tensor, seq: torch.Tensor, scale: Optional[float] = None
) -> torch.Tensor:
    """q [B, D], seq [B, L, D+1] (channel D the 0/1 mask) -> [B, D]."""
    if q.dim() != 2 or seq.dim() != 3 or seq.shape[0] != q.shape[0] \
            or seq.shape[2] != q.shape[1] + 1:
        raise ValueError(
            f"seq_attn_pool: expected q [B, D] and seq [B, L, D+1], got "
            f"{tuple(q.shape)} and {tuple(seq.shape)}"
        )
    if scale is None:
        scale = float(q.shape[1]) ** -0.5
    if _takes_native(q, seq):
        return SeqAttnPoolFn.apply(q, seq, float(scale))
    return seq_attn_pool_reference(q, seq, float(scale))
