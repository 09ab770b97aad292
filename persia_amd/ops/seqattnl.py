"""Target-attention pooling for raw slots of any length up to 1024
(csrc/seqattnl.hip): ``seq_attn_pool``'s function with the sample streamed.

``seq_attn_pool_long(q, seq, scale=None)`` is
``ops.reference.seq_attn_pool_reference`` -- the definition of
``ops.seqattn.seq_attn_pool`` -- for samples that do not fit that kernel's
whole-sample LDS image.  On the GPU one block of four waves streams a sample's
rows through LDS in chunks with an online softmax, one kernel per direction;
the backward recomputes scores and probabilities in two streamed passes, so
nothing but ``q`` and ``seq`` is saved.

The native path is taken for f16 CUDA tensors when the extension is built and
``seq_attn_long_feasible(L, D)`` holds (D % 8 == 0, 8 <= D <= 256, 1 <= L <=
1024); everything else runs the reference.  ``PA_SEQ_ATTN_LONG=0`` forces the
reference (A/B); read once at import.  ``models.TargetAttentionPool`` and
``models.SelfAttentionPool`` call this where ``prefers_long`` says so: the
shapes ``seq_attn_pool`` has no kernel for, and those above
``LONG_ABOVE_BYTES``.
"""
import os
from typing import Optional

import torch

from persia_amd.ops import native, native_available
from persia_amd.ops.reference import seq_attn_pool_reference

_ENABLED = os.environ.get("PA_SEQ_ATTN_LONG", "1") != "0"

# The models' switch: a sample whose backward footprint in seqattn.hip,
# L (D+1) 2 + 8 (L + D) + 48 bytes, is above this goes to the long op, as does
# every shape that kernel refuses (its own limit is 65536).  Measured
# (docs/ARCHITECTURE.md, the streamed pooling section): at (L, D) = (200, 64),
# 28160 bytes, and (200, 128), 54272 bytes, where seqattn.hip runs one wave
# per block, the long kernels' slowest repetition beats its fastest.  Nothing
# was measured below 28160 bytes, so the switch stands just under it.
LONG_ABOVE_BYTES = 28000


def prefers_long(L: int, D: int) -> bool:
    """True if the models pool (L, D) samples on the GPU with
    ``seq_attn_pool_long``; needs the extension."""
    return (not native().seq_attn_feasible(L, D)
            or L * (D + 1) * 2 + 8 * (L + D) + 48 > LONG_ABOVE_BYTES)


class SeqAttnPoolLongFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, seq, scale: float):
        q, seq = q.contiguous(), seq.contiguous()
        out = native().seq_attn_long_fwd(q, seq, scale)
        ctx.save_for_backward(q, seq)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, g):
        q, seq = ctx.saved_tensors
        g = g.to(torch.float16).contiguous()
        dq, dseq = native().seq_attn_long_bwd(g, q, seq, ctx.scale)
        return dq, dseq, None


def _takes_native(q: torch.Tensor, seq: torch.Tensor) -> bool:
    return (
        _ENABLED
        and q.is_cuda
        and seq.is_cuda
        and q.dtype == torch.float16
        and seq.dtype == torch.float16
        and native_available()
        and native().seq_attn_long_feasible(seq.shape[1], q.shape[1])
    )


def seq_attn_pool_long(
    q: torch.Tensor, seq: torch.Tensor, scale: Optional[float] = None
) -> torch.Tensor:
    """q [B, D], seq [B, L, D+1] (channel D the 0/1 mask) -> [B, D]."""
    if q.dim() != 2 or seq.dim() != 3 or seq.shape[0] != q.shape[0] \
            or seq.shape[2] != q.shape[1] + 1:
        raise ValueError(
            f"seq_attn_pool_long: expected q [B, D] and seq [B, L, D+1], got "
            f"{tuple(q.shape)} and {tuple(seq.shape)}"
        )
    if scale is None:
        scale = float(q.shape[1]) ** -0.5
    if _takes_native(q, seq):
        return SeqAttnPoolLongFn.apply(q, seq, float(scale))
    return seq_attn_pool_reference(q, seq, float(scale))
