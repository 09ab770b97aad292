"""Self-attention among the rows of a raw slot of any length up to 1024
(csrc/seqsal.hip): ``seq_self_attn``'s function with the keys streamed.

``seq_self_attn_long(seq, Wqkv, bqkv, heads, causal=False, residual=False)``
is ``ops.reference.seq_self_attn_reference`` -- the definition of
``ops.seqsa.seq_self_attn`` -- for sequences that do not fit that kernel's one
64-row tile.  On the GPU a projection kernel writes ``[q | k | v]`` of every
row to an f16 workspace, the attention kernel streams 64-row key tiles of it
through LDS with an online softmax and returns the log-sum-exp of every row
and head; the backward projects again, takes ``dQ`` with the queries
stationary and ``dK``, ``dV`` with the keys stationary, and finishes with the
projection's backward and the ordered sum of its per-block weight-gradient
partials.  Forward saves the inputs and the log-sum-exp only.

The native path is taken for an f16 CUDA ``seq`` with f32 CUDA parameters
when the extension is built and ``seq_self_attn_long_feasible(L, D, heads)``
holds (D in {32, 64}, D / heads in {16, 32}, 1 <= L <= 1024); everything else
runs the reference.  ``PA_SEQ_SELF_ATTN_LONG=0`` forces the reference (A/B);
read once at import.  ``models.SelfAttentionLayer`` and
``models.SeqEncoderLayer`` call this for L > 64 and ``seq_self_attn`` up to 64.
"""
import os

import torch

from persia_amd.ops import native, native_available
from persia_amd.ops.reference import seq_self_attn_reference

_ENABLED = os.environ.get("PA_SEQ_SELF_ATTN_LONG", "1") != "0"


class SeqSelfAttnLongFn(torch.autograd.Function):
    """Takes the f32 master of Wqkv and rounds it to f16 inside, so its f32
    gradient passes straight through the rounding."""

    @staticmethod
    def forward(ctx, seq, Wqkv, bqkv, heads, causal, residual):
        ctx.set_materialize_grads(False)
        seq, bqkv = seq.contiguous(), bqkv.contiguous()
        W16 = Wqkv.half().contiguous()
        out, lse = native().seq_self_attn_long_fwd(seq, W16, bqkv, heads, causal,
                                                   residual)
        ctx.save_for_backward(seq, W16, bqkv, lse)
        ctx.flags = (heads, causal, residual)
        return out

    @staticmethod
    def backward(ctx, g_out):
        if g_out is None:
            return (None,) * 6
        g_out = g_out.to(torch.float16).contiguous()
        grads = native().seq_self_attn_long_bwd(g_out, *ctx.saved_tensors,
                                                *ctx.flags)
        return (*grads, None, None, None)


def _takes_native(seq, Wqkv, bqkv, heads) -> bool:
    return (
        _ENABLED
        and seq.is_cuda
        and seq.dtype == torch.float16
        and all(p.is_cuda and p.dtype == torch.float32 for p in (Wqkv, bqkv))
        and native_available()
        and native().seq_self_attn_long_feasible(seq.shape[1], seq.shape[2] - 1,
                                                 heads)
    )


def seq_self_attn_long(seq, Wqkv, bqkv, heads, causal=False, residual=False):
    """seq [B, L, D+1] (channel D the 0/1 mask), Wqkv [3D, D], bqkv [3D] ->
    out [B, L, D+1], channel D copied."""
    if seq.dim() != 3 or seq.shape[2] < 2:
        raise ValueError(
            f"seq_self_attn_long: expected seq [B, L, D+1], got {tuple(seq.shape)}")
    D = seq.shape[2] - 1
    if heads < 1 or D % heads:
        raise ValueError(
            f"seq_self_attn_long: {heads} heads do not divide D = {D}")
    if Wqkv.shape != (3 * D, D) or bqkv.shape != (3 * D,):
        raise ValueError(
            f"seq_self_attn_long: expected Wqkv [{3 * D}, {D}] and bqkv "
            f"[{3 * D}], got {tuple(Wqkv.shape)}, {tuple(bqkv.shape)}")
    if not _takes_native(seq, Wqkv, bqkv, heads):
        return seq_self_attn_reference(seq, Wqkv, bqkv, heads, causal, residual)
    return SeqSelfAttnLongFn.apply(seq, Wqkv, bqkv, int(heads), bool(causal),
                                   bool(residual))
