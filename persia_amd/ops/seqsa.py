"""Multi-head self-attention among the rows of a raw slot (csrc/seqsa.hip).

``seq_self_attn(seq, Wqkv, bqkv, heads, causal=False, residual=False)`` lets
every valid row of the ``(B, sample_fixed_size, dim+1)`` f16 tensor of a raw
slot attend to the valid rows of its sample (``causal``: to those not after
it) -- the Behavior Sequence Transformer's layer, or SASRec's with the causal
mask -- and returns a tensor of the same layout, mask channel included, so the
pooling kernels consume it unchanged.  Parameters are in
``torch.nn.MultiheadAttention``'s ``in_proj_weight`` / ``in_proj_bias``
layout.  On the GPU one persistent MFMA kernel projects the rows, computes
``QK^T``, selects by the mask, runs the softmax and ``PV`` per sample without
touching global memory in between, and one kernel runs the backward (plus the
ordered sum of the per-block weight-gradient partials); forward saves the
inputs only.

The native path is taken for an f16 CUDA ``seq`` with f32 CUDA parameters
when the extension is built and ``seq_self_attn_feasible(L, D, heads)`` holds
(D in {32, 64}, D / heads in {16, 32}, L <= 64); everything else runs
``ops.reference.seq_self_attn_reference``.  ``PA_SEQ_SELF_ATTN=0`` forces the
reference (A/B); read once at import.
"""
import os

import torch

from persia_amd.ops import native, native_available
from persia_amd.ops.reference import seq_self_attn_reference

_ENABLED = os.environ.get("PA_SEQ_SELF_ATTN", "1") != "0"


class SeqSelfAttnFn(torch.autograd.Function):
    """Takes the f32 master of Wqkv and rounds it to f16 inside, so its f32
    gradient passes straight through the rounding."""

    @staticmethod
    def forward(ctx, seq, Wqkv, bqkv, heads, causal, residual):
        ctx.set_materialize_grads(False)
        seq, bqkv = seq.contiguous(), bqkv.contiguous()
        W16 = Wqkv.half().contiguous()
        ctx.save_for_backward(seq, W16, bqkv)
        ctx.flags = (heads, causal, residual)
        return native().seq_self_attn_fwd(seq, W16, bqkv, heads, causal, residual)

    @staticmethod
    def backward(ctx, g_out):
        if g_out is None:
            return (None,) * 6
        g_out = g_out.to(torch.float16).contiguous()
        grads = native().seq_self_attn_bwd(g_out, *ctx.saved_tensors, *ctx.flags)
        return (*grads, None, None, None)


def _takes_native(seq, Wqkv, bqkv, heads) -> bool:
    return (
        _ENABLED
        and seq.is_cuda
        and seq.dtype == torch.float16
        and all(p.is_cuda and p.dtype == torch.float32 for p in (Wqkv, bqkv))
        and native_available()
        and native().seq_self_attn_feasible(seq.shape[1], seq.shape[2] - 1, heads)
    )


def seq_self_attn(seq, Wqkv, bqkv, heads, causal=False, residual=False):
    """seq [B, L, D+1] (channel D the 0/1 mask), Wqkv [3D, D], bqkv [3D] ->
    out [B, L, D+1], channel D copied."""
    if seq.dim() != 3 or seq.shape[2] < 2:
        raise ValueError(
            f"seq_self_attn: expected seq [B, L, D+1], got {tuple(seq.shape)}")
    D = seq.shape[2] - 1
    if heads < 1 or D % heads:
        raise ValueError(f"seq_self_attn: {heads} heads do not divide D = {D}")
    if Wqkv.shape != (3 * D, D) or bqkv.shape != (3 * D,):
        raise ValueError(
            f"seq_self_attn: expected Wqkv [{3 * D}, {D}] and bqkv [{3 * D}], "
            f"got {tuple(Wqkv.shape)}, {tuple(bqkv.shape)}")
    if not _takes_native(seq, Wqkv, bqkv, heads):
        return seq_self_attn_reference(seq, Wqkv, bqkv, heads, causal, residual)
    return SeqSelfAttnFn.apply(seq, Wqkv, bqkv, int(heads), bool(causal),
                               bool(residual))
