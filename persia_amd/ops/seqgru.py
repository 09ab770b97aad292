"""GRU / AUGRU over a raw slot's sequence (csrc/seqgru.hip).

``seq_gru(seq, Wx, Wh, bx, bh, att=None)`` runs a GRU over the rows of the
``(B, sample_fixed_size, dim+1)`` f16 tensor of a raw slot -- parameters in
``torch.nn.GRU``'s layout, gate order (r, z, n) -- and returns every state and
the last one.  An invalid row carries the state through, so ``last`` is the
state after the last valid row whatever the mask pattern.  With ``att`` (one
weight per row) the update gate is scaled by it: DIEN's AUGRU.  On the GPU one
persistent MFMA kernel runs the recurrence and one the backward through time
(plus the ordered sum of the per-block weight-gradient partials); forward
saves the inputs and ``states`` only.

The native path is taken for an f16 CUDA ``seq`` with f32 CUDA parameters
when the extension is built and ``seq_gru_feasible(L, D, H)`` holds;
everything else runs ``ops.reference.seq_gru_reference``.  ``PA_SEQ_GRU=0``
forces the reference (A/B); read once at import.
"""
import os

import torch

from persia_amd.ops import native, native_available
from persia_amd.ops.reference import seq_gru_reference

_ENABLED = os.environ.get("PA_SEQ_GRU", "1") != "0"


class SeqGRUFn(torch.autograd.Function):
    """Takes the f32 masters of Wx and Wh and rounds them to f16 inside, so
    their f32 gradients pass straight through the rounding."""

    @staticmethod
    def forward(ctx, seq, Wx, Wh, bx, bh, att):
        ctx.set_materialize_grads(False)
        seq, bx, bh = seq.contiguous(), bx.contiguous(), bh.contiguous()
        Wx, Wh = Wx.half().contiguous(), Wh.half().contiguous()
        att = None if att is None else att.contiguous()
        states, last = native().seq_gru_fwd(seq, Wx, Wh, bx, bh, att)
        ctx.save_for_backward(seq, states, Wx, Wh, bx, bh, att)
        return states, last

    @staticmethod
    def backward(ctx, g_states, g_last):
        seq, states, Wx, Wh, bx, bh, att = ctx.saved_tensors
        g_states, g_last = (None if g is None else g.to(torch.float16).contiguous()
                            for g in (g_states, g_last))
        return tuple(native().seq_gru_bwd(g_states, g_last, seq, states, Wx, Wh,
                                          bx, bh, att))


def _takes_native(seq, Wx, Wh, bx, bh, att) -> bool:
    par = (Wx, Wh, bx, bh) + (() if att is None else (att,))
    return (
        _ENABLED
        and seq.is_cuda
        and seq.dtype == torch.float16
        and all(p.is_cuda and p.dtype == torch.float32 for p in par)
        and native_available()
        and native().seq_gru_feasible(seq.shape[1], seq.shape[2] - 1, Wh.shape[1])
    )


def seq_gru(seq, Wx, Wh, bx, bh, att=None):
    """seq [B, L, D+1] (channel D the 0/1 mask), Wx [3H, D], Wh [3H, H], bx,
    bh [3H], att [B, L] or None -> (states [B, L, H], last [B, H])."""
    if seq.dim() != 3 or seq.shape[2] < 2:
        raise ValueError(
            f"seq_gru: expected seq [B, L, D+1], got {tuple(seq.shape)}")
    (B, L, D), H = seq.shape, Wh.shape[-1]
    D -= 1
    if Wx.shape != (3 * H, D) or Wh.shape != (3 * H, H) \
            or bx.shape != (3 * H,) or bh.shape != (3 * H,):
        raise ValueError(
            f"seq_gru: expected Wx [3H, {D}], Wh [3H, H], bx and bh [3H], got "
            f"{tuple(Wx.shape)}, {tuple(Wh.shape)}, {tuple(bx.shape)}, "
            f"{tuple(bh.shape)}")
    if att is not None and att.shape != (B, L):
        raise ValueError(
            f"seq_gru: expected att [{B}, {L}], got {tuple(att.shape)}")
    if not _takes_native(seq, Wx, Wh, bx, bh, att):
        return seq_gru_reference(seq, Wx, Wh, bx, bh, att)
    return SeqGRUFn.apply(seq, Wx, Wh, bx, bh, att)
