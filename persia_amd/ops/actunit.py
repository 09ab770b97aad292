"""DIN activation-unit (MLP attention) pooling over a raw slot
(csrc/actunit.hip).

``act_unit_pool(q, seq, W1, b1, w2, b2)`` scores every row of the ``(B,
sample_fixed_size, dim+1)`` f16 tensor of a raw slot with a one-hidden-layer
MLP over ``[q, k, q-k, q*k]`` and sums the valid rows with the scores as
weights (no softmax).  On the GPU the first layer is folded into a per-sample
matrix ``M_b = (Wk-Wd) + Wp * q_b`` and a per-sample bias ``u_b = (Wq+Wd) q_b
+ b1``: torch computes ``u`` (one addmm, autograd handles it), one HIP kernel
does everything else in forward and one in backward (plus the ordered sum of
the per-block weight-gradient partials).  Nothing but the inputs is saved.

The native path is taken for f16 CUDA ``q`` and ``seq`` with f32 CUDA
parameters when the extension is built and ``act_unit_feasible(L, D, H)``
holds; everything else runs ``ops.reference.act_unit_pool_reference``.
``PA_ACT_UNIT=0`` forces the reference (A/B); read once at import.
"""
import os

import torch

from persia_amd.ops import native, native_available
from persia_amd.ops.reference import act_unit_pool_reference

_ENABLED = os.environ.get("PA_ACT_UNIT", "1") != "0"


class ActUnitPoolFn(torch.autograd.Function):
    """Takes the f32 masters of Wb = Wk-Wd and Wp and rounds them to f16
    inside, so their f32 gradients pass straight through the rounding."""

    @staticmethod
    def forward(ctx, q, seq, u, Wb, Wp, w2, b2):
        q, seq, u, w2 = (t.contiguous() for t in (q, seq, u, w2))
        Wb, Wp = Wb.half().contiguous(), Wp.half().contiguous()
        out = native().act_unit_fwd(q, seq, u, Wb, Wp, w2, b2)
        ctx.save_for_backward(q, seq, u, Wb, Wp, w2, b2)
        return out

    @staticmethod
    def backward(ctx, g):
        q, seq, u, Wb, Wp, w2, b2 = ctx.saved_tensors
        g = g.to(torch.float16).contiguous()
        return tuple(native().act_unit_bwd(g, q, seq, u, Wb, Wp, w2, b2))


def _takes_native(q, seq, W1, b1, w2, b2) -> bool:
    return (
        _ENABLED
        and q.is_cuda
        and seq.is_cuda
        and q.dtype == torch.float16
        and seq.dtype == torch.float16
        and all(p.is_cuda and p.dtype == torch.float32 for p in (W1, b1, w2, b2))
        and native_available()
        and native().act_unit_feasible(seq.shape[1], q.shape[1], W1.shape[0])
    )


def act_unit_pool(
    q: torch.Tensor,
    seq: torch.Tensor,
    W1: torch.Tensor,
    b1: torch.Tensor,
    w2: torch.Tensor,
    b2: torch.Tensor,
) -> torch.Tensor:
    """q [B, D], seq [B, L, D+1] (channel D the 0/1 mask), W1 [H, 4D] (column
    blocks Wq | Wk | Wd | Wp), b1 [H], w2 [H], b2 [] -> [B, D]."""
    if q.dim() != 2 or seq.dim() != 3 or seq.shape[0] != q.shape[0] \
            or seq.shape[2] != q.shape[1] + 1:
        raise ValueError(
            f"act_unit_pool: expected q [B, D] and seq [B, L, D+1], got "
            f"{tuple(q.shape)} and {tuple(seq.shape)}"
        )
    D, H = q.shape[1], W1.shape[0]
    if W1.shape != (H, 4 * D) or b1.shape != (H,) or w2.shape != (H,) \
            or b2.numel() != 1:
        raise ValueError(
            f"act_unit_pool: expected W1 [H, {4 * D}], b1 [H], w2 [H], b2 [], "
            f"got {tuple(W1.shape)}, {tuple(b1.shape)}, {tuple(w2.shape)}, "
            f"{tuple(b2.shape)}"
        )
    if not _takes_native(q, seq, W1, b1, w2, b2):
        return act_unit_pool_reference(q, seq, W1, b1, w2, b2)
    Wq, Wk, Wd, Wp = (W1[:, i * D:(i + 1) * D] for i in range(4))
    u = torch.addmm(b1, q.float(), (Wq + Wd).t())
    return ActUnitPoolFn.apply(q, seq, u, Wk - Wd, Wp, w2, b2.reshape(()))
