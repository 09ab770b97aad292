"""The DCN-v2 low-rank cross tower as one autograd node (csrc/cross.hip).

``cross_stack(x0, Vs, Us, bs)`` computes, for layers l = 0..n-1 with
x_0 = x0 [B, D], V_l [r, D], U_l [D, r] and b_l [D],

    h_l     = bf16(x_l V_l^T)                     (f32 accumulate, one rounding)
    x_{l+1} = bf16(x0 * (h_l U_l^T + b_l) + x_l)  (the projection stays in f32)

and returns x_n.  The backward walks the layers last to first on
``cross_bwd_dh`` / ``cross_bwd_dx``, recomputes the projection instead of
saving it, and takes dU_l / dV_l from the dense tower's wgrad kernels
(``ops.dense._wgrad``: ``_sideband_grad`` slots and the weight dtype are
honoured exactly as by ``FusedLinearFn``).

The native path is taken for a contiguous bf16 CUDA ``x0`` with CUDA
parameters when the extension is built and ``cross_feasible(D, r)`` holds
(D % 32 == 0, r % 32 == 0, 32 <= r <= 256; any B); everything else runs
``ops.reference.cross_stack_reference``.  ``PA_CROSS_STACK=0`` forces the
reference (A/B); read once at import.
"""
import os

import torch

from persia_amd.ops import native, native_available
from persia_amd.ops.dense import _wgrad
from persia_amd.ops.reference import cross_stack_reference

_ENABLED = os.environ.get("PA_CROSS_STACK", "1") != "0"


class CrossStackFn(torch.autograd.Function):
    """``apply(x0, n, V_0.., U_0.., b_0..)``.  Takes the master weights and
    rounds them to bf16 inside (per call, as FusedLinearFn does), so their
    gradients pass straight through the rounding.  Saves x_l and the bf16 h_l
    of every layer: a layer's output is the next layer's input."""

    @staticmethod
    def forward(ctx, x0, n, *params):
        C = native()
        Vs, Us, bs = params[:n], params[n:2 * n], params[2 * n:]
        V_bf = [v.to(torch.bfloat16).contiguous() for v in Vs]
        U_bf = [u.to(torch.bfloat16).contiguous() for u in Us]
        b_f = [b.float().contiguous() for b in bs]
        xs, hs = [x0], []
        for V, U, b in zip(V_bf, U_bf, b_f):
            out, h = C.cross_fwd(x0, xs[-1], V, U, b)
            xs.append(out)
            hs.append(h)
        ctx.save_for_backward(*xs[:-1], *hs, *V_bf, *U_bf, *b_f)
        ctx.n = n
        ctx.w_dtypes = [p.dtype for p in params]
        ctx.sides = [getattr(p, "_sideband_grad", None) for p in params]
        return xs[-1]

    @staticmethod
    def backward(ctx, g):
        C = native()
        n, t = ctx.n, ctx.saved_tensors
        xs, hs, V_bf, U_bf, b_f = (t[i * n:(i + 1) * n] for i in range(5))
        x0 = xs[0]
        r, D = V_bf[0].shape
        g = g.to(torch.bfloat16).contiguous()
        grads = [None] * (3 * n)
        dx0 = torch.empty(0, dtype=torch.bfloat16, device=g.device)
        for l in range(n - 1, -1, -1):
            # the NT kernels take K-contiguous operands: U^T for dp U and
            # V^T for dh V, made here from the bf16 images
            dp, dh, part = C.cross_bwd_dh(g, x0, U_bf[l].t().contiguous())
            b_side = ctx.sides[2 * n + l]
            if b_side is not None:
                C.cross_db_reduce_into(part, b_side)
            else:
                grads[2 * n + l] = C.cross_db_reduce(part).to(
                    ctx.w_dtypes[2 * n + l])
            grads[n + l] = _wgrad(C, dp, hs[l], ctx.sides[n + l],
                                  ctx.w_dtypes[n + l], r)
            grads[l] = _wgrad(C, dh, xs[l], ctx.sides[l], ctx.w_dtypes[l], D)
            g, dx0 = C.cross_bwd_dx(g, dh, hs[l], V_bf[l].t().contiguous(),
                                    U_bf[l], b_f[l], dx0, l == 0)
        return (dx0 if ctx.needs_input_grad[0] else None, None, *grads)


def _takes_native(x0, Vs, Us, bs) -> bool:
    return (
        _ENABLED
        and x0.is_cuda and x0.dtype == torch.bfloat16 and x0.is_contiguous()
        and all(p.is_cuda for p in (*Vs, *Us, *bs))
        and native_available()
        and native().cross_feasible(x0.shape[1], Vs[0].shape[0])
    )


def cross_stack(x0, Vs, Us, bs):
    """x0 [B, D], Vs n x [r, D], Us n x [D, r], bs n x [D] -> x_n [B, D]."""
    Vs, Us, bs = tuple(Vs), tuple(Us), tuple(bs)
    n = len(Vs)
    if x0.dim() != 2 or n < 1 or len(Us) != n or len(bs) != n:
        raise ValueError(
            f"cross_stack: expected x0 [B, D] and n >= 1 of each of V, U, b, "
            f"got {tuple(x0.shape)} and {n}, {len(Us)}, {len(bs)}")
    D = x0.shape[1]
    r = Vs[0].shape[0] if Vs[0].dim() == 2 else -1
    if r < 1 or any(tuple(V.shape) != (r, D) or tuple(U.shape) != (D, r)
                    or tuple(b.shape) != (D,) for V, U, b in zip(Vs, Us, bs)):
        raise ValueError(
            f"cross_stack: expected V [r, D], U [D, r], b [D] with D = {D}, got "
            f"{[tuple(p.shape) for p in (*Vs, *Us, *bs)]}")
    if not _takes_native(x0, Vs, Us, bs):
        # f32 master biases beside bf16 weights: the reference runs in x0's dtype
        Vs, Us, bs = ([p.to(x0.dtype) for p in ps] for ps in (Vs, Us, bs))
        return cross_stack_reference(x0, Vs, Us, bs)
    return CrossStackFn.apply(x0, n, *Vs, *Us, *bs)
