"""Fused dense layers over the CDNA4 MFMA kernels (csrc/dense.hip).

``FusedLinear`` = bf16 GEMM + bias + ReLU in ONE kernel (forward), with
hand-written dgrad / wgrad / bias-grad kernels in backward — replacing a
hipBLASLt GEMM plus an elementwise cascade per layer.  f32 master weights,
bf16 activations (the bench's dtype contract).  Since the XOR-swizzled LDS
staging fix (wgrad 113 -> 252 TF) this path BEATS the graphed hipBLASLt
dense step end-to-end and is the bench default for dim-128 towers.
``FusedMLP`` runs consecutive layers as one backward chain (``FusedChainFn``)
so the ReLU backward and the bias gradient ride in the dgrad GEMM epilogue.

Constraints (asserted): hidden widths N % 32 == 0 (dgrad reuses the GEMM
kernel with K=N); input features are zero-padded to a multiple of 32.
"""
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F


def _wgrad_via_blas() -> bool:
    # default: the hand-written wgrad (XOR-swizzled LDS staging) — it beats
    # hipBLASLt 2-4x on the DLRM shapes; "blas" kept as an A/B switch
    import os

    return os.environ.get("PA_FUSED_WGRAD", "own") == "blas"


def _pad32(x: torch.Tensor, dim: int, mult: int = 128) -> torch.Tensor:
    """Zero-pad dim to a multiple of `mult` (the glds-pipelined GEMM v2
    needs K % 64 and the tr-read wgrad K % 128; zero K-columns are inert —
    the extra flops are cheaper than falling off the v2 kernels)."""
    k = x.shape[dim]
    pad = (-k) % mult
    if pad == 0:
        return x
    padding = [0, 0] * (x.dim() - 1 - dim) + [0, pad]
    return F.pad(x, padding)


def _fused_drelu() -> bool:
    # default: consecutive FusedLinear layers of a FusedMLP run as ONE
    # backward chain whose dgrad GEMMs apply the producer's ReLU mask and
    # column-sum its bias gradient in their epilogue; "0" keeps the
    # per-layer path (relu_bwd_bias pass per layer) as an A/B switch
    import os

    return os.environ.get("PA_FUSED_DRELU", "1") != "0"


def _own_bias_grad(C, g, out, act, b_side, b_dtype):
    """ReLU mask + bias gradient of a layer whose incoming gradient is NOT
    already masked (standalone layer / last layer of a chain).
    -> (masked g, db or None when accumulated into the side-band slot)."""
    N = g.shape[1]
    pow2 = N >= 8 and (N & (N - 1)) == 0
    if act == 1 and pow2 and b_side is not None:
        # one fused pass: relu mask + bias column sums straight into the
        # side-band slot (saves re-reading the 16 MB masked gradient)
        return C.relu_bwd_bias(g, out, b_side), None
    if act == 1:
        g = C.relu_bwd(g, out)
    if b_side is not None:
        C.bias_grad_into(g, b_side)
        return g, None
    db = C.bias_grad(g)
    if db.dtype != b_dtype:
        db = db.to(b_dtype)
    return g, db


def _dgrad(C, g, w_bf, mask=None, db=None, n_bias=0):
    """dX = g @ W (full padded width).  With `mask` (the ReLU output that
    produced this layer's input, padded like dX) the GEMM epilogue also
    applies the ReLU backward and accumulates the masked gradient's column
    sums into db[:n_bias]."""
    # trans_b path consumes the [N, Kp] weight directly; at the big square
    # shape the transposed-staging kernel loses to an explicit W^T + the
    # glds NT path (51 vs 33+8 us measured, tools/dgrad_probe.py)
    if w_bf.shape[0] >= 1024 and w_bf.shape[1] >= 1024:
        w_op, trans_b = w_bf.t().contiguous(), 0
    else:
        w_op, trans_b = w_bf, 1
    if mask is None:
        return C.gemm_nt_bias_act(
            g, w_op, torch.empty(0, device=g.device), 0, 0, trans_b
        )
    return C.dgrad_drelu_bias(g, w_op, trans_b, mask, db, n_bias)


def _wgrad(C, g, x_bf, w_side, w_dtype, kw):
    """-> dw, or None when accumulated into the side-band slot."""
    if w_side is not None:
        C.wgrad_into(g, x_bf, w_side)
        return None
    if _wgrad_via_blas():
        # hybrid: the hand-written fwd/dgrad kernels beat hipBLASLt on
        # these shapes but the wgrad kernel trails it (transpose-staging
        # bound) — let the library run the one GEMM it wins
        dw = torch.matmul(g.t(), x_bf).to(w_dtype)
    else:
        dw = C.wgrad(g, x_bf)
        if dw.dtype != w_dtype:
            dw = dw.to(w_dtype)
    if dw.shape[1] != kw:
        dw = dw[:, :kw].contiguous()
    return dw


class FusedLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act: int):
        from persia_amd.ops import native

        C = native()
        x_bf = _pad32(x.to(torch.bfloat16), 1).contiguous()
        w_bf = _pad32(weight.to(torch.bfloat16), 1).contiguous()  # [N, Kp]
        out = C.gemm_nt_bias_act(x_bf, w_bf, bias.float(), act, 0, 0)
        ctx.save_for_backward(x_bf, w_bf, out)
        ctx.act = act
        ctx.k = x.shape[1]       # dx width (input may arrive pre-padded)
        ctx.kw = weight.shape[1]  # dw width (the stored, unpadded weight)
        ctx.w_dtype = weight.dtype
        ctx.b_dtype = bias.dtype
        # side-band gradient targets (set by the bench's flat-buffer scheme):
        # when present, backward ACCUMULATES dw/db straight into these f32
        # slots via atomics and returns None — no dw materialization, cast,
        # pad-slice or AccumulateGrad add per layer
        ctx.w_side = getattr(weight, "_sideband_grad", None)
        ctx.b_side = getattr(bias, "_sideband_grad", None)
        return out

    @staticmethod
    def backward(ctx, g):
        from persia_amd.ops import native

        C = native()
        x_bf, w_bf, out = ctx.saved_tensors
        g = g.to(torch.bfloat16).contiguous()
        g, db = _own_bias_grad(C, g, out, ctx.act, ctx.b_side, ctx.b_dtype)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _dgrad(C, g, w_bf)
            if dx.shape[1] != ctx.k:
                dx = dx[:, : ctx.k]
        dw = _wgrad(C, g, x_bf, ctx.w_side, ctx.w_dtype, ctx.kw)
        return dx, dw, db, None


class FusedChainFn(torch.autograd.Function):
    """A run of consecutive FusedLinear layers as one autograd node:
    ``apply(x, acts, w0, b0, w1, b1, ...)``.  Forward is the per-layer
    forward.  Backward walks the layers last to first; the dgrad GEMM of
    layer i+1 applies layer i's ReLU mask (layer i+1's saved input IS layer
    i's output) and accumulates layer i's bias gradient in its epilogue, so
    only the last layer of the run pays a separate mask + column-sum pass."""

    @staticmethod
    def forward(ctx, x, acts, *params):
        from persia_amd.ops import native

        C = native()
        weights, biases = params[0::2], params[1::2]
        saved, widths = [], []
        h = x
        for w, b, act in zip(weights, biases, acts):
            x_bf = _pad32(h.to(torch.bfloat16), 1).contiguous()
            w_bf = _pad32(w.to(torch.bfloat16), 1).contiguous()  # [N, Kp]
            widths.append(h.shape[1])  # dx width (x may arrive pre-padded)
            h = C.gemm_nt_bias_act(x_bf, w_bf, b.float(), act, 0, 0)
            saved += [x_bf, w_bf]
        ctx.save_for_backward(*saved, h)
        ctx.acts = tuple(acts)
        ctx.widths = widths
        ctx.kws = [w.shape[1] for w in weights]
        ctx.w_dtypes = [w.dtype for w in weights]
        ctx.b_dtypes = [b.dtype for b in biases]
        # side-band gradient targets, as in FusedLinearFn
        ctx.w_sides = [getattr(w, "_sideband_grad", None) for w in weights]
        ctx.b_sides = [getattr(b, "_sideband_grad", None) for b in biases]
        return h

    @staticmethod
    def backward(ctx, g):
        from persia_amd.ops import native

        C = native()
        *saved, out = ctx.saved_tensors
        L = len(ctx.acts)
        g = g.to(torch.bfloat16).contiguous()
        grads = [None] * (2 * L)
        dx = None
        g, grads[2 * L - 1] = _own_bias_grad(
            C, g, out, ctx.acts[-1], ctx.b_sides[-1], ctx.b_dtypes[-1]
        )
        for i in range(L - 1, -1, -1):
            x_bf, w_bf = saved[2 * i], saved[2 * i + 1]
            dx = None
            if i > 0 and ctx.acts[i - 1] == 1:
                # fused: layer i-1 gets its gradient masked, and its bias
                # gradient accumulated (slot: added to, never zeroed here)
                n_prev = ctx.widths[i]
                db = ctx.b_sides[i - 1]
                fresh = db is None
                if fresh:
                    db = torch.zeros(n_prev, dtype=torch.float32,
                                     device=g.device)
                dx = _dgrad(C, g, w_bf, mask=x_bf, db=db, n_bias=n_prev)
                if fresh:
                    if db.dtype != ctx.b_dtypes[i - 1]:
                        db = db.to(ctx.b_dtypes[i - 1])
                    grads[2 * i - 1] = db
            elif i > 0 or ctx.needs_input_grad[0]:
                dx = _dgrad(C, g, w_bf)
            grads[2 * i] = _wgrad(C, g, x_bf, ctx.w_sides[i], ctx.w_dtypes[i],
                                  ctx.kws[i])
            if dx is not None and dx.shape[1] != ctx.widths[i]:
                dx = dx[:, : ctx.widths[i]]
            if i > 0:
                g = dx.contiguous()
                if ctx.acts[i - 1] != 1:
                    g, grads[2 * i - 1] = _own_bias_grad(
                        C, g, x_bf, 0, ctx.b_sides[i - 1], ctx.b_dtypes[i - 1]
                    )
        return (dx, None, *grads)


class FusedLinear(nn.Module):
    def __init__(self, in_features: int, out_features: int, relu: bool = True,
                 bias: bool = True):
        super().__init__()
        assert out_features % 32 == 0, "FusedLinear needs out_features % 32 == 0"
        self.in_features = in_features
        self.out_features = out_features
        self.relu = relu
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_features))
        else:  # constant zero bias: buffer, so parameter lists align with
            # a bias-free nn.Linear twin
            self.register_buffer("bias", torch.zeros(out_features))
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)

    def _apply(self, fn, recurse=True):
        # keep the bias fp32 through .bfloat16()/.half(): the GEMM epilogue
        # adds it in f32 and bias_grad produces f32 — a low-precision bias
        # only inserts per-step cast kernels on BOTH passes (the profile
        # showed ~24 bias-sized launches/step from exactly this)
        r = super()._apply(fn, recurse)
        if self.bias.dtype != torch.float32:
            if isinstance(self.bias, nn.Parameter):
                self.bias.data = self.bias.data.float()
                if self.bias.grad is not None:
                    self.bias.grad = self.bias.grad.float()
            else:
                self.bias = self.bias.float()
        return r

    def forward(self, x):
        return FusedLinearFn.apply(x, self.weight, self.bias, 1 if self.relu else 0)


class FusedMLP(nn.Module):
    """Stack of FusedLinear layers (+ optional plain final projection when the
    last width isn't a multiple of 32, e.g. the 1-logit head)."""

    def __init__(self, sizes: List[int], last_relu: bool = False):
        super().__init__()
        layers: List[nn.Module] = []
        for i in range(len(sizes) - 1):
            is_last = i == len(sizes) - 2
            relu = (not is_last) or last_relu
            if sizes[i + 1] % 32 == 0:
                layers.append(FusedLinear(sizes[i], sizes[i + 1], relu=relu))
            else:
                lin = nn.Linear(sizes[i], sizes[i + 1])
                layers.append(lin if not relu else nn.Sequential(lin, nn.ReLU()))
        self.layers = nn.ModuleList(layers)

    def forward(self, x):
        layers = list(self.layers)
        fuse = _fused_drelu()
        i = 0
        while i < len(layers):
            l = layers[i]
            if isinstance(l, FusedLinear):
                # maximal run of consecutive FusedLinear layers
                j = i + 1
                while fuse and j < len(layers) and isinstance(layers[j], FusedLinear):
                    j += 1
                if j - i > 1:
                    run = layers[i:j]
                    params = [p for m in run for p in (m.weight, m.bias)]
                    acts = tuple(1 if m.relu else 0 for m in run)
                    x = FusedChainFn.apply(x, acts, *params)
                else:
                    x = l(x)
                i = j
                continue
            # plain final projection (e.g. the 1-logit head): follow its
            # weight dtype — FusedLinear outputs bf16 even when the
            # module holds f32 weights (mixed-precision user models)
            w = next(l.parameters(), None)
            if w is not None and x.dtype != w.dtype:
                x = x.to(w.dtype)
            x = l(x)
            i += 1
        return x


class FusedBCEFn(torch.autograd.Function):
    """BCE-with-logits as 2 kernels (fwd: loss + sigmoid cache, bwd: one
    elementwise) — torch's chain is ~10 launch-bound kernels inside the
    captured step."""

    @staticmethod
    def forward(ctx, logits, label):
        from persia_amd.ops import native

        C = native()
        loss, sig = C.bce_fwd(logits.float().contiguous(),
                              label.float().contiguous())
        ctx.save_for_backward(sig, label)
        ctx.in_dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        from persia_amd.ops import native

        C = native()
        sig, label = ctx.saved_tensors
        dz = C.bce_bwd(sig, label.float(), g.reshape(1).float().contiguous())
        if dz.dtype != ctx.in_dtype:
            dz = dz.to(ctx.in_dtype)
        return dz, None


def fused_bce_with_logits(logits: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
    return FusedBCEFn.apply(logits, label)
