"""The fused DCN-v2 cross stack (ops.cross.cross_stack, csrc/cross.hip): the
cases, operands and f64 / rounded-as-the-kernels models shared with
tests/test_gpu_cross_exact.py, and the CPU side of the op."""
import functools

import pytest
import torch

from persia_amd.models.dcn import CrossLayerV2, DCNv2
from persia_amd.ops import cross_stack, cross_stack_reference

# (B, D, r, layers)
CASES = [
    (1, 32, 32, 1),       # one row, one K step
    (129, 96, 32, 2),     # row tail of 1, odd K-step count, chained layers
    (65, 224, 96, 2),     # a rank that is no power of two nor a multiple of 64
    (200, 160, 64, 3),    # three layers: dx0 accumulates, layer 0 folds g in
    (70, 1696, 256, 2),   # the benchmark's width (53 x 32), the maximum rank
]
IDS = ["x".join(map(str, c)) for c in CASES]


def make_operands(case, device="cpu"):
    """-> x0, g (bf16 [B, D]), Vs, Us, bs (f32 masters, about 1/sqrt(fan-in),
    so values stay O(1) through three layers)."""
    B, D, r, n = case
    gen = torch.Generator().manual_seed(((B * 1009 + D) * 1009 + r) * 1009 + n)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    x0, g = rn(B, D).bfloat16(), rn(B, D).bfloat16()
    Vs = [rn(r, D) / D ** 0.5 for _ in range(n)]
    Us = [rn(D, r) / r ** 0.5 for _ in range(n)]
    bs = [rn(D) / r ** 0.5 for _ in range(n)]
    return tuple(t.to(device) if torch.is_tensor(t) else [p.to(device) for p in t]
                 for t in (x0, g, Vs, Us, bs))


def names(case):
    return ["out", "dx0"] + [f"d{p}{l}" for l in range(case[3]) for p in "VUb"]


@functools.lru_cache(maxsize=None)
def reference(case, dtype, round_as_kernel=False):
    """Forward and every gradient in `dtype` from the operands' bits (the
    weights' bf16 images are part of the op).  round_as_kernel rounds to bf16
    where the kernels do: h, dp, dh, each layer's output, g_l and dx0."""
    x0, g, Vs, Us, bs = make_operands(case)
    n = case[3]
    rnd = (lambda t: t.bfloat16().to(dtype)) if round_as_kernel else (lambda t: t)
    x0, g = x0.to(dtype), g.to(dtype)
    Vs, Us = ([w.bfloat16().to(dtype) for w in ws] for ws in (Vs, Us))
    bs = [b.to(dtype) for b in bs]
    xs, hs = [x0], []
    for V, U, b in zip(Vs, Us, bs):
        hs.append(rnd(xs[-1] @ V.t()))
        xs.append(rnd(x0 * (hs[-1] @ U.t() + b) + xs[-1]))
    res, dx0 = {"out": xs[-1]}, 0
    for l in range(n - 1, -1, -1):
        dp = rnd(g * x0)
        dh = rnd(dp @ Us[l])
        res[f"db{l}"], res[f"dU{l}"] = dp.sum(0), dp.t() @ hs[l]
        res[f"dV{l}"] = dh.t() @ xs[l]
        gl = g + dh @ Vs[l]
        t = dx0 + g * (hs[l] @ Us[l].t() + bs[l])
        dx0 = rnd(t + gl) if l == 0 else rnd(t)
        g = rnd(gl)
    res["dx0"] = dx0
    return res


@functools.lru_cache(maxsize=None)
def E(case):
    """max |f32 rounded as the kernels - f64| per result."""
    lo, hi = reference(case, torch.float32, True), reference(case, torch.float64)
    return {k: (lo[k].double() - hi[k]).abs().max().item() for k in hi}


def _autograd(fn, case):
    x0, g, Vs, Us, bs = make_operands(case)
    x0 = x0.double().requires_grad_(True)
    Vs, Us = ([w.bfloat16().double().requires_grad_(True) for w in ws]
              for ws in (Vs, Us))
    bs = [b.double().requires_grad_(True) for b in bs]
    out = fn(x0, Vs, Us, bs)
    out.backward(g.double())
    res = {"out": out.detach(), "dx0": x0.grad}
    for l, (V, U, b) in enumerate(zip(Vs, Us, bs)):
        res.update({f"dV{l}": V.grad, f"dU{l}": U.grad, f"db{l}": b.grad})
    return res


def _layer_stack(x0, Vs, Us, bs):
    xl = x0
    for V, U, b in zip(Vs, Us, bs):
        layer = CrossLayerV2(V.shape[1], rank=V.shape[0])  # on nn.Linear
        xl = torch.func.functional_call(
            layer, {"v.weight": V, "u.weight": U, "u.bias": b}, (x0, xl))
    return xl


# r < D: CrossLayerV2 keeps the low-rank form
@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_reference_is_the_layer_stack_in_f64(case):
    want = _autograd(_layer_stack, case)
    for got in (_autograd(cross_stack_reference, case),
                reference(case, torch.float64)):
        for k in names(case):
            err = (got[k] - want[k]).abs().max().item()
            assert err <= 1e-12 * want[k].abs().max().item(), (k, err)


def test_cross_stack_on_cpu_is_the_reference():
    x0, g, Vs, Us, bs = make_operands(CASES[1])
    x0 = x0.float()
    out = cross_stack(x0.clone().requires_grad_(True), Vs, Us, bs)
    assert type(out.grad_fn).__name__ != "CrossStackFnBackward"
    assert torch.equal(out, cross_stack_reference(x0, Vs, Us, bs))
    with pytest.raises(ValueError):
        cross_stack(x0, Vs, Us[:1], bs)
    with pytest.raises(ValueError):
        cross_stack(x0, Vs, [U[:, :16] for U in Us], bs)


def test_fused_cross_needs_fused_low_rank():
    kw = dict(num_sparse=3, num_dense=13, dim=32, num_cross=2, deep=(64, 32))
    with pytest.raises(AssertionError):
        DCNv2(cross_rank=32, fused=False, fused_cross=True, **kw)
    with pytest.raises(AssertionError):
        DCNv2(cross_rank=0, fused=True, fused_cross=True, **kw)
    assert DCNv2(cross_rank=32, fused=True, fused_cross=True, **kw).fused_cross
