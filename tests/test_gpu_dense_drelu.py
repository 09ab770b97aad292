"""dReLU + bias-grad fused into the dgrad GEMM epilogue, and FusedMLP's
backward chain built on it.

Everything is compared against the UNFUSED composition of the existing ops
(plain dgrad GEMM -> relu_bwd -> column sum), not against an f32 torch
reference: the two must agree bit for bit on dx, and differ on the f32
atomically-accumulated sums only by summation order.

Reordering bound used throughout: a sum of n f32 addends a_m accumulated in
any order is within n * 2^-24 * sum|a_m| of the exact sum (each of the n-1
roundings is at most 2^-24 relative to a partial sum, itself bounded by
sum|a_m|).  The exact sum is taken in f64 from the same bf16 operands.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _dev():
    return torch.device("cuda", 0)


def _native():
    from persia_amd.ops import native

    return native()


# --------------------------------------------------------------- kernel level
# (id, M, K, N, n_bias, trans_b, expected dispatch).  M, K, N are the
# gemm_nt_bias_act GEMM dimensions: g [M, K], output / mask [M, N].  One
# shape per launcher branch, as small as the branch allows:
#   v1 64x32:  K % 64 != 0 and < 192 128-wide tiles
#   v1 64x64:  K % 64 == 0 and N % 64 == 0 (trans_b, or too few tiles for glds)
#   v1 128x32: K % 64 != 0 and >= 192 tiles (97 m-tiles x 2)
#   glds 128:  trans_b == 0, K >= 256, N % 128 == 0, >= 400 tiles (51 x 8)
#   glds 64:   trans_b == 0, K >= 256, N % 128 != 0, >= 400 64-wide tiles
KERNEL_CASES = [
    ("v1t_64x32", 200, 96, 128, 96, 1, "v1:64x32"),
    ("v1t_64x64", 200, 256, 128, 128, 1, "v1:64x64"),
    ("v1t_128x32", 12328, 96, 256, 256, 1, "v1:128x32"),
    ("glds128_wt", 6472, 1024, 1024, 1024, 0, "glds:128"),
    ("glds64", 17100, 256, 192, 192, 0, "glds:64"),
    # the same v1 tile configs with the operand in [N, K] layout
    ("v1n_64x32", 200, 96, 128, 96, 0, "v1:64x32"),
    ("v1n_64x64", 200, 256, 128, 128, 0, "v1:64x64"),
    ("v1n_128x32", 12328, 96, 256, 256, 0, "v1:128x32"),
]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_dgrad_drelu_bias_matches_unfused(case):
    _, M, K, N, n_bias, trans_b, expect = case
    C = _native()
    assert C.gemm_nt_config(M, N, K, trans_b) == expect
    gen = torch.Generator(device=_dev()).manual_seed(1234 + M + K)
    # asymmetric random operands
    g = (torch.randn(M, K, device=_dev(), generator=gen) * 0.5).to(torch.bfloat16)
    W = (torch.randn(K, N, device=_dev(), generator=gen) * 0.25 + 0.05).to(
        torch.bfloat16)  # the layer weight: [K, N] is the trans_b operand
    W_op = W.contiguous() if trans_b else W.t().contiguous()
    # a ReLU output: >= 0, about half zeros, one dead and one all-live column
    mask = torch.relu(torch.randn(M, N, device=_dev(), generator=gen))
    mask[:, 0] = 0.0
    mask[:, 1] = mask[:, 1].abs() + 0.125
    mask = mask.to(torch.bfloat16).contiguous()
    assert (mask[:, 1] > 0).all() and 0.3 < (mask == 0).float().mean() < 0.7

    empty = torch.empty(0, device=_dev())
    dx_ref = C.relu_bwd(C.gemm_nt_bias_act(g, W_op, empty, 0, 0, trans_b), mask)
    db_ref = dx_ref[:, :n_bias].double().sum(0)
    bound = M * U * dx_ref[:, :n_bias].double().abs().sum(0)

    # db is as wide as the output; only [:n_bias] may be written
    db = torch.zeros(N, dtype=torch.float32, device=_dev())
    dx = C.dgrad_drelu_bias(g, W_op, trans_b, mask, db, n_bias)
    assert torch.equal(dx, dx_ref)
    err = (db[:n_bias].double() - db_ref).abs()
    print(f"db max err {err.max().item():.3e}, min slack "
          f"{(bound - err).min().item():.3e}")
    assert (err <= bound).all()
    assert db[0].item() == 0.0  # dead column
    assert (db[n_bias:] == 0).all()

    # accumulates: a second call into the same db doubles it (2M addends)
    dx2 = C.dgrad_drelu_bias(g, W_op, trans_b, mask, db, n_bias)
    assert torch.equal(dx2, dx_ref)
    err2 = (db[:n_bias].double() - 2 * db_ref).abs()
    assert (err2 <= 4 * bound).all()  # n and sum|a| both double
    assert (db[n_bias:] == 0).all()


# ---------------------------------------------------------------- stack level
STACKS = {
    "odd": ([40, 96, 256, 64], 200),       # padded width 96, M tail
    "wide": ([128, 1024, 1024, 128], 256),  # explicit-W^T dgrad branch
}


def _make_mlp(sizes, last_relu):
    from persia_amd.ops.dense import FusedMLP

    torch.manual_seed(7)
    return FusedMLP(sizes, last_relu=last_relu).to(_dev())


@functools.lru_cache(maxsize=None)
def _reference(stack, last_relu):
    """The same layers applied one by one through FusedLinearFn.apply, plus
    the exact (f64) dw / db of every layer from the per-layer gradients."""
    from persia_amd.ops.dense import FusedLinearFn, _pad32

    sizes, M = STACKS[stack]
    mlp = _make_mlp(sizes, last_relu)
    gen = torch.Generator(device=_dev()).manual_seed(99)
    x = torch.randn(M, sizes[0], device=_dev(), generator=gen).to(torch.bfloat16)
    gup = torch.randn(M, sizes[-1], device=_dev(), generator=gen).to(torch.bfloat16)

    xr = x.clone().requires_grad_(True)
    h, ins, outs, gouts = xr, [], [], {}
    for i, l in enumerate(mlp.layers):
        ins.append(h.detach())
        h = FusedLinearFn.apply(h, l.weight, l.bias, 1 if l.relu else 0)
        h.register_hook(lambda gr, i=i: gouts.__setitem__(i, gr.detach()))
        outs.append(h)
    h.backward(gup)

    exact = []
    for i, l in enumerate(mlp.layers):
        gm = gouts[i].double()
        if l.relu:
            gm = gm * (outs[i].detach().double() > 0)
        xin = ins[i].double()
        dw = gm.t() @ xin
        dw_bound = M * U * (gm.abs().t() @ xin.abs())
        exact.append((dw, dw_bound, gm.sum(0), M * U * gm.abs().sum(0)))
    return {
        "state": {k: v.clone() for k, v in mlp.state_dict().items()},
        "x": x, "gup": gup, "out": h.detach(), "dx": xr.grad.clone(),
        "exact": exact,
        "grads": [(l.weight.grad.clone(), l.bias.grad.clone()) for l in mlp.layers],
    }


def _check_grads(got, exact, scale=1):
    """got: per layer (dw, db) f32; exact: per layer f64 sums and bounds for
    ONE backward; scale=2 checks a doubled accumulation (2M addends)."""
    for i, ((dw, db), (dw64, dwb, db64, dbb)) in enumerate(zip(got, exact)):
        f = scale * scale  # n and sum|a| both scale
        e_w = (dw.double() - scale * dw64).abs()
        e_b = (db.double() - scale * db64).abs()
        print(f"layer {i}: dw err {e_w.max().item():.3e} "
              f"db err {e_b.max().item():.3e}")
        assert (e_w <= f * dwb).all(), f"layer {i} dw"
        assert (e_b <= f * dbb).all(), f"layer {i} db"


@pytest.mark.parametrize("xgrad", [True, False], ids=["xgrad", "nox"])
@pytest.mark.parametrize("side", [False, True], ids=["autograd", "sideband"])
@pytest.mark.parametrize("last_relu", [True, False], ids=["lastrelu", "lastlin"])
@pytest.mark.parametrize("stack", list(STACKS))
def test_fused_mlp_chain_matches_per_layer(stack, last_relu, side, xgrad):
    ref = _reference(stack, last_relu)
    # the per-layer reference itself honours the bound
    _check_grads(ref["grads"], ref["exact"])

    sizes, _ = STACKS[stack]
    mlp = _make_mlp(sizes, last_relu)
    mlp.load_state_dict(ref["state"])
    slots = []
    if side:
        for l in mlp.layers:
            l.weight._sideband_grad = torch.zeros_like(l.weight, dtype=torch.float32)
            l.bias._sideband_grad = torch.zeros_like(l.bias, dtype=torch.float32)
            slots.append((l.weight._sideband_grad, l.bias._sideband_grad))
    x = ref["x"].clone().requires_grad_(xgrad)
    out = mlp(x)
    assert type(out.grad_fn).__name__ == "FusedChainFnBackward"
    assert torch.equal(out, ref["out"])
    out.backward(ref["gup"])
    if xgrad:
        assert torch.equal(x.grad, ref["dx"])
    else:
        assert x.grad is None
    if side:
        for l in mlp.layers:
            assert l.weight.grad is None and l.bias.grad is None
        _check_grads(slots, ref["exact"])
        mlp(x).backward(ref["gup"])  # a second backward ADDS
        _check_grads(slots, ref["exact"], scale=2)
    else:
        _check_grads([(l.weight.grad, l.bias.grad) for l in mlp.layers],
                     ref["exact"])


def test_env_switch_selects_per_layer_path(monkeypatch):
    ref = _reference("odd", True)
    sizes, _ = STACKS["odd"]
    mlp = _make_mlp(sizes, True)
    mlp.load_state_dict(ref["state"])
    monkeypatch.setenv("PA_FUSED_DRELU", "0")
    x = ref["x"].clone().requires_grad_(True)
    out = mlp(x)
    assert type(out.grad_fn).__name__ == "FusedLinearFnBackward"
    out.backward(ref["gup"])
    assert torch.equal(out, ref["out"])
    assert torch.equal(x.grad, ref["dx"])
    _check_grads([(l.weight.grad, l.bias.grad) for l in mlp.layers], ref["exact"])


def test_chain_under_graph_capture():
    """One captured forward+backward with side-band slots, replayed twice ==
    twice one eager backward."""
    ref = _reference("odd", True)
    sizes, _ = STACKS["odd"]
    mlp = _make_mlp(sizes, True)
    mlp.load_state_dict(ref["state"])
    slots = []
    for l in mlp.layers:
        l.weight._sideband_grad = torch.zeros_like(l.weight, dtype=torch.float32)
        l.bias._sideband_grad = torch.zeros_like(l.bias, dtype=torch.float32)
        slots.append((l.weight._sideband_grad, l.bias._sideband_grad))
    x, gup = ref["x"].clone(), ref["gup"].clone()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            mlp(x).backward(gup)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mlp(x).backward(gup)
    for w, b in slots:
        w.zero_()
        b.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    _check_grads(slots, ref["exact"], scale=2)
