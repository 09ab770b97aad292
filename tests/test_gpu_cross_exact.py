"""csrc/cross.hip against the f64 reference of tests/test_cross_cases_cpu.py from
the same input bits.  bf16 results (out, dx0) must be within
2^-8 |ref| + 2^-25 + 4 * E, f32 results (dV, dU, db of every layer) within
4 * E, where E is the error of the f32 reference that rounds to bf16 where the
kernels do (CC.E): the bound of tests/test_gpu_seqffn_exact.py with bf16's
half-ulp in place of f16's.
Worst err/bound on an MI355X: out 0.224 at (129, 96, 32, 2), dx0 0.224 at
(200, 160, 64, 3), every parameter gradient 0.25 (dV1 0.252 at (70, 1696, 256,
2)): the kernels sit on the rounded reference.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import test_cross_cases_cpu as CC
from persia_amd.ops.reference import cross_stack_reference
from test_gpu_dense_exact import _bits, _dev, _native, _ratio

pytestmark = pytest.mark.gpu
_is_native = lambda t: type(t.grad_fn).__name__ == "CrossStackFnBackward"  # noqa: E731
_bf = lambda ws: [w.bfloat16().contiguous() for w in ws]  # noqa: E731


def _kernels(x0, g, Vs, Us, bs):
    """The launchers, layer by layer, as CrossStackFn drives them."""
    C, n = _native(), len(Vs)
    Vs, Us = _bf(Vs), _bf(Us)
    xs, hs, res = [x0], [], {}
    for V, U, b in zip(Vs, Us, bs):
        out, h = C.cross_fwd(x0, xs[-1], V, U, b)
        xs.append(out)
        hs.append(h)
    res["out"] = xs[-1]
    dx0 = torch.empty(0, dtype=torch.bfloat16, device=x0.device)
    for l in range(n - 1, -1, -1):
        dp, dh, part = C.cross_bwd_dh(g, x0, Us[l].t().contiguous())
        res[f"db{l}"] = C.cross_db_reduce(part)
        res[f"dU{l}"], res[f"dV{l}"] = C.wgrad(dp, hs[l]), C.wgrad(dh, xs[l])
        g, dx0 = C.cross_bwd_dx(g, dh, hs[l], Vs[l].t().contiguous(), Us[l],
                                bs[l], dx0, l == 0)
    res["dx0"] = dx0
    return res


@functools.lru_cache(maxsize=None)
def _run(case):
    ops = CC.make_operands(case, _dev())
    return ops, _kernels(*ops)


@pytest.mark.parametrize("case", CC.CASES, ids=CC.IDS)
def test_native_within_bound_and_rows_independent(case):
    B, D, r, n = case
    assert _native().cross_feasible(D, r)
    ops, got = _run(case)
    ref, E = CC.reference(case, torch.float64), CC.E(case)
    for k in CC.names(case):
        want = ref[k].to(_dev())
        rows = k in ("out", "dx0")
        assert got[k].dtype == (torch.bfloat16 if rows else torch.float32), k
        bound = (2.0 ** -8 * want.abs() + 2.0 ** -25 + 4 * E[k] if rows
                 else torch.full_like(want, 4 * E[k]))
        _ratio(got[k], want, bound, f"cross {k} {case}")
    # reversed; the first row alone: a row's results keep their bits
    everyone = torch.arange(B, device=_dev())
    for idx in (everyone.flip(0), everyone[:1]):
        again = _kernels(ops[0][idx].contiguous(), ops[1][idx].contiguous(),
                         *ops[2:])
        for k in ("out", "dx0"):
            assert torch.equal(_bits(again[k]), _bits(got[k][idx])), k


def _reference(x0, Vs, Us, bs):
    return cross_stack_reference(x0, *([p.to(x0.dtype) for p in ps]
                                       for ps in (Vs, Us, bs)))


def _child():  # PA_CROSS_STACK=0 in the environment: the reference runs
    from persia_amd.ops import cross

    x0, _, Vs, Us, bs = CC.make_operands(CC.CASES[1], _dev())
    out = cross.cross_stack(x0.requires_grad_(True), Vs, Us, bs)
    assert not cross._ENABLED and not _is_native(out)
    assert torch.equal(_bits(out), _bits(_reference(x0, Vs, Us, bs)))
    print("child: reference path taken")


def test_dispatch_and_operand_checks():
    from persia_amd.ops import cross_stack

    C = _native()
    case = CC.CASES[3]
    (x0, g, Vs, Us, bs), got = _run(case)
    # feasible bf16 CUDA operands: the launchers' bits through autograd
    leaf = lambda ts: [t.clone().requires_grad_(True) for t in ts]  # noqa: E731
    x, lV, lU, lb = x0.clone().requires_grad_(True), leaf(Vs), leaf(Us), leaf(bs)
    out = cross_stack(x, lV, lU, lb)
    assert _is_native(out)
    out.backward(g)
    assert torch.equal(_bits(out), _bits(got["out"]))
    assert torch.equal(_bits(x.grad), _bits(got["dx0"]))
    for l, b in enumerate(lb):
        assert torch.equal(_bits(b.grad), _bits(got[f"db{l}"])), l
        assert lV[l].grad.shape == Vs[l].shape and lU[l].grad.shape == Us[l].shape
    # infeasible shapes: the reference
    for c in ((5, 96, 48, 1), (5, 320, 288, 1), (5, 40, 32, 1)):
        assert not C.cross_feasible(c[1], c[2])
        a = CC.make_operands(c, _dev())
        ref = cross_stack(a[0].clone().requires_grad_(True), *a[2:])
        assert not _is_native(ref)
        assert torch.equal(_bits(ref), _bits(_reference(a[0], *a[2:])))
    # PA_CROSS_STACK=0 is read at import: a child process
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(tests_dir)
    code = ("import sys; sys.path[:0] = [r'%s', r'%s']; "
            "import test_gpu_cross_exact as T; T._child()" % (repo, tests_dir))
    child = subprocess.run([sys.executable, "-c", code], cwd=repo, text=True,
                           env=dict(os.environ, PA_CROSS_STACK="0"),
                           capture_output=True, timeout=300)
    assert child.returncode == 0 and "reference path taken" in child.stdout, \
        child.stdout[-2000:] + child.stderr[-2000:]
    # the launchers refuse: dtype, device, not contiguous, shapes
    V, U, b = _bf(Vs)[0], _bf(Us)[0], bs[0]
    for args in ((x0.float(), x0, V, U, b), (x0.cpu(), x0, V, U, b),
                 (x0.t().contiguous().t(), x0, V, U, b),
                 (x0, x0, V, U[:, :32].contiguous(), b),
                 (x0, x0, V, U, b[:-1].contiguous())):
        with pytest.raises(RuntimeError):
            C.cross_fwd(*args)
    torch.cuda.synchronize()


def test_dcnv2_fused_cross_is_cross_stack_on_the_same_parameters():
    from persia_amd.models import DCNv2
    from persia_amd.ops import cross_stack

    kw = dict(num_sparse=3, num_dense=13, dim=32, num_cross=2, deep=(64, 32),
              cross_rank=32, fused=True)
    torch.manual_seed(5)
    twin = DCNv2(**kw)
    model = DCNv2(fused_cross=True, **kw)
    keys = model.load_state_dict(twin.state_dict())
    assert not keys.missing_keys and not keys.unexpected_keys
    model = model.bfloat16().to(_dev())
    seen = {}
    model.head.register_forward_pre_hook(lambda m, i: seen.update(x=i[0].detach()))
    gen = torch.Generator().manual_seed(6)
    dense = torch.randn(37, 13, generator=gen).to(_dev())
    embs = [torch.randn(37, 32, generator=gen).to(_dev()) for _ in range(3)]
    model(dense, embs)
    x0 = torch.nn.functional.pad(
        torch.cat([dense.bfloat16()] + [e.bfloat16() for e in embs], 1),
        (0, model.pad))
    want = cross_stack(x0, [c.v.weight for c in model.cross],
                       [c.u.weight for c in model.cross],
                       [c.u.bias for c in model.cross])
    assert _is_native(want)
    assert torch.equal(_bits(seen["x"][:, :model.in_dim]), _bits(want))
