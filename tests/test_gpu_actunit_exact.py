"""csrc/actunit.hip against the f64 reference of tests/test_actunit_cases_cpu.py
from the same input bits.  f16 results (out, dq_k, dseq) must be within
2^-11 |ref| + 2^-25 + 4 * E32, f32 results (du, dWb, dWp, dw2, db2) within
4 * E32, where E32 is the error of the f32 reference on the CPU (AC.e32); the
4 covers another summation order and __expf.  Worst err/bound on an MI355X:
out 0.99 at (5, 3, 32, 16), dq_k 0.97 and dseq 0.99 at (7, 64, 64, 32) (the
f16 store's half ulp); du 0.31, dWp 0.26 and dw2 0.27 at (5, 3, 32, 16), dWb
0.33 and db2 0.65 at (7, 64, 64, 32), the same at max_blocks 0, 1 and 3."""
import functools

import pytest
import torch

import test_actunit_cases_cpu as AC
from test_gpu_dense_exact import _bits, _dev, _native, _ratio

pytestmark = pytest.mark.gpu
_is_native = lambda t: type(t.grad_fn).__name__ == "ActUnitPoolFnBackward"  # noqa: E731
PER_SAMPLE, WEIGHTS = AC.NAMES[:4], AC.NAMES[4:]


def _kernels(ops, max_blocks=0):
    q, seq, g, *par = ops
    C = _native()
    return dict(zip(AC.NAMES, (C.act_unit_fwd(q, seq, *par, max_blocks),
                               *C.act_unit_bwd(g, q, seq, *par, max_blocks))))


@functools.lru_cache(maxsize=None)
def _run(case):
    ops = AC.make_operands(case, _dev())
    return ops, _kernels(ops)


def _within(got, case, what):
    ref, E = AC.reference(case, torch.float64), AC.e32(case)
    for n, t in got.items():
        r = ref[n].to(_dev())
        f16 = n in AC.NAMES[:3]
        assert t.dtype == (torch.float16 if f16 else torch.float32), n
        bound = 4 * E[n] + (2.0 ** -11 * r.abs() + 2.0 ** -25 if f16
                            else torch.zeros_like(r))
        _ratio(t, r, bound, f"act_unit {n} {case} {what}")


@pytest.mark.parametrize("case", AC.CASES, ids=AC.IDS)
def test_native_within_bound_and_structure_bit_for_bit(case):
    B, L, D, H = case
    assert _native().act_unit_feasible(L, D, H)
    ops, got = _run(case)
    _within(got, case, "plan")
    seq = ops[1]
    valid = seq[..., D] != 0
    dseq = got["dseq"]
    assert not _bits(dseq[..., D]).any() and not _bits(dseq[~valid]).any()
    if B > 1:  # the last sample has no valid cell: +0, not -0
        assert not valid[B - 1].any()
        assert not any(_bits(got[n][B - 1]).any() for n in ("out", "dq_k", "du"))
    # again; reversed; the first sample alone; one block; three blocks: the
    # per-sample results keep their bits
    everyone = torch.arange(B, device=_dev())
    for idx, mb in ((everyone, 0), (everyone.flip(0), 0), (everyone[:1], 0),
                    (everyone, 1), (everyone, 3)):
        sub = tuple(t[idx].contiguous() for t in ops[:4]) + ops[4:]
        again = _kernels(sub, mb)
        for n in PER_SAMPLE:
            assert torch.equal(_bits(again[n]), _bits(got[n][idx])), (n, mb)
        if len(idx) == B:  # the whole batch: the sums over it hold the bound
            _within({n: again[n] for n in WEIGHTS}, case, f"max_blocks={mb}")
        if mb:  # and at a fixed grid they keep their bits from run to run
            once_more = _kernels(sub, mb)
            for n in WEIGHTS:
                assert torch.equal(_bits(once_more[n]), _bits(again[n])), (n, mb)


def test_dispatch_and_operand_checks(monkeypatch):
    from persia_amd.ops import actunit
    from persia_amd.ops.reference import act_unit_pool_reference

    C = _native()
    B, L, D, H = case = (7, 64, 64, 32)
    ops, got = _run(case)
    q, seq, g, u, Wb, Wp, w2, b2 = ops
    par = [p.to(_dev()) for p in AC.make_params(case)]

    def pool(q, seq, par):
        leaves = [q.clone().requires_grad_(True), seq.clone().requires_grad_(True),
                  *(p.clone().requires_grad_(True) for p in par)]
        return actunit.act_unit_pool(*leaves), leaves

    # feasible f16 CUDA tensors: the kernels' bits through autograd (with u
    # from the GPU's addmm, as the op computes it)
    W1, b1 = par[:2]
    u = torch.addmm(b1, q.float(), (W1[:, :D] + W1[:, 2 * D:3 * D]).t())
    got = _kernels((q, seq, g, u, *ops[4:]))
    pooled, leaves = pool(q, seq, par)
    pooled.backward(g)
    assert _is_native(pooled)
    assert torch.equal(_bits(pooled), _bits(got["out"]))
    assert torch.equal(_bits(leaves[1].grad), _bits(got["dseq"]))
    assert torch.equal(_bits(leaves[4].grad), _bits(got["dw2"]))
    assert torch.equal(_bits(leaves[5].grad), _bits(got["db2"]))
    dW1 = leaves[2].grad  # column blocks Wq | Wk | Wd | Wp
    assert torch.equal(_bits(dW1[:, D:2 * D]), _bits(got["dWb"]))
    assert torch.equal(_bits(dW1[:, 3 * D:]), _bits(got["dWp"]))
    torch.testing.assert_close(leaves[3].grad, got["du"].sum(0))  # torch's sum
    # CPU tensors, D = 40, H = 24 and the knob off: the reference
    q40, s40, _ = AC.make_case((3, 5, 40), _dev())
    p40 = [p.to(_dev()) for p in AC.make_params((3, 5, 40, 16))]
    p24 = [p.to(_dev()) for p in AC.make_params((7, 64, 64, 24))]
    assert not C.act_unit_feasible(5, 40, 16) and not C.act_unit_feasible(64, 64, 24)
    assert not C.act_unit_feasible(1025, 64, 32) and C.act_unit_feasible(1024, 128, 64)
    cpu = (q.cpu(), seq.cpu(), [p.cpu() for p in par])
    for args in (cpu, (q40, s40, p40), (q, seq, p24)):
        ref, _ = pool(*args)
        assert not _is_native(ref)
        assert torch.equal(_bits(ref), _bits(act_unit_pool_reference(*args[:2], *args[2])))
    monkeypatch.setattr(actunit, "_ENABLED", False)  # what PA_ACT_UNIT=0 sets
    assert not _is_native(pool(q, seq, par)[0])
    monkeypatch.setattr(actunit, "_ENABLED", True)
    # the launchers refuse: dtype, device, not contiguous, shapes, infeasible
    o24 = AC.make_operands((7, 64, 64, 24), _dev())
    bad = [(q.float(), seq, g, *ops[3:]), (q, seq.float(), g, *ops[3:]),
           (q.cpu(), seq, g, *ops[3:]), (q, seq, g, u.half(), *ops[4:]),
           (q, seq, g, u, Wb.float(), *ops[5:]), (q, seq, g, u, Wb, Wp, w2.cpu(), b2),
           (q.t().contiguous().t(), seq, g, *ops[3:]),
           (q, seq.transpose(0, 1).contiguous().transpose(0, 1), g, *ops[3:]),
           (q[:B - 1].contiguous(), seq, g, *ops[3:]),
           (q, seq, g, u[:, :16].contiguous(), *ops[4:]),
           (q, seq, g, u, Wb[:16].contiguous(), *ops[5:]),
           (q, seq, g, u, Wb, Wp, w2, torch.zeros(2, device=_dev())), o24]
    for qx, sx, gx, *px in bad:
        with pytest.raises(RuntimeError):
            C.act_unit_fwd(qx, sx, *px)
        with pytest.raises(RuntimeError):
            C.act_unit_bwd(gx, qx, sx, *px)
    for gx in (g.float(), g.t().contiguous().t(), g[:B - 1].contiguous()):
        with pytest.raises(RuntimeError):
            C.act_unit_bwd(gx, *ops[:2], *ops[3:])
    with pytest.raises(RuntimeError):
        C.act_unit_fwd(*ops[:2], *ops[3:], -1)
    torch.cuda.synchronize()


def test_seqctr_mlp_attention_takes_the_kernels():
    from persia_amd.models import SeqCTR

    torch.manual_seed(5)
    q, seq, _ = AC.make_case((6, 70, 32), _dev())
    embs = [e.requires_grad_(True) for e in (q, seq)]
    model = SeqCTR([32, 32], {1: 0}, num_dense=0, hidden=(), attention="mlp",
                   att_hidden=16).to(_dev())
    seen = {}
    model.act_pools["1"].register_forward_hook(lambda m, i, o: seen.update(o=o))
    model(None, embs).sum().backward()
    assert _is_native(seen["o"])
    assert all(torch.isfinite(e.grad).all() and e.grad.any() for e in embs)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.any()
               for p in model.parameters())
