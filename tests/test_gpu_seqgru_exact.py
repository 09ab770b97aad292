"""csrc/seqgru.hip against the f64 reference of tests/test_seqgru_cases_cpu.py
from the same input bits.  f16 results (states, last, dseq) must be within
2^-11 |ref| + 2^-25 + 4 * E16, f32 results (dWx, dWh, dbx, dbh, datt) within
4 * E16, where E16 is the error of the f32 reference with f16 state operands
on the CPU (GC.e16); the 4 covers another summation order and __expf.  Worst
err/bound on an MI355X: states and last 0.93, dWx 0.37, dbx 0.29 and dbh 0.25
at (1, 1, 32, 32), dseq 0.85 there with att, dWh 0.25 at (5, 3, 32, 32) with
att, datt 0.36 at the mask with holes; end to end the pooled vectors reach
0.84 and the logits and rows stay below 0.001 of their bounds."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_engine_paths as P
import test_seqgru_cases_cpu as GC
from test_gpu_dense_exact import _bits, _dev, _native, _ratio, acc_bound

pytestmark = pytest.mark.gpu
_is_native = lambda t: type(t.grad_fn).__name__ == "SeqGRUFnBackward"  # noqa: E731
PER_SAMPLE, WEIGHTS = ("states", "last", "dseq", "datt"), GC.NAMES[3:7]


def _kernels(ops):
    seq, Wx, Wh, bx, bh, att, gs, gl = ops
    C = _native()
    Wx, Wh = Wx.half(), Wh.half()
    states, last = C.seq_gru_fwd(seq, Wx, Wh, bx, bh, att)
    grads = C.seq_gru_bwd(gs, gl, seq, states, Wx, Wh, bx, bh, att)
    return dict(zip(GC.NAMES, (states, last, *grads)))


@functools.lru_cache(maxsize=None)
def _run(case, att):
    ops = GC.make_operands(case, att, _dev())
    return ops, _kernels(ops)


def _bound(ref, E, n):
    f16 = n in GC.NAMES[:3]
    return 4 * E[n] + (2.0 ** -11 * ref.abs() + 2.0 ** -25 if f16
                       else torch.zeros_like(ref))


@pytest.mark.parametrize("case,att", GC.PARAMS, ids=GC.IDS)
def test_native_within_bound_and_structure_bit_for_bit(case, att):
    B, L, D, H = case
    assert _native().seq_gru_feasible(L, D, H)
    ops, got = _run(case, att)
    ref, E = GC.reference(case, att, torch.float64), GC.e16(case, att)
    assert (got["datt"] is None) == (not att)
    for n in E:
        r = ref[n].to(_dev())
        assert got[n].dtype == (torch.float16 if n in GC.NAMES[:3] else torch.float32)
        _ratio(got[n], r, _bound(r, E, n), f"seq_gru {n} {case} att={att}")
    seq, states, dseq = ops[0], got["states"], got["dseq"]
    valid = seq[..., D] != 0
    assert not _bits(dseq[..., D]).any() and not _bits(dseq[~valid]).any()
    if att:
        assert not _bits(got["datt"][~valid]).any()
    prev = torch.cat([torch.zeros_like(states[:, :1]), states[:, :-1]], 1)
    assert torch.equal(_bits(states[~valid]), _bits(prev[~valid]))
    assert torch.equal(_bits(got["last"]), _bits(states[:, L - 1]))
    if B > 1:  # the last sample has no valid row: +0, not -0
        assert not valid[B - 1].any()
        assert not any(_bits(got[n][B - 1]).any() for n in E if n in PER_SAMPLE)
    # again; reversed; the first sample alone: the per-sample results keep
    # their bits, and so do the weight gradients of the same batch
    everyone = torch.arange(B, device=_dev())
    for idx in (everyone, everyone.flip(0), everyone[:1]):
        sub = (ops[0][idx].contiguous(),) + ops[1:5] + tuple(
            None if t is None else t[idx].contiguous() for t in ops[5:])
        again = _kernels(sub)
        for n in E:
            if n in PER_SAMPLE:
                assert torch.equal(_bits(again[n]), _bits(got[n][idx])), n
            elif idx is everyone:
                assert torch.equal(_bits(again[n]), _bits(got[n])), n


def _child():  # PA_SEQ_GRU=0 in the environment: the reference runs on the GPU
    from persia_amd.ops import seqgru

    seq, *par, att, _, _ = GC.make_operands((5, 3, 32, 32), True, _dev())
    last = seqgru.seq_gru(seq.requires_grad_(True), *par, att)[1]
    assert not seqgru._ENABLED and not _is_native(last)
    assert torch.equal(_bits(last), _bits(GC.seq_gru_reference(seq, *par, att)[1]))
    print("child: reference path taken")


def test_dispatch_and_operand_checks():
    from persia_amd.ops.seqgru import seq_gru

    C = _native()
    B, L, D, H = case = (17, 9, 64, 32)
    ops, got = _run(case, True)
    seq, Wx, Wh, bx, bh, att, gs, gl = ops
    # feasible f16 CUDA tensors: the kernels' bits through autograd
    leaves = [t.clone().requires_grad_(True) for t in ops[:6]]
    states, last = seq_gru(*leaves)
    assert _is_native(states) and _is_native(last)
    torch.autograd.backward([states, last], [gs, gl])
    for n, t in zip(GC.NAMES, (states, last, *(x.grad for x in leaves))):
        assert torch.equal(_bits(t), _bits(got[n])), n
    # only `last` used: g_states arrives as None; without att: no datt
    leaves = [t.clone().requires_grad_(True) for t in ops[:5]]
    seq_gru(*leaves)[1].backward(gl)
    only = C.seq_gru_bwd(None, gl, seq, got["states"], Wx.half(), Wh.half(), bx, bh, att)
    assert only[5] is not None and torch.isfinite(leaves[0].grad).all()
    assert C.seq_gru_bwd(None, gl, seq, C.seq_gru_fwd(seq, Wx.half(), Wh.half(), bx, bh)[0],
                         Wx.half(), Wh.half(), bx, bh)[5] is None
    # CPU tensors and H = 48: the reference
    assert not C.seq_gru_feasible(9, 64, 48) and not C.seq_gru_feasible(9, 40, 32)
    assert not C.seq_gru_feasible(1025, 64, 32) and C.seq_gru_feasible(1024, 128, 64)
    o48 = GC.make_operands((3, 5, 64, 48), True, _dev())
    for args in (tuple(t.cpu() for t in ops[:6]), o48[:6]):
        ref = seq_gru(args[0].clone().requires_grad_(True), *args[1:])
        assert not _is_native(ref[1])
        assert torch.equal(_bits(ref[0]), _bits(GC.seq_gru_reference(*args)[0]))
    with pytest.raises(ValueError):
        seq_gru(seq, Wx[:, :32], Wh, bx, bh)
    with pytest.raises(ValueError):
        seq_gru(seq, Wx, Wh, bx, bh, att[:, :L - 1])
    # PA_SEQ_GRU=0 is read at import: a child process
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(tests_dir)
    code = ("import sys; sys.path[:0] = [r'%s', r'%s']; "
            "import test_gpu_seqgru_exact as T; T._child()" % (repo, tests_dir))
    res = subprocess.run([sys.executable, "-c", code], cwd=repo, text=True,
                         env=dict(os.environ, PA_SEQ_GRU="0"),
                         capture_output=True, timeout=300)
    assert res.returncode == 0 and "reference path taken" in res.stdout, \
        res.stdout[-2000:] + res.stderr[-2000:]
    # the launchers refuse: dtype, device, not contiguous, shapes, infeasible
    x16, h16, st = Wx.half(), Wh.half(), got["states"]
    good = (seq, x16, h16, bx, bh, att)
    bad = [(seq.float(),) + good[1:], (seq.cpu(),) + good[1:],
           (seq, Wx, h16, bx, bh, att), (seq, x16, h16, bx.half(), bh, att),
           (seq, x16, h16, bx, bh.cpu(), att),
           (seq.transpose(0, 1).contiguous().transpose(0, 1),) + good[1:],
           (seq, x16.t().contiguous().t(), h16, bx, bh, att),
           (seq, x16[:, :32].contiguous(), h16, bx, bh, att),
           (seq, x16, h16[:, :16].contiguous(), bx, bh, att),
           (seq, x16, h16, bx[:H].contiguous(), bh, att),
           (seq, x16, h16, bx, bh, att[:, :L - 1].contiguous()),
           (seq, x16, h16, bx, bh, att[:B - 1].contiguous()),
           (seq, x16, h16, bx, bh, att.double()),
           tuple(t.half() if t.dim() == 2 and i < 3 else t
                 for i, t in enumerate(o48[:6]))]
    for args in bad:
        with pytest.raises(RuntimeError):
            C.seq_gru_fwd(*args)
        with pytest.raises(RuntimeError):
            C.seq_gru_bwd(gs, gl, args[0], st, *args[1:])
    for gx, lx, sx in ((gs.float(), gl, st), (gs, gl[:B - 1].contiguous(), st),
                       (gs[:, :L - 1].contiguous(), gl, st), (gs, gl, st.float()),
                       (gs, gl, st[:, :, :16].contiguous())):
        with pytest.raises(RuntimeError):
            C.seq_gru_bwd(gx, lx, seq, sx, *good[1:])
    empty = C.seq_gru_fwd(seq[:0], *good[1:5], att[:0])
    assert empty[0].shape == (0, L, H) and empty[1].shape == (0, H)
    torch.cuda.synchronize()


E2E_LENS = (6, 0, 2, 4, 5, 1)  # of the raw slot h: sfs 4 cuts 2 + 1 ids off


def _e2e(monkeypatch, native):
    """One TrainCtx step of SeqCTR(augru) over slots a (the query), c and h
    (raw, dim 32, sample_fixed_size 4)."""
    from persia_amd.core.schema import EmbeddingSchema, SlotConfig
    from persia_amd.ctx import TrainCtx
    from persia_amd.embedding.data import IDTypeFeature, Label, PersiaBatch
    from persia_amd.models import SeqCTR

    monkeypatch.setattr("persia_amd.ops.seqgru._ENABLED", native)  # the knob
    B, ids = len(E2E_LENS), iter(range(100, 200))  # every id of h is distinct
    slots = {n: SlotConfig(name=n, dim=32) for n in "ac"}
    slots["h"] = SlotConfig(name="h", dim=32, embedding_summation=False,
                            sample_fixed_size=4)
    eng = P.mk_engine(_dev(), "adagrad", EmbeddingSchema(slots=slots))
    rows = {"a": [[b] for b in range(B)], "c": [[50 + b] for b in range(B)],
            "h": [[next(ids) for _ in range(n)] for n in E2E_LENS]}
    batch = PersiaBatch(
        [IDTypeFeature(n, [np.array(s, np.uint64) for s in r])
         for n, r in rows.items()],
        labels=[Label(np.ones((B, 1), np.float32))], requires_grad=True)
    torch.manual_seed(11)
    model = SeqCTR([32, 32, 32], {2: 0}, num_dense=0, hidden=(),
                   attention="augru").to(_dev())
    cap = {"lin": model.mlp[0], "pool": model.gru_pools["2"]}
    cap["pool"].register_forward_hook(lambda m, i, o: cap.update(
        q=i[0].detach(), seq=i[1].detach(), pooled=o))
    model.mlp.register_forward_hook(lambda m, i, o: cap.update(x=i[0].detach()))
    with TrainCtx(model=model, engine=eng, device_id=0, mixed_precision=False,
                  dense_optimizer=torch.optim.SGD(model.parameters(), lr=0.01)
                  ) as ctx:
        tb = eng.process_batch(batch)
        grp = tb._groups[0]
        assert grp.raw_mask is not None  # the native raw path
        s, e = next(sc for sc in grp.slots if sc.name == "h").pos_slice
        keys = grp.uniq_keys[grp.inverse[s:e]]
        before = eng.stores[32].lookup(keys, train=False).clone()
        logits, labels = ctx.forward(tb)
        ctx.backward(torch.nn.functional.binary_cross_entropy_with_logits(
            logits, labels[0].squeeze(1)))
        torch.cuda.synchronize()
        after = eng.stores[32].lookup(keys, train=False).clone()
    return dict(cap, logits=logits.detach(), after=after,
                moved=(after != before).any(dim=1).cpu())


def test_train_ctx_seqctr_augru_native_against_reference(monkeypatch):
    """Bound.  Both runs pool the same f16 rows with the same parameters; each
    pooled vector is within res = 2^-11 |ref| + 2^-25 + 4 * E16[last] of the
    f64 reference of that shape (E16 measured on the CPU from the captured
    operands), so the two differ by at most 2 res.  One f32 linear layer
    carries that to the logit through |W|, plus its accumulation bound.  The
    Adagrad step of a row is lr g / sqrt(G0 + g^2), whose slope in g is at
    most lr / sqrt(G0) = 0.1 / 0.1 = 1, and the gradients of this loss are
    below 1, so the rows agree within 2 max(res)."""
    on, off = _e2e(monkeypatch, True), _e2e(monkeypatch, False)
    assert _is_native(on["pooled"]) and not _is_native(off["pooled"])
    assert torch.equal(_bits(on["seq"]), _bits(off["seq"]))
    assert on["seq"].shape == (6, 4, 33) and not on["seq"][1, :, 32].any()
    pool, q, seq = on["pool"], on["q"], on["seq"]
    par = [p.detach().cpu() for p in (pool.weight_ih_l0, pool.weight_hh_l0,
                                      pool.bias_ih_l0, pool.bias_hh_l0)]
    att = pool.attention_weights(q, seq).cpu()
    ref = GC.seq_gru_reference(seq.cpu().double(), *(p.double() for p in par),
                               att.double())[1]
    r16 = GC.seq_gru_reference(seq.cpu().float(), *par, att,
                               operand_dtype=torch.float16)[1]
    E16 = (r16.double() - ref).abs().max().item()
    res = (2.0 ** -11 * ref.abs() + 2.0 ** -25 + 4 * E16).to(_dev())
    for run in (on, off):
        _ratio(run["pooled"].detach(), ref.to(_dev()), res, "e2e pooled")
    x, W = on["x"].double(), on["lin"].weight.double().abs().t()
    dx = torch.zeros_like(x)
    dx[:, 64:] = 2 * res
    assert torch.equal(on["x"][dx == 0], off["x"][dx == 0])
    S = (x.abs() + dx) @ W + on["lin"].bias.double().abs()
    E = (dx @ W + 2 * acc_bound(S, x.shape[1])).squeeze(1)
    _ratio(on["logits"], off["logits"].double(), E, "e2e logits")
    _ratio(on["after"], off["after"].double(),
           torch.full_like(on["after"], 2 * res.max().item()).double(), "e2e rows")
    # keys of valid cells trained, keys seen only past sample_fixed_size not
    kept = torch.from_numpy(np.concatenate([np.arange(n) for n in E2E_LENS]) < 4)
    assert on["moved"][kept].all() and not on["moved"][~kept].any()
