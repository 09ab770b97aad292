"""csrc/seqattn.hip against the f64 model of tests/test_seqattn_cases_cpu.py
(cases, model and bound are there; nothing here is an atol).  Worst err/bound
on an MI355X: out 0.862 at (5, 3, 8), dq 0.795 at (33, 50, 40), dseq 0.994 at
(7, 64, 64) -- the f16 store's half ulp dominates, as for the f32 reference on
CPU; end to end the pooled vectors reach 0.89 and the logits are bit-equal."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_engine_paths as P
import test_seqattn_cases_cpu as SC
from test_gpu_dense_exact import _bits, _dev, _native, _ratio, acc_bound

pytestmark = pytest.mark.gpu
_is_native = lambda t: type(t.grad_fn).__name__ == "SeqAttnPoolFnBackward"  # noqa: E731


def _kernels(q, seq, g, scale):
    C = _native()
    return (C.seq_attn_fwd(q, seq, scale), *C.seq_attn_bwd(g, q, seq, scale))


@functools.lru_cache(maxsize=None)
def _run(case):
    q, seq, g = SC.make_case(case, _dev())
    return (q, seq, g) + _kernels(q, seq, g, SC.case_scale(case))


@pytest.mark.parametrize("case", SC.CASES, ids=SC.IDS)
def test_native_within_bound_and_structure_bit_for_bit(case):
    (B, L, D), scale = case, SC.case_scale(case)
    assert _native().seq_attn_feasible(L, D)
    q, seq, g, *got = _run(case)
    mdl = SC.seqattn_model(q, seq, g, scale)
    for name, t in zip(mdl, got):
        assert t.dtype == torch.float16
        _ratio(t, *mdl[name], f"seq_attn {name} {case}")
    out, dq, dseq = got
    valid = seq[..., D] != 0
    assert not _bits(dseq[..., D]).any() and not _bits(dseq[~valid]).any()
    if B > 1:  # the last sample has no valid cell: +0, not -0
        assert not valid[B - 1].any()
        assert not _bits(out[B - 1]).any() and not _bits(dq[B - 1]).any()
    # again; in reverse order; the first sample alone (B = 1): the same bits
    everyone = torch.arange(B, device=_dev())
    for idx in (everyone, everyone.flip(0), everyone[:1]):
        again = _kernels(*(t[idx].contiguous() for t in (q, seq, g)), scale)
        for name, a, b in zip(mdl, again, got):
            assert torch.equal(_bits(a), _bits(b[idx])), (name, idx.tolist())


def _child():  # PA_SEQ_ATTN=0 in the environment: the reference runs on the GPU
    from persia_amd.ops import seqattn

    q, seq, _ = SC.make_case((5, 3, 8), _dev())
    out = seqattn.seq_attn_pool(q.requires_grad_(True), seq)
    assert not seqattn._ENABLED and not _is_native(out)
    assert torch.equal(_bits(out), _bits(SC.seq_attn_pool_reference(q, seq)))
    print("child: reference path taken")


def test_dispatch_and_operand_checks():
    from persia_amd.ops.seqattn import seq_attn_pool

    C = _native()
    B, L, D = case = (33, 50, 40)
    q, seq, g, *got = _run(case)
    assert all(C.seq_attn_feasible(l, d) for d in (8, 16, 32, 40, 64, 128)
               for l in range(1, 201))
    # feasible f16 CUDA tensors: the kernels, forward and backward
    qa, sa = q.clone().requires_grad_(True), seq.clone().requires_grad_(True)
    pooled = seq_attn_pool(qa, sa)
    pooled.backward(g)
    assert _is_native(pooled)
    for a, b in zip((pooled, qa.grad, sa.grad), got):
        assert torch.equal(_bits(a), _bits(b))
    # CPU tensors and a shape without a kernel (77 KB of rows): the reference
    qb, sb, _ = SC.make_case((2, 300, 128), _dev())
    assert not C.seq_attn_feasible(300, 128) and not C.seq_attn_feasible(50, 12)
    for qx, sx in ((q.cpu(), seq.cpu()), (qb, sb)):
        ref = seq_attn_pool(qx.clone().requires_grad_(True), sx)
        assert not _is_native(ref)
        assert torch.equal(_bits(ref), _bits(SC.seq_attn_pool_reference(qx, sx)))
    # PA_SEQ_ATTN=0 is read at import: a child process
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(tests_dir)
    code = ("import sys; sys.path[:0] = [r'%s', r'%s']; "
            "import test_gpu_seqattn_exact as T; T._child()" % (repo, tests_dir))
    res = subprocess.run([sys.executable, "-c", code], cwd=repo, text=True,
                         env=dict(os.environ, PA_SEQ_ATTN="0"),
                         capture_output=True, timeout=300)
    assert res.returncode == 0 and "reference path taken" in res.stdout, \
        res.stdout[-2000:] + res.stderr[-2000:]
    # the launchers refuse: dtype, device, not contiguous, shapes, infeasible
    bad = [(q.float(), seq, g), (q, seq.float(), g), (q.cpu(), seq, g),
           (q.t().contiguous().t(), seq, g), (q[:, :D - 8].contiguous(), seq, g),
           (q, seq.transpose(0, 1).contiguous().transpose(0, 1), g),
           (q[:B - 1].contiguous(), seq, g), (qb, sb, qb)]
    for qx, sx, gx in bad:
        with pytest.raises(RuntimeError):
            C.seq_attn_fwd(qx, sx, 1.0)
        with pytest.raises(RuntimeError):
            C.seq_attn_bwd(gx, qx, sx, 1.0)
    for gx in (g.float(), g.t().contiguous().t(), g[:B - 1].contiguous()):
        with pytest.raises(RuntimeError):
            C.seq_attn_bwd(gx, q, seq, 1.0)
    torch.cuda.synchronize()


E2E_LENS = (6, 0, 2, 4, 5, 1)  # of the raw slot h: sfs 4 cuts 2 + 1 ids off


def _e2e(monkeypatch, native):
    """One TrainCtx step of SeqCTR over slots a (the query), c and h (raw)."""
    from persia_amd.core.schema import EmbeddingSchema, SlotConfig
    from persia_amd.ctx import TrainCtx
    from persia_amd.embedding.data import IDTypeFeature, Label, PersiaBatch
    from persia_amd.models import SeqCTR

    monkeypatch.setattr("persia_amd.ops.seqattn._ENABLED", native)  # the knob
    B, ids = len(E2E_LENS), iter(range(100, 200))  # every id of h is distinct
    slots = {n: SlotConfig(name=n, dim=8) for n in "ac"}
    slots["h"] = SlotConfig(name="h", dim=8, embedding_summation=False,
                            sample_fixed_size=4)
    eng = P.mk_engine(_dev(), "adagrad", EmbeddingSchema(slots=slots))
    rows = {"a": [[b] for b in range(B)], "c": [[50 + b] for b in range(B)],
            "h": [[next(ids) for _ in range(n)] for n in E2E_LENS]}
    batch = PersiaBatch(
        [IDTypeFeature(n, [np.array(s, np.uint64) for s in r])
         for n, r in rows.items()],
        labels=[Label(np.ones((B, 1), np.float32))], requires_grad=True)
    torch.manual_seed(11)
    model = SeqCTR([8, 8, 8], {2: 0}, num_dense=0, hidden=()).to(_dev())
    cap = {"lin": model.mlp[0]}
    model.pool.register_forward_hook(lambda m, i, o: cap.update(
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
        before = eng.stores[8].lookup(keys, train=False).clone()
        logits, labels = ctx.forward(tb)
        ctx.backward(torch.nn.functional.binary_cross_entropy_with_logits(
            logits, labels[0].squeeze(1)))
        torch.cuda.synchronize()
        moved = (eng.stores[8].lookup(keys, train=False) != before).any(dim=1)
    return dict(cap, logits=logits.detach(), moved=moved.cpu())


def test_train_ctx_seqctr_native_against_reference(monkeypatch):
    on, off = _e2e(monkeypatch, True), _e2e(monkeypatch, False)
    assert _is_native(on["pooled"]) and not _is_native(off["pooled"])
    assert torch.equal(_bits(on["seq"]), _bits(off["seq"]))
    assert on["seq"].shape == (6, 4, 9) and not on["seq"][1, :, 8].any()
    ref, bound = SC.seqattn_model(on["q"], on["seq"], on["q"], 8 ** -0.5)["out"]
    for run in (on, off):
        _ratio(run["pooled"].detach(), ref, bound, "e2e pooled")
    # logits (one f32 linear layer): the inputs differ by at most 2 * bound, in
    # the pooled columns 16..23 only; |W| carries that to the logit, and each
    # run adds the layer's accumulation bound
    x, W = on["x"].double(), on["lin"].weight.double().abs().t()
    dx = torch.zeros_like(x)
    dx[:, 16:] = 2 * bound
    assert torch.equal(on["x"][dx == 0], off["x"][dx == 0])
    S = (x.abs() + dx) @ W + on["lin"].bias.double().abs()
    E = (dx @ W + 2 * acc_bound(S, x.shape[1])).squeeze(1)
    _ratio(on["logits"], off["logits"].double(), E, "e2e logits")
    # keys of valid cells trained, keys seen only past sample_fixed_size not
    kept = torch.from_numpy(np.concatenate([np.arange(n) for n in E2E_LENS]) < 4)
    assert kept.sum() == 15 and (~kept).sum() == 3
    assert on["moved"][kept].all() and not on["moved"][~kept].any()
