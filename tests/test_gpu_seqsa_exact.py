"""csrc/seqsa.hip against the f64 reference of tests/test_seqsa_cases_cpu.py
from the same input bits.  f16 results (out, dseq) must be within
2^-11 |ref| + 2^-25 + 4 * E16, f32 results (dWqkv, dbqkv) within 4 * E16,
where E16 is the error of the f32 reference with f16 operands on the CPU
(SC.e16); the 4 covers another summation order and __expf.  Worst err/bound
on an MI355X: out 0.52, dWqkv 0.27 and dbqkv 0.27 at (2, 17, 64, 2), dseq
0.73 at (1, 1, 32, 1), all without the causal flag; end to end the
self-attention output reaches 0.37."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_engine_paths as P
import test_seqsa_cases_cpu as SC
from test_gpu_dense_exact import _bits, _dev, _native, _ratio

pytestmark = pytest.mark.gpu
_is_native = lambda t: type(t.grad_fn).__name__ == "SeqSelfAttnFnBackward"  # noqa: E731


def _kernels(ops, heads, causal, residual, max_blocks=0):
    seq, W, b, g = ops
    C, W16 = _native(), W.half()
    out = C.seq_self_attn_fwd(seq, W16, b, heads, causal, residual, max_blocks)
    grads = C.seq_self_attn_bwd(g, seq, W16, b, heads, causal, residual, max_blocks)
    return dict(zip(SC.NAMES, (out, *grads)))


@functools.lru_cache(maxsize=None)
def _run(case, causal):
    ops = SC.make_operands(case, _dev())
    return ops, _kernels(ops, case[3], causal, SC.residual_of(case),
                         2 if case == SC.BLOCKS else 0)


def _bound(ref, E):
    return 2.0 ** -11 * ref.abs() + 2.0 ** -25 + 4 * E


@pytest.mark.parametrize("case,causal", SC.PARAMS, ids=SC.IDS)
def test_native_within_bound_and_structure_bit_for_bit(case, causal):
    B, L, D, heads = case
    assert _native().seq_self_attn_feasible(L, D, heads)
    ops, got = _run(case, causal)
    ref, E = SC.reference(case, causal, torch.float64), SC.e16(case, causal)
    for n in SC.NAMES:
        r, f16 = ref[n].to(_dev()), n in ("out", "dseq")
        assert got[n].dtype == (torch.float16 if f16 else torch.float32)
        bound = _bound(r, E[n]) if f16 else torch.full_like(r, 4 * E[n])
        _ratio(got[n], r, bound, f"seq_self_attn {n} {case} causal={causal}")
    seq, out, dseq = ops[0], got["out"], got["dseq"]
    valid = seq[..., D] != 0
    assert not _bits(out[..., :D][~valid]).any()
    assert torch.equal(_bits(out[..., D]), _bits(seq[..., D]))
    assert not _bits(dseq[..., D]).any() and not _bits(dseq[~valid]).any()
    if B > 1:  # the last sample has no valid row: +0, not -0
        assert not valid[B - 1].any()
        assert not _bits(out[B - 1, :, :D]).any() and not _bits(dseq[B - 1]).any()
    # again; reversed; the first sample alone: the per-sample results keep
    # their bits, and so do the weight gradients of the same batch and grid
    everyone = torch.arange(B, device=_dev())
    for idx in (everyone, everyone.flip(0), everyone[:1]):
        sub = (ops[0][idx].contiguous(), ops[1], ops[2], ops[3][idx].contiguous())
        again = _kernels(sub, heads, causal, SC.residual_of(case),
                         2 if case == SC.BLOCKS else 0)
        for n in SC.NAMES:
            if n in ("out", "dseq"):
                assert torch.equal(_bits(again[n]), _bits(got[n][idx])), n
            elif idx is everyone:
                assert torch.equal(_bits(again[n]), _bits(got[n])), n


def _child():  # PA_SEQ_SELF_ATTN=0 in the environment: the reference runs
    from persia_amd.ops import seqsa

    seq, W, b, _ = SC.make_operands((5, 3, 32, 2), _dev())
    out = seqsa.seq_self_attn(seq.requires_grad_(True), W, b, 2)
    assert not seqsa._ENABLED and not _is_native(out)
    assert torch.equal(_bits(out), _bits(SC.seq_self_attn_reference(seq, W, b, 2)))
    print("child: reference path taken")


def test_dispatch_and_operand_checks():
    from persia_amd.ops.seqsa import seq_self_attn

    C = _native()
    B, L, D, heads = case = (2, 17, 64, 2)
    res = SC.residual_of(case)
    ops, got = _run(case, True)
    seq, W, b, g = ops
    # feasible f16 CUDA tensors: the kernels' bits through autograd
    leaves = [t.clone().requires_grad_(True) for t in (seq, W, b)]
    out = seq_self_attn(*leaves, heads, causal=True, residual=res)
    assert _is_native(out)
    out.backward(g)
    for n, t in zip(SC.NAMES, (out, *(x.grad for x in leaves))):
        assert torch.equal(_bits(t), _bits(got[n])), n
    # infeasible shapes and CPU tensors: the reference
    for shape in ((17, 128, 4), (17, 48, 3), (17, 64, 8), (65, 64, 2)):
        assert not C.seq_self_attn_feasible(*shape), shape
    assert C.seq_self_attn_feasible(64, 64, 4)
    for c in ((2, 5, 128, 4), (2, 5, 48, 3), (2, 5, 64, 8), (2, 65, 64, 2), None):
        args = (SC.make_operands(c, _dev())[:3] + (c[3],) if c else
                tuple(t.cpu() for t in ops[:3]) + (heads,))
        ref = seq_self_attn(args[0].clone().requires_grad_(True), *args[1:],
                            causal=True)
        assert not _is_native(ref)
        assert torch.equal(_bits(ref), _bits(
            SC.seq_self_attn_reference(*args, causal=True)))
    for bad in ((seq, W, b, 5), (seq, W[:, :32], b, heads), (seq, W, b[:D], heads),
                (seq[0], W, b, heads)):
        with pytest.raises(ValueError):
            seq_self_attn(*bad)
    # PA_SEQ_SELF_ATTN=0 is read at import: a child process
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(tests_dir)
    code = ("import sys; sys.path[:0] = [r'%s', r'%s']; "
            "import test_gpu_seqsa_exact as T; T._child()" % (repo, tests_dir))
    child = subprocess.run([sys.executable, "-c", code], cwd=repo, text=True,
                           env=dict(os.environ, PA_SEQ_SELF_ATTN="0"),
                           capture_output=True, timeout=300)
    assert child.returncode == 0 and "reference path taken" in child.stdout, \
        child.stdout[-2000:] + child.stderr[-2000:]
    # the launchers refuse: dtype, device, not contiguous, shapes, infeasible
    W16 = W.half()
    o128 = SC.make_operands((2, 5, 128, 4), _dev())
    bad = [(seq.float(), W16, b, heads), (seq.cpu(), W16, b, heads),
           (seq, W, b, heads), (seq, W16, b.half(), heads),
           (seq, W16, b.cpu(), heads),
           (seq.transpose(0, 1).contiguous().transpose(0, 1), W16, b, heads),
           (seq, W16.t().contiguous().t(), b, heads),
           (seq, W16[:, :32].contiguous(), b, heads),
           (seq, W16[:D].contiguous(), b, heads),
           (seq, W16, b[:D].contiguous(), heads), (seq, W16, b, 3),
           (seq, W16, b, 8), (o128[0], o128[1].half(), o128[2], 4)]
    for args in bad:
        with pytest.raises(RuntimeError):
            C.seq_self_attn_fwd(*args)
        with pytest.raises(RuntimeError):
            C.seq_self_attn_bwd(g if args[0] is seq else torch.zeros_like(
                args[0], dtype=torch.float16), *args)
    for gx in (g.float(), g[:B - 1].contiguous(), g[:, :L - 1].contiguous(),
               g.cpu(), g.transpose(0, 1).contiguous().transpose(0, 1)):
        with pytest.raises(RuntimeError):
            C.seq_self_attn_bwd(gx, seq, W16, b, heads)
    assert C.seq_self_attn_fwd(seq[:0], W16, b, heads).shape == (0, L, D + 1)
    empty = C.seq_self_attn_bwd(g[:0], seq[:0], W16, b, heads)
    assert empty[0].shape == (0, L, D + 1) and empty[1].shape == (3 * D, D)
    assert not empty[1].any() and not empty[2].any()
    torch.cuda.synchronize()


E2E_LENS = (6, 0, 2, 4, 5, 1)  # of the raw slot h: sfs 4 cuts 2 + 1 ids off


def _e2e(monkeypatch, native):
    """One TrainCtx step of SeqCTR(self) over slots a (the query), c and h
    (raw, dim 32, sample_fixed_size 4)."""
    from persia_amd.core.schema import EmbeddingSchema, SlotConfig
    from persia_amd.ctx import TrainCtx
    from persia_amd.embedding.data import IDTypeFeature, Label, PersiaBatch
    from persia_amd.models import SeqCTR

    monkeypatch.setattr("persia_amd.ops.seqsa._ENABLED", native)  # the knob
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
                   attention="self", heads=2).to(_dev())
    cap = {"pool": model.sa_pools["2"]}
    cap["pool"].layer.register_forward_hook(lambda m, i, o: cap.update(
        seq=i[0].detach(), sa=o))
    with TrainCtx(model=model, engine=eng, device_id=0, mixed_precision=False,
                  dense_optimizer=torch.optim.SGD(model.parameters(), lr=0.01)
                  ) as ctx:
        par = [p.detach().clone() for p in (cap["pool"].in_proj_weight,
                                            cap["pool"].in_proj_bias)]
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
    return dict(cap, par=par, moved=(after != before).any(dim=1).cpu())


def test_train_ctx_seqctr_self_native_against_reference(monkeypatch):
    on, off = _e2e(monkeypatch, True), _e2e(monkeypatch, False)
    assert _is_native(on["sa"]) and not _is_native(off["sa"])
    assert torch.equal(_bits(on["seq"]), _bits(off["seq"]))
    assert on["seq"].shape == (6, 4, 33) and not on["seq"][1, :, 32].any()
    seq, (W, b) = on["seq"].cpu(), (p.cpu() for p in on["par"])
    ref = SC.seq_self_attn_reference(seq.double(), W.double(), b.double(), 2,
                                     residual=True)
    r16 = SC.seq_self_attn_reference(seq.float(), W, b, 2, residual=True,
                                     operand_dtype=torch.float16)
    E16 = (r16.double() - ref).abs().max().item()
    for run in (on, off):
        _ratio(run["sa"].detach(), ref.to(_dev()), _bound(ref, E16).to(_dev()),
               "e2e self-attention output")
    # keys of valid cells trained, keys seen only past sample_fixed_size not
    kept = torch.from_numpy(np.concatenate([np.arange(n) for n in E2E_LENS]) < 4)
    assert on["moved"][kept].all() and not on["moved"][~kept].any()
