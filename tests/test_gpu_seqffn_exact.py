"""csrc/seqffn.hip against the f64 reference of tests/test_seqffn_cases_cpu.py
from the same input bits.  f16 results (out, dx, da) must be within
2^-11 |ref| + 2^-25 + 4 * E16, f32 results (the ten parameter gradients)
within 4 * E16, where E16 is the error of the f32 reference with f16 operands
on the CPU (SC.e16): the bound of tests/test_gpu_seqsa_exact.py, unchanged.
Worst err/bound on an MI355X: out 0.34 and da 0.57 at (3, 7, 64, 256), dx 0.50
at (5, 13, 32, 96), every parameter gradient 0.25 (the kernels sit on the
emulated reference); the encoder layer end to end 0.30."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_engine_paths as P
import test_seqffn_cases_cpu as SC
from persia_amd.ops.reference import seq_self_attn_reference
from test_gpu_dense_exact import _bits, _dev, _native, _ratio

pytestmark = pytest.mark.gpu
_is_native = lambda t: type(t.grad_fn).__name__ == "SeqFfnFnBackward"  # noqa: E731
_ROWS = ("out", "dx", "da")


def _kernels(ops, max_blocks=0):
    t = [w.half() if w.dim() == 2 else w for w in ops[:-1]]
    C = _native()
    out = C.seq_ffn_fwd(*t, 1e-5, max_blocks)
    return dict(zip(SC.NAMES, (out, *C.seq_ffn_bwd(ops[-1], *t, 1e-5, max_blocks))))


@functools.lru_cache(maxsize=None)
def _run(case):
    ops = SC.make_operands(case, _dev())
    return ops, _kernels(ops, 2 if case == SC.BLOCKS else 0)


def _bound(ref, E):
    return 2.0 ** -11 * ref.abs() + 2.0 ** -25 + 4 * E


@pytest.mark.parametrize("case", SC.CASES, ids=SC.IDS)
def test_native_within_bound_and_structure_bit_for_bit(case):
    B, L, D, F = case
    assert _native().seq_ffn_feasible(D, F)
    ops, got = _run(case)
    ref, E = SC.reference(case, torch.float64), SC.e16(case)
    for n in SC.NAMES:
        r = ref[n].to(_dev())
        assert got[n].dtype == (torch.float16 if n in _ROWS else torch.float32)
        bound = _bound(r, E[n]) if n in _ROWS else torch.full_like(r, 4 * E[n])
        _ratio(got[n], r, bound, f"seq_ffn {n} {case}")
    x = ops[0]
    valid = x[..., D] != 0
    assert torch.equal(_bits(got["out"][..., D]), _bits(x[..., D]))
    for n in _ROWS:  # +0, not -0
        assert not _bits(got[n][..., :D][~valid]).any(), n
        assert n == "out" or not _bits(got[n][..., D]).any(), n
    assert B == 1 or not valid[B - 1].any()
    # again; reversed; the first sample alone: the per-row results keep their
    # bits, and so do the parameter gradients of the same batch and grid
    everyone = torch.arange(B, device=_dev())
    for idx in (everyone, everyone.flip(0), everyone[:1]):
        sub = tuple(t[idx].contiguous() if t.dim() == 3 else t for t in ops)
        again = _kernels(sub, 2 if case == SC.BLOCKS else 0)
        for n in SC.NAMES:
            if n in _ROWS:
                assert torch.equal(_bits(again[n]), _bits(got[n][idx])), n
            elif idx is everyone:
                assert torch.equal(_bits(again[n]), _bits(got[n])), n


def _child():  # PA_SEQ_FFN=0 in the environment: the reference runs
    from persia_amd.ops import seqffn

    ops = SC.make_operands((5, 13, 32, 96), _dev())
    out = seqffn.seq_ffn(ops[0].requires_grad_(True), *ops[1:-1])
    assert not seqffn._ENABLED and not _is_native(out)
    assert torch.equal(_bits(out), _bits(SC.seq_ffn_reference(*ops[:-1])))
    print("child: reference path taken")


def test_dispatch_and_operand_checks():
    from persia_amd.ops.seqffn import seq_ffn

    C = _native()
    B, L, D, F = case = (5, 13, 32, 96)
    ops, got = _run(case)
    g = ops[-1]
    # feasible f16 CUDA tensors: the kernels' bits through autograd
    leaves = [t.clone().requires_grad_(True) for t in ops[:-1]]
    out = seq_ffn(*leaves)
    assert _is_native(out)
    out.backward(g)
    for n, t in zip(SC.NAMES, (out, *(v.grad for v in leaves))):
        assert torch.equal(_bits(t), _bits(got[n])), n
    # infeasible shapes and CPU tensors: the reference
    for c in ((2, 5, 128, 64), (2, 5, 32, 48), (2, 5, 64, 288), None):
        assert c is None or not C.seq_ffn_feasible(*c[2:])
        args = SC.make_operands(c or case, _dev() if c else "cpu")[:-1]
        ref = seq_ffn(args[0].clone().requires_grad_(True), *args[1:])
        assert not _is_native(ref)
        assert torch.equal(_bits(ref), _bits(SC.seq_ffn_reference(*args)))
    x, a, Wo = ops[:3]
    for bad in ((x[0], a[0]) + ops[2:-1], (x, a[:, :L - 1]) + ops[2:-1],
                (x, a, Wo[:, :16]) + ops[3:-1], ops[:3] + (ops[3][:8],) + ops[4:-1]):
        with pytest.raises(ValueError):
            seq_ffn(*bad)
    # PA_SEQ_FFN=0 is read at import: a child process
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(tests_dir)
    code = ("import sys; sys.path[:0] = [r'%s', r'%s']; "
            "import test_gpu_seqffn_exact as T; T._child()" % (repo, tests_dir))
    child = subprocess.run([sys.executable, "-c", code], cwd=repo, text=True,
                           env=dict(os.environ, PA_SEQ_FFN="0"),
                           capture_output=True, timeout=300)
    assert child.returncode == 0 and "reference path taken" in child.stdout, \
        child.stdout[-2000:] + child.stderr[-2000:]
    # the launchers refuse: dtype, device, not contiguous, shapes, infeasible
    t = [w.half() if w.dim() == 2 else w for w in ops[:-1]]
    swap = lambda i, v: t[:i] + [v] + t[i + 1:]  # noqa: E731
    o128 = SC.make_operands((2, 5, 128, 64), _dev())
    bad = [swap(0, x.float()), swap(0, x.cpu()), swap(1, a[:B - 1].contiguous()),
           swap(0, x.transpose(0, 1).contiguous().transpose(0, 1)),
           swap(2, Wo), swap(2, t[2].t().contiguous().t()), swap(6, t[6][:64].contiguous()),
           swap(3, t[3].half()), swap(7, t[7].cpu()), swap(9, t[9][:16].contiguous()),
           [w.half() if w.dim() == 2 else w for w in o128[:-1]]]
    for args in bad:
        with pytest.raises(RuntimeError):
            C.seq_ffn_fwd(*args)
        with pytest.raises(RuntimeError):
            C.seq_ffn_bwd(torch.zeros_like(args[0], dtype=torch.float16), *args)
    for gx in (g.float(), g[:B - 1].contiguous(), g.cpu()):
        with pytest.raises(RuntimeError):
            C.seq_ffn_bwd(gx, *t)
    e = [x[:0], a[:0]] + t[2:]
    assert C.seq_ffn_fwd(*e).shape == (0, L, D + 1)
    empty = C.seq_ffn_bwd(g[:0], *e)
    assert empty[0].shape == empty[1].shape == (0, L, D + 1)
    assert [tuple(v.shape) for v in empty[2:]] == [tuple(v.shape) for v in t[2:]]
    assert not any(v.any() for v in empty[2:])
    torch.cuda.synchronize()


E2E_LENS = (6, 0, 2, 4, 5, 1)  # of the raw slot h: sfs 4 cuts 2 + 1 ids off


def _e2e(monkeypatch, native):
    """One TrainCtx step of SeqCTR(bst) over slots a (the query), c and h
    (raw, dim 32, sample_fixed_size 4)."""
    from persia_amd.core.schema import EmbeddingSchema, SlotConfig
    from persia_amd.ctx import TrainCtx
    from persia_amd.embedding.data import IDTypeFeature, Label, PersiaBatch
    from persia_amd.models import SeqCTR

    monkeypatch.setattr("persia_amd.ops.seqffn._ENABLED", native)  # the knob
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
                   attention="bst", heads=2, ffn=64).to(_dev())
    enc = model.sa_pools["2"].encoder
    cap = {"enc": enc}
    enc.register_forward_hook(lambda m, i, o: cap.update(seq=i[0].detach(), y=o))
    with TrainCtx(model=model, engine=eng, device_id=0, mixed_precision=False,
                  dense_optimizer=torch.optim.SGD(model.parameters(), lr=0.01)
                  ) as ctx:
        cap["state"] = {k: v.detach().cpu().double().clone()
                        for k, v in enc.state_dict().items()}
        tb = eng.process_batch(batch)
        logits, labels = ctx.forward(tb)
        ctx.backward(torch.nn.functional.binary_cross_entropy_with_logits(
            logits, labels[0].squeeze(1)))
        torch.cuda.synchronize()
    return cap


def test_train_ctx_seqctr_bst_native_against_reference(monkeypatch):
    from persia_amd.models import SeqEncoderLayer

    on, off = _e2e(monkeypatch, True), _e2e(monkeypatch, False)
    assert _is_native(on["y"]) and not _is_native(off["y"])
    assert torch.equal(_bits(on["seq"]), _bits(off["seq"]))
    assert on["seq"].shape == (6, 4, 33) and not on["seq"][1, :, 32].any()
    seq = on["seq"].cpu()
    layer = SeqEncoderLayer(32, 2, 64).double()
    layer.load_state_dict(on["state"])
    ref = layer(seq.double()).detach()
    sa = layer.self_attn
    a16 = seq_self_attn_reference(seq.float(), sa.in_proj_weight.float(),
                                     sa.in_proj_bias.float(), 2,
                                     operand_dtype=torch.float16)
    f32 = [p.float() for p in (
        sa.out_proj.weight, sa.out_proj.bias, layer.norm1.weight, layer.norm1.bias,
        layer.linear1.weight, layer.linear1.bias, layer.linear2.weight,
        layer.linear2.bias, layer.norm2.weight, layer.norm2.bias)]
    r16 = SC.seq_ffn_reference(seq.float(), a16.half().float(), *f32,
                               operand_dtype=torch.float16).detach()
    E16 = (r16.double() - ref).abs().max().item()
    for run in (on, off):
        _ratio(run["y"].detach(), ref.to(_dev()), _bound(ref, E16).to(_dev()),
               "e2e encoder-layer output")
