"""csrc/seqsal.hip against the f64 reference of tests/test_seqsal_cases_cpu.py
from the same input bits.  f16 results (out, dseq) must be within
2^-11 |ref| + 2^-25 + 4 * E16, f32 results (dWqkv, dbqkv) within 4 * E16,
where E16 is the error of the f32 reference with f16 operands on the CPU
(SL.e16); the 4 covers another summation order, __expf and the rounding of the
un-normalised probabilities.  Worst err/bound on an MI355X: out 0.59 at
(3, 64, 32, 1), dseq 0.72 at (2, 129, 64, 4), dWqkv 0.25 at (2, 65, 64, 2)
causal, dbqkv 0.26 at (3, 200, 64, 2) causal."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import test_seqsal_cases_cpu as SL
from test_gpu_dense_exact import _bits, _dev, _native, _ratio

pytestmark = pytest.mark.gpu
_node = lambda t: type(t.grad_fn).__name__  # noqa: E731


def _nodes(t):  # the names of every autograd node behind t
    seen, stack = set(), [t.grad_fn]
    while stack:
        f = stack.pop()
        if f is not None and f not in seen:
            seen.add(f)
            stack.extend(nf for nf, _ in f.next_functions)
    return {type(f).__name__ for f in seen}


def _kernels(ops, heads, causal, residual, max_blocks=0):
    seq, W, b, g = ops
    C, W16 = _native(), W.half()
    out, lse = C.seq_self_attn_long_fwd(seq, W16, b, heads, causal, residual,
                                        max_blocks)
    grads = C.seq_self_attn_long_bwd(g, seq, W16, b, lse, heads, causal, residual,
                                     max_blocks)
    return dict(zip(SL.NAMES, (out, *grads)), lse=lse)


@functools.lru_cache(maxsize=None)
def _run(case, causal):
    ops = SL.make_operands(case, _dev())
    return ops, _kernels(ops, case[3], causal, SL.residual_of(case),
                         2 if case == SL.BLOCKS else 0)


@pytest.mark.parametrize("case,causal", SL.PARAMS, ids=SL.IDS)
def test_native_within_bound_and_structure_bit_for_bit(case, causal):
    B, L, D, heads = case
    assert _native().seq_self_attn_long_feasible(L, D, heads)
    ops, got = _run(case, causal)
    ref, E = SL.reference(case, causal, torch.float64), SL.e16(case, causal)
    for n in SL.NAMES:
        r, f16 = ref[n].to(_dev()), n in ("out", "dseq")
        assert got[n].dtype == (torch.float16 if f16 else torch.float32)
        bound = (2.0 ** -11 * r.abs() + 2.0 ** -25 + 4 * E[n] if f16
                 else torch.full_like(r, 4 * E[n]))
        _ratio(got[n], r, bound, f"seq_self_attn_long {n} {case} causal={causal}")
    seq, out, dseq = ops[0], got["out"], got["dseq"]
    valid = seq[..., D] != 0
    assert not _bits(out[..., :D][~valid]).any()
    assert torch.equal(_bits(out[..., D]), _bits(seq[..., D]))
    assert not _bits(dseq[..., D]).any() and not _bits(dseq[~valid]).any()
    assert got["lse"].shape == (B, heads, L)
    # again; reversed; the first sample alone: the per-sample results keep
    # their bits, and so do the weight gradients of the same batch and grid
    everyone = torch.arange(B, device=_dev())
    for idx in (everyone, everyone.flip(0), everyone[:1]):
        sub = (ops[0][idx].contiguous(), ops[1], ops[2], ops[3][idx].contiguous())
        again = _kernels(sub, heads, causal, SL.residual_of(case),
                         2 if case == SL.BLOCKS else 0)
        for n in ("out", "dseq", "lse"):
            assert torch.equal(_bits(again[n]), _bits(got[n][idx])), n
        if idx is everyone:
            for n in ("dWqkv", "dbqkv"):
                assert torch.equal(_bits(again[n]), _bits(got[n])), n


def _child():  # PA_SEQ_SELF_ATTN_LONG=0 in the environment: the reference runs
    from persia_amd.ops import seqsal

    seq, W, b, _ = SL.make_operands(SL.CASES[0], _dev())
    out = seqsal.seq_self_attn_long(seq.requires_grad_(True), W, b, 2)
    assert not seqsal._ENABLED and _node(out) != "SeqSelfAttnLongFnBackward"
    assert torch.equal(_bits(out), _bits(SL.SC.seq_self_attn_reference(seq, W, b, 2)))
    print("child: reference path taken")


def test_dispatch_and_operand_checks():
    from persia_amd.models.din import SelfAttentionLayer, SeqEncoderLayer
    from persia_amd.ops.seqsa import seq_self_attn
    from persia_amd.ops.seqsal import seq_self_attn_long

    C, reference = _native(), SL.SC.seq_self_attn_reference
    B, L, D, heads = case = SL.CASES[0]
    assert case == (2, 65, 64, 2)
    res = SL.residual_of(case)
    ops, got = _run(case, True)
    seq, W, b, g = ops
    # feasible f16 CUDA tensors: the kernels' bits through autograd
    leaves = [t.clone().requires_grad_(True) for t in (seq, W, b)]
    out = seq_self_attn_long(*leaves, heads, causal=True, residual=res)
    assert _node(out) == "SeqSelfAttnLongFnBackward"
    out.backward(g)
    for n, t in zip(SL.NAMES, (out, *(x.grad for x in leaves))):
        assert torch.equal(_bits(t), _bits(got[n])), n
    # the models: the long kernels past 64 rows, the short ones up to them
    torch.manual_seed(5)
    enc = SeqEncoderLayer(64, 2, 64).to(_dev())
    for n, want in ((65, "SeqSelfAttnLongFnBackward"), (17, "SeqSelfAttnFnBackward")):
        x = seq[:, :n].contiguous()
        assert _node(SelfAttentionLayer(2)(x, *leaves[1:])) == want
        assert want in _nodes(enc(x)), n
    # seq_self_attn itself does not change at L = 65
    assert torch.equal(_bits(seq_self_attn(seq, W, b, heads, causal=True)),
                       _bits(reference(seq, W, b, heads, causal=True)))
    # infeasible shapes and CPU tensors: the reference
    for shape in ((5, 128, 4), (5, 48, 3), (5, 64, 8), (1025, 32, 1)):
        assert not C.seq_self_attn_long_feasible(*shape), shape
    assert C.seq_self_attn_long_feasible(1024, 64, 4)
    for c in ((2, 5, 128, 4), (2, 5, 48, 3), (2, 5, 64, 8), (1, 1025, 32, 1), None):
        args = (SL.SC.make_operands(c, _dev())[:3] + (c[3],) if c else
                tuple(t.cpu() for t in ops[:3]) + (heads,))
        ref = seq_self_attn_long(args[0].clone().requires_grad_(True), *args[1:],
                                 causal=True)
        assert _node(ref) != "SeqSelfAttnLongFnBackward"
        assert torch.equal(_bits(ref), _bits(reference(*args, causal=True)))
    for bad in ((seq, W, b, 5), (seq, W[:, :32], b, heads), (seq[0], W, b, heads)):
        with pytest.raises(ValueError):
            seq_self_attn_long(*bad)
    # PA_SEQ_SELF_ATTN_LONG=0 is read at import: a child process
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(tests_dir)
    code = ("import sys; sys.path[:0] = [r'%s', r'%s']; "
            "import test_gpu_seqsal_exact as T; T._child()" % (repo, tests_dir))
    child = subprocess.run([sys.executable, "-c", code], cwd=repo, text=True,
                           env=dict(os.environ, PA_SEQ_SELF_ATTN_LONG="0"),
                           capture_output=True, timeout=300)
    assert child.returncode == 0 and "reference path taken" in child.stdout, \
        child.stdout[-2000:] + child.stderr[-2000:]
    # the launchers refuse: dtype, device, not contiguous, lse's shape
    W16, lse = W.half(), got["lse"]
    bad = [(seq.float(), W16, b, heads), (seq.cpu(), W16, b, heads),
           (seq, W, b, heads),
           (seq.transpose(0, 1).contiguous().transpose(0, 1), W16, b, heads),
           (seq, W16, b, 8)]
    for args in bad:
        with pytest.raises(RuntimeError):
            C.seq_self_attn_long_fwd(*args)
        with pytest.raises(RuntimeError):
            C.seq_self_attn_long_bwd(g, *args[:3], lse, args[3])
    for gx, lx in ((g.float(), lse), (g, lse[:, :1].contiguous()), (g, lse.half()),
                   (g, lse.transpose(1, 2).contiguous().transpose(1, 2))):
        with pytest.raises(RuntimeError):
            C.seq_self_attn_long_bwd(gx, seq, W16, b, lx, heads)
    out0, lse0 = C.seq_self_attn_long_fwd(seq[:0], W16, b, heads)
    assert out0.shape == (0, L, D + 1) and lse0.shape == (0, heads, L)
    empty = C.seq_self_attn_long_bwd(g[:0], seq[:0], W16, b, lse0, heads)
    assert empty[0].shape == (0, L, D + 1) and empty[1].shape == (3 * D, D)
    assert not empty[1].any() and not empty[2].any()
    torch.cuda.synchronize()
