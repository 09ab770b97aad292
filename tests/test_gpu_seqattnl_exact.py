"""csrc/seqattnl.hip against the f64 reference of
tests/test_seqattnl_cases_cpu.py from the same input bits: every f16 result
within 2^-11 |ref| + 2^-25 + 4 * E32 (cases, reference and bound are there;
nothing here is an atol).  Worst err/bound on an MI355X: out 0.961 at
(3, 65, 64), dq 0.965 at (2, 130, 256), dseq 0.975 at (3, 257, 64) -- the f16
store's half ulp dominates, as for the f32 reference on the CPU (0.961, 0.964,
0.975)."""
import functools

import pytest
import torch

import test_seqattnl_cases_cpu as LC
from test_gpu_dense_exact import _bits, _dev, _native, _ratio

pytestmark = pytest.mark.gpu
_node = lambda t: type(t.grad_fn).__name__  # noqa: E731
LONG, SHORT = "SeqAttnPoolLongFnBackward", "SeqAttnPoolFnBackward"


def _kernels(q, seq, g, scale):
    C = _native()
    return (C.seq_attn_long_fwd(q, seq, scale),
            *C.seq_attn_long_bwd(g, q, seq, scale))


@functools.lru_cache(maxsize=None)
def _run(case):
    q, seq, g = LC.make_case(case, _dev())
    return (q, seq, g) + _kernels(q, seq, g, LC.case_scale(case))


@pytest.mark.parametrize("case", LC.CASES, ids=LC.IDS)
def test_native_within_bound_and_structure_bit_for_bit(case):
    (B, L, D), scale = case, LC.case_scale(case)
    assert _native().seq_attn_long_feasible(L, D)
    q, seq, g, *got = _run(case)
    for name, t in zip(LC.NAMES, got):
        ref, bound = (x.to(_dev()) for x in LC.reference(case)[name])
        assert t.dtype == torch.float16
        _ratio(t, ref, bound, f"seq_attn_long {name} {case}")
    out, dq, dseq = got
    valid = seq[..., D] != 0
    assert not _bits(dseq[..., D]).any() and not _bits(dseq[~valid]).any()
    if B > 1:  # the last sample has no valid row: +0, not -0
        assert not valid[B - 1].any()
        assert not _bits(out[B - 1]).any() and not _bits(dq[B - 1]).any()
    # again; in reverse order; the first sample alone (B = 1): the same bits
    everyone = torch.arange(B, device=_dev())
    for idx in (everyone, everyone.flip(0), everyone[:1]):
        again = _kernels(*(t[idx].contiguous() for t in (q, seq, g)), scale)
        for name, a, b in zip(LC.NAMES, again, got):
            assert torch.equal(_bits(a), _bits(b[idx])), (name, idx.tolist())


def test_dispatch_and_operand_checks(monkeypatch):
    from persia_amd.models import SelfAttentionPool, TargetAttentionPool
    from persia_amd.ops.seqattn import seq_attn_pool
    from persia_amd.ops.seqattnl import prefers_long, seq_attn_pool_long

    C, reference = _native(), LC.seq_attn_pool_reference
    B, L, D = case = (2, 300, 128)
    q, seq, g, *got = _run(case)
    # feasible f16 CUDA tensors: the kernels' bits through autograd
    qa, sa = q.clone().requires_grad_(True), seq.clone().requires_grad_(True)
    pooled = seq_attn_pool_long(qa, sa)
    pooled.backward(g)
    assert _node(pooled) == LONG
    for a, b in zip((pooled, qa.grad, sa.grad), got):
        assert torch.equal(_bits(a), _bits(b))
    # the models: the long kernels where the short one has none, else the short
    assert not C.seq_attn_feasible(L, D) and not C.seq_attn_feasible(512, 64)
    via = TargetAttentionPool()(qa, sa)
    assert _node(via) == LONG and torch.equal(_bits(via), _bits(got[0]))
    assert prefers_long(200, 64) and not prefers_long(50, 64)  # as measured
    qs, ss, _ = LC.SC.make_case((33, 50, 40), _dev())
    short = TargetAttentionPool()(qs.requires_grad_(True), ss)
    assert _node(short) == SHORT
    assert torch.equal(_bits(short), _bits(seq_attn_pool(qs, ss)))
    torch.manual_seed(5)
    ql, sl, _ = LC.SC.make_case((2, 512, 64), _dev())
    assert _node(SelfAttentionPool(64, heads=2).to(_dev())(ql, sl)) == LONG
    # the reference: CPU tensors, D % 8 != 0, L past 1024, the knob off
    assert not C.seq_attn_long_feasible(5, 12)
    assert not C.seq_attn_long_feasible(1025, 8)
    assert not C.seq_attn_long_feasible(5, 264)
    assert C.seq_attn_long_feasible(1024, 256)
    q12, s12, _ = LC.SC.make_case((2, 5, 12), _dev())
    q1025, s1025, _ = LC.SC.make_case((1, 1025, 8), _dev())
    for qx, sx in ((q.cpu(), seq.cpu()), (q12, s12), (q1025, s1025)):
        ref = seq_attn_pool_long(qx.clone().requires_grad_(True), sx)
        assert _node(ref) != LONG
        assert torch.equal(_bits(ref), _bits(reference(qx, sx)))
    monkeypatch.setattr("persia_amd.ops.seqattnl._ENABLED", False)  # the knob
    off = seq_attn_pool_long(qa, sa)
    assert _node(off) != LONG and torch.equal(_bits(off), _bits(reference(q, seq)))
    # the launchers refuse: dtype, device, not contiguous, shapes, infeasible
    bad = [(q.float(), seq, g), (q, seq.float(), g), (q.cpu(), seq, g),
           (q.t().contiguous().t(), seq, g), (q[:, :D - 8].contiguous(), seq, g),
           (q, seq.transpose(0, 1).contiguous().transpose(0, 1), g),
           (q[:B - 1].contiguous(), seq, g), (q12, s12, q12),
           (q1025, s1025, q1025)]
    for qx, sx, gx in bad:
        with pytest.raises(RuntimeError):
            C.seq_attn_long_fwd(qx, sx, 1.0)
        with pytest.raises(RuntimeError):
            C.seq_attn_long_bwd(gx, qx, sx, 1.0)
    for gx in (g.float(), g.t().contiguous().t(), g[:B - 1].contiguous()):
        with pytest.raises(RuntimeError):
            C.seq_attn_long_bwd(gx, q, seq, 1.0)
    assert C.seq_attn_long_fwd(q[:0], seq[:0], 1.0).shape == (0, D)
    dq0, ds0 = C.seq_attn_long_bwd(g[:0], q[:0], seq[:0], 1.0)
    assert dq0.shape == (0, D) and ds0.shape == (0, L, D + 1)
    torch.cuda.synchronize()
