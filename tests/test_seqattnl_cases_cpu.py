"""Cases, f64 reference and bound of tests/test_gpu_seqattnl_exact.py, and the
checks of them that need no GPU.

The f64 reference is `seqattn_model`'s (tests/test_seqattn_cases_cpu.py).  An
f16 result must be within 2^-11 |ref| + 2^-25 + 4 * E32, where E32 is the
largest absolute error, per output tensor and case, of `seq_attn_pool_reference`
run in float32 on the CPU against that reference -- measured here and never on
the kernels; the 4 covers another summation order (chunks, waves, the online
rescaling) and __expf."""
import functools

import pytest
import torch

import test_seqattn_cases_cpu as SC
from persia_amd.ops.reference import seq_attn_pool_reference
from persia_amd.ops.seqattnl import seq_attn_pool_long

# (B, L, D), chunks of 64 / 32 / 16 rows for D <= 64 / 128 / 256: a single
# row; one row into the second chunk; wave 0 gets a second chunk; the shape
# seqattn.hip refuses; refused, the smallest chunk; the limit; a 9-half row
# pitch over many chunks; scores beyond +-50; seq one half into its storage
BIG_SCORES = (3, 200, 64)
OFFSET_VIEW = (2, 130, 64)
CASES = [(1, 1, 8), (3, 65, 64), (3, 257, 64), (2, 300, 128), (2, 130, 256),
         (1, 1024, 64), (2, 1024, 8), BIG_SCORES, OFFSET_VIEW]
IDS = ["x".join(map(str, c)) for c in CASES]
NAMES = ("out", "dq", "dseq")


def case_scale(case):
    return (80.0 if case == BIG_SCORES else 1.0) * case[2] ** -0.5


def last_quarter(case):  # cases whose sample 1 is valid in its last rows only
    return case[0] >= 3 and case[1] >= 65


def make_case(case, device="cpu"):
    """`SC.make_case`; with `last_quarter` sample 1 loses every valid row
    before its last quarter, so whole leading chunks -- and whole waves --
    meet none."""
    B, L, D = case
    q, seq, g = SC.make_case(case)
    if last_quarter(case):
        seq[1, :L - L // 4, D] = 0.0
    flat = seq.reshape(-1)
    if case == OFFSET_VIEW:
        flat = torch.cat([flat[:1], flat]).to(device)[1:]
        assert flat.data_ptr() % 4 == 2
    return q.to(device), flat.to(device).view(B, L, D + 1), g.to(device)


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> {name: (f64 reference, bound)} on the CPU."""
    q, seq, g = make_case(case)
    scale = case_scale(case)
    mdl = SC.seqattn_model(q, seq, g, scale)
    r32 = SC._run_reference(q, seq, g, scale, torch.float32)
    res = {}
    for n, t in zip(NAMES, r32):
        ref = mdl[n][0]
        e32 = (t.double() - ref).abs().max().item()
        res[n] = (ref, 2.0 ** -11 * ref.abs() + 2.0 ** -25 + 4 * e32)
    return res


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_and_f32_reference_within_bound(case):
    (B, L, D), scale = case, case_scale(case)
    q, seq, g = make_case(case)
    valid = seq[..., D] != 0
    if last_quarter(case):
        assert not valid[1, :L - L // 4].any() and valid[1, L - L // 4:].any()
    if B > 1:
        assert not valid[B - 1].any()
    if case == BIG_SCORES:
        s = scale * (seq[..., :D].double() * q.double().unsqueeze(1)).sum(-1)
        # +54.7 and -57.7 with make_case's seed; 100 apart within sample 0
        assert s[valid].max() > 50 and s[valid].min() < -50
        assert s[0][valid[0]].max() - s[0][valid[0]].min() > 88  # e^-88 < 2^-126
    # the f32 reference stored to f16: E32 and one f16 rounding
    got = SC._run_reference(q, seq, g, scale, torch.float16)
    for n, t in zip(NAMES, got):
        ref, bound = reference(case)[n]
        assert t.dtype == torch.float16 and torch.isfinite(ref).all()
        SC.worst_ratio(t, ref, bound, f"f32 reference {n} {case}")
    # on CPU tensors the long op is the reference, bit for bit
    qa = q.clone().requires_grad_(True)
    out = seq_attn_pool_long(qa, seq, scale)
    assert torch.equal(out.view(torch.int16), got[0].view(torch.int16))


def test_target_attention_pool_on_cpu_is_the_reference():
    from persia_amd.models import TargetAttentionPool

    q, seq, _ = make_case((2, 300, 128))
    assert torch.equal(
        TargetAttentionPool()(q, seq).view(torch.int16),
        seq_attn_pool_reference(q, seq).view(torch.int16))
    with pytest.raises(ValueError):
        seq_attn_pool_long(q[:, :64], seq)
