"""Cases and references of tests/test_gpu_seqsal_exact.py, and the checks of
them that need no GPU.  `reference` and `e16` are test_seqsa_cases_cpu's, over
this file's cases: `seq_self_attn_reference` (what csrc/seqsal.hip computes)
forward and backward from one set of input bits, and the max abs difference
per tensor between its f32 run with f16 operands and its f64 run."""
import functools

import pytest
import torch

import test_seqsa_cases_cpu as SC

# (B, L, D, heads): one row in the second tile (the shape seqsa.hip refuses);
# exactly one tile, dh 32; dh 16 and one full strip in the second tile; three
# tiles, the last of one row; the benchmark's L; several items per block
# (max_blocks = 2 on the GPU); key tiles without a valid row
HOLES = (3, 150, 32, 2)
BLOCKS = (5, 17, 32, 2)
CASES = [(2, 65, 64, 2), (3, 64, 32, 1), (2, 80, 32, 2), (2, 129, 64, 4),
         (3, 200, 64, 2), BLOCKS, HOLES]
PARAMS = [(c, causal) for c in CASES for causal in (False, True)]
IDS = ["x".join(map(str, c)) + ("-causal" if causal else "") for c, causal in PARAMS]
NAMES = SC.NAMES


def residual_of(case):  # alternates by case
    return CASES.index(case) % 2 == 1


def make_operands(case, device="cpu"):
    seq, W, b, g = SC.make_operands(case)
    if case == HOLES:  # sample 0: no valid row in its leading key tile;
        B, L, D, _ = case  # sample 1: none in its middle one; sample 2: none
        l = torch.arange(L)
        third = l % 3 == 1
        seq[0, :, D] = (third & (l >= 64)).half()
        seq[1, :, D] = (third & ~((l >= 64) & (l < 128))).half()
        seq[2, :, D] = 0
        g = torch.nan_to_num(g, nan=0.25)
        g[..., D] = float("nan")
        g[seq[..., D] == 0] = float("nan")
    return tuple(t.to(device) for t in (seq, W, b, g))


@functools.lru_cache(maxsize=None)
def reference(case, causal, dtype, operand_dtype=None):
    return SC.run_reference(make_operands(case), case[3], causal,
                            residual_of(case), dtype, operand_dtype)


@functools.lru_cache(maxsize=None)
def e16(case, causal):
    r16 = reference(case, causal, torch.float32, torch.float16)
    r64 = reference(case, causal, torch.float64)
    return {n: (r16[n].double() - r64[n]).abs().max().item() for n in NAMES}


@pytest.mark.parametrize("case,causal", PARAMS, ids=IDS)
def test_invalid_rows_reach_nothing(case, causal):
    B, L, D, heads = case
    ops = make_operands(case)
    seq = ops[0]
    valid = seq[..., D] != 0
    if case == HOLES:
        assert not valid[0, :64].any() and valid[0, 64:].any()
        assert valid[1, :64].any() and not valid[1, 64:128].any()
        assert valid[1, 128:].any() and not valid[2].any()
    r64, E = reference(case, causal, torch.float64), e16(case, causal)
    for n in NAMES:
        assert torch.isfinite(r64[n]).all(), n
        print(f"{n} {case} causal={causal}: E16 {E[n]:.3g} of max "
              f"{r64[n].abs().max():.3g}")
    poisoned = seq.clone()  # NaN in every invalid row: the same bits
    poisoned[..., :D][~valid] = float("nan")
    again = SC.run_reference((poisoned,) + ops[1:], heads, causal,
                             residual_of(case), torch.float64)
    for n in NAMES:
        assert torch.equal(again[n], r64[n]), n
