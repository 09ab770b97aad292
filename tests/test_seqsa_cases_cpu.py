"""Cases and references of tests/test_gpu_seqsa_exact.py, and the checks of
them that need no GPU.

`reference(case, causal, dtype, operand_dtype)` runs `seq_self_attn_reference`
(what csrc/seqsa.hip computes) forward and backward from one set of input
bits; `e16(case, causal)` is the max abs difference per tensor between its f32
run with f16 operands (the kernels' approximation, emulated) and its f64 run
without -- the E16 of the GPU test's bounds, measured here on the CPU and never
on the kernels."""
import functools

import pytest
import torch
import torch.nn.functional as F

from persia_amd.ops.reference import seq_self_attn_reference
from test_seqattn_cases_cpu import make_case

# (B, L, D, heads): one row; dh 16 and less than a strip; the strip boundary
# from both sides; all four strips; an odd number of strips; several samples
# per block (max_blocks = 2 on the GPU); a mask with regular holes
HOLES = (4, 12, 32, 2)  # valid at l % 3 == 1 only, the last sample empty
BLOCKS = (9, 5, 32, 2)
CASES = [(1, 1, 32, 1), (5, 3, 32, 2), (3, 16, 64, 4), (2, 17, 64, 2),
         (3, 64, 64, 2), (2, 33, 32, 1), BLOCKS, HOLES]
PARAMS = [(c, causal) for c in CASES for causal in (False, True)]
IDS = ["x".join(map(str, c)) + ("-causal" if causal else "") for c, causal in PARAMS]
NAMES = ("out", "dseq", "dWqkv", "dbqkv")


def residual_of(case):  # alternates by case
    return CASES.index(case) % 2 == 1


def make_operands(case, device="cpu"):
    """-> seq f16, Wqkv, bqkv f32 (weights ~ 1/sqrt(D)), g_out f16 (its mask
    channel and its invalid rows NaN: never read)."""
    B, L, D, heads = case
    seq = make_case((B, L, D))[1]
    if case == HOLES:
        seq[..., D] = (torch.arange(L) % 3 == 1).half()
        seq[B - 1, :, D] = 0
        seq[0, 1, :D] = 0.25  # make_case's Inf / NaN row is valid here
    gen = torch.Generator().manual_seed(((B * 1009 + L) * 1009 + D) * 1009 + heads)
    W = torch.randn(3 * D, D, generator=gen) * D ** -0.5
    b = torch.randn(3 * D, generator=gen) * 0.1
    g = (torch.randn(B, L, D + 1, generator=gen) * 0.5).half()
    g[..., D] = float("nan")
    g[seq[..., D] == 0] = float("nan")
    return tuple(t.to(device) for t in (seq, W, b, g))


def run_reference(ops, heads, causal, residual, dtype, operand_dtype=None):
    """-> {name: tensor} of NAMES in `dtype`."""
    seq, W, b, g = ops
    leaves = [t.to(dtype).requires_grad_(True) for t in (seq, W, b)]
    out = seq_self_attn_reference(*leaves, heads, causal, residual, operand_dtype)
    # the invalid rows and channel D of g reach nothing: any finite value
    out.backward(torch.nan_to_num(g.to(dtype), nan=1.0))
    return dict(zip(NAMES, [out.detach()] + [t.grad for t in leaves]))


@functools.lru_cache(maxsize=None)
def reference(case, causal, dtype, operand_dtype=None):
    return run_reference(make_operands(case), case[3], causal, residual_of(case),
                         dtype, operand_dtype)


@functools.lru_cache(maxsize=None)
def e16(case, causal):
    r16 = reference(case, causal, torch.float32, torch.float16)
    r64 = reference(case, causal, torch.float64)
    return {n: (r16[n].double() - r64[n]).abs().max().item() for n in NAMES}


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", [(5, 3, 32, 2), (2, 17, 64, 2)], ids=str)
def test_f64_reference_is_sdpa_on_a_full_mask(case, causal):
    B, L, D, heads = case
    seq, W, b, g = make_operands(case)
    seq = torch.where(torch.isfinite(seq), seq, torch.zeros_like(seq))
    seq[..., D] = 1
    g = torch.nan_to_num(g, nan=1.0)
    got = run_reference((seq, W, b, g), heads, causal, False, torch.float64)
    x = seq[..., :D].double().requires_grad_(True)
    W64, b64 = (t.double().requires_grad_(True) for t in (W.half(), b))
    q, k, v = ((x @ W64.t() + b64).reshape(B, L, 3, heads, D // heads)
               .permute(2, 0, 3, 1, 4))
    o = F.scaled_dot_product_attention(q, k, v, is_causal=causal)
    o = o.transpose(1, 2).reshape(B, L, D)
    o.backward(g[..., :D].double())
    want = (o, x.grad, W64.grad, b64.grad)
    for n, w in zip(NAMES, want):
        t = got[n][..., :D] if n in ("out", "dseq") else got[n]
        assert (t - w.detach()).abs().max() <= 1e-10, n


@pytest.mark.parametrize("case,causal", PARAMS, ids=IDS)
def test_invalid_rows_reach_nothing(case, causal):
    B, L, D, heads = case
    ops = make_operands(case)
    seq = ops[0]
    valid = seq[..., D] != 0
    r64, E = reference(case, causal, torch.float64), e16(case, causal)
    for n in NAMES:
        assert torch.isfinite(r64[n]).all(), n
        print(f"{n} {case} causal={causal}: E16 {E[n]:.3g} of max "
              f"{r64[n].abs().max():.3g}")
    # NaN in every invalid row: the same bits
    poisoned = seq.clone()
    poisoned[..., :D][~valid] = float("nan")
    again = run_reference((poisoned,) + ops[1:], heads, causal, residual_of(case),
                          torch.float64)
    for n in NAMES:
        assert torch.equal(again[n], r64[n]), n
    out, dseq = r64["out"], r64["dseq"]
    assert not dseq[..., D].any() and not dseq[~valid].any()
    assert not out[..., :D][~valid].any()
    assert torch.equal(out[..., D], seq[..., D].double())
    if B > 1:  # the sample without a valid row
        assert not valid[B - 1].any() and not out[B - 1].any()
    if case == HOLES:
        assert not valid[:, 0].any() and not valid[:, L - 1].any() and valid[0, 1]


def test_seqctr_self_attention_runs_on_cpu():
    from persia_amd.models import SelfAttentionPool, SeqCTR

    torch.manual_seed(3)
    q, seq, _ = make_case((6, 4, 8))
    embs = [e.requires_grad_(True) for e in (q, seq, torch.randn(6, 16).half())]
    model = SeqCTR(dims=[8, 8, 16], seq_query={1: 0}, num_dense=5, hidden=(32,),
                   attention="self", heads=2)
    pool = model.sa_pools["1"]
    assert isinstance(pool, SelfAttentionPool) and pool.heads == 2
    mha = torch.nn.MultiheadAttention(8, 2)
    assert pool.in_proj_weight.shape == mha.in_proj_weight.shape
    assert pool.in_proj_bias.shape == mha.in_proj_bias.shape
    with torch.no_grad():
        pool.in_proj_bias.uniform_(-0.1, 0.1)
    logits = model([torch.randn(6, 5)], embs)
    assert logits.shape == (6,) and logits.dtype == torch.float32
    logits.sum().backward()
    assert all(torch.isfinite(e.grad).all() and e.grad.any() for e in embs)
    assert not embs[1].grad[5].any()  # the sample without a valid cell
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.any()
               for p in pool.parameters())
