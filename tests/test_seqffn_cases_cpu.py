"""Cases and references of tests/test_gpu_seqffn_exact.py, and the checks of
them that need no GPU.

`reference(case, dtype, operand_dtype)` runs `seq_ffn_reference` (what
csrc/seqffn.hip computes) forward and backward from one set of input bits;
`e16(case)` is the max abs difference per tensor between its f32 run with f16
operands (the kernels' approximation, emulated) and its f64 run without -- the
E16 of the GPU test's bounds, measured here on the CPU and never on the
kernels."""
import functools

import pytest
import torch

from persia_amd.ops.reference import seq_ffn_reference

# (B, L, D, F): one row, one hidden chunk; 21 rows (a strip boundary inside a
# tile, the widest F); 65 rows (one row into a second tile, F no power of two);
# 196 rows over 2 blocks (max_blocks = 2 on the GPU); wholly invalid strips
BLOCKS, SKIP = (7, 28, 64, 64), (3, 48, 64, 128)
CASES = [(1, 1, 32, 32), (3, 7, 64, 256), (5, 13, 32, 96), BLOCKS, SKIP]
IDS = ["x".join(map(str, c)) for c in CASES]
PARAMS = ("Wo", "bo", "g1", "be1", "W1", "b1", "W2", "b2", "g2", "be2")
NAMES = ("out", "dx", "da") + tuple("d" + n for n in PARAMS)


def make_operands(case, device="cpu"):
    """-> x, a f16, the ten f32 parameters, g_out f16.  Lengths are ragged, the
    last sample of a batch (and the middle one of SKIP) has no valid row;
    invalid rows of x, a, g and channel D of a and g are NaN / Inf."""
    B, L, D, F = case
    gen = torch.Generator().manual_seed(((B * 1009 + L) * 1009 + D) * 1009 + F)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    if B > 1:
        lens[B - 1] = 0
    if case == SKIP:
        lens[0], lens[1] = L, 0
    valid = torch.arange(L)[None, :] < lens[:, None]
    x, a, g = ((torch.randn(B, L, D + 1, generator=gen) * 0.5).half()
               for _ in range(3))
    for t, junk in ((x, float("nan")), (a, float("inf")), (g, float("nan"))):
        t[~valid] = junk
        t[..., D] = junk
    x[..., D] = valid.half()
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    par = dict(Wo=r(D, D) * D ** -0.5, bo=r(D) * 0.1, g1=1 + r(D) * 0.1,
               be1=r(D) * 0.1, W1=r(F, D) * D ** -0.5, b1=r(F) * 0.1,
               W2=r(D, F) * F ** -0.5, b2=r(D) * 0.1, g2=1 + r(D) * 0.1,
               be2=r(D) * 0.1)
    return tuple(t.to(device) for t in (x, a, *(par[n] for n in PARAMS), g))


def run_reference(ops, dtype, operand_dtype=None):
    """-> {name: tensor} of NAMES in `dtype`."""
    leaves = [t.to(dtype).requires_grad_(True) for t in ops[:-1]]
    out = seq_ffn_reference(*leaves, operand_dtype=operand_dtype)
    # the invalid rows and channel D of g reach nothing: any finite value
    out.backward(torch.nan_to_num(ops[-1].to(dtype), nan=1.0))
    return dict(zip(NAMES, [out.detach()] + [t.grad for t in leaves]))


@functools.lru_cache(maxsize=None)
def reference(case, dtype, operand_dtype=None):
    return run_reference(make_operands(case), dtype, operand_dtype)


@functools.lru_cache(maxsize=None)
def e16(case):
    r16, r64 = reference(case, torch.float32, torch.float16), reference(case, torch.float64)
    return {n: (r16[n].double() - r64[n]).abs().max().item() for n in NAMES}


@pytest.mark.parametrize("causal", [False, True])
def test_encoder_layer_loads_a_torch_state_dict(causal):
    from persia_amd.models import SeqEncoderLayer

    B, L, D, heads, F = 3, 6, 16, 2, 32
    torch.manual_seed(5)
    ref = torch.nn.TransformerEncoderLayer(D, heads, F, dropout=0.0,
                                           batch_first=True).double().train()
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() == 1:
                p.uniform_(-0.5, 0.5)  # the zero biases too
            else:
                p.copy_(p.half().double())  # f16-representable matrices
    layer = SeqEncoderLayer(D, heads, F, causal).double()
    layer.load_state_dict(ref.state_dict())
    valid = torch.arange(L)[None, :] < torch.tensor([L, 4, 1])[:, None]
    seq = torch.cat([torch.randn(B, L, D).double(), valid.double()[..., None]], 2)
    want = ref(seq[..., :D], src_key_padding_mask=~valid,
               src_mask=torch.ones(L, L, dtype=torch.bool).triu(1) if causal else None)
    got = layer(seq)
    assert (got[..., :D][valid] - want[valid]).abs().max() <= 1e-12
    assert torch.equal(got[..., D], seq[..., D])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_invalid_rows_reach_nothing(case):
    B, L, D, F = case
    ops = make_operands(case)
    valid = ops[0][..., D] != 0
    r64, E = reference(case, torch.float64), e16(case)
    for n in NAMES:
        assert torch.isfinite(r64[n]).all(), n
        print(f"{n} {case}: E16 {E[n]:.3g} of max {r64[n].abs().max():.3g}")
    for n in ("out", "dx", "da"):
        assert not r64[n][~valid].any() and (n == "out" or not r64[n][..., D].any())
    assert torch.equal(r64["out"][..., D], ops[0][..., D].double())
    assert not valid[B - 1].any() or B == 1
    # other junk in the invalid rows: the same bits
    other = [t.clone() for t in ops]
    other[0][..., :D][~valid], other[1][~valid], other[-1][~valid] = 3.0, float("nan"), 2.0
    again = run_reference(other, torch.float64)
    assert all(torch.equal(again[n], r64[n]) for n in NAMES)


def test_reference_gradcheck():
    """In the rows, a and the vectors; the matrices' gradients pass straight
    through a rounding, which no difference quotient sees."""
    D, ops = 4, make_operands((2, 3, 4, 8))
    x, a = (torch.nan_to_num(t.double(), 0.0, 0.0, 0.0) for t in ops[:2])
    mask = x[..., D:].clone()
    leaves = [t.double().requires_grad_(t.dim() == 1) for t in ops[2:-1]]
    rows = [x[..., :D].requires_grad_(True), a.requires_grad_(True)]

    def fn(xr, a, *par):
        return seq_ffn_reference(torch.cat([xr, mask], -1), a, *par)[..., :D]

    assert mask.sum() >= 1 and not mask[1].any()
    assert torch.autograd.gradcheck(fn, rows + leaves, eps=1e-6, atol=1e-6)


def test_seqctr_bst_runs_on_cpu():
    from persia_amd.models import SeqCTR, SeqEncoderLayer
    from test_seqattn_cases_cpu import make_case

    torch.manual_seed(3)
    q, seq, _ = make_case((6, 4, 8))
    embs = [e.requires_grad_(True) for e in (q, seq, torch.randn(6, 16).half())]
    model = SeqCTR(dims=[8, 8, 16], seq_query={1: 0}, num_dense=5, hidden=(32,),
                   attention="bst", heads=2)
    enc = model.sa_pools["1"].encoder
    assert isinstance(enc, SeqEncoderLayer) and enc.ffn == 32
    logits = model([torch.randn(6, 5)], embs)
    logits.sum().backward()
    assert torch.isfinite(logits).all() and not embs[1].grad[5].any()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in enc.parameters())
