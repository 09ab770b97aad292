"""Cases and references of tests/test_gpu_seqgru_exact.py, and the checks of
them that need no GPU.

`reference(case, att, dtype)` runs `seq_gru_reference` (what csrc/seqgru.hip
computes) forward and backward, with gradients for both outputs, from one set
of input bits; `e16(case, att)` is the max abs difference per tensor between
its f32 run with f16 state operands (the kernels' approximation, emulated) and
its f64 run without -- the E16 of the GPU test's bounds, measured here on the
CPU and never on the kernels."""
import functools

import pytest
import torch

from persia_amd.ops.reference import seq_gru_reference
from test_seqattn_cases_cpu import make_case

# one row; one chunk; a sample-tile and a chunk boundary (8 steps, 4 at D =
# 128); three tiles and four waves; several K-steps; a mask with regular holes
HOLES = (4, 12, 32, 32)  # valid at t % 3 == 1 only: t = 0 and t = L-1 are not
CASES = [(1, 1, 32, 32), (5, 3, 32, 32), (17, 9, 64, 32), (33, 17, 32, 64),
         (3, 40, 64, 64), (2, 20, 128, 64), HOLES]  # (B, L, D, H)
PARAMS = [(c, a) for c in CASES for a in (False, True)]
IDS = ["x".join(map(str, c)) + ("-att" if a else "") for c, a in PARAMS]
NAMES = ("states", "last", "dseq", "dWx", "dWh", "dbx", "dbh", "datt")


def make_operands(case, att, device="cpu"):
    """-> seq f16, Wx, Wh, bx, bh f32 (weights ~ 0.5/sqrt(fan_in)), att f32 in
    (0, 1) with NaN at the invalid rows (or None), g_states, g_last f16."""
    B, L, D, H = case
    seq = make_case((B, L, D))[1]
    if case == HOLES:
        seq[..., D] = (torch.arange(L) % 3 == 1).half()
        seq[B - 1, :, D] = 0
        seq[0, 1, :D] = 0.25  # make_case's Inf / NaN row is valid here
    gen = torch.Generator().manual_seed(((B * 1009 + L) * 1009 + D) * 1009 + H)
    Wx = torch.randn(3 * H, D, generator=gen) * (0.5 * D ** -0.5)
    Wh = torch.randn(3 * H, H, generator=gen) * (0.5 * H ** -0.5)
    bx, bh = (torch.randn(3 * H, generator=gen) * 0.1 for _ in range(2))
    a = torch.rand(B, L, generator=gen) * 0.98 + 0.01
    a[seq[..., D] == 0] = float("nan")
    gs, gl = ((torch.randn(*s, generator=gen) * 0.5).half()
              for s in ((B, L, H), (B, H)))
    ops = (seq, Wx, Wh, bx, bh, a if att else None, gs, gl)
    return tuple(t if t is None else t.to(device) for t in ops)


def run_reference(ops, dtype, operand_dtype=None):
    """-> {name: tensor} of NAMES (datt None without att), in `dtype`."""
    *ins, gs, gl = ops
    leaves = [t if t is None else t.to(dtype).requires_grad_(True) for t in ins]
    states, last = seq_gru_reference(*leaves, operand_dtype=operand_dtype)
    torch.autograd.backward([states, last], [gs.to(dtype), gl.to(dtype)])
    grads = [leaves[i].grad for i in (0, 1, 2, 3, 4)]
    datt = None if leaves[5] is None else leaves[5].grad
    return dict(zip(NAMES, [states.detach(), last.detach(), *grads, datt]))


@functools.lru_cache(maxsize=None)
def reference(case, att, dtype, operand_dtype=None):
    return run_reference(make_operands(case, att), dtype, operand_dtype)


@functools.lru_cache(maxsize=None)
def e16(case, att):
    r16 = reference(case, att, torch.float32, torch.float16)
    r64 = reference(case, att, torch.float64)
    return {n: (r16[n].double() - r64[n]).abs().max().item()
            for n in NAMES if r64[n] is not None}


@pytest.mark.parametrize("case", [(5, 3, 32, 32), (3, 40, 64, 64)], ids=str)
def test_f64_reference_is_torch_gru_on_a_full_mask(case):
    B, L, D, H = case
    seq, Wx, Wh, bx, bh, _, gs, gl = make_operands(case, False)
    seq = torch.where(torch.isfinite(seq), seq, torch.zeros_like(seq))
    seq[..., D] = 1
    got = run_reference((seq, Wx, Wh, bx, bh, None, gs, gl), torch.float64)
    gru = torch.nn.GRU(D, H, batch_first=True).double()
    par = [p.half().double() if p.dim() == 2 else p.double()
           for p in (Wx, Wh, bx, bh)]
    with torch.no_grad():
        for dst, src in zip((gru.weight_ih_l0, gru.weight_hh_l0,
                             gru.bias_ih_l0, gru.bias_hh_l0), par):
            dst.copy_(src)
    x = seq[..., :D].double().requires_grad_(True)
    states, hn = gru(x)
    torch.autograd.backward([states, hn[0]], [gs.double(), gl.double()])
    want = (states, hn[0], x.grad, gru.weight_ih_l0.grad, gru.weight_hh_l0.grad,
            gru.bias_ih_l0.grad, gru.bias_hh_l0.grad)
    for n, w in zip(NAMES, want):
        g = got[n][..., :D] if n == "dseq" else got[n]
        assert (g - w.detach()).abs().max() <= 1e-10, n


@pytest.mark.parametrize("case,att", PARAMS, ids=IDS)
def test_invalid_rows_reach_nothing_and_carry_the_state(case, att):
    B, L, D, H = case
    ops = make_operands(case, att)
    seq = ops[0]
    valid = seq[..., D] != 0
    r64, E = reference(case, att, torch.float64), e16(case, att)
    for n in E:
        assert torch.isfinite(r64[n]).all(), n
        print(f"{n} {case} att={att}: E16 {E[n]:.3g} of max {r64[n].abs().max():.3g}")
    # NaN in every invalid row (att's are NaN already): the same bits
    poisoned = seq.clone()
    poisoned[..., :D][~valid] = float("nan")
    again = run_reference((poisoned,) + ops[1:], torch.float64)
    for n in E:
        assert torch.equal(again[n], r64[n]), n
    assert not r64["dseq"][..., D].any() and not r64["dseq"][~valid].any()
    if att:
        assert not r64["datt"][~valid].any()
    states = r64["states"]
    prev = torch.cat([torch.zeros_like(states[:, :1]), states[:, :-1]], 1)
    assert torch.equal(states[~valid], prev[~valid])
    assert torch.equal(r64["last"], states[:, -1])
    if B > 1:  # the sample without a valid row
        assert not valid[B - 1].any() and not states[B - 1].any()
    if case == HOLES:
        assert not valid[:, 0].any() and not valid[:, L - 1].any() and valid[0, 1]


@pytest.mark.parametrize("attention", ["gru", "augru"])
def test_seqctr_gru_modes_run_on_cpu(attention):
    from persia_amd.models import InterestGRUPool, SeqCTR

    torch.manual_seed(3)
    q, seq, _ = make_case((6, 4, 8))
    embs = [e.requires_grad_(True) for e in (q, seq, torch.randn(6, 16).half())]
    model = SeqCTR(dims=[8, 8, 16], seq_query={1: 0}, num_dense=5, hidden=(32,),
                   attention=attention)
    pool = model.gru_pools["1"]
    assert isinstance(pool, InterestGRUPool) and pool.hidden == 8
    assert [tuple(p.shape) for p in pool.parameters()] == \
        [tuple(p.shape) for p in torch.nn.GRU(8, 8).parameters()]
    logits = model([torch.randn(6, 5)], embs)
    assert logits.shape == (6,) and logits.dtype == torch.float32
    logits.sum().backward()
    assert all(torch.isfinite(e.grad).all() and e.grad.any() for e in embs)
    assert not embs[1].grad[5].any()  # the sample without a valid cell
    assert all(p.grad is not None and p.grad.any() for p in pool.parameters())
