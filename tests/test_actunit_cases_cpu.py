"""Cases and references of tests/test_gpu_actunit_exact.py, and the checks of
them that need no GPU.

`reference(case, dtype)` runs `act_unit_prepared_reference` (the part of the
activation-unit pooling that csrc/actunit.hip computes) forward and backward
from one set of input bits; `e32(case)` is the max abs error per tensor of its
f32 run against its f64 run -- the E32 of the GPU test's bounds, measured here
on the CPU and never on the kernels."""
import functools

import pytest
import torch

from persia_amd.ops.reference import (act_unit_pool_reference,
                                      act_unit_prepared_reference)
from test_seqattn_cases_cpu import make_case

# one row in a strip, a strip boundary, a tile boundary, more than one tile;
# one and several K-steps (D / 32), one and several column tiles (H / 16)
CASES = [(1, 1, 32, 16), (5, 3, 32, 16), (3, 17, 32, 48), (7, 64, 64, 32),
         (3, 65, 64, 64), (2, 130, 128, 64)]  # (B, L, D, H)
IDS = ["x".join(map(str, c)) for c in CASES]
NAMES = ("out", "dq_k", "dseq", "du", "dWb", "dWp", "dw2", "db2")


def make_params(case):
    """-> f32 W1 [H, 4D] ~ 0.5/sqrt(D), b1 [H], w2 [H] ~ 0.5, b2 []."""
    B, L, D, H = case
    gen = torch.Generator().manual_seed(((B * 1009 + L) * 1009 + D) * 1009 + H)
    W1 = torch.randn(H, 4 * D, generator=gen) * (0.5 * D ** -0.5)
    b1, w2 = torch.randn(H, generator=gen) * 0.1, torch.randn(H, generator=gen) * 0.5
    return W1, b1, w2, torch.randn((), generator=gen) * 0.1


def make_operands(case, device="cpu"):
    """-> q, seq, g (f16), u (f32), Wb, Wp (f16), w2, b2 (f32): what the
    native entries take, prepared in f32 on the CPU once."""
    B, L, D, H = case
    q, seq, g = make_case((B, L, D))
    W1, b1, w2, b2 = make_params(case)
    Wq, Wk, Wd, Wp = (W1[:, i * D:(i + 1) * D] for i in range(4))
    u = torch.addmm(b1, q.float(), (Wq + Wd).t())
    ops = (q, seq, g, u, (Wk - Wd).half(), Wp.half(), w2, b2)
    return tuple(t.to(device) for t in ops)


@functools.lru_cache(maxsize=None)
def reference(case, dtype):
    """-> {name: tensor} of NAMES, computed in `dtype` on the CPU."""
    q, seq, g, *par = (t.cpu() for t in make_operands(case))
    leaves = [t.to(dtype).requires_grad_(True) for t in (q, seq, *par)]
    out = act_unit_prepared_reference(*leaves)
    out.backward(g.to(dtype))
    return dict(zip(NAMES, [out.detach()] + [t.grad for t in leaves]))


@functools.lru_cache(maxsize=None)
def e32(case):
    r32, r64 = reference(case, torch.float32), reference(case, torch.float64)
    return {n: (r32[n].double() - r64[n]).abs().max().item() for n in NAMES}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_f32_reference_agrees_with_f64_and_invalid_rows_reach_nothing(case):
    B, L, D, H = case
    r32, r64, E = reference(case, torch.float32), reference(case, torch.float64), e32(case)
    for n in NAMES:
        assert torch.isfinite(r64[n]).all() and r64[n].abs().max() > 0, n
        # f32 arithmetic over sums of at most B * L * max(D, H) terms: far
        # below the f16 resolution of the results
        scale = r64[n].abs().max().item()
        print(f"{n} {case}: E32 {E[n]:.3g} of max {scale:.3g}")
        assert E[n] <= 2.0 ** -16 * scale, (n, E[n], scale)
    seq = make_operands(case)[1]
    valid = seq[..., D] != 0
    assert not r64["dseq"][..., D].any() and not r64["dseq"][~valid].any()
    if L >= 3:  # the planted Inf / NaN row is invalid and next to a valid one
        assert not valid[0, 1] and valid[0, 2] and not torch.isfinite(seq[0, 1]).all()
    if B > 1:
        assert not valid[B - 1].any()
        assert not any(r64[n][B - 1].any() for n in ("out", "dq_k", "du"))


@pytest.mark.parametrize("case", [(5, 3, 32, 16), (3, 65, 64, 64)], ids=str)
def test_prepared_reference_is_the_concat_mlp(case):
    """The folded form against DIN's own: an MLP over [q, k, q-k, q*k], with
    the same f16-rounded M_b (so in f64 only the association differs)."""
    B, L, D, H = case
    q, seq, _ = make_case((B, L, D))
    W1, b1, w2, b2 = (t.double() for t in make_params(case))
    got = act_unit_pool_reference(q.double(), seq.double(), W1, b1, w2, b2)
    valid = seq[..., D] != 0
    k = torch.where(valid.unsqueeze(-1), seq[..., :D].double(), torch.zeros(()).double())
    qe = q.double().unsqueeze(1).expand_as(k)
    h = torch.cat([qe, k, qe - k, qe * k], dim=2) @ W1.t() + b1
    w = torch.where(valid, torch.sigmoid(h) @ w2 + b2, torch.zeros(()).double())
    ref = (w.unsqueeze(-1) * k).sum(1)
    # the f16 rounding of M_b moves h by at most 2^-11 * sum |M k|
    assert (got - ref).abs().max() <= 2.0 ** -9 * ref.abs().max()


def test_modules_run_on_cpu_and_default_seqctr_is_unchanged():
    from persia_amd.models import ActivationUnitPool, SeqCTR

    torch.manual_seed(3)
    q, seq, _ = make_case((6, 4, 8))
    embs = [e.requires_grad_(True) for e in (q, seq, torch.randn(6, 16).half())]
    pool = ActivationUnitPool(8, hidden=16)
    assert torch.equal(pool(q, seq), act_unit_pool_reference(
        q, seq, pool.W1, pool.b1, pool.w2, pool.b2))
    model = SeqCTR(dims=[8, 8, 16], seq_query={1: 0}, num_dense=5, hidden=(32,),
                   attention="mlp", att_hidden=16)
    logits = model([torch.randn(6, 5)], embs)
    assert logits.shape == (6,) and logits.dtype == torch.float32
    logits.sum().backward()
    assert all(torch.isfinite(e.grad).all() and e.grad.any() for e in embs)
    assert not embs[1].grad[5].any()  # the sample without a valid cell
    assert all(p.grad is not None and p.grad.any()
               for p in model.act_pools["1"].parameters())
    plain = SeqCTR(dims=[8, 8, 16], seq_query={1: 0}, num_dense=5, hidden=(32,))
    assert [n for n, _ in plain.named_modules()] == \
        ["", "pool", "mlp", "mlp.0", "mlp.1", "mlp.2"]
    assert [n for n, _ in plain.named_parameters()] == \
        ["mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"]
