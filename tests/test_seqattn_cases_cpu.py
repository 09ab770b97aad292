"""Cases, f64 model and error bound of tests/test_gpu_seqattn_exact.py, and
the checks of them that need no GPU.

`seqattn_model` is target-attention pooling (ops/seqattn.py) and its backward
in f64 from the f16 input bits, with a per-element bound carried through the
expression tree of csrc/seqattn.hip; docs/ARCHITECTURE.md ("error model" of
the pooling section) derives every term.  Measured worst err/bound of the f32
reference on CPU: out 0.862, dq 0.795, dseq 0.994 (the f16 store dominates).
"""
import pytest
import torch

from persia_amd.ops.reference import seq_attn_pool_reference
from test_gpu_dense_exact import acc_bound, f16_store_bound
from test_tower_cases_cpu import (EPS32, EXP_ULPS, MINN32, U24, rel_err,
                                  worst_ratio)

CASES = [(1, 1, 8), (5, 3, 8), (33, 50, 40), (7, 64, 64), (3, 65, 64),
         (4, 50, 128), (2, 200, 128)]  # (B, L, D)
IDS = [f"{b}x{l}x{d}" for b, l, d in CASES]
BIG_SCORES = (7, 64, 64)   # scale 80/sqrt(D): scores beyond +-55
OFFSET_VIEW = (5, 3, 8)    # seq starts one half into its storage


def case_scale(case):
    return (80.0 if case == BIG_SCORES else 1.0) * case[2] ** -0.5


def make_case(case, device="cpu"):
    """-> f16 q [B, D], seq [B, L, D+1], g [B, D].  Cell 0 and about 70% of the
    others are valid, in no order.  Sample 0 (L >= 3): cell 1 invalid with an
    Inf and a NaN, cell 2 a valid all-zero row.  The last sample (B > 1): no
    valid cell, and an Inf."""
    B, L, D = case
    gen = torch.Generator().manual_seed((B * 1000003 + L) * 1000003 + D)
    q, k, g = ((torch.randn(*s, generator=gen) * 0.5).half()
               for s in ((B, D), (B, L, D), (B, D)))
    mask = torch.rand(B, L, generator=gen) < 0.7
    mask[:, 0] = True
    if L >= 3:
        mask[0, 1], mask[0, 2] = False, True
        k[0, 1, 0], k[0, 1, D - 1], k[0, 2] = float("inf"), float("nan"), 0.0
    if B > 1:
        mask[B - 1], k[B - 1, 0, 1] = False, float("-inf")
    flat = torch.cat([k, mask.half().unsqueeze(-1)], dim=2).reshape(-1)
    if case == OFFSET_VIEW:
        flat = torch.cat([flat[:1], flat]).to(device)[1:]
        assert flat.data_ptr() % 4 == 2
    return q.to(device), flat.to(device).view(B, L, D + 1), g.to(device)


def seqattn_model(q, seq, g, scale):
    """-> {"out" | "dq" | "dseq": (f64 reference, per-element bound)}."""
    u, D, L = U24, q.shape[1], seq.shape[1]
    sc = torch.tensor(scale, dtype=torch.float32).item()  # the kernel's f32
    valid = seq[..., D] != 0
    v, col = valid.unsqueeze(-1), (lambda t: t.unsqueeze(-1))
    zero = torch.zeros((), dtype=torch.float64, device=q.device)
    k = torch.where(v, seq[..., :D].double(), zero)  # invalid rows: no part
    ak, q64, g64 = k.abs(), q.double().unsqueeze(1), g.double().unsqueeze(1)
    rowsum = lambda t: t.sum(1, keepdim=True)  # noqa: E731
    rnd = lambda x, E: E + u * (x.abs() + E)  # noqa: E731  one more rounding

    s = sc * (k * q64).sum(-1)
    E_s = rnd(s, abs(sc) * acc_bound((ak * q64.abs()).sum(-1), D))
    m = s.masked_fill(~valid, float("-inf")).max(1, keepdim=True).values
    a = torch.where(valid, s - torch.where(torch.isfinite(m), m, zero), zero)
    E_a = E_s + u * (a.abs() + E_s + E_s.max(1, keepdim=True).values)
    e = torch.where(valid, a.exp(), zero)
    r, d = torch.expm1(E_a), 2 * a.abs() * u + EXP_ULPS * EPS32
    E_e = torch.where(valid, e * (r + d + r * d) + 2 * MINN32, zero)
    den, E_den = rowsum(e), rowsum(E_e) + L * u * rowsum(e + E_e)
    den = torch.where(den > 0, den, torch.ones_like(den))
    p = e / den
    E_p = (E_e + p * E_den) / (den - E_den)
    E_p = torch.where(valid, E_p + 2 * u * (1 + u) * (p + E_p) + MINN32, zero)
    P = p + E_p
    out = (col(p) * k).sum(1)
    E_out = (col(E_p) * ak).sum(1) + acc_bound((col(P) * ak).sum(1), L)

    dp, E_dp = (k * g64).sum(-1), acc_bound((ak * g64.abs()).sum(-1), D)
    diff = dp - rowsum(p * dp)
    E_t = rowsum(E_p * dp.abs() + P * E_dp) + \
        acc_bound(rowsum(P * (dp.abs() + E_dp)), L + 6)
    E_diff = rnd(diff, E_dp + E_t)
    ds = p * diff
    E_ds = rnd(ds, E_p * (diff.abs() + E_diff) + p * E_diff)
    dq = sc * (col(ds) * k).sum(1)
    E_dq = rnd(dq, abs(sc) * ((col(E_ds) * ak).sum(1) +
                              acc_bound((col(ds.abs() + E_ds) * ak).sum(1), L)))
    t1, E_c = col(p) * g64, rnd(sc * ds, abs(sc) * E_ds)
    dk = torch.where(v, t1 + col(sc * ds) * q64, zero)
    E_dk = rnd(dk, rnd(t1, col(E_p) * g64.abs()) + col(E_c) * q64.abs())
    pad = torch.zeros_like(dk[..., :1])
    dseq, E_dseq = torch.cat([dk, pad], 2), torch.cat([E_dk * v, pad], 2)
    return {"out": (out, f16_store_bound(E_out, out)),
            "dq": (dq, f16_store_bound(E_dq, dq)),
            "dseq": (dseq, f16_store_bound(E_dseq, dseq))}


def _run_reference(q, seq, g, scale, dtype):
    q = q.detach().to(dtype).requires_grad_(True)
    seq = seq.detach().to(dtype).requires_grad_(True)
    out = seq_attn_pool_reference(q, seq, scale)
    out.backward(g.to(dtype))
    return out.detach(), q.grad, seq.grad


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_and_model_agree(case):
    (B, L, D), scale = case, case_scale(case)
    q, seq, g = make_case(case)
    mdl = seqattn_model(q, seq, g, scale)
    # the model's formulas against f64 autograd (minus the masked Inf / NaN)
    finite = torch.where(torch.isfinite(seq), seq, torch.zeros_like(seq))
    sc32 = torch.tensor(scale, dtype=torch.float32).item()
    for name, t in zip(mdl, _run_reference(q, finite, g, sc32, torch.float64)):
        assert rel_err(t, mdl[name][0]) <= 2.0 ** -40, name
    # the f32 reference on the f16 bits, Inf and NaN in place
    got = _run_reference(q, seq, g, scale, torch.float16)
    for name, t in zip(mdl, got):
        assert t.dtype == torch.float16
        worst_ratio(t, *mdl[name], f"reference {name} {case}")
    valid = seq[..., D] != 0
    assert not got[2][..., D].any() and not got[2][~valid].any()
    if L >= 3:  # a hole before a valid all-zero row: the mask is no prefix
        assert not valid[0, 1] and valid[0, 2] and not seq[0, 2, :D].any()
    if B > 1:
        assert not valid[B - 1].any() and not got[0][B - 1].any()
    if case == BIG_SCORES:
        s = scale * (seq[..., :D].double() * q.double().unsqueeze(1)).sum(-1)
        assert s[valid].max() > 55 and s[valid].min() < -55


def test_seqctr_runs_on_cpu_with_a_raw_slot_input():
    from persia_amd.models import SeqCTR, TargetAttentionPool

    torch.manual_seed(3)
    q, seq, _ = make_case((6, 4, 8))  # the query and the raw slot's tensor
    embs = [e.requires_grad_(True) for e in (q, seq, torch.randn(6, 16).half())]
    model = SeqCTR(dims=[8, 8, 16], seq_query={1: 0}, num_dense=5, hidden=(32,))
    logits = model([torch.randn(6, 5)], embs)
    assert logits.shape == (6,) and logits.dtype == torch.float32
    logits.sum().backward()
    assert all(torch.isfinite(e.grad).all() and e.grad.any() for e in embs)
    assert not embs[1].grad[5].any()  # the sample without a valid cell
    assert torch.equal(TargetAttentionPool()(embs[0], embs[1]),
                       seq_attn_pool_reference(embs[0], embs[1]))
