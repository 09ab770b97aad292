"""Case generators and references of tests/test_gpu_glue_exact.py, and the
checks of them that need no GPU.

The glue kernels: `interact_fwd_top` / `interact_bwd_top` (the packed DLRM
interaction writing the whole top-MLP input and reading the full-width
gradient), `head_fwd` / `head_bwd` (the 1-logit head) and `pad_k` (the
K-padding of a ragged weight).

References and bounds (imported from test_gpu_dense_exact.py, none invented):

* top input and its backward: bit-equal to the composition they replace, see
  `top_fwd_composition` / `top_bwd_composition` (they take the packed
  kernels' results as arguments, so the same functions serve the CPU check
  of their own logic and the GPU comparison).
* head logit: K exact bf16 x bf16 products summed in f32 in any order, plus
  the bias add: acc_bound(S, K) with S = sum |h||w| + |b|, then one bf16
  store: bf16_store_bound.
* head dh: one exact product, one bf16 rounding: bit-equal to
  (dz.float() * w.float()).bfloat16().
* head dw / db: B exact products (db: B values) summed in f32 in any order:
  colsum_bound(B + 1, S) (the + 1 as for the fused layers' db), then one
  bf16 store.
"""
import pytest
import torch

from test_gpu_dense_exact import acc_bound, bf16_store_bound, colsum_bound

INTERACT_B = (1, 3, 65, 200)
INTERACT_SD = ((1, 8), (2, 16), (26, 128), (64, 8))
HEAD_B = (1, 63, 1000)
HEAD_K = (8, 96, 256)
PAD_K_SHAPES = ((512, 13), (1024, 479), (32, 128))


def _seed(*shape):
    seed = 0
    for s in shape:
        seed = seed * 1000003 + int(s)
    return torch.Generator().manual_seed(seed % (2 ** 62))


def n_pairs(S):
    return (S + 1) * S // 2


def pads_of(S, D):
    """pad = 0 (an eager top) and the pad to the fused GEMM's K % 128."""
    k = D + n_pairs(S)
    return (0, (-k) % 128)


def interact_case(B, S, D, pad, device="cpu"):
    """-> x bf16 [B, D], base f16 slot-major [S*B, D], g bf16 [B, D+P+pad]."""
    gen = _seed(B, S, D, pad)
    x = (torch.randn(B, D, generator=gen) * 0.5).to(torch.bfloat16)
    base = (torch.randn(S * B, D, generator=gen) * 0.5).to(torch.float16)
    g = (torch.randn(B, D + n_pairs(S) + pad, generator=gen) * 0.25).to(torch.bfloat16)
    return x.to(device), base.to(device), g.to(device)


def top_fwd_composition(x, inter, pad):
    return torch.cat([x, inter, x.new_zeros(x.shape[0], pad)], dim=1)


def top_bwd_composition(g, dx_inter, D):
    """The summed gradient of x as autograd forms it: the interaction's own
    bf16 dx plus the x block of g, added in f32, rounded to bf16 again."""
    return (dx_inter.float() + g[:, :D].float()).to(torch.bfloat16)


def shift_pairs(g, D, P):
    """The negative control: g's pair block moved by one column."""
    out = g.clone()
    out[:, D:D + P] = torch.roll(g[:, D:D + P], 1, dims=1)
    return out


def head_case(B, K, device="cpu"):
    """-> h bf16 [B, K], w bf16 [1, K], b bf16 [1], dz bf16 [B, 1]."""
    gen = _seed(B, K)
    h = (torch.randn(B, K, generator=gen) * 0.5).to(torch.bfloat16)
    w = (torch.randn(1, K, generator=gen) * 0.25 + 0.05).to(torch.bfloat16)
    b = torch.randn(1, generator=gen).to(torch.bfloat16)
    dz = (torch.randn(B, 1, generator=gen) / B).to(torch.bfloat16)
    return h.to(device), w.to(device), b.to(device), dz.to(device)


def head_model(h, w, b, dz):
    """-> {logit, dw, db: (f64 ref, bound)} on the actual input bits."""
    h64, w64, b64, dz64 = (t.detach().double() for t in (h, w, b, dz))
    B, K = h.shape
    logit = h64 @ w64.t() + b64
    S = h64.abs() @ w64.abs().t() + b64.abs()
    dw = dz64.t() @ h64
    Sw = dz64.abs().t() @ h64.abs()
    db = dz64.sum(0)
    Sb = dz64.abs().sum(0)
    return {
        "logit": (logit, bf16_store_bound(acc_bound(S, K), logit)),
        "dw": (dw, bf16_store_bound(colsum_bound(B + 1, Sw), dw)),
        "db": (db, bf16_store_bound(colsum_bound(B + 1, Sb), db)),
    }


def head_dh_reference(dz, w):
    return (dz.float() * w.float()).to(torch.bfloat16)


def pad_k_case(N, K, device="cpu"):
    return torch.randn(N, K, generator=_seed(N, K)).to(torch.bfloat16).to(device)


def pad_k_reference(w, mult=128):
    return torch.nn.functional.pad(w, (0, (-w.shape[1]) % mult))


def within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: err/bound {ratio:.4g}")
    assert bool((err <= bound).all()), f"{what}: worst err/bound {ratio:.4g}"
    return ratio


# ================================================================ CPU checks
@pytest.mark.parametrize("K", HEAD_K)
@pytest.mark.parametrize("B", HEAD_B)
def test_head_torch_composition_is_inside_the_bounds(B, K):
    """The f32 torch composition of the head stays inside the bounds against
    f64 (so the bounds admit a correct implementation), and a wrong one (bias
    dropped) does not."""
    h, w, b, dz = head_case(B, K)
    mdl = head_model(h, w, b, dz)
    logit = (h.float() @ w.float().t() + b.float()).to(torch.bfloat16)
    within(logit, *mdl["logit"], "logit")
    within((dz.float().t() @ h.float()).to(torch.bfloat16), *mdl["dw"], "dw")
    within(dz.float().sum(0).to(torch.bfloat16), *mdl["db"], "db")
    with pytest.raises(AssertionError):
        within((h.float() @ w.float().t()).to(torch.bfloat16), *mdl["logit"], "no bias")
    # dh: the f32 product of two bf16 values is exact, so f64 agrees
    dh = head_dh_reference(dz, w)
    assert torch.equal(dh, (dz.double() * w.double()).to(torch.bfloat16))


def test_top_compositions():
    S, D, B = 2, 16, 3
    P = n_pairs(S)
    for pad in pads_of(S, D):
        x, base, g = interact_case(B, S, D, pad)
        assert g.shape == (B, D + P + pad)
        inter = g[:, D:D + P]  # any [B, P] block
        top = top_fwd_composition(x, inter, pad)
        assert top.shape == g.shape and torch.equal(top[:, :D], x)
        assert torch.equal(top[:, D:D + P], inter) and (top[:, D + P:] == 0).all()
    assert pads_of(26, 128) == (0, 33) and pads_of(1, 8)[1] == 119
    # two roundings are not one: the composition differs from the f32 sum
    # rounded once on some element of a large enough sample
    gen = _seed(7)
    a = torch.randn(4096, 8, generator=gen)
    g = torch.randn(4096, 8, generator=gen).to(torch.bfloat16)
    twice = top_bwd_composition(g, a.to(torch.bfloat16), 8)
    once = (a + g.float()).to(torch.bfloat16)
    assert not torch.equal(twice, once)
    shifted = shift_pairs(g, 2, 4)
    assert torch.equal(shifted[:, :2], g[:, :2]) and torch.equal(shifted[:, 6:], g[:, 6:])
    assert not torch.equal(shifted, g)


@pytest.mark.parametrize("shape", PAD_K_SHAPES)
def test_pad_k_reference_shapes(shape):
    w = pad_k_case(*shape)
    out = pad_k_reference(w)
    assert out.shape == (shape[0], -(-shape[1] // 128) * 128)
    assert torch.equal(out[:, :shape[1]], w) and (out[:, shape[1]:] == 0).all()


def test_head_module_is_a_plain_linear_on_cpu():
    """HeadLinear keeps nn.Linear's parameters, init stream and CPU math, and
    is not a FusedLinear."""
    from persia_amd.ops.dense import FusedLinear, FusedMLP, HeadLinear

    torch.manual_seed(3)
    a = HeadLinear(16, 1)
    torch.manual_seed(3)
    b = torch.nn.Linear(16, 1)
    assert list(a.state_dict()) == list(b.state_dict())
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q) and p.dtype == q.dtype
    x = torch.randn(5, 16)
    assert torch.equal(a(x), b(x))
    mlp = FusedMLP([32, 32, 1])
    assert isinstance(mlp.layers[-1], HeadLinear)
    assert isinstance(mlp.layers[-1], torch.nn.Linear)
    assert not isinstance(mlp.layers[-1], FusedLinear)
