"""Dense and interaction kernels against f64 references, elementwise bounds.

Every comparison takes the exact result in f64 (torch) from the SAME bf16 /
f16 operand bits the kernel reads, and allows an error derived per element
from the arithmetic the kernel performs -- never an atol.

With S the same product formed from absolute values (|A| @ |B|^T + |bias|,
|dC|^T @ |A|, ...) and n the reduction length:

  f32 accumulation   E = (n + 1) * 2^-23 * S
      bf16 x bf16 products are exact in f32; each of the n accumulations and
      the bias add is charged one FULL f32 ulp of a partial sum that never
      exceeds S.  A full ulp (not the half ulp of round-to-nearest) also
      covers an MFMA that truncates or aligns to the largest addend.
      Split-M atomics add one rounding per part: n + splitm.
  bf16 store         E + 2^-8  * (|ref| + E)
  f16 store          E + 2^-11 * (|ref| + E) + 2^-25
      (2^-25 is half the spacing of f16 subnormals, below 2^-14, where the
      relative term alone no longer describes round-to-nearest)
  ReLU               1-Lipschitz: the same bound holds after it
  column sums        n * 2^-24 * sum|a|   (f32 addends in any order, as in
                     test_gpu_dense_drelu.py; a pre-filled accumulator counts
                     as one more addend)

A plain f32 torch product measured against f64 with these bounds stays at
err/bound 0.016 (f32 out), 0.98 (bf16 out, the rounding term is tight by
construction), 0.003 (wgrad) and 1.3e-4 (bias-grad).  Each test prints its
own worst err/bound.  The kernels on an MI355X: GEMM 0.0063 (f32 out) and
0.980 (bf16 out) in every family including glds3; dgrad dx 0.961, its db
0.0028; wgrad 0.013, wgrad_into 0.0027; bias-grad 2.6e-4 at M >= 777 (0.5 by
construction where one addend meets a pre-filled accumulator); interaction
0.996 (bf16 stores) and 0.998 (f16 dbase).  No constant had to be raised.

Operands are asymmetric random values (A, g, V: randn * 0.5; B, W:
randn * 0.25 + 0.05), seeded from the shape.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23   # one f32 ulp, relative
U24 = 2.0 ** -24     # f32 round-to-nearest unit (column-sum bound)
REL_BF16 = 2.0 ** -8
REL_F16 = 2.0 ** -11
F16_SUBNORMAL = 2.0 ** -25


def _dev():
    return torch.device("cuda", 0)


def _native():
    from persia_amd.ops import native

    return native()


def _gen(*shape):
    seed = 0
    for s in shape:
        seed = seed * 1000003 + int(s)
    return torch.Generator(device=_dev()).manual_seed(seed % (2 ** 62))


def _randn(gen, *shape):
    return torch.randn(*shape, device=_dev(), generator=gen)


# ---------------------------------------------------------------- the bounds
def acc_bound(S, n):
    """f32 accumulation of n exact products (+ one more add): (n+1) ulps of S."""
    return (n + 1) * EPS32 * S


def bf16_store_bound(E, ref):
    return E + REL_BF16 * (ref.abs() + E)


def f16_store_bound(E, ref):
    """Round-to-nearest f16 store.  2^-11 relative holds for normal f16 only;
    below 2^-14 the spacing is a constant 2^-24, so the store can be off by
    2^-25 whatever |ref| is.  Measured on gfx950 at (B, F, D) = (32773, 3, 8):
    321 references fall in that range and reach err/bound 105 with the
    relative term alone, 0.998 with the 2^-25 term (which is 3e-8 absolute --
    no room for a wrong kernel to hide in)."""
    return E + REL_F16 * (ref.abs() + E) + F16_SUBNORMAL


def colsum_bound(n, abs_sum):
    """n f32 addends accumulated in any order."""
    return n * U24 * abs_sum


def _ratio(got, ref, bound, what):
    """Worst err/bound of `got` against the f64 `ref`; asserts it is <= 1."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    bad = int((~(err <= bound)).sum().item())  # a NaN counts as bad
    print(f"{what}: err/bound {ratio:.4g}")
    assert bad == 0, f"{what}: {bad} of {err.numel()} elements exceed the " \
                     f"bound, worst err/bound {ratio:.4g}"
    return ratio


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------- a. gemm_nt_bias_act
# (M, K, N, trans_b values, expected dispatch, also with out_f32=1)
GEMM_CASES = [
    (1, 32, 8, (0, 1), "v1:128x32", True),       # one row, one K step, 8 cols
    (129, 96, 72, (0, 1), "v1:128x32", False),   # M tail of 1, N tail, 3 steps
    (200, 96, 128, (0, 1), "v1:64x32", True),    # M tail
    (127, 64, 64, (0, 1), "v1:64x64", False),    # single K step, M < tile
    (200, 320, 128, (0, 1), "v1:64x64", False),  # odd step count
    (6472, 256, 1024, (0,), "glds:128", True),   # minimum K, M tail of 72
    (6472, 320, 1024, (0,), "glds:128", False),  # odd step count
    (17025, 256, 192, (0,), "glds:64", False),   # last M tile holds one row
    (25601, 256, 128, (0,), "glds:64", True),    # N%128==0, < 400 wide tiles
]


def _gemm_operands(M, K, N):
    gen = _gen(M, K, N)
    A = (_randn(gen, M, K) * 0.5).to(torch.bfloat16).contiguous()
    B = (_randn(gen, N, K) * 0.25 + 0.05).to(torch.bfloat16).contiguous()
    bias = _randn(gen, N)
    return A, B, bias


def _gemm_reference(A, B, bias):
    """f64 product and absolute-value product, with and without the bias."""
    prod = A.double() @ B.double().t()
    S = A.double().abs() @ B.double().abs().t()
    return {
        True: (prod + bias.double(), S + bias.double().abs()),
        False: (prod, S),
    }


def _check_gemm(C, A, B, bias, refs, trans_b, f32_too, tag):
    """All act x bias (x out_f32) variants of one operand layout.
    -> (worst ratio, {variant: output})."""
    K = A.shape[1]
    B_op = B.t().contiguous() if trans_b else B
    empty = torch.empty(0, device=_dev())
    worst, outs = 0.0, {}
    for with_bias in (True, False):
        ref0, S = refs[with_bias]
        E = acc_bound(S, K)
        for act in (0, 1):
            ref = torch.relu(ref0) if act else ref0
            for f32 in ((0, 1) if f32_too else (0,)):
                out = C.gemm_nt_bias_act(A, B_op, bias if with_bias else empty,
                                         act, f32, trans_b)
                assert out.dtype == (torch.float32 if f32 else torch.bfloat16)
                bound = E if f32 else bf16_store_bound(E, ref)
                what = f"{tag} trans_b={trans_b} bias={int(with_bias)} " \
                       f"act={act} f32={f32}"
                worst = max(worst, _ratio(out, ref, bound, what))
                outs[(with_bias, act, f32)] = out
    return worst, outs


@pytest.mark.parametrize("case", GEMM_CASES,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in GEMM_CASES])
def test_gemm_nt_bias_act_exact(case):
    M, K, N, trans_bs, expect, f32_too = case
    C = _native()
    for tb in trans_bs:
        assert C.gemm_nt_config(M, N, K, tb) == expect
    A, B, bias = _gemm_operands(M, K, N)
    refs = _gemm_reference(A, B, bias)
    worst, per_layout = 0.0, {}
    for tb in trans_bs:
        w, per_layout[tb] = _check_gemm(C, A, B, bias, refs, tb, f32_too,
                                        f"gemm {M}x{K}x{N}")
        worst = max(worst, w)
    print(f"gemm {M}x{K}x{N} {expect}: worst err/bound {worst:.4g}")
    if len(trans_bs) == 2:
        # same v1 tile config => the same MFMA sequence on the same LDS
        # image (the trans_b staging writes the [n][k] image element by
        # element instead of by vector): bit-identical results
        for key, out0 in per_layout[0].items():
            assert torch.equal(_bits(out0), _bits(per_layout[1][key])), key


# Kernels selected by environment variables that the extension reads once
# into statics: each gets one fresh child process.
def _child(kind):
    """Runs in the child; any failed assertion makes its exit code non-zero."""
    C = _native()
    if kind in ("gemm_v3", "gemm_v2off"):
        M, K, N = 6472, 256, 1024
        cfg = C.gemm_nt_config(M, N, K, 0)
        if kind == "gemm_v3":
            assert cfg == "glds3:128", cfg
        else:
            assert cfg.startswith("v1:"), cfg
        A, B, bias = _gemm_operands(M, K, N)
        worst, _ = _check_gemm(C, A, B, bias, _gemm_reference(A, B, bias), 0,
                               True, f"{kind} {cfg}")
    elif kind == "wgrad_v1":
        cfg = C.wgrad_config(320, 1024, 1024)
        assert cfg.startswith("v1:"), cfg
        worst = _check_wgrad(C, 320, 1024, 1024, "v1")
    else:
        raise ValueError(kind)
    torch.cuda.synchronize()
    print(f"child {kind}: worst err/bound {worst:.4g}")


@pytest.mark.parametrize("kind,var,value", [
    ("gemm_v3", "PA_GEMM_V3", "1"),
    ("gemm_v2off", "PA_GEMM_V2", "0"),
    ("wgrad_v1", "PA_WGRAD_TR", "0"),
])
def test_env_selected_kernels_in_child(kind, var, value):
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(tests_dir)
    env = dict(os.environ)
    for v in ("PA_GEMM_V3", "PA_GEMM_V2", "PA_WGRAD_TR"):
        env.pop(v, None)
    env[var] = value
    code = ("import sys; sys.path[:0] = [r'%s', r'%s']; "
            "import test_gpu_dense_exact as T; T._child(%r)"
            % (repo, tests_dir, kind))
    out = subprocess.run([sys.executable, "-c", code], cwd=repo, env=env,
                         capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert f"child {kind}: worst err/bound" in out.stdout


# ------------------------------------------------------- b. dgrad_drelu_bias
DGRAD_CASES = [
    (129, 96, 72, 0, "v1:128x32"), (129, 96, 72, 1, "v1:128x32"),
    (17025, 256, 192, 0, "glds:64"),  # one-row last M tile
]


@pytest.mark.parametrize("case", DGRAD_CASES,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}-t{c[3]}" for c in DGRAD_CASES])
def test_dgrad_drelu_bias_exact(case):
    M, K, N, trans_b, expect = case
    C = _native()
    assert C.gemm_nt_config(M, N, K, trans_b) == expect
    gen = _gen(M, K, N, 77)
    g = (_randn(gen, M, K) * 0.5).to(torch.bfloat16).contiguous()
    W = (_randn(gen, N, K) * 0.25 + 0.05).to(torch.bfloat16).contiguous()
    W_op = W.t().contiguous() if trans_b else W
    # a ReLU output: >= 0, about half exact zeros
    mask = torch.relu(_randn(gen, M, N)).to(torch.bfloat16).contiguous()
    assert 0.3 < (mask == 0).float().mean().item() < 0.7
    live = mask.double() > 0
    ref = torch.where(live, g.double() @ W.double().t(), 0.0)
    E = acc_bound(g.double().abs() @ W.double().abs().t(), K)
    bound = bf16_store_bound(E, ref)

    worst = 0.0
    for n_bias in (N, N - 8, 0):
        db0 = _randn(gen, N)  # non-zero accumulator
        db = db0.clone()
        dx = C.dgrad_drelu_bias(g, W_op, trans_b, mask, db, n_bias)
        worst = max(worst, _ratio(dx, ref, bound, f"dx n_bias={n_bias}"))
        assert (dx[~live] == 0).all()
        # column sums of the kernel's OWN dx, added to db0: M + 1 addends
        own = dx[:, :n_bias].double()
        db_ref = db0[:n_bias].double() + own.sum(0)
        db_bound = colsum_bound(M + 1, own.abs().sum(0) + db0[:n_bias].double().abs())
        if n_bias:
            worst = max(worst, _ratio(db[:n_bias], db_ref, db_bound,
                                      f"db n_bias={n_bias}"))
        assert torch.equal(_bits(db[n_bias:]), _bits(db0[n_bias:]))
    print(f"dgrad_drelu_bias {M}x{K}x{N} trans_b={trans_b}: "
          f"worst err/bound {worst:.4g}")


# ------------------------------------------------------ c. wgrad / wgrad_into
def _parse_wgrad_config(cfg):
    kind, s, c = cfg.split(":")
    assert kind in ("tr", "v1") and s.startswith("splitm=") and c.startswith("chunk=")
    return kind, int(s[len("splitm="):]), int(c[len("chunk="):])


def test_wgrad_config_every_part_starts_inside():
    """Host only.  No part of the M split may start at or past row M: the tr
    kernel stages whole 64-row steps from its part's first row without a row
    guard."""
    C = _native()
    bad = []
    for N, K in ((1024, 1024), (2048, 1024), (64, 64), (72, 40), (512, 480)):
        for M in range(1, 8193):
            kind, splitm, chunk = _parse_wgrad_config(C.wgrad_config(M, N, K))
            ok = splitm >= 1 and chunk >= 1 and (splitm - 1) * chunk < M
            if kind == "tr":
                ok = ok and M % 64 == 0 and chunk % 64 == 0 and \
                    (splitm - 1) * chunk + 64 <= M
            if not ok:
                bad.append((M, N, K, kind, splitm, chunk))
    assert not bad, f"{len(bad)} shapes with an out-of-range part: {bad[:8]}"


def _wgrad_operands(M, N, K):
    gen = _gen(M, N, K, 5)
    dC = (_randn(gen, M, N) * 0.5).to(torch.bfloat16).contiguous()
    A = (_randn(gen, M, K) * 0.25 + 0.05).to(torch.bfloat16).contiguous()
    return gen, dC, A


def _wgrad_reference(C, dC, A):
    M = dC.shape[0]
    _, splitm, _ = _parse_wgrad_config(C.wgrad_config(M, dC.shape[1], A.shape[1]))
    ref = dC.double().t() @ A.double()
    bound = (M + splitm + 1) * EPS32 * (dC.double().abs().t() @ A.double().abs())
    return ref, bound


def _check_wgrad(C, M, N, K, kind):
    cfg = C.wgrad_config(M, N, K)
    assert cfg.startswith(kind + ":"), cfg
    _, dC, A = _wgrad_operands(M, N, K)
    ref, bound = _wgrad_reference(C, dC, A)
    dW = C.wgrad(dC, A)
    assert dW.dtype == torch.float32
    return _ratio(dW, ref, bound, f"wgrad {M}x{N}x{K} {cfg}")


# tr: splitm=1 (plain stores), uneven parts, even parts, and the two shapes
# whose rounded chunks used to leave parts past the end
WGRAD_CASES = [("tr", M, 1024, 1024) for M in (64, 192, 256, 320, 576)] + [
    ("v1", 1, 8, 8),
    ("v1", 40, 64, 64),    # splitm=1: plain stores
    ("v1", 64, 64, 64),
    ("v1", 65, 64, 64),    # part 1 is a single row
    ("v1", 100, 64, 64),
    ("v1", 200, 72, 40),   # tails in N and K
    ("v1", 1024, 64, 32),
]


@pytest.mark.parametrize("case", WGRAD_CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in WGRAD_CASES])
def test_wgrad_exact(case):
    kind, M, N, K = case
    C = _native()
    _check_wgrad(C, M, N, K, kind)
    if (kind, M) == ("tr", 64) or case[1:] == (40, 64, 64):
        assert _parse_wgrad_config(C.wgrad_config(M, N, K))[1] == 1
    if case[1:] == (65, 64, 64):
        assert C.wgrad_config(M, N, K) == "v1:splitm=2:chunk=64"
    if case[1:] == (320, 1024, 1024):
        assert C.wgrad_config(M, N, K) == "tr:splitm=3:chunk=128"


# (kind, M, N, K of A, kmax = width of out)
WGRAD_INTO_CASES = [
    ("v1", 200, 64, 64, 64),
    ("v1", 200, 64, 64, 40),        # out [64, 40] against A [200, 64]
    ("tr", 256, 1024, 1024, 1024),
    ("tr", 256, 1024, 1024, 1000),  # out [1024, 1000] against A [256, 1024]
]


@pytest.mark.parametrize("case", WGRAD_INTO_CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-k{c[4]}"
                              for c in WGRAD_INTO_CASES])
def test_wgrad_into_exact(case):
    """Accumulates twice into a pre-filled `out` that sits inside a larger
    buffer of sentinels: result = initial + 2 * ref within the doubled bound,
    and nothing outside `out` changes (row stride and kmax honoured)."""
    kind, M, N, K, kmax = case
    C = _native()
    assert C.wgrad_config(M, N, K).startswith(kind + ":")
    gen, dC, A = _wgrad_operands(M, N, K)
    ref, bound = _wgrad_reference(C, dC, A)
    ref, bound = ref[:, :kmax], bound[:, :kmax]
    guard = 4096
    buf = _randn(gen, guard + N * kmax + guard) + 3.0
    before = buf.clone()
    out = buf[guard:guard + N * kmax].view(N, kmax)
    C.wgrad_into(dC, A, out)
    C.wgrad_into(dC, A, out)
    init = before[guard:guard + N * kmax].view(N, kmax).double()
    _ratio(out, init + 2 * ref, 2 * bound, f"wgrad_into {case}")
    assert torch.equal(_bits(buf[:guard]), _bits(before[:guard]))
    assert torch.equal(_bits(buf[guard + N * kmax:]),
                       _bits(before[guard + N * kmax:]))


def test_wgrad_operand_checks():
    C = _native()
    dev = _dev()
    bf = dict(dtype=torch.bfloat16, device=dev)
    dC, A = torch.ones(64, 16, **bf), torch.ones(64, 24, **bf)
    out = torch.zeros(16, 24, device=dev)
    C.wgrad(dC, A)  # the well-formed call passes
    C.wgrad_into(dC, A, out)
    bad_pairs = [
        (dC.float(), A),                           # dtype
        (dC, A.float()),
        (torch.ones(16, 64, **bf).t(), A),         # not contiguous
        (dC, torch.ones(24, 64, **bf).t()),
        (dC, A.cpu()),                             # different devices
        (dC, torch.ones(65, 24, **bf)),            # row counts differ
        (torch.ones(64, 12, **bf), A),             # N % 8
        (dC, torch.ones(64, 20, **bf)),            # K % 8
    ]
    for d, a in bad_pairs:
        with pytest.raises(RuntimeError):
            C.wgrad(d, a)
        with pytest.raises(RuntimeError):
            C.wgrad_into(d, a, out)
    for o in (out.double(), torch.zeros(24, 16, device=dev).t(),
              torch.zeros(8, 24, device=dev), torch.zeros(16, 32, device=dev),
              out.cpu()):
        with pytest.raises(RuntimeError):
            C.wgrad_into(dC, A, o)
    torch.cuda.synchronize()


def test_relu_bwd_bias_operand_checks():
    C = _native()
    bf = dict(dtype=torch.bfloat16, device=_dev())
    g = torch.ones(4, 16, **bf)
    db = torch.zeros(16, device=_dev())
    C.relu_bwd_bias(g, g, db)
    for o in (torch.ones(5, 16, **bf), torch.ones(4, 32, **bf), g.float(),
              g.to(torch.float16)):
        with pytest.raises(RuntimeError):
            C.relu_bwd_bias(g, o, db)
    torch.cuda.synchronize()


# ------------------------------------ d. bias-grad, relu_bwd, relu_bwd_bias
BIAS_SHAPES = [
    (1, 8), (7, 24), (777, 360), (1, 8192), (3, 8192),
    (777, 4096),  # total8 is no multiple of the grid stride: unrolled + tail
    (1000, 256),
]
POW2_SHAPES = [s for s in BIAS_SHAPES if s[1] & (s[1] - 1) == 0]


@pytest.mark.parametrize("shape", BIAS_SHAPES, ids=[f"{m}x{n}" for m, n in BIAS_SHAPES])
def test_bias_grad_exact(shape):
    M, N = shape
    C = _native()
    gen = _gen(M, N, 3)
    a = (_randn(gen, M, N) * 0.5).to(torch.bfloat16).contiguous()
    ref, abs_sum = a.double().sum(0), a.double().abs().sum(0)
    _ratio(C.bias_grad(a), ref, colsum_bound(M, abs_sum), f"bias_grad {M}x{N}")
    out0 = _randn(gen, N)  # pre-filled accumulator: one more addend
    out = out0.clone()
    C.bias_grad_into(a, out)
    _ratio(out, out0.double() + ref,
           colsum_bound(M + 1, abs_sum + out0.double().abs()),
           f"bias_grad_into {M}x{N}")


def _relu_operands(M, N):
    gen = _gen(M, N, 9)
    g = (_randn(gen, M, N) * 0.5).to(torch.bfloat16).contiguous()
    out = _randn(gen, M, N).to(torch.bfloat16)
    sel = torch.rand(M, N, device=_dev(), generator=gen)
    out[sel < 0.15] = 0.0
    out[(sel >= 0.15) & (sel < 0.3)] = -0.0
    out = out.contiguous()
    expect = torch.where(out > 0, g, torch.zeros_like(g))
    return gen, g, out, expect


@pytest.mark.parametrize("shape", BIAS_SHAPES, ids=[f"{m}x{n}" for m, n in BIAS_SHAPES])
def test_relu_bwd_bit_exact(shape):
    M, N = shape
    C = _native()
    _, g, out, expect = _relu_operands(M, N)
    if M * N >= 64:
        assert (_bits(out) == -32768).any() and (_bits(out) == 0).any()
    assert torch.equal(_bits(C.relu_bwd(g, out)), _bits(expect))


@pytest.mark.parametrize("shape", POW2_SHAPES, ids=[f"{m}x{n}" for m, n in POW2_SHAPES])
def test_relu_bwd_bias_exact(shape):
    M, N = shape
    C = _native()
    gen, g, out, expect = _relu_operands(M, N)
    db0 = _randn(gen, N)
    db = db0.clone()
    g_eff = C.relu_bwd_bias(g, out, db)
    assert torch.equal(_bits(g_eff), _bits(expect))
    e = g_eff.double()
    _ratio(db, db0.double() + e.sum(0),
           colsum_bound(M + 1, e.abs().sum(0) + db0.double().abs()),
           f"relu_bwd_bias db {M}x{N}")


# ------------------------------------------------------------ e. interaction
# (B, F, D) -> waves per block picked (pick_waves) by
#                  fwd  bwd  packed bwd
#   (1, 2, 8)       4    4    4     P = 1, D padded to 32
#   (5, 16, 40)     4    4    4     F exactly a tile, Dp = 48 with d < D guard
#   (7, 17, 64)     4    4    4
#   (33, 33, 128)   4    2    2     Fk = 64 in the backward
#   (6, 65, 128)    2    1    1
#   (3, 65, 256)    1    0    0     backward images exceed the 64 KB LDS limit
#   (32773, 3, 8)   4    4    4     > 8192 * 4 samples: second grid-stride lap
# (the packed forward uses the same image as the plain forward)
INTERACT_CASES = [(1, 2, 8), (5, 16, 40), (7, 17, 64), (33, 33, 128),
                  (6, 65, 128), (3, 65, 256), (32773, 3, 8)]
_INTERACT_IDS = [f"{b}x{f}x{d}" for b, f, d in INTERACT_CASES]


def _interact_reference(V, g):
    """V [B, F, D] bf16, g [B, P] bf16 -> f64 references and bounds of the
    forward (bf16 store) and of dV = sym(G) @ V (accumulation bound only)."""
    B, F, D = V.shape
    Vd = V.double()
    li, lj = torch.tril_indices(F, F, offset=-1, device=V.device)
    fwd = torch.bmm(Vd, Vd.transpose(1, 2))[:, li, lj]
    fwd_S = torch.bmm(Vd.abs(), Vd.abs().transpose(1, 2))[:, li, lj]
    G = torch.zeros(B, F, F, dtype=torch.float64, device=V.device)
    G[:, li, lj] = g.double()
    G = G + G.transpose(1, 2)
    bwd = torch.bmm(G, Vd)
    bwd_E = acc_bound(torch.bmm(G.abs(), Vd.abs()), F)
    return fwd, bf16_store_bound(acc_bound(fwd_S, D), fwd), bwd, bwd_E


def _pair_grad(gen, B, P):
    g = _randn(gen, B, P) * 0.5
    g[torch.rand(B, P, device=_dev(), generator=gen) < 0.3] = 0.0
    return g.to(torch.bfloat16).contiguous()


@pytest.mark.parametrize("case", INTERACT_CASES, ids=_INTERACT_IDS)
def test_interact_exact(case):
    B, F, D = case
    C = _native()
    gen = _gen(B, F, D)
    V = (_randn(gen, B, F, D) * 0.5).to(torch.bfloat16).contiguous()
    g = _pair_grad(gen, B, F * (F - 1) // 2)
    fwd, fwd_bound, bwd, bwd_E = _interact_reference(V, g)
    _ratio(C.interact_fwd(V), fwd, fwd_bound, f"interact_fwd {case}")
    if not C.interact_feasible(F, D):
        # no backward kernel fits this shape: the binding must say so
        assert case == (3, 65, 256)
        with pytest.raises(RuntimeError, match="exceeds LDS"):
            C.interact_bwd(g, V)
        return
    _ratio(C.interact_bwd(g, V), bwd, bf16_store_bound(bwd_E, bwd),
           f"interact_bwd {case}")


@pytest.mark.parametrize("case", INTERACT_CASES, ids=_INTERACT_IDS)
def test_interact_packed_exact(case):
    """x bf16 [B, D] + slot-major f16 base [S*B, D], S = F - 1.  The kernels
    round base to bf16 (nearest even) while staging, so the operand bits of
    the reference are base.to(bfloat16)."""
    B, F, D = case
    S = F - 1
    C = _native()
    if not C.interact_packed_feasible(F, D):
        assert case == (3, 65, 256)
        return
    gen = _gen(B, F, D, 1)
    x = (_randn(gen, B, D) * 0.5).to(torch.bfloat16).contiguous()
    base = (_randn(gen, S * B, D) * 0.5).to(torch.float16).contiguous()
    g = _pair_grad(gen, B, F * (F - 1) // 2)
    V = torch.cat([x.unsqueeze(1),
                   base.view(S, B, D).permute(1, 0, 2).to(torch.bfloat16)], dim=1)
    fwd, fwd_bound, bwd, bwd_E = _interact_reference(V, g)
    _ratio(C.interact_fwd_packed(x, base), fwd, fwd_bound,
           f"interact_fwd_packed {case}")
    dx, dbase = C.interact_bwd_packed(g, x, base)
    assert dx.dtype == torch.bfloat16 and dbase.dtype == torch.float16
    _ratio(dx, bwd[:, 0], bf16_store_bound(bwd_E[:, 0], bwd[:, 0]),
           f"interact_bwd_packed dx {case}")
    ref_db = bwd[:, 1:].permute(1, 0, 2).reshape(S * B, D)
    E_db = bwd_E[:, 1:].permute(1, 0, 2).reshape(S * B, D)
    _ratio(dbase, ref_db, f16_store_bound(E_db, ref_db),
           f"interact_bwd_packed dbase {case}")
    # how much the subnormal term of the f16 bound matters for this case
    sub = (ref_db != 0) & (ref_db.abs() < 2.0 ** -14)
    if sub.any():
        err = (dbase.double() - ref_db).abs()[sub]
        rel_only = (E_db + REL_F16 * (ref_db.abs() + E_db))[sub]
        print(f"  {int(sub.sum().item())} f16-subnormal references; worst "
              f"err/bound without the 2^-25 term {(err / rel_only).max().item():.4g}")
