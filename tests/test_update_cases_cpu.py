"""Cases, f64 models and per-element bounds of tests/test_gpu_update_exact.py,
and the checks of them that need no GPU.

The sparse update kernels (update_kernel, scatter_update_kernel<HINTS>,
scatter_update_multi_kernel<2|4, HINTS>) all inline csrc/optim.h.  This file
holds

* f64 one-step models of SGD, Adagrad (per column and vectorwise-shared) and
  Adam, written from optim.h: they take the operand BITS the kernel receives
  (the f32 row, the f32-rounded hyper-parameters and beta powers, the
  f16/bf16/f32 gradients, the f32 scales) and do everything downstream in f64,
  `om1 = 1 - beta1`, `c1 = 1/(1 - beta1^t)`, `gsq/dim` and the weight clamp
  included.  The ordered reduction rule of pa_reduce_positions and the row
  rules (missing key, NaN row, empty key) are part of the model;
* a running error bound carried next to every f64 value (class V).  An f32
  operation whose exact result is x adds 2^-24 |x| (round to nearest), plus
  2^-149 where x can be subnormal and the operation is not exact there
  (products, quotients, roots; sums of f32 values are exact in the subnormal
  range).  The error an operand already carries goes through the operation by
  the operation's worst slope over the operand's interval, not only at its
  centre, so the bound also holds at the singular points: sqrt at v = 0,
  rsqrt at a small accumulator, a quotient whose divisor is uncertain.  The
  rounding term is taken on |x| + (error so far), so nothing is first-order
  only and no blanket factor is needed.  A sum that starts from an exact 0
  is exact.  Contracting a*b + c to one fma only removes the rounding of the
  product, so the bound covers either fusion choice of pa_adagrad_acc and
  whatever the compiler contracts elsewhere.  sqrtf and / are correctly
  rounded (the build passes no fast-math flag).  rsqrtf: no ROCm document
  that states its error is installed next to the toolchain this was written
  against, so it is allotted 2 ulp = 4 * 2^-24 |x| (RSQRT_ULPS);
* seeded case generators: arbitrary non-fresh state, non-default
  hyper-parameters that make every term observable, real scales, the
  position lists and the special keys listed at make_case;
* CPU checks: a plain unfused f32 loop that mirrors optim.h meets every
  bound on every case, CpuEmbeddingStore.update_gradients meets them on the
  f32-gradient cases, and six wrong variants of the f32 loop break them, so
  the bounds are neither unreachable nor slack enough to hide those bugs.

Known divergence, left as it is: with a weight bound set, pa_clamp_weight
(fminf/fmaxf) turns a NaN weight into -bound, torch's clamp_ in
ops/reference.py keeps the NaN.  The only way to a NaN weight from a finite
row is Adam with an inf gradient (inf/inf), so the f32-gradient Adam cases
that the CPU store is held to run without a weight bound.
"""
import functools

import numpy as np
import pytest
import torch

from persia_amd.core import hashing
from persia_amd.core.store import CpuEmbeddingStore
from persia_amd.embedding import EmbeddingConfig
from persia_amd.embedding.optim import SGD, Adagrad, Adam

U32 = 2.0 ** -24        # unit roundoff of f32
TINY32 = 2.0 ** -149    # smallest f32 subnormal
MINN32 = 2.0 ** -126    # smallest f32 normal
RSQRT_ULPS = 2          # see the module docstring

F32 = np.float32


def _f(x):
    return np.asarray(x, dtype=np.float32)


# ------------------------------------------------------- running error bound


class V:
    """f64 value(s) `v` of an expression and a bound `e` on |f32 result - v|."""

    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) + np.asarray(e, dtype=np.float64)

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])


def C(x):
    """A constant as the kernel holds it: rounded to f32 once, then exact."""
    return V(np.float64(np.float32(x)))


def _rounded(v, e, units=1, inexact_subnormal=True):
    """The f32 operation rounds a value within e of v."""
    with np.errstate(all="ignore"):
        r = e + units * U32 * (np.abs(v) + e)
        if inexact_subnormal:  # an exact 0 comes from an exact 0 operand
            sub = (np.abs(v) - e < MINN32) & ~((v == 0) & (e == 0))
            r = r + np.where(sub, TINY32, 0.0)
    return V(v, r)


def v_add(a, b, sign=1.0):
    with np.errstate(all="ignore"):
        v = a.v + sign * b.v
        out = _rounded(v, a.e + b.e, inexact_subnormal=False)
        # adding to an exact zero is exact
        exact = ((a.v == 0) & (a.e == 0)) | ((b.v == 0) & (b.e == 0))
        out.e = np.where(exact, a.e + b.e, out.e)
    return out


def v_sub(a, b):
    return v_add(a, b, -1.0)


def v_mul(a, b):
    with np.errstate(all="ignore"):
        e = np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e
        return _rounded(a.v * b.v, np.where((a.e == 0) & (b.e == 0), 0.0, e))


def v_div(a, b):
    with np.errstate(all="ignore"):
        q = a.v / b.v
        lo = np.abs(b.v) - b.e  # the divisor's smallest magnitude
        e = np.where(lo > 0, (a.e + np.abs(q) * b.e) / lo, np.inf)
        e = np.where((a.e == 0) & (b.e == 0), 0.0, e)
        return _rounded(q, e)


def v_sqrt(a):
    """|sqrt(x') - sqrt(x)| over |x' - x| <= e, x' >= 0: the larger of the two
    one-sided differences, each written without cancellation."""
    with np.errstate(all="ignore"):
        r = np.sqrt(a.v)
        lo = np.sqrt(np.maximum(a.v - a.e, 0.0))
        hi = np.sqrt(a.v + a.e)
        down = np.where(a.v >= a.e, a.e / np.maximum(r + lo, 1e-300), r)
        up = a.e / np.maximum(hi + r, 1e-300)
        e = np.where(a.e == 0, 0.0, np.maximum(down, up))
        return _rounded(r, e)


def v_rsqrt(a):
    """x^-1/2 is convex and decreasing: the worst point is x - e."""
    with np.errstate(all="ignore"):
        r = a.v ** -0.5
        lo = a.v - a.e
        slo, sx = np.sqrt(np.maximum(lo, 0.0)), np.sqrt(a.v)
        e = np.where(lo > 0, a.e / ((sx + slo) * sx * slo), np.inf)
        e = np.where(a.e == 0, 0.0, e)
        return _rounded(r, e, units=2 * RSQRT_ULPS)  # 1 ulp <= 2 * 2^-24 |r|


def v_clamp(a, bound32):
    """pa_clamp_weight: fminf(fmaxf(w, -b), b) when b > 0 -- exact, 1-Lipschitz,
    and a NaN w comes out as -b."""
    b = float(np.float32(bound32))
    if not b > 0.0:
        return a
    # an inf or NaN w clamps to exactly +-b
    return V(np.fmin(np.fmax(a.v, -b), b), np.where(np.isfinite(a.v), a.e, 0.0))


# ------------------------------------------------------------ optimizer args

OPTS = ("sgd", "adagrad", "adagrad_shared", "adam")


def make_optimizer(optname, init_acc=0.01, dyadic_betas=False):
    """Non-default everywhere, so every term of optim.h moves the result."""
    if optname == "sgd":
        return SGD(lr=0.07, weight_decay=0.03)
    if optname in ("adagrad", "adagrad_shared"):
        return Adagrad(lr=0.05, initial_accumulator_value=init_acc,
                       g_square_momentum=0.9, eps=3e-7,
                       vectorwise_shared=optname == "adagrad_shared")
    # dyadic betas: 1 - beta and 1 - beta^3 are the same number whether the
    # subtraction is done on the f32-rounded operand (kernel) or in f64 before
    # rounding (CpuEmbeddingStore) -- see test_cpu_store_meets_bounds
    betas = (0.875, 0.9921875) if dyadic_betas else (0.85, 0.995)
    return Adam(lr=0.004, betas=betas, eps=2e-6)


def opt_params(opt):
    """(code, p0..p3) as store.py _opt_params hands them to the kernels."""
    if isinstance(opt, SGD):
        return 0, (opt.lr, opt.weight_decay, 0.0, 0.0)
    if isinstance(opt, Adagrad):
        return 1, (opt.lr, opt.g_square_momentum, opt.eps,
                   1.0 if opt.vectorwise_shared else 0.0)
    return 2, (opt.lr, opt.betas[0], opt.betas[1], opt.eps)


def row_width(opt, dim):
    return dim + opt.require_space(dim)


# ------------------------------------------------------------- the f64 model


def model_reduce(grads64, perm, ustarts, seg_id, seg_scale, n, dim):
    """pa_reduce_positions for keys 0..n-1 -> V [n, dim].  grads64: the
    gradient bits widened to f64.  Round r handles the r-th position of every
    key that has one, so the order within a key is the kernel's."""
    lo = ustarts[:n].astype(np.int64)
    lens = ustarts[1:n + 1].astype(np.int64) - lo
    acc = V(np.zeros((n, dim)))
    for r in range(int(lens.max()) if n else 0):
        ks = np.nonzero(lens > r)[0]
        s = seg_id[perm[lo[ks] + r]]
        live = s >= 0
        if seg_scale is not None:
            live = live & (np.where(s >= 0, seg_scale[np.maximum(s, 0)], 0) != 0)
        ks, s = ks[live], s[live]
        if not len(ks):
            continue
        term = V(grads64[s])
        if seg_scale is not None:
            term = v_mul(term, V(seg_scale[s].astype(np.float64)[:, None]))
        new = v_add(acc[ks], term)
        acc.v[ks], acc.e[ks] = new.v, new.e
    return acc


def model_optimizer(opt, wb, powers, rows32, g, dim):
    """One step of optim.h on every row -> V [n, row_width]."""
    code, (p0, p1, p2, p3) = opt_params(opt)
    P0, P1, P2, P3 = C(p0), C(p1), C(p2), C(p3)
    rows = np.asarray(rows32, dtype=np.float32).astype(np.float64)
    w = V(rows[:, :dim])
    if code == 0:
        wn = v_sub(w, v_mul(P0, v_add(g, v_mul(P1, w))))
        out = [v_clamp(wn, wb)]
    elif code == 1:
        shared = float(np.float32(p3)) > 0.5
        acc = V(rows[:, dim:dim + 1] if shared else rows[:, dim:2 * dim])
        wn = v_sub(w, v_mul(v_mul(P0, g), v_rsqrt(v_add(acc, P2))))
        if shared:
            gg = v_mul(g, g)
            gsq = V(np.zeros((rows.shape[0], 1)))
            for c in range(dim):  # dim additions in some order; terms >= 0
                gsq = v_add(gsq, gg[:, c:c + 1])
            an = v_add(v_mul(acc, P1), v_div(gsq, V(float(dim))))
        else:
            an = v_add(v_mul(acc, P1), v_mul(g, g))
        out = [v_clamp(wn, wb), an]
    else:
        b1p, b2p = powers
        one = V(1.0)
        om1, om2 = v_sub(one, P1), v_sub(one, P2)
        c1 = v_div(one, v_sub(one, C(b1p)))
        c2 = v_div(one, v_sub(one, C(b2p)))
        m, v = V(rows[:, dim:2 * dim]), V(rows[:, 2 * dim:3 * dim])
        mn = v_add(v_mul(P1, m), v_mul(om1, g))
        vn = v_add(v_mul(P2, v), v_mul(v_mul(om2, g), g))
        step = v_div(v_mul(P0, v_mul(mn, c1)), v_add(P3, v_sqrt(v_mul(vn, c2))))
        out = [v_clamp(v_sub(w, step), wb), mn, vn]
    return V(np.concatenate([o.v for o in out], axis=1),
             np.concatenate([o.e for o in out], axis=1))


class Expected:
    """rows: V [n, row_width] after the call; misses/nans: the two skip
    counters' increments; touched: which keys' rows the call writes."""

    def __init__(self, rows, misses, nans, touched):
        self.rows, self.misses, self.nans, self.touched = rows, misses, nans, touched


def model_step(case, rows32, resident, powers=None):
    """The whole call on keys 0..n-1 of the case.  rows32 [n, row_width]: the
    rows before the call (any value where not resident)."""
    n, dim = case.n, case.dim
    g = model_reduce(case.grads64, case.perm, case.ustarts, case.seg_id,
                     case.seg_scale, n, dim)
    stepped = model_optimizer(case.opt, case.wb, powers or case.powers,
                              rows32, g, dim)
    nonempty = case.keys[:n] != 0
    miss = nonempty & ~resident
    nan = nonempty & resident & np.isnan(g.v).any(axis=1)
    touched = nonempty & resident & ~nan
    before = np.asarray(rows32, dtype=np.float32).astype(np.float64)
    rows = V(np.where(touched[:, None], stepped.v, before),
             np.where(touched[:, None], stepped.e, 0.0))
    return Expected(rows, int(miss.sum()), int(nan.sum()), touched)


def worst_ratio(got32, ref, rows=None):
    """max |got - v| / e over the elements whose model value is finite; an
    element whose model value is inf or NaN must be that same inf, or NaN.
    -> inf when any element fails outright."""
    got = np.asarray(got32, dtype=np.float32).astype(np.float64)
    v, e = ref.v, ref.e
    if rows is not None:
        got, v, e = got[rows], v[rows], e[rows]
    with np.errstate(all="ignore"):
        fin = np.isfinite(v)
        same = np.where(np.isnan(v), np.isnan(got), got == v)
        if not same[~fin].all() or not np.isfinite(got[fin]).all():
            return np.inf
        d = np.abs(got - v)[fin]
        ratio = np.where(d == 0, 0.0, d / np.maximum(e[fin], 1e-300))
    return float(ratio.max()) if ratio.size else 0.0


# ------------------------------------------------------------ case generators

# dim -> the scatter_update variant that takes it
PACKED_DIMS = (1, 2, 4, 8, 16, 32)       # 64/dim keys per wave
QUAD_DIMS = (3, 24, 48, 64, 128)         # four keys per wave
DUAL_DIMS = (129, 192, 256)              # two keys per wave
SINGLE_DIMS = (257, 320, 512)            # one key per wave
ALL_DIMS = PACKED_DIMS + QUAD_DIMS + DUAL_DIMS + SINGLE_DIMS
# the weight bound bites on about half of every variant's dims
BOUND_DIMS = (1, 4, 16, 3, 48, 128, 192, 320)
WEIGHT_BOUND = 0.3
ADAM_STEP = 3  # one-step cases run the third step's beta powers

# special keys, first in every reduce-kind case; single-position keys follow
(K_MULTI, K_HOT, K_DEAD, K_ZERO_SCALE, K_MISSING, K_NAN, K_INF_NAN, K_INF,
 K_ZERO_STATE) = range(9)
N_SPECIAL = 12  # 9 named + 3 plain single keys: whole waves of 2 and 4 keys
HOT_POSITIONS = 300
N_PAD_EXTRA = 13
N_FILLER = 200  # resident rows no update ever names


def keys_per_wave(dim):
    if dim < 64 and 64 % dim == 0:
        return 64 // dim
    return 4 if dim <= 128 else 2 if dim <= 256 else 1


def case_keys(dim):
    """64 k + 3 keys: the last wave is partial at 2, at 4 and at 64/dim keys
    per wave, and scatter_update launches at least three blocks of four
    waves."""
    return 64 * max(5, (3 * 4 * keys_per_wave(dim) + 63) // 64) + 3


def mix(signs):
    return hashing.splitmix64(np.asarray(signs, dtype=np.uint64)).view(np.int64)


class Case:
    pass


def _state_rows(rng, opt, n, dim):
    """Arbitrary non-fresh rows: weights in +-0.5, accumulators and v over
    fourteen decades and exactly 0 in places, m of both signs."""
    code, _ = opt_params(opt)
    w = rng.uniform(-0.5, 0.5, (n, dim))
    if code == 0:
        return _f(w)
    ns = opt.require_space(dim)
    if code == 1:
        acc = 10.0 ** rng.uniform(-12, 2, (n, ns))
        acc[rng.random((n, ns)) < 0.1] = 0.0
        return _f(np.concatenate([w, acc], axis=1))
    m = 10.0 ** rng.uniform(-6, 0, (n, dim)) * rng.choice([-1.0, 1.0], (n, dim))
    v = 10.0 ** rng.uniform(-12, 1, (n, dim))
    zero = rng.random((n, dim)) < 0.1
    v[zero] = 0.0
    m[zero & (rng.random((n, dim)) < 0.7)] = 0.0
    return _f(np.concatenate([w, m, v], axis=1))


_TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
SCALE_MODES = ("rsqrt", "loss", "null")


def make_case(dim, optname, gdtype="f16", kind="reduce", scale_mode=None,
              seed=0, n=None, init_acc=0.01, dyadic_betas=False, wb=None):
    """One update call on `n` unique keys (padded with empty keys to n_pad and
    counted by a device-side u_count).

    kind "reduce": positions, perm, seg_id and seg_scale as the fused kernels
    and grad_scatter read them.  Keys 0..8 are, in order: a key of 2-5
    positions; a hot key of 300 positions, one of them dead and, where there
    are scales, one scaled by 0 whose gradient is NaN; a key whose positions
    all have seg_id < 0; a key whose scales are all 0 (its gradients NaN), or
    a second dead key without scales; a key that is not in the table; a key
    with a NaN gradient; a key of two positions holding +inf and -inf in one
    column; a key with a lone +inf; a key with a zero gradient on a row whose
    state is 0.  Every other key has one position, so the waves past key 11
    are all-single ones.
    kind "rows": one f32 gradient row per key and nothing to reduce, which is
    store_update's input; the special keys that exist are the missing, NaN,
    lone-inf and zero-state ones.

    scale_mode: "rsqrt" 1/sqrt(k), "loss" the same times a loss-scale
    reciprocal of 1/1024, "null" no seg_scale array."""
    c = Case()
    rng = np.random.default_rng([seed, dim, OPTS.index(optname),
                                 ("f16", "bf16", "f32").index(gdtype)])
    c.dim, c.optname, c.gdtype, c.kind = dim, optname, gdtype, kind
    c.opt = make_optimizer(optname, init_acc, dyadic_betas)
    c.wb = (WEIGHT_BOUND if dim in BOUND_DIMS else 0.0) if wb is None else wb
    c.powers = None
    if optname == "adam":
        c.powers = tuple(b ** ADAM_STEP for b in c.opt.betas)
    c.n = n = case_keys(dim) if n is None else n
    c.n_pad = n + N_PAD_EXTRA
    c.rw = row_width(c.opt, dim)
    if kind != "reduce":
        scale_mode = "null"
    elif scale_mode is None:  # every mode meets every optimizer and variant
        i = ALL_DIMS.index(dim) if dim in ALL_DIMS else 0
        scale_mode = SCALE_MODES[(i + OPTS.index(optname)) % 3]
    c.scale_mode = scale_mode

    c.signs = np.arange(1, n + 1, dtype=np.uint64) + np.uint64(1000 * dim)
    c.keys = np.concatenate([mix(c.signs), np.zeros(N_PAD_EXTRA, np.int64)])
    c.resident = np.ones(n, dtype=bool)
    c.resident[K_MISSING] = False
    c.rows = _state_rows(rng, c.opt, n, dim)
    c.rows[K_ZERO_STATE, dim:] = 0.0
    c.filler_signs = np.arange(1, N_FILLER + 1, dtype=np.uint64) + np.uint64(1 << 40)
    c.filler_rows = _state_rows(rng, c.opt, N_FILLER, dim)

    lens = np.ones(n, dtype=np.int64)
    if kind == "reduce":
        lens[K_MULTI] = 2 + (dim + OPTS.index(optname)) % 4
        lens[K_HOT] = HOT_POSITIONS
        lens[K_DEAD] = 3
        lens[K_ZERO_SCALE] = 2
        lens[K_INF_NAN] = 2
    nnz = int(lens.sum())
    c.ustarts = np.zeros(c.n_pad + 1, dtype=np.int64)
    c.ustarts[1:n + 1] = np.cumsum(lens)
    c.ustarts[n + 1:] = nnz
    if kind == "reduce":
        c.perm = rng.permutation(nnz).astype(np.int64)
        c.seg_id = rng.permutation(nnz).astype(np.int64)
    else:
        c.perm = np.arange(nnz, dtype=np.int64)
        c.seg_id = np.arange(nnz, dtype=np.int64)

    def positions(u):  # position indices (values of perm) of key u
        return c.perm[c.ustarts[u]:c.ustarts[u + 1]]

    g = rng.standard_normal((nnz, dim))
    g[rng.random((nnz, dim)) < 0.05] = 0.0
    if scale_mode == "null":
        c.seg_scale = None
    else:
        sc = 1.0 / np.sqrt(rng.integers(1, 10, nnz).astype(np.float64))
        c.seg_scale = _f(_f(sc) * F32(1.0 / 1024 if scale_mode == "loss" else 1.0))
    g[c.seg_id[positions(K_ZERO_STATE)]] = 0.0
    g[c.seg_id[positions(K_NAN)[0]], dim // 2] = np.nan
    g[c.seg_id[positions(K_INF)[0]], 0] = np.inf
    if kind == "reduce":
        pa, pb = positions(K_INF_NAN)
        g[c.seg_id[pa], dim - 1], g[c.seg_id[pb], dim - 1] = np.inf, -np.inf
        hot = positions(K_HOT)
        dead = [hot[17]] + list(positions(K_DEAD))
        zero = list(positions(K_ZERO_SCALE))
        if c.seg_scale is None:
            dead += zero
        else:
            zero.append(hot[101])
            for p in zero:
                c.seg_scale[c.seg_id[p]] = 0.0
                g[c.seg_id[p]] = np.nan
        for p in dead:
            g[c.seg_id[p]] = 7.0  # must never be read into the sum
        c.dead_rows = c.seg_id[np.array(dead)].copy()
        c.seg_id[np.array(dead)] = -1
    c.grads = torch.from_numpy(g).to(_TORCH_DT[gdtype])
    c.grads64 = c.grads.double().numpy()
    # a column that stays finite only because of eps exists
    z = c.rows[K_ZERO_STATE]
    assert (z[dim:] == 0).all()
    return c


@functools.lru_cache(maxsize=None)
def cached_case(dim, optname, gdtype="f16", kind="reduce", scale_mode=None,
                init_acc=0.01, dyadic_betas=False):
    """Shared read-only between tests."""
    return make_case(dim, optname, gdtype, kind, scale_mode,
                     init_acc=init_acc, dyadic_betas=dyadic_betas)


def stride_case(dim, n, seed=0):
    """Grid-stride cases: SGD, n single-position f16 keys (or f32 rows for
    dim 4 / update_kernel), no special keys but a missing one; keys that
    overflow their probe window at insert are found by the probe and become
    misses too."""
    kind = "rows" if dim == 4 else "reduce"
    rng = np.random.default_rng([seed, dim, n])
    c = Case()
    c.dim, c.optname, c.kind = dim, "sgd", kind
    c.gdtype = "f32" if kind == "rows" else "f16"
    c.opt, c.wb, c.powers = make_optimizer("sgd"), WEIGHT_BOUND, None
    c.n, c.n_pad, c.rw = n, n + N_PAD_EXTRA, dim
    c.signs = np.arange(1, n + 1, dtype=np.uint64) + np.uint64(7 << 32)
    c.keys = np.concatenate([mix(c.signs), np.zeros(N_PAD_EXTRA, np.int64)])
    c.resident = np.ones(n, dtype=bool)
    c.resident[K_MISSING] = False
    c.rows = _f(rng.uniform(-0.5, 0.5, (n, dim)))
    c.filler_signs = np.zeros(0, dtype=np.uint64)
    c.filler_rows = np.zeros((0, dim), dtype=np.float32)
    c.ustarts = np.minimum(np.arange(c.n_pad + 1, dtype=np.int64), n)
    c.perm = rng.permutation(n).astype(np.int64) if kind == "reduce" \
        else np.arange(n, dtype=np.int64)
    c.seg_id = np.arange(n, dtype=np.int64)
    c.scale_mode = "rsqrt" if kind == "reduce" else "null"
    c.seg_scale = _f(1.0 / np.sqrt(rng.integers(1, 10, n))) \
        if kind == "reduce" else None
    c.grads = torch.from_numpy(rng.standard_normal((n, dim))).to(
        _TORCH_DT[c.gdtype])
    c.grads64 = c.grads.double().numpy()
    return c


# capacity of the grid-stride tables: load factor ~0.26 (n / capacity)
STRIDE_UPDATE = dict(dim=4, n=65536 + 4 * 1000 + 3, capacity=1 << 18)
STRIDE_QUAD = dict(dim=3, n=262144 + 4 * 2000 + 3, capacity=1 << 20)
# Not built: a grid-stride case of the packed kernel at dim 1 needs more than
# 64 * 4 * 16384 = 4.2 M keys, whose f64 model and position lists alone take
# longer than the few seconds a test may; the two-keys-per-wave kernel needs
# more than 131072 keys of dim >= 129, an arena of over 256 MB.  Their
# grid-stride loops are the same line as the four-key kernel's.


# ------------------------------------------------- the plain f32 mirror loop

BUGS = ("moments_swapped", "eps_dropped", "momentum_ignored", "stale_power",
        "dropped_addend", "zero_scale_nan")


def f32_reduce(case, bug=None):
    """pa_reduce_positions in unfused f32, position by position."""
    n, dim = case.n, case.dim
    g32 = case.grads.float().numpy()
    out = np.zeros((n, dim), dtype=np.float32)
    with np.errstate(all="ignore"):
        for u in range(n):
            acc = np.zeros(dim, dtype=np.float32)
            lo, hi = int(case.ustarts[u]), int(case.ustarts[u + 1])
            drop = lo + 5 if bug == "dropped_addend" and hi - lo > 100 else -1
            for p in range(lo, hi):
                s = case.seg_id[case.perm[p]]
                if s < 0 or p == drop:
                    continue
                sc = F32(1.0) if case.seg_scale is None else case.seg_scale[s]
                if sc == 0 and bug != "zero_scale_nan":
                    continue
                acc = acc + g32[s] * sc
            out[u] = acc
    return out


def f32_optimizer(opt, wb, powers, rows, g, dim, bug=None):
    """optim.h in unfused numpy f32 (every operand an np.float32)."""
    code, ps = opt_params(opt)
    p0, p1, p2, p3 = (F32(p) for p in ps)
    wb = F32(wb)
    rows = np.array(rows, dtype=np.float32)
    w = rows[:, :dim]
    one = F32(1.0)

    def clamp(x):
        return np.fmin(np.fmax(x, -wb), wb) if wb > 0 else x

    with np.errstate(all="ignore"):
        if code == 0:
            rows[:, :dim] = clamp(w - p0 * (g + p1 * w))
        elif code == 1:
            shared = p3 > 0.5
            acc = rows[:, dim:dim + 1] if shared else rows[:, dim:]
            eps = F32(0.0) if bug == "eps_dropped" else p2
            mom = one if bug == "momentum_ignored" else p1
            wn = clamp(w - p0 * g * (one / np.sqrt(acc + eps)))
            if shared:
                gsq = np.zeros((rows.shape[0], 1), dtype=np.float32)
                for c in range(dim):
                    gsq = gsq + g[:, c:c + 1] * g[:, c:c + 1]
                an = acc * mom + gsq / F32(dim)
            else:
                an = acc * mom + g * g
            rows[:, :dim], rows[:, dim:] = wn, an
        else:
            b1p, b2p = (F32(p) for p in powers)
            eps = F32(0.0) if bug == "eps_dropped" else p3
            om1, om2 = one - p1, one - p2
            c1, c2 = one / (one - b1p), one / (one - b2p)
            m, v = rows[:, dim:2 * dim], rows[:, 2 * dim:]
            if bug == "moments_swapped":
                m, v = v, m
            mn = p1 * m + om1 * g
            vn = p2 * v + om2 * g * g
            wn = clamp(w - p0 * (mn * c1) / (eps + np.sqrt(vn * c2)))
            rows[:, :dim], rows[:, dim:2 * dim], rows[:, 2 * dim:] = wn, mn, vn
    assert rows.dtype == np.float32
    return rows


def f32_step(case, rows32, resident, powers=None, bug=None):
    """-> (rows after, misses, nans) of the mirror loop."""
    powers = powers or case.powers
    if bug == "stale_power":
        powers = tuple(p / b for p, b in zip(powers, case.opt.betas))
    g = f32_reduce(case, bug)
    stepped = f32_optimizer(case.opt, case.wb, powers, rows32, g, case.dim, bug)
    nonempty = case.keys[:case.n] != 0
    nan = nonempty & resident & np.isnan(g).any(axis=1)
    touched = nonempty & resident & ~nan
    out = np.where(touched[:, None], stepped, np.asarray(rows32, np.float32))
    return out, int((nonempty & ~resident).sum()), int(nan.sum())


# ------------------------------------------------------------------ CPU checks

# one dim per kernel variant and row shape keeps the CPU suite quick; the GPU
# file runs every dim
CPU_DIMS = (1, 16, 3, 64, 129, 257)


def _grid():
    for dim in CPU_DIMS:
        for optname in OPTS:
            yield dim, optname


@pytest.mark.parametrize("dim,optname", list(_grid()))
def test_f32_loop_meets_every_bound(dim, optname):
    case = cached_case(dim, optname)
    exp = model_step(case, case.rows, case.resident)
    got, misses, nans = f32_step(case, case.rows, case.resident)
    assert (misses, nans) == (exp.misses, exp.nans) == (1, 2)
    r = worst_ratio(got, exp.rows)
    print(f"dim {dim} {optname}: f32 loop err/bound {r:.3f}")
    assert r <= 1.0
    # the lone inf was applied, the zero-gradient keys stepped
    w_inf = exp.rows.v[K_INF, 0]  # -inf, Adam's inf/inf, or either clamped
    assert exp.touched[K_INF]
    assert w_inf == -np.float32(case.wb) if case.wb else not np.isfinite(w_inf)
    assert exp.touched[K_DEAD] and exp.touched[K_ZERO_SCALE]


@pytest.mark.parametrize("gdtype", ["f32", "bf16"])
@pytest.mark.parametrize("optname", OPTS)
def test_f32_loop_meets_bounds_other_gradient_types(optname, gdtype):
    for dim in (24, 320):
        case = cached_case(dim, optname, gdtype, dyadic_betas=True)
        exp = model_step(case, case.rows, case.resident)
        got, misses, nans = f32_step(case, case.rows, case.resident)
        assert (misses, nans) == (exp.misses, exp.nans)
        assert worst_ratio(got, exp.rows) <= 1.0


def _applies(bug, optname):
    return {
        "moments_swapped": optname == "adam",
        "eps_dropped": optname != "sgd",
        "momentum_ignored": optname in ("adagrad", "adagrad_shared"),
        "stale_power": optname == "adam",
        "dropped_addend": True,
        "zero_scale_nan": True,
    }[bug]


@pytest.mark.parametrize("bug", BUGS)
def test_wrong_variants_break_the_bound(bug):
    """Each wrong variant of the f32 loop fails, on every optimizer it can
    touch and at a packed, a multi-key and a one-key dim."""
    ran = 0
    for dim in (16, 64, 257):
        for optname in OPTS:
            if not _applies(bug, optname):
                continue
            # zero_scale_nan needs a scale array to hold a 0
            case = cached_case(dim, optname, "f16", "reduce",
                               "rsqrt" if bug == "zero_scale_nan" else None)
            exp = model_step(case, case.rows, case.resident)
            got, misses, nans = f32_step(case, case.rows, case.resident, bug=bug)
            r = worst_ratio(got, exp.rows)
            assert r > 1.0 or (misses, nans) != (exp.misses, exp.nans), (
                bug, dim, optname, r)
            ran += 1
    assert ran >= 3


def test_eps_is_what_keeps_the_zero_state_row_finite():
    for optname in ("adagrad", "adagrad_shared", "adam"):
        case = cached_case(64, optname)  # no weight bound to clamp the NaN
        exp = model_step(case, case.rows, case.resident)
        assert np.isfinite(exp.rows.v[K_ZERO_STATE]).all()
        got, _, _ = f32_step(case, case.rows, case.resident, bug="eps_dropped")
        assert np.isnan(got[K_ZERO_STATE, :64]).all()


def _cpu_store(case):
    store = CpuEmbeddingStore(
        case.dim, 4096, case.opt,
        EmbeddingConfig(emb_initialization=(-0.5, 0.5), weight_bound=case.wb))
    store.import_rows(case.signs[case.resident], case.rows[case.resident])
    if case.powers:
        store.beta1_power, store.beta2_power = case.powers
    return store


def _export(store, case):
    signs, inner = store.export_keys(case.signs)
    assert np.array_equal(signs, case.signs[case.resident])
    rows = case.rows.copy()
    rows[case.resident] = inner
    return rows


@pytest.mark.parametrize("optname", OPTS)
@pytest.mark.parametrize("dim", [8, 24, 320])
def test_cpu_store_meets_bounds(dim, optname):
    """CpuEmbeddingStore.update_gradients on the f32-gradient cases, fed the
    f32 loop's reduced gradient.  It computes 1 - beta and 1 - beta^t in f64
    before rounding where the kernel subtracts the rounded operands, which is
    the same number only for dyadic betas, and its clamp keeps a NaN (module
    docstring), so the Adam cases run without a bound."""
    case = cached_case(dim, optname, "f32", dyadic_betas=True) \
        if optname != "adam" else _adam_f32_case(dim)
    exp = model_step(case, case.rows, case.resident)
    store = _cpu_store(case)
    reduced = torch.from_numpy(f32_reduce(case))
    keys = torch.from_numpy(case.keys[:case.n].copy())
    assert store.update_gradients(keys, reduced) == exp.misses == 1
    r = worst_ratio(_export(store, case), exp.rows, rows=case.resident)
    print(f"dim {dim} {optname}: CpuEmbeddingStore err/bound {r:.3f}")
    assert r <= 1.0
    # NaN by reduction (+inf + -inf) and NaN gradient: rows untouched; every
    # position dead or scaled by 0: a zero-gradient step, not a skip
    after = _export(store, case)
    for u in (K_NAN, K_INF_NAN):
        assert np.array_equal(after[u], case.rows[u])
        assert not exp.touched[u]
    red = reduced.numpy()
    assert np.isnan(red[K_INF_NAN]).any() and not red[K_DEAD].any()
    assert exp.touched[K_DEAD] and exp.touched[K_ZERO_SCALE]
    if optname != "adagrad_shared":
        assert not np.array_equal(after[K_DEAD], case.rows[K_DEAD])


@functools.lru_cache(maxsize=None)
def _adam_f32_case(dim):
    return make_case(dim, "adam", "f32", dyadic_betas=True, wb=0.0)


def test_zero_gradient_step_moves_the_row():
    """SGD weight decay and Adam momentum move the weights of a key with no
    contributing position; Adagrad and Adam state decays."""
    for optname in OPTS:
        case = cached_case(64, optname)
        exp = model_step(case, case.rows, case.resident)
        before = case.rows[K_DEAD].astype(np.float64)
        after = exp.rows.v[K_DEAD]
        if optname in ("sgd", "adam"):
            assert (after[:64] != before[:64]).any()
        else:
            assert np.array_equal(after[:64], before[:64])
        if optname != "sgd":
            assert (np.abs(after[64:]) <= np.abs(before[64:])).all()
            assert (after[64:] != before[64:]).any()


def test_case_shapes_cover_the_partial_waves():
    for dim in ALL_DIMS:
        n, kpw = case_keys(dim), keys_per_wave(dim)
        assert n % 2 == 1 and n % 4 == 3
        assert kpw == 1 or n % kpw != 0
        assert n > 3 * 4 * kpw  # more than three blocks of four waves
    assert N_SPECIAL % 4 == 0


def test_stride_generator_overflows_under_one_percent():
    """The grid-stride cases' generator at a sixteenth of the size and the
    same load factor, on the sequential oracle: the keys that find no slot at
    insert stay under 1 % (here: none)."""
    for spec in (STRIDE_UPDATE, STRIDE_QUAD):
        n, cap = spec["n"] // 16, spec["capacity"] // 16
        case = stride_case(spec["dim"], n)
        store = CpuEmbeddingStore(case.dim, cap, case.opt, EmbeddingConfig())
        store.import_rows(case.signs, case.rows)
        assert len(store) >= 0.99 * n
