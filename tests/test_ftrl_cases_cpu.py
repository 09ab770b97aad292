"""Cases, f64 model and per-element bounds of the FTRL-Proximal optimizer
(csrc/optim.h pa_ftrl, opt code 3), and the checks of them that need no GPU.
tests/test_gpu_ftrl_exact.py holds the kernels to the same model.

The bound machinery (class V, the v_* operations, model_reduce, worst_ratio,
make_case) is that of tests/test_update_cases_cpu.py, with its rules: operand
bits in, 2^-24 per f32 operation, the subnormal term, errors carried through
the worst slope.  The model is written from optim.h:

    ilr   = 1 / lr                      (rounded once, pa_opt_args)
    n1    = n + g*g                     (an fma in the kernel: one rounding
                                         fewer, which the bound covers)
    s1    = sqrt(n1);  s0 = sqrt(n)
    sigma = (s1 - s0) * ilr
    z1    = z + (g - sigma*w)
    q     = (beta + s1) * ilr + l2
    w1    = clamp_weight((clip(z1, -l1, +l1) - z1) / q)

clip is exact and 1-Lipschitz; its result carries no error where |z1| is
beyond l1 by more than z1's bound, and where |z1| is inside l1 by at least
that bound clip(z1) and z1 are the same f32 number, so their difference is an
exact 0.  There is no slack factor.

There is no reference implementation of FTRL to compare against; that the
formula is FTRL is checked by test_equals_online_gradient_descent.

Cases: make_case(dim, "adam", ...) has FTRL's row width and the right kind of
state (m of both signs for z; v >= 0 over fourteen decades with exact zeros
for n; the all-zero-state row).  ftrl_case() takes its geometry and gradients
and swaps in an Ftrl whose parameters make every term observable.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import test_engine_paths as P
import test_update_cases_cpu as UC
from test_update_cases_cpu import (  # noqa: F401  (v_clamp, make_case: re-exported)
    C, V, make_case, model_reduce, v_add, v_clamp, v_div, v_mul, v_sqrt,
    v_sub, worst_ratio,
)

from persia_amd.core.store import CpuEmbeddingStore, make_store
from persia_amd.embedding import EmbeddingConfig
from persia_amd.embedding.optim import SGD, Ftrl

F32 = np.float32

# non-default everywhere: every term of the step moves the result
FTRL = dict(lr=0.06, beta=0.7, l1=0.4, l2=0.02)
# the same, every parameter an f32 number (see test_cpu_store_meets_bounds)
FTRL_DYADIC = dict(lr=0.0625, beta=0.75, l1=0.375, l2=0.015625)

# one dim per lane layout and row shape: packed 1, 4, 16; four keys per wave
# 3, 64; two keys 129; one key 257
DIMS = (1, 4, 16, 3, 64, 129, 257)


# ------------------------------------------------------------------ the cases


def ftrl_case(dim, gdtype="f16", kind="reduce", wb=None, seed=0, opt=None,
              scale_mode=None):
    """make_case's Adam case of this shape with an Ftrl in the optimizer's
    place: same keys, rows, positions, scales and gradients."""
    c = make_case(dim, "adam", gdtype, kind, scale_mode, seed=seed, wb=wb)
    c.opt = opt if opt is not None else Ftrl(**FTRL)
    c.optname, c.powers = "ftrl", None
    assert c.rw == dim + c.opt.require_space(dim)
    return c


@functools.lru_cache(maxsize=None)
def _cached(dim, gdtype, kind, wb):
    return ftrl_case(dim, gdtype, kind, wb)


def cached_case(dim, gdtype="f16", kind="reduce", wb=None):
    """Shared read-only between tests (the GPU file included)."""
    return _cached(dim, gdtype, kind, wb)


# -------------------------------------------------------------- the f64 model


def v_shrink(z, l1_32):
    """clip(z, -l1, +l1) - z as the kernel computes it."""
    l1 = float(np.float32(l1_32))
    with np.errstate(all="ignore"):
        beyond = np.abs(z.v) - l1 > z.e
        clip = V(np.clip(z.v, -l1, l1), np.where(beyond, 0.0, z.e))
        d = v_sub(clip, z)
        inside = np.abs(z.v) + z.e <= l1
        return V(np.where(inside, 0.0, d.v), np.where(inside, 0.0, d.e))


def model_optimizer(opt, wb, rows, g, dim, f32_rows=True):
    """One pa_ftrl step on every row -> V [n, 3*dim].  f32_rows=False takes
    the rows as the f64 numbers they are (test_equals_online_gradient_descent
    chains the model's own values)."""
    LR, BETA, L2 = C(opt.lr), C(opt.beta), C(opt.l2)
    if f32_rows:
        rows = np.asarray(rows, dtype=np.float32)
    rows = np.asarray(rows).astype(np.float64)
    w, z, n = (V(rows[:, i * dim:(i + 1) * dim]) for i in range(3))
    ilr = v_div(V(1.0), LR)
    n1 = v_add(n, v_mul(g, g))
    s1, s0 = v_sqrt(n1), v_sqrt(n)
    sigma = v_mul(v_sub(s1, s0), ilr)
    z1 = v_add(z, v_sub(g, v_mul(sigma, w)))
    q = v_add(v_mul(v_add(BETA, s1), ilr), L2)
    w1 = v_clamp(v_div(v_shrink(z1, opt.l1), q), wb)
    out = (w1, z1, n1)
    return V(np.concatenate([o.v for o in out], axis=1),
             np.concatenate([o.e for o in out], axis=1))


def model_step(case, rows32, resident, powers=None):
    """UC.model_step with the FTRL step: the whole call on keys 0..n-1."""
    n, dim = case.n, case.dim
    g = model_reduce(case.grads64, case.perm, case.ustarts, case.seg_id,
                     case.seg_scale, n, dim)
    stepped = model_optimizer(case.opt, case.wb, rows32, g, dim)
    nonempty = case.keys[:n] != 0
    miss = nonempty & ~resident
    nan = nonempty & resident & np.isnan(g.v).any(axis=1)
    touched = nonempty & resident & ~nan
    before = np.asarray(rows32, dtype=np.float32).astype(np.float64)
    rows = V(np.where(touched[:, None], stepped.v, before),
             np.where(touched[:, None], stepped.e, 0.0))
    return UC.Expected(rows, int(miss.sum()), int(nan.sum()), touched)


# ------------------------------------------------- the plain f32 mirror loop

BUGS = ("sigma_from_n1_twice", "sigma_w_dropped", "beta_dropped",
        "l2_dropped", "l1_clip_dropped", "z_n_swapped")


def f32_optimizer(opt, wb, rows, g, dim, bug=None):
    """pa_ftrl in unfused numpy f32 (every operand an np.float32)."""
    lr, beta, l1, l2 = (F32(p) for p in (opt.lr, opt.beta, opt.l1, opt.l2))
    wb, one, zero = F32(wb), F32(1.0), F32(0.0)
    rows = np.array(rows, dtype=np.float32)
    zi, ni = (2, 1) if bug == "z_n_swapped" else (1, 2)
    w = rows[:, :dim]
    z, n = rows[:, zi * dim:(zi + 1) * dim], rows[:, ni * dim:(ni + 1) * dim]
    if bug == "beta_dropped":
        beta = zero
    if bug == "l2_dropped":
        l2 = zero
    if bug == "l1_clip_dropped":
        l1 = zero
    with np.errstate(all="ignore"):
        ilr = one / lr
        n1 = n + g * g
        s1 = np.sqrt(n1)
        s0 = np.sqrt(n1 if bug == "sigma_from_n1_twice" else n)
        sigma = (s1 - s0) * ilr
        z1 = z + (g - (zero if bug == "sigma_w_dropped" else sigma * w))
        q = (beta + s1) * ilr + l2
        w1 = (np.fmin(np.fmax(z1, -l1), l1) - z1) / q
        if wb > 0:
            w1 = np.fmin(np.fmax(w1, -wb), wb)
        out = rows.copy()
        out[:, :dim] = w1
        out[:, zi * dim:(zi + 1) * dim] = z1
        out[:, ni * dim:(ni + 1) * dim] = n1
    assert out.dtype == np.float32
    return out


def f32_step(case, rows32, resident, bug=None):
    """-> (rows after, misses, nans) of the mirror loop."""
    g = UC.f32_reduce(case)
    stepped = f32_optimizer(case.opt, case.wb, rows32, g, case.dim, bug)
    nonempty = case.keys[:case.n] != 0
    nan = nonempty & resident & np.isnan(g).any(axis=1)
    touched = nonempty & resident & ~nan
    out = np.where(touched[:, None], stepped, np.asarray(rows32, np.float32))
    return out, int((nonempty & ~resident).sum()), int(nan.sum())


# ------------------------------------------------------------------ CPU checks


@pytest.mark.parametrize("wb", [UC.WEIGHT_BOUND, 0.0], ids=["bound", "no_bound"])
@pytest.mark.parametrize("dim", DIMS)
def test_f32_loop_meets_every_bound(dim, wb):
    case = cached_case(dim, wb=wb)
    exp = model_step(case, case.rows, case.resident)
    got, misses, nans = f32_step(case, case.rows, case.resident)
    assert (misses, nans) == (exp.misses, exp.nans) == (1, 2)
    r = worst_ratio(got, exp.rows)
    w = got[exp.touched][:, :dim]
    zeros = float((w == 0).mean())
    print(f"dim {dim} wb {case.wb}: f32 loop err/bound {r:.3f}, "
          f"{100 * zeros:.0f}% of the weights exactly 0")
    assert r <= 1.0
    # both sides of the l1 threshold are exercised
    assert 0.05 < zeros < 0.98
    # the lone inf was applied: NaN weight, or -bound where clamped
    w_inf = exp.rows.v[UC.K_INF, 0]
    assert exp.touched[UC.K_INF]
    assert w_inf == -np.float32(case.wb) if case.wb else np.isnan(w_inf)
    assert exp.touched[UC.K_DEAD] and exp.touched[UC.K_ZERO_SCALE]
    # the zero-gradient step from zero state: (0, 0, 0), exactly
    assert not exp.rows.v[UC.K_ZERO_STATE].any()
    assert not exp.rows.e[UC.K_ZERO_STATE].any()


@pytest.mark.parametrize("gdtype", ["f32", "bf16"])
def test_f32_loop_meets_bounds_other_gradient_types(gdtype):
    for dim in (24, 320):
        case = cached_case(dim, gdtype)
        exp = model_step(case, case.rows, case.resident)
        got, misses, nans = f32_step(case, case.rows, case.resident)
        assert (misses, nans) == (exp.misses, exp.nans)
        assert worst_ratio(got, exp.rows) <= 1.0


@pytest.mark.parametrize("bug", BUGS)
def test_wrong_variants_break_the_bound(bug):
    """Each wrong variant of the f32 loop fails at every lane layout."""
    for dim in DIMS:
        case = cached_case(dim)
        exp = model_step(case, case.rows, case.resident)
        got, _, _ = f32_step(case, case.rows, case.resident, bug=bug)
        r = worst_ratio(got, exp.rows)
        print(f"{bug} dim {dim}: err/bound {r:.3g}")
        assert r > 1.0, (bug, dim, r)


@functools.lru_cache(maxsize=None)
def _rows_case(dim):
    return ftrl_case(dim, "f32", "rows", wb=0.0, opt=Ftrl(**FTRL_DYADIC))


@pytest.mark.parametrize("dim", [8, 24, 320])
def test_cpu_store_meets_bounds(dim):
    """CpuEmbeddingStore.update_gradients (ops/reference.py ftrl_update) on the
    f32 one-row-per-key cases.  torch divides by the Python float lr where the
    kernel multiplies by the reciprocal of the f32-rounded lr, which is the
    same number up to the model's roundings only when lr is an f32 number, so
    these cases use dyadic parameters.  An inf gradient makes the weight NaN
    and torch's clamp_ keeps a NaN where pa_clamp_weight returns -bound
    (test_update_cases_cpu's module docstring), so, as with Adam, they run
    without a weight bound."""
    case = _rows_case(dim)
    exp = model_step(case, case.rows, case.resident)
    store = UC._cpu_store(case)
    reduced = torch.from_numpy(UC.f32_reduce(case))
    keys = torch.from_numpy(case.keys[:case.n].copy())
    assert store.update_gradients(keys, reduced) == exp.misses == 1
    after = UC._export(store, case)
    r = worst_ratio(after, exp.rows, rows=case.resident)
    print(f"dim {dim}: CpuEmbeddingStore err/bound {r:.3f}")
    assert r <= 1.0
    assert exp.nans == 1 and not exp.touched[UC.K_NAN]
    assert np.array_equal(after[UC.K_NAN], case.rows[UC.K_NAN])
    assert np.isnan(after[UC.K_INF, 0]) and exp.touched[UC.K_INF]
    # the mirror loop on the same cases
    got, _, _ = f32_step(case, case.rows, case.resident)
    assert worst_ratio(got, exp.rows) <= 1.0


def test_equals_online_gradient_descent():
    """The independent derivation.  With l1 = l2 = 0, from zero state and zero
    weights, FTRL-Proximal is online gradient descent with the per-coordinate
    rate lr / (beta + sqrt(n_t)), exactly in real arithmetic (McMahan et al.
    2013, section 3).  50 steps of the model chained in f64 against that
    recursion, to 1e-9 relative."""
    T, rows_n, dim = 50, 5, 7
    opt = Ftrl(lr=0.06, beta=0.7)
    lr, beta = float(F32(opt.lr)), float(F32(opt.beta))
    rng = np.random.default_rng(5)
    rows = np.zeros((rows_n, 3 * dim))
    w_ogd, n_ogd = np.zeros((rows_n, dim)), np.zeros((rows_n, dim))
    for _ in range(T):
        g = rng.standard_normal((rows_n, dim)) * 10.0 ** rng.uniform(-3, 1)
        rows = model_optimizer(opt, 0.0, rows, V(g), dim, f32_rows=False).v
        n_ogd = n_ogd + g * g
        w_ogd = w_ogd - lr / (beta + np.sqrt(n_ogd)) * g
        scale = np.abs(w_ogd).max()
        assert np.abs(rows[:, :dim] - w_ogd).max() <= 1e-9 * scale
        assert np.allclose(rows[:, 2 * dim:], n_ogd, rtol=1e-12, atol=0)
    assert scale > 0.01  # the weights went somewhere


@pytest.mark.parametrize("dim", [4, 64, 257])
def test_l1_above_every_z_gives_exact_zero_weights(dim):
    """l1 beyond every |z1|: every updated weight is exactly +0.0 or -0.0 --
    in the model with a zero bound, in the f32 loop and in the CPU store --
    while z and n moved."""
    case = ftrl_case(dim, "f32", "rows", wb=0.0,
                     opt=Ftrl(lr=0.0625, beta=0.75, l1=1e6, l2=0.015625))
    exp = model_step(case, case.rows, case.resident)
    finite = exp.touched & np.isfinite(exp.rows.v).all(axis=1)
    assert finite.sum() >= case.n - 4
    assert np.abs(exp.rows.v[finite, dim:2 * dim]).max() < 1e6
    assert not exp.rows.v[finite, :dim].any()
    assert not exp.rows.e[finite, :dim].any()
    got, _, _ = f32_step(case, case.rows, case.resident)
    store = UC._cpu_store(case)
    store.update_gradients(torch.from_numpy(case.keys[:case.n].copy()),
                           torch.from_numpy(UC.f32_reduce(case)))
    for after in (got, UC._export(store, case)):
        assert (after[finite, :dim] == 0).all()
        assert worst_ratio(after, exp.rows, rows=finite) <= 1.0
        moved = after[finite, dim:] != case.rows[finite, dim:]
        assert moved[:, :dim].mean() > 0.8 and moved[:, dim:].mean() > 0.8
    assert (case.rows[finite, :dim] != 0).mean() > 0.9  # they were not 0 before


def test_constructor_validation_and_row_shape():
    o = Ftrl()
    assert (o.kind, o.lr, o.beta, o.l1, o.l2) == ("ftrl", 0.05, 1.0, 0.0, 0.0)
    assert o.require_space(8) == 16 and o.require_space(1) == 2
    assert o.state_init(8) == 0.0
    Ftrl(lr=1e-3, beta=1e-3, l1=0.0, l2=0.0)
    for bad in (dict(lr=0.0), dict(lr=-1.0), dict(beta=0.0), dict(beta=-0.5),
                dict(l1=-1e-9), dict(l2=-1e-9), dict(lr=float("nan"))):
        with pytest.raises(ValueError):
            Ftrl(**bad)
    store = make_store(8, 256, o, EmbeddingConfig(), torch.device("cpu"))
    assert isinstance(store, CpuEmbeddingStore)
    assert store.row_width == 24 and store.opt_space == 16


# ---------------------------------------------------------------- engine level


def _engine(optimizer, schema=None):
    return P.EmbeddingEngine(
        schema=schema or P.mixed_schema(),
        hyper=EmbeddingConfig(emb_initialization=(-0.5, 0.5)),
        optimizer=optimizer,
        gconf=P.GlobalConfig(capacity=1 << 14),
        device=P.CPU,
        dist_ctx=P.DistContext(1, 0),
    )


def _mixed_step(eng, step):
    """One lookup and update of the mixed schema (sum, sum+sqrt, raw and
    hashstack slots, variable lengths), as test_gpu_engine_paths drives it."""
    tb = eng.process_batch(P.mixed_batch(step))
    gen = torch.Generator().manual_seed(200 + step)
    raw = next(p for p in tb.payloads if p.is_raw)
    g_raw = torch.randn(raw.raw_distinct.shape[0] - 1, 16, generator=gen)
    for group in tb._groups:
        group.sum_base.requires_grad_(True)
        group.sum_base.grad = torch.randn(group.sum_base.shape,
                                          generator=gen).half()
    eng.apply_gradients_base(tb, raw_grads={"r": g_raw}, loss_scale=4.0)


def test_engine_lookup_update_dump_load(tmp_path):
    """An EmbeddingEngine on the CPU device with Ftrl on the mixed schema:
    lookups and updates run; dump then load into a second FTRL engine gives
    the same rows bit for bit; the same checkpoint loaded into an SGD engine
    (row width dim) gives the same weights.  Lookup, checkpoint and the row
    width adaptation know nothing of FTRL."""
    opt = Ftrl(lr=0.05, beta=1.0, l1=0.01, l2=0.001)
    eng = _engine(opt)
    fresh = P.table(_engine(opt))
    for step in range(P.STEPS):
        _mixed_step(eng, step)
    t = P.table(eng)
    assert t.keys() == {8, 16} and all(len(t[d][0]) > 0 for d in t)
    assert not any(len(fresh[d][0]) for d in fresh)
    for dim, (_, rows) in t.items():
        assert rows.shape[1] == 3 * dim
        assert np.isfinite(rows).all()
        assert (rows[:, 2 * dim:] >= 0).all() and (rows[:, 2 * dim:] > 0).any()
        assert (rows[:, dim:2 * dim] != 0).any()
        assert (rows[:, :dim] == 0).any()  # l1 zeroes some weights
    eng.dump(str(tmp_path))
    twin = _engine(Ftrl(lr=0.05, beta=1.0, l1=0.01, l2=0.001))
    twin.load(str(tmp_path))
    P.assert_tables_equal(t, P.table(twin))
    # a further step on both: still the same bits
    _mixed_step(eng, P.STEPS)
    _mixed_step(twin, P.STEPS)
    P.assert_tables_equal(P.table(eng), P.table(twin))
    sgd = _engine(SGD(lr=0.1))
    sgd.load(str(tmp_path))
    ts = P.table(sgd)
    for dim in t:
        assert np.array_equal(ts[dim][0], t[dim][0])
        assert ts[dim][1].shape[1] == dim
        assert np.array_equal(ts[dim][1], t[dim][1][:, :dim])


# ------------------------------------------------------------- a training run

_EXAMPLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "examples", "adult_income")
TRAIN_STEPS = 120


def _train_losses():
    from persia_amd.ctx import TrainCtx
    from persia_amd.data import DataLoader, IterableDataset
    from persia_amd.embedding.data import PersiaBatch
    from persia_amd.utils import setup_seed

    sys.path.insert(0, _EXAMPLE)
    try:
        from data_generator import make_dataloader, make_dataset
        from model import DNN
    finally:
        sys.path.remove(_EXAMPLE)

    class Data(IterableDataset):
        def __init__(self):
            super().__init__(buffer_size=10)
            self.data = make_dataset(n_samples=TRAIN_STEPS * 128)

        def __iter__(self):
            for dense, feats, label in make_dataloader(*self.data, 128):
                yield PersiaBatch(feats, non_id_type_features=[dense],
                                  labels=[label], requires_grad=True)

    setup_seed(3)
    model = DNN()
    losses = []
    with TrainCtx(
        model=model,
        embedding_optimizer=Ftrl(lr=0.1, beta=1.0, l1=1e-4, l2=1e-4),
        dense_optimizer=torch.optim.SGD(model.parameters(), lr=0.05),
        embedding_config=EmbeddingConfig(),
        embedding_schema=os.path.join(_EXAMPLE, "config", "embedding_config.yml"),
        global_config=os.path.join(_EXAMPLE, "config", "global_config.yml"),
        mixed_precision=False,
        device_id=-1,
    ) as ctx:
        loader = DataLoader(Data(), reproducible=True, embedding_staleness=1)
        loss_fn = torch.nn.BCELoss()
        for tb in loader:
            pred, labels = ctx.forward(tb)
            loss = loss_fn(pred.squeeze(1), labels[0].squeeze(1).float())
            ctx.backward(loss)
            losses.append(float(loss.detach()))
    return losses


def test_training_run_learns():
    """TRAIN_STEPS deterministic CPU steps of the adult-income example's model
    and generator through TrainCtx(embedding_optimizer=Ftrl(...)): the mean
    loss of the last quarter of steps is below that of the first quarter.
    Measured: first quarter 0.4964, last quarter 0.3833."""
    losses = _train_losses()
    assert len(losses) == TRAIN_STEPS and np.isfinite(losses).all()
    q = TRAIN_STEPS // 4
    first, last = float(np.mean(losses[:q])), float(np.mean(losses[-q:]))
    print(f"FTRL training run: first quarter {first:.4f}, last quarter {last:.4f}")
    assert last < first
