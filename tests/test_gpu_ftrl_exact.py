"""The FTRL arms of the sparse update kernels (opt code 3: update_kernel<true>,
scatter_update_kernel<HINTS, true>, scatter_update_multi_kernel<2|4, HINTS,
true>) against the f64 model and per-element bounds of
tests/test_ftrl_cases_cpu.py, from arbitrary (non-fresh) z and n.

The shape is that of tests/test_gpu_update_exact.py, whose helpers this file
uses: every run compares whole rows -- w, z and n -- of every key with the
model run from the rows the kernel itself read, asserts both skip counters
exactly, and asserts that keys, ticks and every arena row the call had no
business writing (other keys' rows, the filler rows, the rows of missing, NaN
and empty keys) are the same bits before and after.

One dim per lane layout: packed 1, 4, 16; four keys per wave 3, 64; two keys
129; one key 257; each with and without a weight bound.  Entry points:
store_update on f32 rows; scatter_update with and without u_count and with
hints (bit-equal to the unhinted twin); update_local on f16 gradients, hinted
and unhinted; its fallback on f32 and bf16 gradients and at dim 513; a chain
of four steps.  Engine level: three batches with Ftrl, exported tables bitwise
equal with PA_BAG_FAST, PA_RAW_FAST and PA_UPDATE_HINTS on against off.  An
out-of-range optimizer code raises on the host.

Worst err/bound measured on an MI355X (gfx950) per kernel family, one-step
tests and the chains (the figures near 1 are single roundings, where half an
ulp is the bound itself; none reaches 1):

    family                                   one step   chain
    update_kernel (store_update)             0.988      -
    grad_scatter + update_kernel (fallback)  0.997      -
    scatter_update_kernel, packed dims       0.987      0.997
    scatter_update_multi_kernel<4>           0.961      0.993
    scatter_update_multi_kernel<2>           0.990      0.9998
    scatter_update_kernel, one key per wave  0.999      0.9999

Hinted runs give the figures of their unhinted twins, being the same bits.

All tests are @pytest.mark.gpu."""
import numpy as np
import pytest
import torch

import test_bag_cases_cpu as BC
import test_engine_paths as P
import test_ftrl_cases_cpu as FC
import test_gpu_update_exact as G
import test_raw_cases_cpu as RC
import test_update_cases_cpu as UC

from persia_amd.embedding.optim import Ftrl

pytestmark = pytest.mark.gpu

_BOUNDS = [UC.WEIGHT_BOUND, 0.0]
_BOUND_IDS = ["bound", "no_bound"]
_FUSED_DIMS = (16, 64, 129, 257)  # one dim per fused kernel variant

_model_cache = {}


def _one_step_model(case, before):
    """One-step tests all start from the imported rows: one model run per
    case."""
    assert np.array_equal(before.resident, case.resident)
    assert np.array_equal(before.rows[case.resident], case.rows[case.resident])
    if id(case) not in _model_cache:
        _model_cache[id(case)] = (
            case, FC.model_step(case, case.rows, case.resident))
    return _model_cache[id(case)][1]


def _family(dim, suffix=""):
    return "ftrl " + G._family(dim) + suffix


@pytest.mark.parametrize("padded", [True, False], ids=["u_count", "exact"])
@pytest.mark.parametrize("wb", _BOUNDS, ids=_BOUND_IDS)
@pytest.mark.parametrize("dim", FC.DIMS)
def test_scatter_update(dim, wb, padded):
    case = FC.cached_case(dim, wb=wb)
    store = G._store(case)
    assert store._opt_code == 3 and store.row_width == 3 * dim
    before = G._Before(store, case)
    G._scatter_update(store, case, padded)
    exp = G._check(store, case, before, _family(dim),
                   expect=_one_step_model(case, before))
    assert (exp.misses, exp.nans) == (1, 2)


@pytest.mark.parametrize("wb", _BOUNDS, ids=_BOUND_IDS)
@pytest.mark.parametrize("dim", FC.DIMS)
def test_scatter_update_hinted(dim, wb):
    """With the hints a lookup emits: within the bound, and -- from non-zero
    z and n -- the same bits as the twin store's unhinted call."""
    case = FC.cached_case(dim, wb=wb)
    store, twin = G._store(case), G._store(case)
    hints = G._emitted_hints(store, case)
    before = G._Before(store, case)
    G._scatter_update(store, case, True, hints)
    G._scatter_update(twin, case, True)
    G._check(store, case, before, _family(dim, " hinted"),
             expect=_one_step_model(case, before))
    # the claims of one import race, so the twins place keys differently:
    # compare key by key
    res = torch.from_numpy(case.resident).to(G._dev())
    rows = [s.arena[G._slots(s, case)[res]] for s in (store, twin)]
    assert torch.equal(rows[0].view(torch.int32), rows[1].view(torch.int32))
    assert torch.equal(twin._skipped, store._skipped)


@pytest.mark.parametrize("hinted", [False, True], ids=["plain", "hinted"])
@pytest.mark.parametrize("dim", _FUSED_DIMS)
def test_update_local_f16(dim, hinted):
    case = FC.cached_case(dim)
    store = G._store(case)
    d = G._on_device(case)
    hints = G._emitted_hints(store, case) if hinted else (None, None)
    before = G._Before(store, case)
    store.update_local(d["grads"], d["perm"], d["ustarts"], d["seg_id"],
                       d["scale"], d["uniq"], d["u_count"], *hints)
    G._check(store, case, before, _family(dim, " hinted" if hinted else ""),
             expect=_one_step_model(case, before))


@pytest.mark.parametrize("wb", _BOUNDS, ids=_BOUND_IDS)
@pytest.mark.parametrize("dim", [1, 3, 64, 129, 257, 513])
def test_store_update(dim, wb):
    """update_kernel<true> on one f32 gradient row per key."""
    case = FC.cached_case(dim, "f32", "rows", wb)
    store = G._store(case)
    d = G._on_device(case)
    before = G._Before(store, case)
    store.update_gradients(d["uniq"][:case.n], d["grads"])
    exp = G._check(store, case, before, "ftrl update_kernel",
                   expect=_one_step_model(case, before))
    assert (exp.misses, exp.nans) == (1, 1)


@pytest.mark.parametrize("gdtype", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [8, 24, 320])
def test_update_local_fallback(dim, gdtype):
    """f32 and bf16 gradients leave the fused kernel: a host read of the
    padded count, grad_scatter into an f32 buffer, then store_update."""
    case = FC.cached_case(dim, gdtype)
    store = G._store(case)
    d = G._on_device(case)
    before = G._Before(store, case)
    store.update_local(d["grads"], d["perm"], d["ustarts"], d["seg_id"],
                       d["scale"], d["uniq"], d["u_count"])
    G._check(store, case, before, "ftrl grad_scatter + update_kernel",
             expect=_one_step_model(case, before))


def test_update_local_fallback_dim_513():
    """One past scatter_update's limit: f16 gradients, same fallback."""
    case = FC.cached_case(513)
    store = G._store(case)
    d = G._on_device(case)
    before = G._Before(store, case)
    store.update_local(d["grads"], d["perm"], d["ustarts"], d["seg_id"],
                       d["scale"], d["uniq"], d["u_count"])
    G._check(store, case, before, "ftrl grad_scatter + update_kernel",
             expect=_one_step_model(case, before))


_N_FRESH = 30  # the last keys are not imported: the first lookup creates them
_CHAIN_STEPS = 4


@pytest.mark.parametrize("dim", _FUSED_DIMS)
def test_chain_of_steps(dim):
    """Four update_local calls (odd steps plain, even steps hinted) on one
    store, new gradients each step.  Every step is checked from the rows the
    previous step left; the 30 rows the lookup created start from z = n = 0
    and a seeded non-zero weight, which the first step rewrites."""
    steps = [FC.ftrl_case(dim, seed=t) for t in range(1, _CHAIN_STEPS + 1)]
    first = steps[0]
    fresh = range(first.n - _N_FRESH, first.n)
    store = G._store(first, skip=fresh)
    d0 = G._on_device(first)
    created = store.lookup(d0["uniq"][first.n - _N_FRESH:first.n], train=True)
    assert created.shape == (_N_FRESH, dim)
    torch.cuda.synchronize()
    rows = G._Before(store, first).rows[first.n - _N_FRESH:]
    assert (rows[:, dim:] == 0).all() and (rows[:, :dim] != 0).any()
    for t, case in enumerate(steps, start=1):
        assert np.array_equal(case.keys, first.keys)
        d = G._on_device(case)
        hints = G._emitted_hints(store, case) if t % 2 == 0 else (None, None)
        before = G._Before(store, case)
        store.update_local(d["grads"], d["perm"], d["ustarts"], d["seg_id"],
                           d["scale"], d["uniq"], d["u_count"], *hints)
        G._check(store, case, before, _family(dim, " chain"),
                 expect=FC.model_step(case, before.rows, before.resident))
        G._dev_cache.pop(id(case), None)
    assert store._skipped.tolist() == [_CHAIN_STEPS, 2 * _CHAIN_STEPS]


# ---------------------------------------------------------------- engine level


def _ftrl():
    return Ftrl(lr=0.06, beta=0.7, l1=0.02, l2=0.02)


def _engine(schema=None, capacity=1 << 14):
    return P.EmbeddingEngine(
        schema=schema or P.single_schema(),
        hyper=P.EmbeddingConfig(emb_initialization=(-0.5, 0.5)),
        optimizer=_ftrl(),
        gconf=P.GlobalConfig(capacity=capacity),
        device=G._dev(),
        dist_ctx=P.DistContext(1, 0),
    )


def _assert_trained(t, untouched):
    """Exported tables hold FTRL rows that three updates moved."""
    assert P.tables_differ(untouched, t)
    for dim, (_, rows) in t.items():
        assert rows.shape[1] == 3 * dim and np.isfinite(rows).all()
        assert (rows[:, 2 * dim:] > 0).any() and (rows[:, dim:2 * dim] != 0).any()


def test_engine_bag_fast_on_off_bitwise(monkeypatch):
    """The bag schema (multi-ID sum slots a, b: dim 8; c, d: dim 16), three
    batches, PA_BAG_FAST on against off: the same exported tables."""
    names = tuple(P.SINGLE_SLOTS)
    tables = []
    for knob in (True, False):
        monkeypatch.setenv("PA_BAG_FAST", "1" if knob else "0")
        eng = _engine()
        assert eng._bag_fast == knob
        for step in range(P.STEPS):
            tb = eng.process_batch(BC.bag_batch(step, names))
            assert (tb._groups[0].slot_hint is not None) == knob
            P.set_base_grads(tb, P.slot_grads(100 + step, G._dev()))
            eng.apply_gradients_base(tb, loss_scale=4.0)
        tables.append(P.table(eng))
    monkeypatch.setenv("PA_BAG_FAST", "1")
    untouched = _engine()
    for step in range(P.STEPS):
        untouched.process_batch(BC.bag_batch(step, names))
    _assert_trained(tables[0], P.table(untouched))
    P.assert_tables_equal(tables[0], tables[1])


def _dyadic_cell_grads(seed):
    """Seeded f16 gradient per slot of RC.raw_schema, (B, dim) for a sum slot
    and (B*sfs, dim) for a raw slot's cells, every value a multiple of 1/8 in
    [-4, 4].  With the raw path off a raw slot's cells are summed per key by
    index_add_ in no fixed order, with it on by the ordered reduction; such
    values (and the power-of-two loss scale) make every partial sum exact, so
    the two orders give the same reduced gradient."""
    gen = torch.Generator().manual_seed(seed)
    return {
        n: (torch.randint(-32, 33, (P.B * (sfs or 1), d), generator=gen)
            .float() / 8).half().to(G._dev())
        for n, (d, sfs, _sq) in RC.RAW_SLOTS.items()
    }


def test_engine_raw_fast_on_off_bitwise(monkeypatch):
    """The raw schema (sum, sum+sqrt and raw slots in one group, a raw slot
    alone, a plain bag group), three batches, PA_RAW_FAST on against off: the
    same exported tables."""
    import test_gpu_raw_exact as GR

    tables = []
    for knob in (True, False):
        monkeypatch.setenv("PA_RAW_FAST", "1" if knob else "0")
        eng = _engine(RC.raw_schema())
        assert eng._raw_fast == knob
        for step in range(P.STEPS):
            tb = eng.process_batch(RC.raw_batch(step))
            GR._assert_raw_path(tb, knob)
            grads = _dyadic_cell_grads(100 + step)
            if knob:
                GR._feed_on(tb, grads)
                eng.apply_gradients_base(tb, loss_scale=4.0)
            else:
                eng.apply_gradients_base(tb, GR._feed_off(tb, grads),
                                         loss_scale=4.0)
        tables.append(P.table(eng))
    untouched = _engine(RC.raw_schema())
    for step in range(P.STEPS):
        untouched.process_batch(RC.raw_batch(step))
    assert tables[0].keys() == {8, 16, 24}
    _assert_trained(tables[0], P.table(untouched))
    for dim in tables[0]:
        diff = np.abs(tables[0][dim][1] - tables[1][dim][1]).max()
        print(f"raw fast on/off dim {dim}: rows {tables[0][dim][1].shape}, "
              f"max diff {diff:.3e}")
    P.assert_tables_equal(tables[0], tables[1])


def test_engine_update_hints_on_off_bitwise(monkeypatch):
    """The single-ID schema, three batches, PA_UPDATE_HINTS on against off."""
    tables = []
    for knob in ("1", "0"):
        monkeypatch.setenv("PA_UPDATE_HINTS", knob)
        eng = _engine()
        for step in range(P.STEPS):
            tb = eng.process_batch(P.single_batch(step))
            assert (tb._groups[0].slot_hint is not None) == (knob == "1")
            P.set_base_grads(tb, P.slot_grads(100 + step, G._dev()))
            eng.apply_gradients_base(tb, loss_scale=4.0)
        for store in eng.stores.values():
            assert store._skipped.tolist() == [0, 0]
        tables.append(P.table(eng))
    untouched = _engine()
    for step in range(P.STEPS):
        untouched.process_batch(P.single_batch(step))
    _assert_trained(tables[0], P.table(untouched))
    P.assert_tables_equal(tables[0], tables[1])


# ------------------------------------------------------------ optimizer codes


@pytest.mark.parametrize("code", [-1, 4, 17])
def test_unknown_optimizer_code_raises_on_the_host(code):
    """No kernel has a default arm any more; scatter_update and store_update
    reject a code outside 0..3 before any launch, so the table keeps its
    bits."""
    from persia_amd.ops import native

    case = FC.cached_case(16)
    store = G._store(case)
    d = G._on_device(case)
    before = G._Before(store, case)
    dim, _, params, b1p, b2p, wb, skipped = store._update_args()
    n = case.n_pad
    with pytest.raises(RuntimeError, match="unknown optimizer code"):
        native().scatter_update(
            store.keys, store.ticks, store.arena, d["uniq"][:n], d["grads"],
            d["perm"], d["ustarts"][:n + 1], d["seg_id"], d["scale"], dim,
            code, params, b1p, b2p, wb, skipped, d["u_count"])
    rows = torch.zeros(case.n, dim, device=G._dev())
    with pytest.raises(RuntimeError, match="unknown optimizer code"):
        native().store_update(store.keys, store.ticks, store.arena,
                              d["uniq"][:case.n], rows, dim, code, params,
                              b1p, b2p, wb, skipped)
    torch.cuda.synchronize()
    assert torch.equal(store.arena, before.arena)
    assert torch.equal(store.keys, before.keys)
    assert store._skipped.tolist() == before.skipped.tolist()
