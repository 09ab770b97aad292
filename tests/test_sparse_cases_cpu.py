"""Scenario generators of tests/test_gpu_sparse_exact.py, and the checks of
those scenarios that need no GPU.

Three families:

* table scenarios in the ORDER-INDEPENDENT regime.  Claims of one launch race,
  so the slot a key gets depends on thread order -- unless no two keys of a
  batch share a probe window.  Keys are ``(counter << 6) | home_bucket`` on a
  64-bucket table; a batch visits home buckets ``o, o + 4, ...`` (16 disjoint
  windows of PROBE_BUCKETS = 4 buckets tiling the table, one of them wrapping
  from bucket 63 to bucket 2) and does at most one thing per window.  The
  check here is the condition that makes the GPU comparison meaningful: the
  sequential oracle lands in the same state under a random permutation of
  every batch.
* reduction cases (segment_sum, grad_scatter, grad_scatter_idx): an f64
  reference from the same operand bits and the per-element bound; here a plain
  f32 loop is held to the bound, and a loop that drops an addend is shown to
  break it, so the constants are neither too tight nor loose enough to hide a
  dropped addend.
* dedup inputs and the numpy reference of the padded dedup.
"""
import numpy as np
import pytest
import torch

from persia_amd.core import hashing
from persia_amd.core.store import (BUCKET_SIZE, PROBE_BUCKETS,
                                   CpuEmbeddingStore, row_init)
from persia_amd.embedding import EmbeddingConfig
from persia_amd.embedding.optim import SGD, Adagrad, Adam

from test_gpu_dense_exact import EPS32, f16_store_bound

# ------------------------------------------------------------ table scenarios

N_BUCKETS = 64
CAPACITY = N_BUCKETS * BUCKET_SIZE  # 512 slots
TABLE_DIM = 4                       # Adagrad row: 4 weights + 4 accumulators
N_BATCHES = 120                     # fills the table, then evicts
N_BATCHES_ADMIT = 260               # half the fresh keys are refused
SEEDS = (0, 1, 2)
VARIANTS = ("plain", "admit", "spill")
WINDOWS = N_BUCKETS // PROBE_BUCKETS


def window_key(counter, home):
    """A mixed key whose home bucket is `home` (the table masks the low six
    bits).  counter >= 1 keeps it off the empty sentinel."""
    assert counter >= 1 and 0 <= home < N_BUCKETS
    return (counter << 6) | home


def table_scenario(seed, n_batches=N_BATCHES):
    """-> list of u64 key arrays, one per batch.  Per window: skip it, insert
    a fresh key, or re-touch an earlier key of the same home bucket (recent
    ones are mostly resident, old ones mostly evicted)."""
    rng = np.random.default_rng(seed)
    counter = 0
    history = {h: [] for h in range(N_BUCKETS)}
    batches = []
    for _ in range(n_batches):
        o = int(rng.integers(0, PROBE_BUCKETS))
        keys = []
        for w in range(WINDOWS):
            home = o + PROBE_BUCKETS * w
            r = rng.random()
            if r < 0.15:
                continue
            past = history[home]
            if r < 0.75 or not past:
                counter += 1
                k = window_key(counter, home)
                past.append(k)
            elif rng.random() < 0.5:
                k = past[-1 - int(rng.integers(0, min(3, len(past))))]
            else:
                k = past[int(rng.integers(0, len(past)))]
            keys.append(k)
        batches.append(np.array(keys, dtype=np.uint64))
    # the windows of one batch are pairwise disjoint
    for b in batches:
        homes = np.sort((b & np.uint64(N_BUCKETS - 1)).astype(np.int64))
        gaps = np.diff(np.concatenate([homes, homes[:1] + N_BUCKETS]))
        assert len(b) <= 1 or gaps.min() >= PROBE_BUCKETS
    return batches


def scenario_for(seed, variant):
    return table_scenario(
        seed, N_BATCHES_ADMIT if variant == "admit" else N_BATCHES)


def table_store_args(variant):
    """(optimizer, hyper, spill_capacity) of one scenario variant.  0.5 is
    dyadic: the kernel compares the admission draw with a float, the oracle
    with a double."""
    assert variant in VARIANTS
    hyper = EmbeddingConfig(
        emb_initialization=(-0.5, 0.5),
        admit_probability=0.5 if variant == "admit" else 1.0,
    )
    opt = Adagrad(lr=0.1, initial_accumulator_value=0.01)
    # the tier never fills, so its LRU order (the eviction log's order within
    # a batch is an atomic counter's) never decides anything
    return opt, hyper, (1 << 16 if variant == "spill" else 0)


class CountingCpuStore(CpuEmbeddingStore):
    """The oracle, counting claims: evictions = claims - slots filled."""

    claims = 0

    def _probe_or_claim(self, k, tick):
        slot, is_new = super()._probe_or_claim(k, tick)
        self.claims += int(is_new)
        return slot, is_new

    @property
    def evictions(self):
        return self.claims - len(self)


def make_oracle(variant):
    opt, hyper, spill = table_store_args(variant)
    return CountingCpuStore(TABLE_DIM, CAPACITY, opt, hyper, spill_capacity=spill)


def as_keys(keys_u64):
    return torch.from_numpy(np.ascontiguousarray(keys_u64, dtype=np.uint64)
                            .view(np.int64).copy())


def stamp_row(batch_no, key, row_width):
    """The per-batch pattern written over a touched row (spill variant), so an
    evicted row differs from its init."""
    base = float(batch_no + 1) + float(int(key) % 1024) / 1024.0
    return torch.arange(row_width, dtype=torch.float32) * 0.125 + base


def oracle_slots(store, keys_u64):
    return np.array([store._probe(k) for k in keys_u64], dtype=np.int64)


def spill_dict(store):
    keys, rows = store.spill.export()
    return {int(k): rows[i].copy() for i, k in enumerate(keys)}


class OracleRun:
    """The oracle stepped through a scenario one batch at a time (the GPU
    tests step a HIP store alongside).  The spill variant stamps every touched
    row after its batch and checks that a restored row returns stamped."""

    def __init__(self, variant):
        self.variant = variant
        self.store = make_oracle(variant)
        self.stamped = {}
        self.stats = dict(misses=0, restored=0)

    def step(self, b_no, keys, order=None):
        """Look the batch up (train), in `order` when given.
        -> (rows in the order of `keys`, slot of every key after the batch,
            {index in keys: expected emb} of the rows restored from the tier)."""
        st = self.store
        order = np.arange(len(keys)) if order is None else order
        spilled = [i for i, k in enumerate(keys)
                   if st.spill is not None and k in st.spill]
        rows = st.lookup(as_keys(keys[order]), train=True)
        back = torch.empty_like(rows)
        back[torch.from_numpy(order)] = rows
        slots = oracle_slots(st, keys)
        self.stats["misses"] += int((slots < 0).sum())
        restored = {}
        for i in spilled:
            k = keys[i]
            restored[i] = stamp_row(self.stamped[int(k)], k, st.row_width)[:TABLE_DIM]
            assert torch.equal(back[i], restored[i]), (b_no, int(k))
        self.stats["restored"] += len(restored)
        return back, slots, restored

    def stamp(self, b_no, keys, slots):
        """Spill variant: overwrite the touched rows; -> the rows written, for
        the twin to write at the same slots."""
        rows = torch.stack([stamp_row(b_no, k, self.store.row_width) for k in keys])
        for k, s, r in zip(keys, slots, rows):
            assert s >= 0
            self.store.arena[s] = r
            self.stamped[int(k)] = b_no
        return rows


def run_oracle(variant, batches, perm_seed=None):
    """Drive the oracle through a scenario, each batch optionally permuted.
    -> (store, per-batch rows in the scenario's own order, stats)."""
    run = OracleRun(variant)
    rng = np.random.default_rng(perm_seed) if perm_seed is not None else None
    out = []
    for b_no, keys in enumerate(batches):
        order = rng.permutation(len(keys)) if rng is not None else None
        rows, slots, _ = run.step(b_no, keys, order)
        out.append(rows)
        if variant == "spill":
            run.stamp(b_no, keys, slots)
    return run.store, out, run.stats


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("seed", SEEDS)
def test_table_scenario_is_order_independent(seed, variant):
    batches = scenario_for(seed, variant)
    a, rows_a, st_a = run_oracle(variant, batches)
    b, rows_b, st_b = run_oracle(variant, batches, perm_seed=1000 + seed)
    miss_a = st_a["misses"]
    assert np.array_equal(a.keys, b.keys)
    assert np.array_equal(a.ticks, b.ticks)
    assert torch.equal(a.arena, b.arena)
    for ra, rb in zip(rows_a, rows_b):
        assert torch.equal(ra, rb)
    n_query = sum(len(k) for k in batches)
    n_distinct = len(set(np.concatenate(batches).tolist()))
    print(f"seed {seed} {variant}: {n_query} queries, {n_distinct} distinct, "
          f"{a.evictions} evictions, {len(a)} resident, {miss_a} misses")
    assert a.evictions == b.evictions and st_a == st_b
    assert len(a) == CAPACITY
    assert a.evictions >= 500
    if variant == "admit":
        # a refused key reads as a miss, and nothing else does: one claim per
        # window per batch never overflows
        assert miss_a > 100
    else:
        assert miss_a == 0
    if variant == "spill":
        da, db = spill_dict(a), spill_dict(b)
        assert da.keys() == db.keys() and len(da) > 0
        for k in da:
            assert np.array_equal(da[k], db[k])
        assert st_a["restored"] > 0


def test_scenario_covers_the_wrapping_window():
    """Some batch has offset 1, 2 or 3, whose last window wraps past bucket
    63, and every home bucket is used."""
    batches = table_scenario(SEEDS[0])
    homes = np.concatenate(batches) & np.uint64(N_BUCKETS - 1)
    assert set(homes.tolist()) == set(range(N_BUCKETS))


# --------------------------------------------------------- init / gather cases

INIT_DIMS = (4, 8, 32, 24, 48, 64, 65, 96, 128, 200)
INIT_OPTS = ("sgd", "adagrad_shared", "adagrad", "adam")
INIT_COUNTS = (1, 2, 63, 64, 65, 257)
INIT_BOUNDS = ((-0.5, 0.5), (-0.01, 0.01))


def init_opts_for(dim):
    """Two optimizers per dim, rotating: all four row widths (dim, dim + 1,
    2 dim, 3 dim) occur among the packed dims and among the dual-kernel
    dims."""
    i = INIT_DIMS.index(dim)
    return INIT_OPTS[i % 4], INIT_OPTS[(i + 1 + (i // 4) % 2) % 4]


def mk_init_opt(name):
    if name == "sgd":
        return SGD(lr=0.1)
    if name == "adagrad":
        return Adagrad(lr=0.1, initial_accumulator_value=0.0625)
    if name == "adagrad_shared":
        return Adagrad(lr=0.1, initial_accumulator_value=0.03,
                       vectorwise_shared=True)
    return Adam(lr=0.01)


def is_packed(dim):
    return dim < 64 and 64 % dim == 0


_row_cache = {}


def expected_row(key, dim, bounds, opt):
    """Full arena row of a freshly claimed key: row_init + state_init."""
    ck = (int(key), dim, bounds, opt.kind, opt.require_space(dim))
    if ck not in _row_cache:
        sign = int(hashing.splitmix64_inv(np.array([key], dtype=np.uint64))[0])
        row = np.full(dim + opt.require_space(dim),
                      np.float32(opt.state_init(dim)), dtype=np.float32)
        row[:dim] = row_init(sign, dim, *bounds)
        _row_cache[ck] = row
    return _row_cache[ck]


def mixed_keys(lo, n):
    """n distinct mixed keys (signs lo .. lo + n - 1), none the sentinel."""
    k = hashing.splitmix64(np.arange(lo, lo + n, dtype=np.uint64))
    assert (k != 0).all()
    return k


def positions_for(uniq, rng):
    """Position keys of a batch whose unique keys are `uniq`: every key gets
    1, 2 or 5 positions (cycling, so the dual kernel sees single/single,
    single/multi and multi/multi pairs), shuffled."""
    reps = np.array([(1, 1, 2, 1, 5)[i % 5] for i in range(len(uniq))])
    pos = np.repeat(uniq, reps)
    return pos[rng.permutation(len(pos))]


def test_init_cases_cover_every_row_width():
    for packed in (True, False):
        widths = set()
        for dim in INIT_DIMS:
            if is_packed(dim) != packed:
                continue
            for name in init_opts_for(dim):
                widths.add(mk_init_opt(name).require_space(dim) // max(dim, 1)
                           if name != "adagrad_shared" else "shared")
            assert len(set(init_opts_for(dim))) == 2
        assert widths == {0, "shared", 1, 2}, (packed, widths)


@pytest.mark.parametrize("bounds", INIT_BOUNDS)
def test_cpu_store_init_is_row_init_plus_state_init(bounds):
    opt = mk_init_opt("adagrad")
    store = CpuEmbeddingStore(24, 1024, opt,
                              EmbeddingConfig(emb_initialization=bounds))
    keys = mixed_keys(1, 65)
    rows = store.lookup(as_keys(keys), train=True)
    for i, k in enumerate(keys):
        exp = expected_row(k, 24, bounds, opt)
        slot = store._probe(k)
        assert np.array_equal(store.arena[slot].numpy(), exp)
        assert np.array_equal(rows[i].numpy(), exp[:24])


# ------------------------------------------------------------- reduction cases

RED_DIMS = (8, 24, 64, 96, 200)
RED_LENS = (0, 1, 2, 7, 65)
RED_COUNTS = (1, 37, 257)
N_GRAD_ROWS = 40


def _lens(rng, count):
    """Run / segment lengths from RED_LENS, all of them present when there
    is room; a single run is the longest one."""
    if count == 1:
        return np.array([RED_LENS[-1]])
    lens = rng.choice(RED_LENS, size=count, p=(0.15, 0.3, 0.3, 0.15, 0.1))
    lens[: len(RED_LENS)] = RED_LENS
    return lens[rng.permutation(count)]


def _rng(*tag):
    seed = 0
    for t in tag:
        seed = seed * 1000003 + int(t)
    return np.random.default_rng(seed)


def segment_case(dim, n_seg, with_scale):
    """Operands of one segment_sum call (f32; the caller casts rows)."""
    rng = _rng(1, dim, n_seg, with_scale)
    lens = _lens(rng, n_seg)
    nnz = int(lens.sum())
    n_rows = 50
    offsets = np.zeros(n_seg + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    rows = (rng.standard_normal((n_rows, dim)) * 0.5 + 0.05).astype(np.float32)
    scale = (np.maximum(lens, 1) ** -0.5 * 0.75).astype(np.float32)
    return dict(
        dim=dim, lens=torch.from_numpy(lens), nnz=nnz,
        rows=torch.from_numpy(rows),
        inverse=torch.from_numpy(rng.integers(0, n_rows, size=nnz)),
        offsets=torch.from_numpy(offsets),
        scale=torch.from_numpy(scale) if with_scale else torch.empty(0),
    )


def segment_reference(rows, case):
    """f64 sum of the SAME row bits, the absolute-value sum, and the bound of
    the f16 result: L adds and the scale multiply, a full f32 ulp each --
    E = (L + 1) 2^-23 scale S -- then the f16 store."""
    n_seg = case["lens"].numel()
    seg = torch.repeat_interleave(torch.arange(n_seg), case["lens"])
    g = rows.double()[case["inverse"]]
    ref = torch.zeros(n_seg, case["dim"], dtype=torch.float64)
    S = torch.zeros_like(ref)
    ref.index_add_(0, seg, g)
    S.index_add_(0, seg, g.abs())
    sc = (case["scale"].double() if case["scale"].numel()
          else torch.ones(n_seg, dtype=torch.float64))[:, None]
    ref, S = ref * sc, S * sc
    E = (case["lens"].double()[:, None] + 1) * EPS32 * S
    return ref, f16_store_bound(E, ref)


def scatter_case(dim, U, with_scale, pad=0):
    """Operands of one grad_scatter / grad_scatter_idx call.  Gradient rows
    with scale 0 are NaN; some positions have seg_id -1.  Without a scale the
    NaN rows are referenced by no position.  `pad` appends empty runs: the
    nnz-padded tail of a device-counted dedup."""
    rng = _rng(2, dim, U, with_scale)
    lens = _lens(rng, U)
    nnz = int(lens.sum())
    ustarts = np.zeros(U + 1 + pad, dtype=np.int64)
    np.cumsum(lens, out=ustarts[1 : U + 1])
    ustarts[U + 1 :] = nnz
    grads = (rng.standard_normal((N_GRAD_ROWS, dim)) * 0.5 + 0.05).astype(np.float32)
    scale = rng.uniform(0.3, 1.7, size=N_GRAD_ROWS).astype(np.float32)
    dead = np.array([3, 17, 31])
    scale[dead] = 0.0
    grads[dead] = np.nan
    seg_id = rng.integers(0, N_GRAD_ROWS, size=nnz)
    seg_id[rng.random(nnz) < 0.1] = -1
    if not with_scale:
        seg_id[np.isin(seg_id, dead)] = -1
    return dict(
        dim=dim, U=U, lens=torch.from_numpy(lens), nnz=nnz,
        grads=torch.from_numpy(grads),
        perm=torch.from_numpy(rng.permutation(nnz)),
        ustarts=torch.from_numpy(ustarts),
        seg_id=torch.from_numpy(seg_id),
        scale=torch.from_numpy(scale) if with_scale else torch.empty(0),
    )


def scatter_reference(grads, case, prefill=None):
    """f64 reduction of the SAME gradient bits, and E = 2 L 2^-23 S with
    S = sum |g scale| over the L contributing positions: one ulp for each
    product and one for each add (a fused multiply-add does better).  A
    pre-filled accumulator is one more addend."""
    U, dim = case["U"], case["dim"]
    run = torch.repeat_interleave(torch.arange(U), case["lens"])
    s = case["seg_id"][case["perm"]]
    sc_all = (case["scale"].double() if case["scale"].numel()
              else torch.ones(N_GRAD_ROWS, dtype=torch.float64))
    live = (s >= 0) & (sc_all[s.clamp_min(0)] != 0)
    sl = s.clamp_min(0)
    term = torch.where(live[:, None], grads.double()[sl] * sc_all[sl][:, None],
                       torch.zeros((), dtype=torch.float64))
    ref = torch.zeros(U, dim, dtype=torch.float64)
    S = torch.zeros_like(ref)
    ref.index_add_(0, run, term)
    S.index_add_(0, run, term.abs())
    L = torch.zeros(U, dtype=torch.float64)
    L.index_add_(0, run, live.double())
    L = L[:, None].expand(U, dim).clone()
    if prefill is not None:
        ref, S, L = ref + prefill.double(), S + prefill.double().abs(), L + 1
    return ref, 2 * L * EPS32 * S, L


def _f32_segment_loop(rows, case, drop_last=False):
    """What the kernel does, in plain numpy f32."""
    r = rows.float().numpy()
    inv, off = case["inverse"].numpy(), case["offsets"].numpy()
    n_seg = len(off) - 1
    out = np.zeros((n_seg, case["dim"]), dtype=np.float32)
    for s in range(n_seg):
        acc = np.zeros(case["dim"], dtype=np.float32)
        for k in range(off[s], off[s + 1] - int(drop_last)):
            acc = acc + r[inv[k]]
        sc = case["scale"].numpy()[s] if case["scale"].numel() else np.float32(1)
        out[s] = acc * sc
    return torch.from_numpy(out).half()


def _f32_scatter_loop(grads, case, skip_scale=False):
    g = grads.float().numpy()
    perm, sid, us = (case[k].numpy() for k in ("perm", "seg_id", "ustarts"))
    sc = case["scale"].numpy() if case["scale"].numel() else None
    out = np.zeros((case["U"], case["dim"]), dtype=np.float32)
    for u in range(case["U"]):
        for p in range(us[u], us[u + 1]):
            s = sid[perm[p]]
            if s < 0 or (sc is not None and sc[s] == 0):
                continue
            w = np.float32(1) if (sc is None or skip_scale) else sc[s]
            out[u] = out[u] + g[s] * w
    return torch.from_numpy(out)


def _worst(got, ref, bound):
    err = (got.double() - ref).abs()
    return (err / bound.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("dim", RED_DIMS)
def test_segment_bound_fits_f32_and_rejects_dropped_addend(dim):
    case = segment_case(dim, 37, True)
    for rows in (case["rows"], case["rows"].half()):
        ref, bound = segment_reference(rows, case)
        good = _worst(_f32_segment_loop(rows, case), ref, bound)
        bad = _worst(_f32_segment_loop(rows, case, drop_last=True), ref, bound)
        print(f"segment dim {dim} {rows.dtype}: err/bound {good:.3g}, "
              f"last addend dropped {bad:.3g}")
        assert good <= 1.0 < 10.0 < bad


@pytest.mark.parametrize("dim", RED_DIMS)
def test_scatter_bound_fits_f32_and_rejects_ignored_scale(dim):
    case = scatter_case(dim, 37, True)
    for grads in (case["grads"], case["grads"].half(), case["grads"].bfloat16()):
        ref, E, L = scatter_reference(grads, case)
        assert not torch.isnan(ref).any()  # the NaN rows never enter
        assert (ref[L == 0] == 0).all()
        got = _f32_scatter_loop(grads, case)
        good = _worst(got, ref, E)
        good16 = _worst(got.half(), ref, f16_store_bound(E, ref))
        bad = _worst(_f32_scatter_loop(grads, case, skip_scale=True), ref, E)
        print(f"scatter dim {dim} {grads.dtype}: err/bound {good:.3g} (f32), "
              f"{good16:.3g} (f16 out), scale ignored {bad:.3g}")
        assert good <= 1.0 and good16 <= 1.0 < 10.0 < bad


# ------------------------------------------------------------------ dedup cases

DEDUP_NNZ = (1, 2, 255, 256, 257, 4099)
DEDUP_KINDS = ("random", "all_equal", "all_distinct", "sorted")


def dedup_input(nnz, kind):
    """u64 keys; half of the random ones are >= 2^63, where the signed and
    the unsigned order differ."""
    rng = _rng(3, nnz, DEDUP_KINDS.index(kind))
    pool = rng.integers(1, 2 ** 64, size=max(1, nnz // 3 + 1), dtype=np.uint64)
    if kind == "all_equal":
        return np.full(nnz, pool[0] | np.uint64(1 << 63), dtype=np.uint64)
    if kind == "all_distinct":
        k = hashing.splitmix64(np.arange(1, nnz + 1, dtype=np.uint64))
        return k[rng.permutation(nnz)]
    keys = pool[rng.integers(0, len(pool), size=nnz)]
    return np.sort(keys) if kind == "sorted" else keys


def dedup_reference(keys_u64):
    """np.unique on the uint64 view -> uniq, inverse, ustarts, and the one
    permutation a STABLE sort gives."""
    uniq, inverse, counts = np.unique(keys_u64, return_inverse=True,
                                      return_counts=True)
    ustarts = np.zeros(len(uniq) + 1, dtype=np.int64)
    np.cumsum(counts, out=ustarts[1:])
    perm = np.argsort(keys_u64, kind="stable")
    return uniq, inverse.astype(np.int64), ustarts, perm.astype(np.int64)


@pytest.mark.parametrize("kind", DEDUP_KINDS)
@pytest.mark.parametrize("nnz", DEDUP_NNZ)
def test_engine_dedup_matches_numpy(nnz, kind):
    from persia_amd.core.engine import _dedup

    keys = dedup_input(nnz, kind)
    if nnz > 2 and kind in ("random", "all_distinct"):
        assert (keys >= np.uint64(1 << 63)).any() and (keys < np.uint64(1 << 63)).any()
    uniq, inverse, ustarts, _ = dedup_reference(keys)
    u, inv, perm, us = _dedup(as_keys(keys))
    assert np.array_equal(u.numpy().view(np.uint64), uniq)
    assert np.array_equal(inv.numpy(), inverse)
    assert np.array_equal(us.numpy(), ustarts)
    assert np.array_equal(keys[perm.numpy()], np.sort(keys))
