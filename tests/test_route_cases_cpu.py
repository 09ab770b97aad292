"""Cases and plain numpy models of tests/test_gpu_route_exact.py, and the
checks of them that need no GPU.

The fused distributed path is sign prep -> padded all-to-all routing ->
owner-side lookup -> owner-side merge and update.  A lease has one device, so
the native owner-side kernels never meet a buffer shaped like a real
multi-rank receive: `world` buckets of `cap` entries, each sorted and
zero-padded (the padding sits BETWEEN buckets), the same key in several
buckets.  This file builds such buffers without any collective:

* route_model: the bucket layout of one rank's sorted unique keys, from
  hashing.owner_of and a straight loop.  Route cases put keys on both sides of
  every owner threshold ceil(r 2^32 / world) << 32 for non-power-of-two worlds;
  the model is held to the CPU branch of EmbeddingEngine._a2a_route.
* exchange_model: what every owner receives when `world` ranks route their
  keys, and even_a2a, the even all-to-all as a slice-and-concatenate (it is its
  own inverse, so it carries keys and gradients out and rows back).
* sign-prep cases: many slots in one call, empty slots, hash-stack rounds and
  prefixes mixed, ragged samples, ids over the whole u64 range and the one id
  whose mixed key is the empty key; the model is held to
  EmbeddingEngine._prepare_slot_keys.
* wire_lookup_model / check_wire_lookup: what an owner's training lookup of a
  receive buffer must return (every occurrence of a key the f16 bits of its
  seeded init row, every padding entry a zero row), held to
  CpuEmbeddingStore.lookup_wire.
* dyadic gradients whose every partial sum is exact in f16 and f32, so the
  order and the sharding of a reduction cannot change a bit.

The last section shows the assertions have teeth: a route model that keeps the
wrong keys of an over-full segment, one that floors the threshold, and a lookup
result with one duplicate's row zeroed are all rejected.

Exchange cases, one reading made explicit: "200-600 unique keys per rank from
a shared pool of about 400" cannot all come from the pool, so a rank takes
up to 380 keys of a 400-key shared pool (the first 40 go to every rank) and
private keys up to its size.
"""
import functools
import types

import numpy as np
import pytest
import torch

from persia_amd.core import hashing
from persia_amd.core.store import (BUCKET_SIZE, CpuEmbeddingStore)
from persia_amd.embedding import EmbeddingConfig

import test_sparse_cases_cpu as SC
from test_sparse_cases_cpu import as_keys, expected_row

U64 = np.uint64
ZERO_REMAP = U64(0xD1B54A32D192ED03)


def _u64(xs):
    return np.array([int(x) & ((1 << 64) - 1) for x in xs], dtype=np.uint64)


# ---------------------------------------------------------------- route model


def route_model(uniq_u64, n_valid, world, cap, owner_fn=hashing.owner_of,
                keep_last=False):
    """-> (send u64[world*cap], idx i64[n_pad], dropped_keys).  The first
    `cap` keys of an owner's segment, in sorted order, take its bucket; the
    rest and the padding tail point at the dummy index world*cap.
    `owner_fn` / `keep_last` exist for the wrong variants at the end of this
    file."""
    uniq_u64 = np.asarray(uniq_u64, dtype=np.uint64)
    n_pad = len(uniq_u64)
    dummy = world * cap
    send = np.zeros(world * cap, dtype=np.uint64)
    idx = np.full(n_pad, dummy, dtype=np.int64)
    owner = owner_fn(uniq_u64[:n_valid], world)
    seen = [0] * world
    total = np.bincount(owner, minlength=world) if n_valid else [0] * world
    dropped = 0
    for i in range(n_valid):
        o = int(owner[i])
        pos = seen[o]
        seen[o] += 1
        if keep_last:  # wrong: the LAST cap keys of the segment
            pos -= max(0, int(total[o]) - cap)
        if 0 <= pos < cap:
            idx[i] = o * cap + pos
            send[o * cap + pos] = uniq_u64[i]
        else:
            dropped += 1
    return send, idx, dropped


def floor_owner(keys, world):
    """Wrong: owner thresholds floor(r 2^32 / world) in place of the ceil."""
    hi = (np.asarray(keys, dtype=np.uint64) >> U64(32)).astype(np.int64)
    owner = np.zeros(len(hi), dtype=np.int64)
    for r in range(1, world):
        owner += hi >= (r << 32) // world
    return owner


ROUTE_WORLDS = (1, 2, 3, 5, 6, 7, 8, 12)
ROUTE_VARIANTS = ("padded", "full", "one_owner", "none_valid", "empty",
                  "cap_exact", "cap_plus_one", "cap_one")


def threshold_keys(world):
    out = [1, (1 << 64) - 1]
    for r in range(1, world):
        hi = -((-r << 32) // world)  # ceil(r 2^32 / world)
        t = hi << 32
        out += [t - 1, t, t + 1, t | 0xFFFFFFFF, (hi - 1) << 32]
    return out


class RouteCase:
    def __init__(self, world, variant, uniq, n_valid, cap):
        self.world, self.variant = world, variant
        self.uniq, self.n_valid, self.cap = uniq, n_valid, cap
        self.n_pad = len(uniq)
        self.id = f"w{world}-{variant}"


@functools.lru_cache(maxsize=None)
def route_case(world, variant):
    rng = np.random.default_rng([11, world, ROUTE_VARIANTS.index(variant)])
    keys = np.unique(np.concatenate([
        _u64(threshold_keys(world)),
        rng.integers(1, 2 ** 64, size=300, dtype=np.uint64)]))
    assert (keys >= U64(1 << 63)).any() and (keys < U64(1 << 63)).any()
    owner = hashing.owner_of(keys, world)
    counts = np.bincount(owner, minlength=world)
    big = int(counts.argmax())
    cap = int(counts.max()) + 3
    pad = 37
    if variant == "full":
        pad = 0
    elif variant == "one_owner":
        keys = keys[owner == world // 2]
        cap = len(keys) + 3
    elif variant == "none_valid":
        keys, pad = keys[:0], 41
    elif variant == "empty":
        keys, pad = keys[:0], 0
    elif variant == "cap_exact":
        cap = int(counts.max())
    elif variant == "cap_plus_one":
        cap = int(counts.max()) - 1
        # only the largest segment is over-full, by exactly one key
        keep = np.ones(len(keys), dtype=bool)
        for o in range(world):
            if o != big and counts[o] > cap:
                keep[np.nonzero(owner == o)[0][cap:]] = False
        keys = keys[keep]
    elif variant == "cap_one":
        cap = 1
    uniq = np.concatenate([keys, np.zeros(pad, dtype=np.uint64)])
    return RouteCase(world, variant, uniq, len(keys), cap)


def all_route_cases():
    return [route_case(w, v) for w in ROUTE_WORLDS for v in ROUTE_VARIANTS]


# ------------------------------------------------------- the CPU engine's chain


@functools.lru_cache(maxsize=None)
def _cpu_engine():
    from persia_amd.core.comm import DistContext
    from persia_amd.core.engine import EmbeddingEngine
    from persia_amd.core.schema import EmbeddingSchema, GlobalConfig, SlotConfig
    from persia_amd.embedding.optim import SGD

    return EmbeddingEngine(
        schema=EmbeddingSchema(slots={"f0": SlotConfig(name="f0", dim=8)}),
        hyper=EmbeddingConfig(), optimizer=SGD(lr=0.1),
        gconf=GlobalConfig(capacity=64), device=torch.device("cpu"),
        dist_ctx=DistContext(1, 0))


def engine_route(case, counted=True):
    """The CPU branch of EmbeddingEngine._a2a_route on one case -> (send
    [world*cap], idx, what it added to the overflow counter).  counted=False
    hands it the exact (unpadded) keys and no count."""
    eng = _cpu_engine()
    n = case.n_pad if counted else case.n_valid
    plan = types.SimpleNamespace(
        dim=8, a2a_world=case.world, a2a_cap=case.cap,
        a2a_ar=torch.arange(n, dtype=torch.int64),
        a2a_ones=torch.ones(n, dtype=torch.int64))
    before = eng.check_a2a_overflow()
    send, idx = eng._a2a_route(
        plan, as_keys(case.uniq[:n]),
        torch.tensor([case.n_valid], dtype=torch.int64) if counted else None)
    return (send.numpy().view(np.uint64)[:case.world * case.cap], idx.numpy(),
            eng.check_a2a_overflow() - before)


def check_route_model(case, **wrong):
    """The self-checks of the route model on one case; the wrong variants
    must trip one of them."""
    w, cap = case.world, case.cap
    send, idx, dropped = route_model(case.uniq, case.n_valid, w, cap, **wrong)
    for counted in (True, False):
        e_send, e_idx, e_over = engine_route(case, counted)
        n = len(e_idx)
        assert np.array_equal(e_send, send), (case.id, counted)
        assert np.array_equal(e_idx, idx[:n]), (case.id, counted)
        # the counter's unit is dropped KEYS
        assert e_over == dropped, (case.id, counted)
    valid = case.uniq[:case.n_valid]
    kept = idx[:case.n_valid] < w * cap
    # kept and dropped keys partition the input; a kept key sits where idx says
    assert int((~kept).sum()) == dropped
    assert np.array_equal(send[idx[:case.n_valid][kept]], valid[kept])
    assert np.array_equal(np.sort(send[send != 0]), valid[kept])
    assert (idx[case.n_valid:] == w * cap).all()
    owner = hashing.owner_of(valid, w)
    assert (np.diff(owner) >= 0).all()  # monotone over the sorted keys
    assert (valid[1:] > valid[:-1]).all()
    for o in range(w):
        bucket = send[o * cap:(o + 1) * cap]
        fill = int((bucket != 0).sum())
        assert (bucket[fill:] == 0).all() and (bucket[:fill] != 0).all()
        assert (hashing.owner_of(bucket[:fill], w) == o).all()
    return send, idx, dropped


@pytest.mark.parametrize("world", ROUTE_WORLDS)
def test_route_model_is_the_cpu_engine_chain(world):
    for variant in ROUTE_VARIANTS:
        case = route_case(world, variant)
        send, idx, dropped = check_route_model(case)
        counts = np.bincount(
            hashing.owner_of(case.uniq[:case.n_valid], world), minlength=world)
        if variant in ("padded", "full", "one_owner", "cap_exact"):
            assert dropped == 0 and case.n_valid > 0
        if variant == "cap_exact":
            assert counts.max() == case.cap
        if variant == "one_owner":
            assert (counts > 0).sum() == 1
        if variant in ("none_valid", "empty"):
            assert dropped == 0 and not send.any()
            assert case.n_pad == (41 if variant == "none_valid" else 0)
        if variant == "cap_plus_one":
            # exactly one key is dropped: the largest of the over-full segment
            assert dropped == 1 and counts.max() == case.cap + 1
            o = int(counts.argmax())
            seg = case.uniq[:case.n_valid][
                hashing.owner_of(case.uniq[:case.n_valid], world) == o]
            lost = case.uniq[:case.n_valid][idx[:case.n_valid] == world * case.cap]
            assert lost.tolist() == [seg.max()]
        if variant == "cap_one":
            # more keys are dropped than owners overflow: the two units differ
            assert dropped == int(np.maximum(counts - 1, 0).sum())
            assert dropped > int((counts > 1).sum()) > 0


def test_route_cases_straddle_every_threshold():
    for world in ROUTE_WORLDS:
        case = route_case(world, "padded")
        keys = set(case.uniq[:case.n_valid].tolist())
        for r in range(1, world):
            hi = -((-r << 32) // world)
            assert hi * world >= r << 32 > (hi - 1) * world
            t = hi << 32
            assert {t - 1, t, t + 1, t | 0xFFFFFFFF, (hi - 1) << 32} <= keys
            o = hashing.owner_of(_u64([t - 1, t, (hi - 1) << 32]), world)
            assert o.tolist() == [r - 1, r, r - 1]
        assert {1, (1 << 64) - 1} <= keys


def test_overflow_counter_counts_dropped_keys():
    """One counter, one unit: the CPU branch of _a2a_route adds the number of
    keys that found no room, as the native route does."""
    case = route_case(5, "cap_one")
    counts = np.bincount(hashing.owner_of(case.uniq[:case.n_valid], 5), minlength=5)
    _, _, over = engine_route(case)
    assert over == int((counts - 1).clip(min=0).sum()) > 5


# ------------------------------------------------------------- exchange model


def even_a2a(bufs, world, cap):
    """The even all-to-all over per-rank buffers of world*cap rows (numpy or
    torch): rank o receives bucket o of every rank s, source-major."""
    cat = torch.cat if torch.is_tensor(bufs[0]) else np.concatenate
    return [cat([bufs[s][o * cap:(o + 1) * cap] for s in range(world)])
            for o in range(world)]


class Exchange:
    """sends[s] / idx[s]: rank s's route; recv_keys[o]: what owner o gets.
    Rows come back with even_a2a(rows_local) and go to rank s's unique keys
    through idx[s] (after a zero row is appended); gradients packed at idx[s]
    go forward with even_a2a."""

    def __init__(self, per_rank_uniq, world, cap):
        self.world, self.cap = world, cap
        self.per_rank = [np.asarray(u, dtype=np.uint64) for u in per_rank_uniq]
        routes = [route_model(u, len(u), world, cap) for u in self.per_rank]
        self.sends = [r[0] for r in routes]
        self.idx = [r[1] for r in routes]
        self.dropped = sum(r[2] for r in routes)
        self.recv_keys = even_a2a(self.sends, world, cap)


def exchange_model(per_rank_uniq, world, cap):
    return Exchange(per_rank_uniq, world, cap)


EXCHANGE_WORLDS = (2, 3, 5, 8)
POOL = 400
EVERYWHERE = 40


@functools.lru_cache(maxsize=None)
def exchange_case(world):
    rng = np.random.default_rng([12, world])
    pool = SC.mixed_keys(1 << 20, POOL)
    per_rank = []
    for s in range(world):
        size = int(rng.integers(200, 601))
        n_shared = int(rng.integers(min(250, size), min(380, size) + 1))
        shared = np.concatenate([
            pool[:EVERYWHERE],
            pool[EVERYWHERE + rng.permutation(POOL - EVERYWHERE)
                 [:n_shared - EVERYWHERE]]])
        private = SC.mixed_keys((2 + s) << 20, size - n_shared)
        per_rank.append(np.unique(np.concatenate([shared, private])))
        assert len(per_rank[-1]) == size
    cap = 3 + max(int(np.bincount(hashing.owner_of(u, world),
                                  minlength=world).max()) for u in per_rank)
    return exchange_model(per_rank, world, cap)


def large_exchange():
    """4096 distinct keys, each in all 8 buckets of one owner's buffer."""
    keys = np.sort(SC.mixed_keys(5 << 20, 4096))
    return np.tile(keys, 8)


@pytest.mark.parametrize("world", EXCHANGE_WORLDS)
def test_exchange_cases_overlap_and_fit(world):
    ex = exchange_case(world)
    assert ex.dropped == 0
    allk = np.concatenate(ex.per_rank)
    uniq, n_ranks = np.unique(allk, return_counts=True)
    assert all(200 <= len(u) <= 600 for u in ex.per_rank)
    assert (n_ranks == world).sum() >= EVERYWHERE
    shared = np.isin(uniq, SC.mixed_keys(1 << 20, POOL))
    assert (n_ranks[shared] > 1).mean() > 0.5
    for o in range(world):
        rk = ex.recv_keys[o]
        assert len(rk) == world * ex.cap
        for s in range(world):
            b = rk[s * ex.cap:(s + 1) * ex.cap]
            mine = ex.per_rank[s][hashing.owner_of(ex.per_rank[s], world) == o]
            assert np.array_equal(b[:len(mine)], mine) and not b[len(mine):].any()
            assert len(mine) < ex.cap  # zero padding between the buckets
        nz = rk[rk != 0]
        assert len(np.unique(nz)) < len(nz)  # duplicates across buckets
    # every key reaches exactly its owner, once per rank that holds it
    got = np.concatenate(ex.recv_keys)
    assert np.array_equal(np.sort(got[got != 0]), np.sort(allk))
    # the way back: a rank's keys return through idx
    back = even_a2a(ex.recv_keys, world, ex.cap)
    for s in range(world):
        assert np.array_equal(back[s][ex.idx[s]], ex.per_rank[s])


# ----------------------------------------------------------- owner-side lookup

WIRE_BOUNDS = (-0.5, 0.5)


def wire_lookup_model(recv_keys, dim, opt, bounds=WIRE_BOUNDS):
    """f16 rows of a training lookup of fresh keys: the init row of every
    occurrence of a key, zeros at the padding."""
    recv_keys = np.asarray(recv_keys, dtype=np.uint64)
    out = np.zeros((len(recv_keys), dim), dtype=np.float16)
    uniq, inverse = np.unique(recv_keys, return_inverse=True)
    rows = np.stack([
        np.zeros(dim, np.float32) if k == 0
        else expected_row(k, dim, bounds, opt)[:dim] for k in uniq])
    out[:] = rows.astype(np.float16)[inverse]
    return out


def check_wire_lookup(rows_f16, recv_keys, dim, opt, bounds=WIRE_BOUNDS):
    """rows_f16: numpy float16 [n, dim].  Bits, not values."""
    exp = wire_lookup_model(recv_keys, dim, opt, bounds)
    got = np.ascontiguousarray(rows_f16).view(np.uint16)
    bad = np.nonzero((got != exp.view(np.uint16)).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        kind = ("zeros" if not np.asarray(rows_f16[i], np.float32).any()
                else "other values")
        raise AssertionError(
            f"{len(bad)} of {len(recv_keys)} rows differ from the init row; "
            f"first: position {i}, key {int(recv_keys[i]):#x}, got {kind} "
            f"{np.asarray(rows_f16[i][:4], np.float32)}")
    return exp


def _wire_store(dim, opt, capacity=1 << 13):
    return CpuEmbeddingStore(
        dim, capacity, opt, EmbeddingConfig(emb_initialization=WIRE_BOUNDS))


@pytest.mark.parametrize("world", EXCHANGE_WORLDS)
def test_cpu_store_wire_lookup_is_the_model(world):
    ex = exchange_case(world)
    opt = SC.mk_init_opt("adagrad")
    o = world - 1
    store = _wire_store(24, opt)
    rk = ex.recv_keys[o]
    rows = store.lookup_wire(as_keys(rk), True, torch.float16).numpy()
    check_wire_lookup(rows, rk, 24, opt)
    distinct = np.unique(rk[rk != 0])
    assert len(store) == len(distinct)
    signs, _ = store.export_rows()
    assert len(np.unique(signs)) == len(signs) == len(distinct)
    again = store.lookup_wire(as_keys(rk), True, torch.float16).numpy()
    assert np.array_equal(again.view(np.uint16), rows.view(np.uint16))


# full-table variant: 64 buckets, every slot holds an older, stamped row; one
# new key per disjoint probe window, so each has a non-current victim
FULL_DIM = 24
FULL_WORLD = 8


def full_table_case():
    """-> (old signs, old stamped rows [512, row_width], recv_keys): the
    duplicate-heavy buffer of 16 new keys, each in all 8 buckets."""
    opt = SC.mk_init_opt("adagrad")
    rw = FULL_DIM + opt.require_space(FULL_DIM)
    old = _u64([SC.window_key(c, h) for h in range(SC.N_BUCKETS)
                for c in range(1, BUCKET_SIZE + 1)])
    rows = torch.stack([SC.stamp_row(3, k, rw) for k in old]).numpy()
    new = np.sort(_u64([SC.window_key(100 + w, 1 + 4 * w)
                        for w in range(SC.WINDOWS)]))
    cap = len(new) + 2
    bucket = np.concatenate([new, np.zeros(2, dtype=np.uint64)])
    assert len(bucket) == cap
    return hashing.splitmix64_inv(old), rows, np.tile(bucket, FULL_WORLD), opt


def test_full_table_case_on_the_cpu_store():
    signs, rows, rk, opt = full_table_case()
    store = CpuEmbeddingStore(
        FULL_DIM, SC.CAPACITY, opt,
        EmbeddingConfig(emb_initialization=WIRE_BOUNDS))
    store.import_rows(signs, rows)
    assert len(store) == SC.CAPACITY  # full, every row stamped (>= 4)
    assert store.arena.min().item() >= 4.0
    out = store.lookup_wire(as_keys(rk), True, torch.float16).numpy()
    check_wire_lookup(out, rk, FULL_DIM, opt)
    assert np.abs(out.astype(np.float32)).max() <= 0.5  # no stamp
    new = np.unique(rk[rk != 0])
    assert len(store) == SC.CAPACITY  # every new key evicted, none overflowed
    assert all(store._probe(k) >= 0 for k in new)
    assert int((store.ticks == store.tick - 1).sum()) == len(new) == 16


# ------------------------------------------------------------ dyadic gradients


def dyadic_grads(rng, n, dim):
    """f16 [n, dim], multiples of 2^-6 in [-4, 4]."""
    g = rng.integers(-256, 257, size=(n, dim)).astype(np.float32) / 64.0
    return torch.from_numpy(g).half()


def assert_sums_exact(grads, keys, max_addends=8):
    """Every partial sum of at most `max_addends` of these gradients is a
    multiple of 2^-6 no larger than 32: 11 significant bits, exact in f16
    (and f32), whatever the order.  `keys`: the key of every gradient row."""
    g = grads.double().numpy()
    assert np.array_equal(g * 64, np.round(g * 64)) and np.abs(g).max() <= 4.0
    _, counts = np.unique(np.asarray(keys), return_counts=True)
    assert counts.max() <= max_addends
    assert max_addends * 4.0 * 64 <= 2 ** 11
    # and indeed: the f16 running sum of the worst key equals the f64 one
    worst = torch.full((max_addends, 1), 4.0, dtype=torch.float16)
    acc = torch.zeros(1, dtype=torch.float16)
    for r in worst:
        acc = (acc + r).half()
    assert acc.item() == 4.0 * max_addends


def test_dyadic_gradients_sum_exactly_in_f16():
    rng = np.random.default_rng(5)
    g = dyadic_grads(rng, 64, 8)
    keys = np.repeat(np.arange(8), 8)
    assert_sums_exact(g, keys)
    for order in (np.arange(64), rng.permutation(64)):
        acc = torch.zeros(8, 8, dtype=torch.float16)
        for i in order:
            acc[keys[i]] = (acc[keys[i]] + g[i]).half()
        ref = torch.zeros(8, 8, dtype=torch.float64)
        ref.index_add_(0, torch.from_numpy(keys), g.double())
        assert torch.equal(acc.double(), ref)


# ------------------------------------------------------------- sign-prep cases

SPACING = (1 << 56) - 1  # feature_index_prefix_bit = 8
PREP_TOTALS = (1, 255, 256, 257, 4099)
ID_EDGES = (0, (1 << 63) - 1, 1 << 63, (1 << 64) - 1)
UNMIX_ZERO = int(hashing.splitmix64_inv(np.zeros(1, dtype=np.uint64))[0])


class PrepSlot:
    def __init__(self, name, values, offsets, rounds, size, prefix):
        self.name, self.values, self.offsets = name, values, offsets
        self.rounds, self.size, self.prefix = rounds, size, prefix


def _ragged_offsets(rng, n):
    """Sample lengths summing to n with an empty sample first, last, and two
    adjacent empty ones in between."""
    k = min(n, 6)
    cuts = np.sort(rng.choice(np.arange(1, n), size=k - 1, replace=False)) \
        if k > 1 else np.zeros(0, dtype=np.int64)
    lens = np.diff(np.concatenate([[0], cuts, [n]])).tolist() if n else []
    lens = [0] + lens[:1] + [0, 0] + lens[1:] + [0]
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return off


# (rounds, embedding_size, non-zero prefix?, empty?) per slot
PLAIN_LAYOUT = ((0, 1, True, True), (0, 1, False, False), (0, 1, True, False),
                (0, 1, False, True), (0, 1, False, False), (0, 1, True, False),
                (0, 1, True, True))
STACK_LAYOUT = ((2, 97, True, True), (0, 1, False, False), (1, 1, True, False),
                (2, 97, False, False), (5, 97, False, True), (0, 1, True, False),
                (5, 1, True, False), (0, 1, False, True))


@functools.lru_cache(maxsize=None)
def prep_case(kind, total):
    """Slots of one sign-prep call whose INPUT lengths sum to `total`."""
    layout = PLAIN_LAYOUT if kind == "plain" else STACK_LAYOUT
    rng = np.random.default_rng([13, int(kind == "plain"), total])
    live = [i for i, l in enumerate(layout) if not l[3]]
    if total < len(live):
        live = live[:total]
    share = np.full(len(live), total // len(live))
    share[: total % len(live)] += 1
    if total > 50:  # uneven, still summing to total
        share[0] += 7
        share[-1] -= 7
    sizes = dict(zip(live, share.tolist()))
    slots = []
    for i, (rounds, size, prefixed, _empty) in enumerate(layout):
        n = sizes.get(i, 0)
        vals = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
        edges = list(ID_EDGES)
        if rounds == 0 and not prefixed:
            edges.insert(0, UNMIX_ZERO)  # mixes to the empty key
        m = min(n, len(edges))
        vals[:m] = _u64(edges[:m])
        vals = vals[rng.permutation(n)] if n > 1 else vals
        slots.append(PrepSlot(f"s{i}", vals, _ragged_offsets(rng, n), rounds,
                              size, ((i + 1) << 56) if prefixed else 0))
    assert sum(len(s.values) for s in slots) == total
    return slots


def all_prep_cases():
    return [(k, t) for k in ("plain", "stack") for t in PREP_TOTALS]


def _mix_slot(signs, prefix):
    keys = hashing.splitmix64(hashing.apply_prefix(signs, prefix, SPACING))
    keys[keys == 0] = ZERO_REMAP
    return keys


def sign_prep_model(slots):
    """Mixed keys of the whole call, slot after slot: hash-stack expansion
    (round-major inside each sample), prefix fold, mix, empty-key remap."""
    out = []
    for s in slots:
        vals = s.values
        if s.rounds:
            stacked = hashing.hash_stack(vals, s.rounds, s.size)
            pieces = []
            for b in range(len(s.offsets) - 1):
                lo, hi = s.offsets[b], s.offsets[b + 1]
                pieces += [stacked[r, lo:hi] for r in range(s.rounds)]
            vals = np.concatenate(pieces) if pieces else vals
        out.append(_mix_slot(vals, s.prefix))
    return np.concatenate(out)


def prep_kernel_args(slots):
    """The arrays _group_keys hands sign_prep / sign_prep_stack."""
    in_lens = [len(s.values) for s in slots]
    out_lens = [n * max(s.rounds, 1) for n, s in zip(in_lens, slots)]
    offs = [s.offsets * s.rounds if s.rounds else s.offsets for s in slots]
    return dict(
        values=np.concatenate([s.values for s in slots]).view(np.int64),
        in_starts=np.concatenate([[0], np.cumsum(in_lens)]).astype(np.int64),
        out_starts=np.concatenate([[0], np.cumsum(out_lens)]).astype(np.int64),
        prefixes=_u64([s.prefix for s in slots]).view(np.int64),
        rounds=np.array([s.rounds for s in slots], dtype=np.int32),
        sizes=np.array([s.size if s.rounds else 1 for s in slots], dtype=np.int64),
        off_starts=np.concatenate(
            [[0], np.cumsum([len(o) for o in offs])]).astype(np.int64),
        all_offs=np.concatenate(offs).astype(np.int64),
        n_out=int(sum(out_lens)),
    )


def prep_schema(slots, dim=8):
    """A schema whose slots carry the case's rounds and prefixes (a prefix of
    0 beside non-zero ones is written over the assigned one)."""
    from persia_amd.core.schema import (EmbeddingSchema, HashStackConfig,
                                        SlotConfig)

    schema = EmbeddingSchema(slots={
        s.name: SlotConfig(
            name=s.name, dim=dim,
            hash_stack_config=HashStackConfig(s.rounds, s.size)
            if s.rounds else None)
        for s in slots})
    assert schema.feature_spacing == SPACING
    for s in slots:
        schema.slots[s.name].index_prefix = s.prefix
    return schema


def prep_feats(slots):
    from persia_amd.embedding.data import _FlatIDFeature

    return [_FlatIDFeature(s.name, s.values, s.offsets) for s in slots]


@pytest.mark.parametrize("kind,total", all_prep_cases())
def test_sign_prep_model_is_prepare_slot_keys(kind, total):
    from persia_amd.core.engine import EmbeddingEngine

    slots = prep_case(kind, total)
    stub = types.SimpleNamespace(schema=prep_schema(slots))
    got, pos = [], 0
    args = prep_kernel_args(slots)
    for i, f in enumerate(prep_feats(slots)):
        keys, offsets = EmbeddingEngine._prepare_slot_keys(stub, f)
        got.append(keys)
        # the expanded offsets _group_keys uploads are the CPU path's
        lo = args["off_starts"][i]
        assert np.array_equal(args["all_offs"][lo:lo + len(offsets)], offsets)
        assert args["out_starts"][i] == pos
        pos += len(keys)
    model = sign_prep_model(slots)
    assert np.array_equal(np.concatenate(got), model)
    assert len(model) == args["n_out"] and (model != 0).all()


def test_sign_prep_cases_cover_the_edges():
    for kind, total in all_prep_cases():
        slots = prep_case(kind, total)
        assert 6 <= len(slots) <= 8
        empty = [len(s.values) == 0 for s in slots]
        assert empty[0] and empty[-1] and any(empty[1:-1])
        if total < 255:
            continue
        combos = {(s.rounds > 0, s.prefix != 0) for s in slots if len(s.values)}
        want = {(False, False), (False, True)}
        if kind == "stack":
            want |= {(True, False), (True, True)}
            assert {s.rounds for s in slots} == {0, 1, 2, 5}
            assert {s.size for s in slots if s.rounds} == {1, 97}
        assert combos == want
        for s in slots:
            if not len(s.values):
                continue
            assert set(ID_EDGES) <= set(s.values.tolist())
            lens = np.diff(s.offsets)
            assert lens[0] == 0 and lens[-1] == 0
            assert ((lens[1:] == 0) & (lens[:-1] == 0)).any()
        assert (np.concatenate([s.values for s in slots]) >= U64(1 << 63)).any()
    # the one id whose mixed key is the empty key comes out remapped
    for kind, total in all_prep_cases():
        slots = prep_case(kind, total)
        hit = [s for s in slots if s.rounds == 0 and s.prefix == 0
               and UNMIX_ZERO in s.values.tolist()]
        assert hit, (kind, total)
        keys = _mix_slot(hit[0].values, 0)
        assert keys[hit[0].values.tolist().index(UNMIX_ZERO)] == ZERO_REMAP
    assert hashing.splitmix64(_u64([UNMIX_ZERO]))[0] == 0


# -------------------------------------------------- the assertions have teeth


def test_route_model_keeping_the_wrong_keys_is_rejected():
    check_route_model(route_case(5, "padded"), keep_last=True)  # nothing over-full
    for variant in ("cap_plus_one", "cap_one"):
        with pytest.raises(AssertionError):
            check_route_model(route_case(5, variant), keep_last=True)


def test_route_model_with_floored_thresholds_is_rejected():
    # power-of-two worlds divide 2^32: floor and ceil agree there
    check_route_model(route_case(8, "padded"), owner_fn=floor_owner)
    with pytest.raises(AssertionError):
        check_route_model(route_case(3, "padded"), owner_fn=floor_owner)


def test_lookup_result_with_a_zeroed_duplicate_is_rejected():
    ex = exchange_case(3)
    opt = SC.mk_init_opt("adagrad")
    rk = ex.recv_keys[0]
    rows = wire_lookup_model(rk, 8, opt)
    check_wire_lookup(rows, rk, 8, opt)
    uniq, first, counts = np.unique(rk, return_index=True, return_counts=True)
    k = uniq[(counts > 1) & (uniq != 0)][0]
    dup = np.nonzero(rk == k)[0][1]  # a later occurrence: its peer stays right
    bad = rows.copy()
    bad[dup] = 0
    with pytest.raises(AssertionError, match="zeros"):
        check_wire_lookup(bad, rk, 8, opt)
