"""The native lookup of multi-ID (bag) sum slots against exact models.

Scenarios, the numpy model of bag_plan, the f64 reference and the bound come
from tests/test_bag_cases_cpu.py, which checks them without a GPU.

A. bag_plan, exactly: cat_offsets, seg_id and seg_lens equal the numpy model;
   the scale is 1 bit for bit on a plain slot and within 2 ulp of
   1/sqrt(max(len, 1)) on a sqrt slot; no scale tensor without a sqrt slot.
B. lookup_local_bags against the existing pieces on a twin store: sign_prep ->
   dedup_padded -> store.lookup(u_count) -> segment_sum with the same scale
   tensor.  sums, the dedup tensors and the exported tables are bit-equal,
   over three training steps and an eval lookup of a trained table (which
   leaves keys and rows untouched).  One dim per lane layout of bag_sum.
C. The sums of B against f64 from the same row bits:
   E = (L + 1) 2^-23 scale S, plus 2 * 2^-23 scale S on a sqrt slot, then the
   f16 store bound.  See MEASURED below; no constant had to be raised.
D. Misses (40 keys of one home bucket on a table of one probe window, with
   and without stochastic admission): which key wins a slot is not
   determined, so only the structure is asserted -- every segment is the
   in-order f32 sum of the rows of those of its keys that an eval lookup
   afterwards finds resident.
E. The update hints: a slot hint names the slot that holds the key, a source
   hint is the segment of a key's only position.
F. The engine: PA_BAG_FAST on against off, bit for bit (sum_base at every
   step, the tables after both update contracts, Adagrad and Adam); a
   sqrt-scaling slot against the CPU engine; and that the path was taken,
   stays sync-free through apply_gradients_base, and is not taken by a group
   with a raw or hashstack slot.

MEASURED (MI355X, worst err/bound over all cases of section C):
  bag_sum           0.9956 (dims 512 and 520; 0.945 at dim 2, 0.989 at dims 16
                    and 24, 0.994 at 96, 128 and 256; plain and sqrt slots
                    together -- the f16 store term is tight by construction)
"""
import numpy as np
import pytest
import torch

import test_bag_cases_cpu as BC
import test_engine_paths as P
from test_gpu_dense_exact import _bits, _dev, _native

pytestmark = pytest.mark.gpu

_worst = {}


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _upload(slots):
    from persia_amd.core.engine import pack_bag_buffer

    buf, nnz, B = pack_bag_buffer(BC.bag_feats(slots))
    return torch.from_numpy(buf).to(_dev()), nnz, len(slots), B


def _flags(sqrt_flags):
    return torch.tensor(list(sqrt_flags) if any(sqrt_flags) else [],
                        dtype=torch.int32, device=_dev())


# ------------------------------------------------------------------ A. bag_plan


@pytest.mark.parametrize("kind", ["mixed", "empty_slot", "long", "all_empty"])
@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("S", [1, 3])
def test_bag_plan_matches_numpy_model(S, B, kind):
    slots = BC.bag_slots(S, B, kind)
    up, nnz, _S, _B = _upload(slots)
    plan = up[nnz:]
    for sqrt_flags in ((False,) * S, (True, False, True)[:S]):
        cat, seg_id, lens, scale = BC.plan_model(slots, sqrt_flags)
        g_cat, g_seg, g_lens, g_scale = _native().bag_plan(
            plan, S, B, nnz, _flags(sqrt_flags))
        assert np.array_equal(g_cat.cpu().numpy(), cat)
        assert np.array_equal(g_seg.cpu().numpy(), seg_id)
        assert g_lens.dtype == torch.float32
        assert np.array_equal(g_lens.cpu().numpy(), lens)
        if scale is None:
            assert g_scale.numel() == 0
        else:
            assert g_scale.dtype == torch.float32 and g_scale.numel() == S * B
            BC.check_scale(g_scale.cpu().numpy(), scale,
                           np.repeat(np.asarray(sqrt_flags), B))
    if kind == "long":
        assert (lens == BC.LONG_BAG).sum() == 1
    if kind == "all_empty":
        assert nnz == 0 and g_seg.numel() == 0


# --------------------------------------------- B, C, E. against a twin store

# packed, part of a wave, 1 / 2 (tail past dim) / 2 / 4 / 8 columns per lane,
# and a second pass over the columns
LOOKUP_DIMS = (2, 16, 24, 96, 128, 256, 512, 520)
SQRT = (False, True, True)
SPACING = 1 << 56
PREFIXES = (0, 1 << 56, 2 << 56)


def _mk_store(dim, optname="adagrad", capacity=1 << 14, admit=1.0):
    from persia_amd.core.store import HipEmbeddingStore
    from persia_amd.embedding import EmbeddingConfig

    return HipEmbeddingStore(
        dim, capacity, P.mk_opt(optname),
        EmbeddingConfig(emb_initialization=(-0.5, 0.5),
                        admit_probability=admit), _dev())


def _prefixes(S):
    return torch.tensor(PREFIXES[:S], dtype=torch.int64, device=_dev())


def _twin_lookup(twin, up, nnz, S, B, cat_offsets, scale, train):
    """The same lookup out of the existing pieces -> (sums, dedup, rows)."""
    C = _native()
    keys = C.sign_prep(up[:nnz], up[nnz : nnz + S + 1], _prefixes(S), SPACING)
    d = C.dedup_padded(keys)
    rows = twin.lookup(d[0], train, u_count=d[4])
    return C.segment_sum(rows, d[1], cat_offsets, scale), d, rows


def _sorted_table(store):
    torch.cuda.synchronize()
    signs, rows = store.export_rows()
    order = np.argsort(signs)
    return signs[order], rows[order]


def _assert_same_tables(a, b, what):
    (sa, ra), (sb, rb) = _sorted_table(a), _sorted_table(b)
    assert np.array_equal(sa, sb), f"{what}: signs"
    assert np.array_equal(ra.view(np.int32), rb.view(np.int32)), f"{what}: rows"


def _check_hints(store, res, what):
    (_sums, uniq, _inv, perm, ustarts, u_count, slot_hint, src_hint,
     _cat, seg_id, _lens, _scale) = res
    U = int(u_count.item())
    assert slot_hint.numel() == uniq.numel() == src_hint.numel()
    sh = slot_hint[:U].cpu().numpy()
    assert (sh < store.n_slots).all()
    held = _u64(store.keys)[sh[sh >= 0]]
    assert np.array_equal(held, _u64(uniq)[:U][sh >= 0]), f"{what}: slot_hint"
    us = ustarts[: U + 1].cpu().numpy()
    first = seg_id.cpu().numpy()[perm.cpu().numpy()[us[:-1]]]
    want = np.where(np.diff(us) == 1, first, -1)
    assert np.array_equal(src_hint[:U].cpu().numpy(), want), f"{what}: src_hint"
    return sh


@pytest.mark.parametrize("dim", LOOKUP_DIMS)
def test_lookup_local_bags_matches_twin_and_f64(dim):
    store, twin = _mk_store(dim), _mk_store(dim)
    S, B = 3, 32
    sqrt_seg = np.repeat(np.asarray(SQRT), B)
    ratio = 0.0

    def step(kind, seed, train, hints):
        nonlocal ratio
        slots = BC.bag_slots(S, B, kind, seed=seed)
        up, nnz, _S, _B = _upload(slots)
        res = store.lookup_local_bags(up, nnz, S, B, _prefixes(S), SPACING,
                                      _flags(SQRT), hints, train)
        sums, uniq, inverse, perm, ustarts, u_count = res[:6]
        cat_offsets, seg_id, seg_lens, scale = res[8:]
        what = f"dim {dim} {kind} seed {seed} train {train}"
        assert sums.dtype == torch.float16 and sums.shape == (S * B, dim)
        t_sums, d, rows = _twin_lookup(twin, up, nnz, S, B, cat_offsets, scale,
                                       train)
        assert torch.equal(_bits(sums), _bits(t_sums)), f"{what}: sums"
        U = int(u_count.item())
        for got, ref, name in zip((uniq, inverse, perm, ustarts, u_count), d,
                                  ("uniq", "inverse", "perm", "ustarts",
                                   "u_count")):
            assert got.shape == ref.shape, f"{what}: {name}"
            if name == "ustarts":  # nnz-padded: the tail is unspecified
                got, ref = got[: U + 1], ref[: U + 1]
            assert torch.equal(got, ref), f"{what}: {name}"
        cat, m_seg, m_lens, m_scale = BC.plan_model(slots, SQRT)
        assert np.array_equal(cat_offsets.cpu().numpy(), cat)
        assert np.array_equal(seg_id.cpu().numpy(), m_seg)
        assert np.array_equal(seg_lens.cpu().numpy(), m_lens)
        BC.check_scale(scale.cpu().numpy(), m_scale, sqrt_seg)
        if train and hints:
            _check_hints(store, res, what)
        else:
            assert res[6].numel() == 0 and res[7].numel() == 0
        # C: f64 from the same row bits (a missing key's row is zeros)
        ref, bound = BC.bag_reference(rows.cpu(), inverse.cpu(), cat, sqrt_seg)
        err = (sums.cpu().double() - ref).abs()
        assert bool((err <= bound).all()), f"{what}: f64 bound"
        ratio = max(ratio, BC.worst(sums.cpu(), ref, bound))
        return res

    step("mixed", 0, True, True)
    step("long", 1, True, False)   # hints off: same results, none returned
    res = step("empty_slot", 2, True, True)
    _assert_same_tables(store, twin, f"dim {dim} after training lookups")
    assert store.tick == twin.tick == 4  # one tick per call
    # train the rows both stores hold, then an eval lookup with unseen ids
    U = int(res[5].item())
    g = torch.randn(U, dim, device=_dev(),
                    generator=torch.Generator(_dev()).manual_seed(dim))
    store.update_gradients(res[1][:U], g)
    twin.update_gradients(res[1][:U], g)
    keys_before = store.keys.clone()
    arena_before = store.arena.clone()
    slots = BC.bag_slots(S, B, "mixed", seed=3, vocab=2 * BC.VOCAB)
    up, nnz, _S, _B = _upload(slots)
    step_eval = store.lookup_local_bags(up, nnz, S, B, _prefixes(S), SPACING,
                                        _flags(SQRT), True, False)
    t_sums, d, rows = _twin_lookup(twin, up, nnz, S, B, step_eval[8],
                                   step_eval[11], False)
    assert torch.equal(_bits(step_eval[0]), _bits(t_sums)), "eval sums"
    assert step_eval[6].numel() == 0 and step_eval[7].numel() == 0
    n_miss = int((rows[: int(d[4].item())] == 0).all(dim=1).sum())
    assert n_miss > 0, "the eval batch has unseen ids"
    assert torch.equal(store.keys, keys_before)
    assert torch.equal(_bits(store.arena), _bits(arena_before))
    assert store.tick == twin.tick == 5
    _assert_same_tables(store, twin, f"dim {dim} after the eval lookup")
    ref, bound = BC.bag_reference(rows.cpu(), step_eval[2].cpu(),
                                  step_eval[8].cpu(), sqrt_seg)
    err = (step_eval[0].cpu().double() - ref).abs()
    assert bool((err <= bound).all()), "eval: f64 bound"
    ratio = max(ratio, BC.worst(step_eval[0].cpu(), ref, bound))
    print(f"bag_sum dim {dim}: worst err/bound {ratio:.4f}, "
          f"{n_miss} eval misses")
    _worst["bag_sum"] = max(_worst.get("bag_sum", 0.0), ratio)


def test_all_bags_empty():
    """nnz == 0 is legal: zero sums, no unique key, no hints."""
    store = _mk_store(16)
    S, B = 3, 5
    up, nnz, _S, _B = _upload(BC.bag_slots(S, B, "all_empty"))
    assert nnz == 0
    res = store.lookup_local_bags(up, 0, S, B, _prefixes(S), SPACING,
                                  _flags(SQRT), True, True)
    assert res[0].shape == (S * B, 16) and not res[0].any()
    assert int(res[5].item()) == 0 and res[1].numel() == 0
    assert res[4].cpu().tolist() == [0]
    assert res[8].cpu().tolist() == [0] * (S * B + 1)
    assert len(store) == 0


def test_group_beyond_the_thread_per_position_grid_is_refused():
    """sign_prep, the dedup epilogue and probe_claim run one thread per
    position on a grid capped at 16384 blocks of 256; a larger group is
    refused on the host, before any launch."""
    store = _mk_store(8, capacity=64)
    nnz = 16384 * 256 + 1
    slots = [(np.zeros(nnz, np.uint64), np.array([0, nnz], np.int64))]
    up, _nnz, S, B = _upload(slots)
    with pytest.raises(RuntimeError, match="4194304"):
        store.lookup_local_bags(up, nnz, S, B, _prefixes(S), SPACING,
                                _flags(()), True, True)
    assert len(store) == 0


# ------------------------------------------------------------------- D. misses


def _ids_of_home_bucket(n, home, n_buckets):
    from persia_amd.core import hashing

    ids = np.arange(1, 4096, dtype=np.uint64)
    keys = hashing.splitmix64(ids)
    ids = ids[(keys & np.uint64(n_buckets - 1)) == np.uint64(home)]
    assert len(ids) >= n
    return ids[:n]


@pytest.mark.parametrize("admit", [1.0, 0.5])
def test_misses_contribute_nothing(admit):
    from persia_amd.core.store import BUCKET_SIZE, PROBE_BUCKETS

    dim, S, B = 8, 2, 8
    cap = BUCKET_SIZE * PROBE_BUCKETS
    store = _mk_store(dim, capacity=cap, admit=admit)
    assert store.n_slots == cap
    ids = _ids_of_home_bucket(40, 1, store.n_buckets)
    rng = np.random.default_rng(int(admit * 10))
    pos = np.concatenate([ids, rng.choice(ids, size=10)])
    pos = pos[rng.permutation(len(pos))]
    cuts = np.sort(rng.integers(0, len(pos) + 1, size=S * B - 1))
    cuts[3] = cuts[2]  # an empty bag at least
    bounds = np.concatenate([[0], cuts, [len(pos)]])
    half = bounds[B]
    slots = [(pos[:half], bounds[: B + 1].astype(np.int64)),
             (pos[half:], (bounds[B:] - half).astype(np.int64))]
    up, nnz, _S, _B = _upload(slots)
    no_prefix = torch.zeros(S, dtype=torch.int64, device=_dev())
    res = store.lookup_local_bags(up, nnz, S, B, no_prefix, -1, _flags(()),
                                  True, True)
    sums, uniq, inverse, u_count, cat = res[0], res[1], res[2], res[5], res[8]
    U = int(u_count.item())
    assert U == 40 and res[11].numel() == 0
    sh = _check_hints(store, res, f"admit {admit}")
    rows = store.lookup(uniq[:U], train=False)
    resident = ~(rows == 0).all(dim=1).cpu().numpy()
    print(f"admit {admit}: {int(resident.sum())} of 40 keys resident, "
          f"{int((sh >= 0).sum())} slot hints")
    assert np.array_equal(resident, sh >= 0)
    if admit == 1.0:
        assert resident.sum() == cap  # the window is full, 8 keys overflow
    else:
        assert 5 <= resident.sum() < cap  # about half were refused
    want = BC.f32_bag_loop(rows.cpu().numpy(), inverse.cpu().numpy(),
                           cat.cpu().numpy())
    assert torch.equal(_bits(sums.cpu()), _bits(want))


# ------------------------------------------------------------------ F. engine

NAMES = tuple(P.SINGLE_SLOTS)  # a, b: dim 8; c, d: dim 16


def _engine(monkeypatch, bag_fast, optname, device=None, schema=None):
    monkeypatch.setenv("PA_BAG_FAST", "1" if bag_fast else "0")
    eng = P.mk_engine(device or _dev(), optname, schema)
    assert eng._bag_fast == bag_fast
    return eng


def _assert_path(tb, taken):
    for g in tb._groups:
        if taken:
            assert g.u_count is not None and g.u_count.is_cuda
            assert g.slot_hint is not None and g.src_hint is not None
            assert g.has_sqrt is not None
        else:
            assert g.u_count is None and g.slot_hint is None


@pytest.mark.parametrize("contract", ["base", "dict"])
@pytest.mark.parametrize("optname", ["adagrad", "adam"])
def test_engine_bag_path_matches_generic_bitwise(monkeypatch, optname, contract):
    on = _engine(monkeypatch, True, optname)
    off = _engine(monkeypatch, False, optname)
    for step in range(P.STEPS):
        batch = BC.bag_batch(step, NAMES)
        grads = P.slot_grads(100 + step, _dev())
        if contract == "dict":
            grads["a"] = grads["a"].clone()
            grads["a"][3, 1] = float("nan")
            grads["c"] = None
        tbs = []
        for eng, taken in ((on, True), (off, False)):
            tb = eng.process_batch(batch)
            _assert_path(tb, taken)
            tbs.append(tb)
        for g_on, g_off in zip(*(tb._groups for tb in tbs)):
            assert torch.equal(_bits(g_on.sum_base), _bits(g_off.sum_base)), \
                f"step {step} dim {g_on.dim}: sum_base"
            assert torch.equal(g_on.cat_offsets, g_off.cat_offsets)
            assert torch.equal(g_on.seg_id, g_off.seg_id)
            assert torch.equal(g_on.seg_lens, g_off.seg_lens)
            for s_on, s_off in zip(g_on.slots, g_off.slots):
                assert s_on.pos_slice == s_off.pos_slice
                assert s_on.sum_seg_base == s_off.sum_seg_base
                assert torch.equal(s_on.seg_offsets, s_off.seg_offsets)
        for p_on, p_off in zip(*(tb.payloads for tb in tbs)):
            assert p_on.name == p_off.name
            assert torch.equal(p_on.sum_tensor, p_off.sum_tensor)
        for eng, tb in zip((on, off), tbs):
            if contract == "base":
                P.set_base_grads(tb, grads)
                eng.apply_gradients_base(tb, loss_scale=4.0)
            else:
                eng.apply_gradients(tb, grads, loss_scale=4.0)
        if contract == "base":
            # nobody materialised the group: the count is still on the device
            _assert_path(tbs[0], True)
    untouched = _engine(monkeypatch, True, optname)
    for step in range(P.STEPS):
        untouched.process_batch(BC.bag_batch(step, NAMES))
    assert P.tables_differ(P.table(untouched), P.table(on))
    P.assert_tables_equal(P.table(on), P.table(off))


def _sqrt_schema():
    from persia_amd.core.schema import EmbeddingSchema, SlotConfig

    return EmbeddingSchema(slots={
        "a": SlotConfig(name="a", dim=16),
        "b": SlotConfig(name="b", dim=16, sqrt_scaling=True),
        "e": SlotConfig(name="e", dim=8),
    })


@pytest.mark.parametrize("optname", ["adagrad", "adam"])
def test_engine_sqrt_slot_matches_cpu_engine(monkeypatch, optname):
    """A sqrt-scaling slot in the bag group, against the CPU engine at the
    tolerance of test_mixed_group_table_matches_cpu_engine."""
    cpu_eng = _engine(monkeypatch, True, optname, P.CPU, _sqrt_schema())
    gpu_eng = _engine(monkeypatch, True, optname, schema=_sqrt_schema())
    for step in range(P.STEPS):
        batch = BC.bag_batch(step, ("a", "b", "e"))
        tb_c = cpu_eng.process_batch(batch)
        tb_g = gpu_eng.process_batch(batch)
        _assert_path(tb_g, True)
        assert [g.has_sqrt for g in tb_g._groups] == [True, False]
        assert tb_g._groups[1].fwd_scale.numel() == 0
        gen = torch.Generator().manual_seed(200 + step)
        for gc, gg in zip(tb_c._groups, tb_g._groups):
            assert gc.dim == gg.dim and gc.sum_base.shape == gg.sum_base.shape
            assert torch.allclose(gc.sum_base.float(), gg.sum_base.float().cpu(),
                                  atol=2e-3, rtol=2e-3)  # one f16 ulp
            g = torch.randn(gc.sum_base.shape, generator=gen).half()
            gc.sum_base.requires_grad_(True)
            gg.sum_base.requires_grad_(True)
            gc.sum_base.grad = g
            gg.sum_base.grad = g.to(_dev())
        cpu_eng.apply_gradients_base(tb_c, loss_scale=4.0)
        gpu_eng.apply_gradients_base(tb_g, loss_scale=4.0)
        _assert_path(tb_g, True)
    t_c, t_g = P.table(cpu_eng), P.table(gpu_eng)
    assert t_c.keys() == t_g.keys() == {8, 16}
    for dim in t_c:
        assert np.array_equal(t_c[dim][0], t_g[dim][0]), f"dim {dim}: signs"
        diff = np.abs(t_c[dim][1] - t_g[dim][1]).max()
        print(f"{optname} dim {dim}: rows {t_c[dim][1].shape}, max diff {diff:.3e}")
        assert np.allclose(t_c[dim][1], t_g[dim][1], atol=1e-5, rtol=1e-5), (
            f"dim {dim}: max diff {diff}"
        )


def test_other_groups_keep_their_paths(monkeypatch):
    """A group with a raw or hashstack slot stays generic; an all-single-ID
    group keeps its own fast path; single-ID slots beside a bag slot are bags
    of length 1."""
    eng = _engine(monkeypatch, True, "adagrad", schema=P.mixed_schema())
    tb = eng.process_batch(P.mixed_batch(0))
    by_dim = {g.dim: g for g in tb._groups}
    assert by_dim[16].u_count is None and by_dim[16].has_sqrt is None
    assert by_dim[8].u_count is not None and by_dim[8].has_sqrt is False
    eng = _engine(monkeypatch, True, "adagrad")
    tb = eng.process_batch(P.single_batch(0))
    assert all(g.u_count is not None and g.has_sqrt is None for g in tb._groups)
    # a and c as bags, b and d single: both groups take the bag path and
    # match the generic one
    off = _engine(monkeypatch, False, "adagrad")
    bags, single = BC.bag_batch(5, NAMES), P.single_batch(5)
    feats = {f.name: f for f in bags.id_type_features}
    for f in single.id_type_features:
        if f.name in ("b", "d"):
            feats[f.name] = f
    bags.id_type_features = [feats[n] for n in NAMES]
    tb_on, tb_off = eng.process_batch(bags), off.process_batch(bags)
    _assert_path(tb_on, True)
    _assert_path(tb_off, False)
    for g_on, g_off in zip(tb_on._groups, tb_off._groups):
        assert torch.equal(_bits(g_on.sum_base), _bits(g_off.sum_base))


def test_prepare_host_batch_builds_the_bag_buffer(monkeypatch):
    eng = _engine(monkeypatch, True, "adagrad")
    batch = BC.bag_batch(0, NAMES)
    eng.prepare_host_batch(batch)
    pins = {k: v for k, v in batch._pinned_cache.items() if k[0] == "bag"}
    assert set(pins) == {("bag", 8), ("bag", 16)}
    assert all(t.is_pinned() for t, _nnz, _B in pins.values())
    eng.process_batch(batch)
    assert all(batch._pinned_cache[k][0] is v[0] for k, v in pins.items())


def test_zz_report_worst_ratios():
    """Not a check of its own: prints what this session measured."""
    for family in sorted(_worst):
        print(f"worst err/bound  {family:48s} {_worst[family]:.4f}")
