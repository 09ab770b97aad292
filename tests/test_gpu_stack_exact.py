"""The native bag lookup of sum slots with hashstack rounds, exactly.

Cases, the numpy index model of the sign-prep kernel and the engine schema
come from tests/test_stack_cases_cpu.py, which checks them without a GPU
(the index model reproduces test_route_cases_cpu.sign_prep_model, the model
of EmbeddingEngine._prepare_slot_keys, on every case).

A. sign_prep_bags on every case: bitwise the index model's keys, and
   sign_prep_stack's on the arrays _group_keys hands it.
B. The stacked lookup_local_bags against a twin built from existing pieces:
   sign_prep_stack -> dedup_padded -> store.lookup(u_count) -> bag_plan on the
   expanded plan -> segment_sum.  All twelve results and the two tables are
   bit-equal over two training batches (the second meets resident rows) and
   an eval batch, with hints on and off, one dim per lane layout of bag_sum.
C. The engine on a pure-sum schema of stacked and unstacked slots (one group
   fed one id per sample, stacked): the bag path is taken, equals
   PA_BAG_FAST=0 bit for bit under both update contracts, keeps the unique
   count on the device; a stacked sqrt slot against the CPU engine.
D. Path choice and the host buffer.
E. Refusals, on the host.
"""
import numpy as np
import pytest
import torch

import test_bag_cases_cpu as BC
import test_engine_paths as P
import test_gpu_bag_exact as GB
import test_route_cases_cpu as RC
import test_stack_cases_cpu as SC
from test_gpu_dense_exact import _bits, _dev, _native

pytestmark = pytest.mark.gpu


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(_dev())


def _upload(slots):
    """-> (device upload, nnz_in, nnz_out, S, B)."""
    buf, nnz_in, nnz_out, B = SC.pack(slots)
    return _t(buf), nnz_in, nnz_out, len(slots), B


def _stack_dev(slots):
    rounds, sizes = SC.rounds_of(slots)
    return _t(rounds, torch.int32), _t(sizes, torch.int64)


def _prefixes(slots):
    return _t(RC._u64([s.prefix for s in slots]).view(np.int64))


def _sign_prep_stack(slots):
    """The generic path's keys: _C.sign_prep_stack on _group_keys' arrays."""
    a = RC.prep_kernel_args(slots)
    return _native().sign_prep_stack(
        _t(a["values"]), _t(a["in_starts"]), _t(a["out_starts"]),
        _t(a["prefixes"]), _t(a["rounds"]), _t(a["sizes"]),
        _t(a["off_starts"]), _t(a["all_offs"]), SC.SPACING, a["n_out"])


# ------------------------------------------------------------ A. the kernel


@pytest.mark.parametrize("tag,slots", SC.all_cases(), ids=SC.CASE_IDS)
def test_sign_prep_bags_matches_the_index_model(tag, slots):
    up, nnz_in, nnz_out, S, B = _upload(slots)
    rounds, sizes = _stack_dev(slots)
    keys = _native().sign_prep_bags(up, nnz_in, nnz_out, S, B,
                                    _prefixes(slots), rounds, sizes,
                                    SC.SPACING)
    assert keys.dtype == torch.int64 and keys.shape == (nnz_out,)
    buf = up.cpu().numpy()
    slot, _sample, rnd, src = SC.index_model(
        buf, nnz_in, nnz_out, S, B, SC.rounds_of(slots)[0])
    want = SC.keys_from_index(buf, nnz_in, slots, slot, rnd, src)
    got = keys.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want)
    assert np.array_equal(got, RC.sign_prep_model(slots))
    if nnz_in:
        assert torch.equal(keys, _sign_prep_stack(slots))


# ---------------------------------------------------- B. against a twin store

SQRT = (False, True, True)
ROUNDS = (2, 0, 3)


def _lookup_case(kind, seed, vocab=BC.VOCAB):
    return [
        RC.PrepSlot(f"s{i}", v, o, r, SC.SIZE if r else 1, SC._prefix(i, 3))
        for i, ((v, o), r) in enumerate(
            zip(BC.bag_slots(3, 32, kind, seed=seed, vocab=vocab), ROUNDS))
    ]


def _twin_lookup(twin, slots, up, nnz_in, nnz_out, S, B, train):
    """The same lookup out of the existing pieces -> the twelve results
    (no hints: tensors of length 0 in their place)."""
    C = _native()
    keys = _sign_prep_stack(slots)
    d = C.dedup_padded(keys)
    rows = twin.lookup(d[0], train, u_count=d[4])
    plan = up[nnz_in : nnz_in + S + 1 + S * (B + 1)]
    cat, seg_id, seg_lens, scale = C.bag_plan(plan, S, B, nnz_out,
                                              GB._flags(SQRT))
    sums = C.segment_sum(rows, d[1], cat, scale)
    none = seg_id[:0]
    return (sums, *d, none, none, cat, seg_id, seg_lens, scale)


NAMES12 = ("sums", "uniq", "inverse", "perm", "ustarts", "u_count",
           "slot_hint", "src_hint", "cat_offsets", "seg_id", "seg_lens",
           "seg_scale")


@pytest.mark.parametrize("hints", [True, False])
@pytest.mark.parametrize("dim", GB.LOOKUP_DIMS)
def test_stacked_lookup_matches_twin(dim, hints):
    store, twin = GB._mk_store(dim), GB._mk_store(dim)
    sqrt_seg = np.repeat(np.asarray(SQRT), 32)

    def step(kind, seed, train, vocab=BC.VOCAB):
        slots = _lookup_case(kind, seed, vocab)
        up, nnz_in, nnz_out, S, B = _upload(slots)
        rounds, sizes = SC.rounds_of(slots)
        res = store.lookup_local_bags(
            up, nnz_in, S, B, _prefixes(slots), SC.SPACING, GB._flags(SQRT),
            hints, train, rounds=rounds, sizes=sizes, nnz_out=nnz_out,
            stack_dev=_stack_dev(slots))
        ref = _twin_lookup(twin, slots, up, nnz_in, nnz_out, S, B, train)
        what = f"dim {dim} {kind} seed {seed} train {train} hints {hints}"
        assert len(res) == len(ref) == 12
        assert res[0].dtype == torch.float16 and res[0].shape == (S * B, dim)
        U = int(res[5].item())
        assert 0 < U < nnz_out  # buckets collide
        for name, got, want in zip(NAMES12, res, ref):
            if name in ("slot_hint", "src_hint"):
                continue
            assert got.shape == want.shape and got.dtype == want.dtype, \
                f"{what}: {name}"
            if name == "ustarts":  # nnz-padded: the tail is unspecified
                got, want = got[: U + 1], want[: U + 1]
            assert torch.equal(_bits(got) if got.is_floating_point() else got,
                               _bits(want) if want.is_floating_point()
                               else want), f"{what}: {name}"
        assert res[1].numel() == res[2].numel() == nnz_out
        cat, m_seg, m_lens, m_scale = BC.plan_model(SC.expanded(slots), SQRT)
        assert np.array_equal(res[8].cpu().numpy(), cat)
        assert np.array_equal(res[9].cpu().numpy(), m_seg)
        assert np.array_equal(res[10].cpu().numpy(), m_lens)
        BC.check_scale(res[11].cpu().numpy(), m_scale, sqrt_seg)
        if train and hints:
            GB._check_hints(store, res, what)
        else:
            assert res[6].numel() == 0 and res[7].numel() == 0
        return res

    step("mixed", 0, True)
    before = len(store)
    step("long", 1, True)  # meets the rows of the first batch
    assert 0 < before < len(store)
    GB._assert_same_tables(store, twin, f"dim {dim} after training lookups")
    keys_before, arena_before = store.keys.clone(), store.arena.clone()
    step("mixed", 3, False, vocab=1 << 20)  # eval, unseen ids among them
    assert torch.equal(store.keys, keys_before)
    assert torch.equal(_bits(store.arena), _bits(arena_before))
    assert store.tick == twin.tick == 4  # one tick per call
    GB._assert_same_tables(store, twin, f"dim {dim} after the eval lookup")


def test_all_bags_empty():
    """nnz == 0 is legal in the stacked form too."""
    store = GB._mk_store(16)
    slots = SC.stack_case(3, 5, "all_empty")
    up, nnz_in, nnz_out, S, B = _upload(slots)
    assert nnz_in == nnz_out == 0
    rounds, sizes = SC.rounds_of(slots)
    res = store.lookup_local_bags(
        up, 0, S, B, _prefixes(slots), SC.SPACING, GB._flags(SQRT), True, True,
        rounds=rounds, sizes=sizes, nnz_out=0)
    assert res[0].shape == (S * B, 16) and not res[0].any()
    assert int(res[5].item()) == 0 and res[1].numel() == 0
    assert res[8].cpu().tolist() == [0] * (S * B + 1)
    assert len(store) == 0


# ------------------------------------------------------------------ C. engine

_engine = GB._engine
_assert_path = GB._assert_path


@pytest.mark.parametrize("contract", ["base", "dict"])
@pytest.mark.parametrize("optname", ["adagrad", "adam"])
@pytest.mark.parametrize("hints", ["1", "0"])
def test_engine_stacked_bag_path_matches_generic_bitwise(monkeypatch, hints,
                                                         optname, contract):
    monkeypatch.setenv("PA_UPDATE_HINTS", hints)
    on = _engine(monkeypatch, True, optname, schema=SC.stack_schema())
    off = _engine(monkeypatch, False, optname, schema=SC.stack_schema())
    assert on._update_hints == (hints == "1")
    for step in range(P.STEPS):
        batch = SC.stack_batch(step)
        grads = P.slot_grads(100 + step, _dev())
        if contract == "dict":
            grads["a"] = grads["a"].clone()
            grads["a"][3, 1] = float("nan")
            grads["c"] = None
        tbs = []
        for eng, taken in ((on, True), (off, False)):
            tb = eng.process_batch(batch)
            # the path was taken: the count is on the device.  (Hints come
            # with it unless PA_UPDATE_HINTS=0.)
            for g in tb._groups:
                if taken:
                    assert g.u_count is not None and g.u_count.is_cuda
                    assert g.has_sqrt is False
                    assert (g.slot_hint is not None) == (hints == "1")
                    assert (g.src_hint is not None) == (hints == "1")
                else:
                    assert g.u_count is None and g.slot_hint is None
            tbs.append(tb)
        for g_on, g_off in zip(*(tb._groups for tb in tbs)):
            what = f"step {step} dim {g_on.dim}"
            assert torch.equal(_bits(g_on.sum_base), _bits(g_off.sum_base)), \
                f"{what}: sum_base"
            assert torch.equal(g_on.cat_offsets, g_off.cat_offsets), what
            assert torch.equal(g_on.seg_id, g_off.seg_id), what
            assert torch.equal(g_on.seg_lens, g_off.seg_lens), what
            assert g_on.inverse.numel() == g_off.inverse.numel()
            for s_on, s_off in zip(g_on.slots, g_off.slots):
                assert s_on.name == s_off.name
                assert s_on.pos_slice == s_off.pos_slice, what
                assert s_on.sum_seg_base == s_off.sum_seg_base, what
                assert torch.equal(s_on.seg_offsets, s_off.seg_offsets), what
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
            assert all(g.u_count is not None and g.u_count.is_cuda
                       for g in tbs[0]._groups)
    untouched = _engine(monkeypatch, True, optname, schema=SC.stack_schema())
    for step in range(P.STEPS):
        untouched.process_batch(SC.stack_batch(step))
    assert P.tables_differ(P.table(untouched), P.table(on))
    P.assert_tables_equal(P.table(on), P.table(off))


def test_engine_stacked_groups_take_the_bag_path(monkeypatch):
    """Both groups, the one fed one id per sample included; positions are the
    expanded ones and collide."""
    eng = _engine(monkeypatch, True, "adagrad", schema=SC.stack_schema())
    batch = SC.stack_batch(0)
    feats = eng._feats_by_dim(batch)
    assert all(getattr(f, "is_single", False) for f in feats[16])
    assert not any(getattr(f, "is_single", False) for f in feats[8])
    assert all(eng._bag_group(d, f) for d, f in feats.items())
    tb = eng.process_batch(batch)
    _assert_path(tb, True)
    by_dim = {g.dim: g for g in tb._groups}
    assert by_dim[16].inverse.numel() == 3 * P.B + P.B  # c: 3 rounds, d: none
    n_a, n_b = (len(f.values) for f in feats[8])
    assert by_dim[8].inverse.numel() == n_a + 2 * n_b
    assert int(by_dim[16].u_count.item()) < 4 * P.B
    plan = eng._plans[("bag", 16, ("c", "d"), P.B)]
    assert plan.rounds == [3, 0] and plan.sizes == [SC.SIZE, 1]
    assert plan.stack_dev[0].is_cuda and plan.stack_dev[0].tolist() == [3, 0]
    again = eng.process_batch(SC.stack_batch(1))
    assert eng._plans[("bag", 16, ("c", "d"), P.B)] is plan  # built once
    _assert_path(again, True)


@pytest.mark.parametrize("optname", ["adagrad", "adam"])
def test_engine_stacked_sqrt_slot_matches_cpu_engine(monkeypatch, optname):
    """b stacked and sqrt-scaling: scaled by rsqrt of the expanded length, as
    the CPU engine's generic path does, at the tolerances of
    test_engine_sqrt_slot_matches_cpu_engine."""
    cpu_eng = _engine(monkeypatch, True, optname, P.CPU, SC.stack_schema(True))
    gpu_eng = _engine(monkeypatch, True, optname,
                      schema=SC.stack_schema(True))
    for step in range(P.STEPS):
        batch = SC.stack_batch(step)
        tb_c = cpu_eng.process_batch(batch)
        tb_g = gpu_eng.process_batch(batch)
        _assert_path(tb_g, True)
        assert [g.has_sqrt for g in tb_g._groups] == [True, False]
        g8 = tb_g._groups[0]
        lens = np.diff(batch.id_type_features[1].offsets)
        want = 1.0 / np.sqrt(np.maximum(2 * lens, 1))
        BC.check_scale(g8.fwd_scale.cpu().numpy(),
                       np.concatenate([np.ones(P.B), want]),
                       np.repeat([False, True], P.B))
        gen = torch.Generator().manual_seed(200 + step)
        for gc, gg in zip(tb_c._groups, tb_g._groups):
            assert gc.dim == gg.dim and gc.sum_base.shape == gg.sum_base.shape
            assert torch.allclose(gc.sum_base.float(),
                                  gg.sum_base.float().cpu(),
                                  atol=2e-3, rtol=2e-3)
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
        print(f"{optname} dim {dim}: rows {t_c[dim][1].shape}, "
              f"max diff {diff:.3e}")
        assert np.allclose(t_c[dim][1], t_g[dim][1], atol=1e-5, rtol=1e-5), (
            f"dim {dim}: max diff {diff}"
        )


# --------------------------------------------- D. path choice, the host buffer


def test_other_groups_keep_their_paths(monkeypatch):
    # a raw slot beside a hashstack slot: generic
    eng = _engine(monkeypatch, True, "adagrad", schema=P.mixed_schema())
    batch = P.mixed_batch(0)
    feats = eng._feats_by_dim(batch)
    assert not eng._bag_group(16, feats[16]) and eng._bag_group(8, feats[8])
    by_dim = {g.dim: g for g in eng.process_batch(batch)._groups}
    assert by_dim[16].u_count is None and by_dim[16].has_sqrt is None
    # spill, PA_FORCE_DIST, PA_BAG_FAST=0 and the CPU device keep the stacked
    # groups generic
    batch = SC.stack_batch(0)
    eng = _engine(monkeypatch, True, "adagrad", schema=SC.stack_schema())
    feats = eng._feats_by_dim(batch)
    assert all(eng._bag_group(d, f) for d, f in feats.items())
    spill = P.mk_engine(_dev(), "adagrad", SC.stack_schema(),
                        spill_capacity=1000)
    monkeypatch.setenv("PA_FORCE_DIST", "1")
    forced = _engine(monkeypatch, True, "adagrad", schema=SC.stack_schema())
    monkeypatch.delenv("PA_FORCE_DIST")
    switched_off = _engine(monkeypatch, False, "adagrad",
                           schema=SC.stack_schema())
    cpu = P.mk_engine(P.CPU, "adagrad", SC.stack_schema())
    assert spill.stores[16].spill is not None and forced._force_dist
    for other in (spill, forced, switched_off, cpu):
        assert not any(other._bag_group(d, f) for d, f in feats.items())
    tb = switched_off.process_batch(batch)
    _assert_path(tb, False)
    # all single-ID and unstacked: the static plan of _process_group_fast
    eng = _engine(monkeypatch, True, "adagrad")
    single = P.single_batch(0)
    assert not any(eng._bag_group(d, f)
                   for d, f in eng._feats_by_dim(single).items())
    tb = eng.process_batch(single)
    assert all(g.u_count is not None and g.has_sqrt is None
               for g in tb._groups)


def test_prepare_host_batch_builds_the_stacked_buffer(monkeypatch):
    eng = _engine(monkeypatch, True, "adagrad", schema=SC.stack_schema())
    batch = SC.stack_batch(0)
    eng.prepare_host_batch(batch)
    pins = {k: v for k, v in batch._pinned_cache.items() if k[0] == "bag"}
    assert set(pins) == {("bag", 8), ("bag", 16)}
    for (t, nnz_in, nnz_out, B) in pins.values():
        assert t.is_pinned() and nnz_out > nnz_in and B == P.B
        assert t.numel() == nnz_in + 2 * (2 + 1) + 2 * (B + 1)
    tb = eng.process_batch(batch)
    _assert_path(tb, True)
    assert all(batch._pinned_cache[k][0] is v[0] for k, v in pins.items())
    assert {k for k in batch._pinned_cache if k[0] == "bag"} == set(pins)


# --------------------------------------------------------------- E. refusals


def _small():
    slots = SC.stack_case(3, 5, "mixed")
    return slots, _upload(slots)


def test_expanded_group_beyond_the_grid_is_refused():
    """The thread-per-position limit holds for the expanded count: 2097153
    ids of 2 rounds are refused on the host, before any launch."""
    store = GB._mk_store(8, capacity=64)
    n = 2097153
    slots = [RC.PrepSlot("s0", np.zeros(n, np.uint64),
                         np.array([0, n], np.int64), 2, SC.SIZE, 0)]
    up, nnz_in, nnz_out, S, B = _upload(slots)
    assert nnz_out == 2 * n == 16384 * 256 + 2
    with pytest.raises(RuntimeError, match="4194304"):
        store.lookup_local_bags(up, nnz_in, S, B, _prefixes(slots), SC.SPACING,
                                GB._flags(()), True, True, rounds=[2],
                                sizes=[SC.SIZE], nnz_out=nnz_out)
    with pytest.raises(RuntimeError, match="4194304"):
        _native().sign_prep_bags(up, nnz_in, nnz_out, S, B, _prefixes(slots),
                                 *_stack_dev(slots), SC.SPACING)
    assert len(store) == 0


@pytest.mark.parametrize("bad", ["rounds_short", "sizes_long", "dev_short",
                                 "negative", "no_buckets", "nnz_out_low",
                                 "nnz_out_high", "upload_short",
                                 "no_nnz_out", "nothing_expands"])
def test_bad_stack_arguments_are_refused(bad):
    store = GB._mk_store(8, capacity=64)
    slots, (up, nnz_in, nnz_out, S, B) = _small()
    rounds, sizes = SC.rounds_of(slots)  # (0, 1, 2)
    kw = dict(rounds=list(rounds), sizes=list(sizes), nnz_out=nnz_out,
              stack_dev=_stack_dev(slots))
    exc = RuntimeError
    if bad == "rounds_short":
        kw["rounds"], exc = kw["rounds"][:2], ValueError
    elif bad == "sizes_long":
        kw["sizes"], exc = kw["sizes"] + [SC.SIZE], ValueError
    elif bad == "dev_short":
        kw["stack_dev"] = (kw["stack_dev"][0][:2], kw["stack_dev"][1])
    elif bad == "negative":
        kw["rounds"][0] = -1
    elif bad == "no_buckets":
        kw["sizes"][2] = 0
    elif bad == "nnz_out_low":
        kw["nnz_out"] = nnz_in - 1
    elif bad == "nnz_out_high":
        kw["nnz_out"] = 2 * nnz_in + 1
    elif bad == "upload_short":
        up = up[:-1].contiguous()
    elif bad == "no_nnz_out":
        kw["nnz_out"], exc = None, ValueError
    elif bad == "nothing_expands":
        kw["rounds"], exc = [0, 1, 1], ValueError
    with pytest.raises(exc):
        store.lookup_local_bags(up, nnz_in, S, B, _prefixes(slots), SC.SPACING,
                                GB._flags(()), True, True, **kw)
    assert len(store) == 0
    # the native entry checks the host copies itself
    if bad in ("rounds_short", "sizes_long", "negative", "no_buckets"):
        with pytest.raises(RuntimeError, match="lookup_local_bags_stack"):
            _native().lookup_local_bags_stack(
                up, nnz_in, nnz_out, S, B, _prefixes(slots), SC.SPACING,
                GB._flags(()), *kw["stack_dev"], kw["rounds"], kw["sizes"], 1,
                store.keys, store.ticks, store.arena,
                *store._lookup_args(True, store.tick))
        assert len(store) == 0
    # the kernel's own binding checks its tensors too
    if bad == "dev_short":
        with pytest.raises(RuntimeError, match="rounds must be i32"):
            _native().sign_prep_bags(up, nnz_in, nnz_out, S, B,
                                     _prefixes(slots), *kw["stack_dev"],
                                     SC.SPACING)
