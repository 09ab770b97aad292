"""The sparse forward kernels against exact models of what they compute.

Scenarios, references and bounds come from tests/test_sparse_cases_cpu.py
(which checks them without a GPU); the bound vocabulary is that of
tests/test_gpu_dense_exact.py.

A. Table semantics, bit for bit.  Claims of one launch race; the outcome is
   determined when no two keys of a batch share a probe window.  In that
   regime (verified on the oracle by permutation invariance) the HIP table
   must hold the sequential CpuEmbeddingStore's keys, ticks and arena after
   every batch: min-tick victim, first-in-scan tie break, current-tick guard,
   the window that wraps at the last bucket, the slot a claim lands in, the
   eviction log (victim key + full row, saved before the overwrite),
   admit_probability < 1, store_probe + store_import, eval lookups and the
   device-side count.
B. Overflow (40 keys of one home bucket in one launch): which key gets which
   slot is not determined, so only the structure every interleaving
   guarantees is asserted.
C. Row init, gather and scatter are bitwise: the reference is row_init +
   state_init.
D. segment_sum, grad_scatter and grad_scatter_idx against f64 from the same
   operand bits.  L is the number of addends, S the same sum over absolute
   values:

     segment_sum        E = (L + 1) 2^-23 scale S   (L adds and the scale
                        multiply, a full f32 ulp each), then the f16 store
                        E + 2^-11 (|ref| + E) + 2^-25
     grad_scatter       E = 2 L 2^-23 S, S = sum |g scale|   (one ulp for
                        each product, one for each add; covers a fused
                        multiply-add).  Accumulate mode: the pre-filled value
                        is one more addend.
     grad_scatter_idx   the same E: as it is for f32 out, through the f16
                        store bound for f16 out

   A plain f32 loop measured against f64 stays at err/bound 0.999
   (segment_sum, f16-out scatter: the store term is tight by construction)
   and 0.25 (f32-out scatter); a dropped addend or an ignored scale gives
   ratios of 1e4 and more.  The kernels on an MI355X: see MEASURED below.
   No constant had to be raised.
E. dedup_padded against np.unique on the uint64 view, exactly, including the
   stable permutation the ordered reduction's determinism rests on.

MEASURED (worst err/bound per kernel over all cases of section D):
  segment_sum       0.995 (f32 rows), 0.999 (f16 rows)
  grad_scatter      0.25 (write mode, every gradient type), 0.23 (accumulate)
  grad_scatter_idx  0.25 (f32 out), 0.997 (f16 out)
"""
import numpy as np
import pytest
import torch

import test_sparse_cases_cpu as S
from test_gpu_dense_exact import _bits, _dev, _native, _ratio, f16_store_bound

pytestmark = pytest.mark.gpu


def _hip_table(variant):
    from persia_amd.core.store import HipEmbeddingStore

    opt, hyper, spill = S.table_store_args(variant)
    return HipEmbeddingStore(S.TABLE_DIM, S.CAPACITY, opt, hyper, _dev(),
                             spill_capacity=spill)


def _dkeys(keys_u64):
    return S.as_keys(keys_u64).to(_dev())


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _assert_same_table(hip, cpu, what):
    assert np.array_equal(_u64(hip.keys), cpu.keys), f"{what}: keys"
    assert np.array_equal(hip.ticks.cpu().numpy().view(np.uint32), cpu.ticks), \
        f"{what}: ticks"
    assert torch.equal(_bits(hip.arena.cpu()), _bits(cpu.arena)), f"{what}: arena"


def _hip_spill_dict(hip):
    keys, rows = hip.spill.export()
    return {int(k): rows[i] for i, k in enumerate(keys)}


def _assert_same_tier(hip, cpu, what):
    dh, dc = _hip_spill_dict(hip), S.spill_dict(cpu)
    assert dh.keys() == dc.keys(), f"{what}: tier keys"
    for k, row in dc.items():
        assert np.array_equal(dh[k].view(np.int32), row.view(np.int32)), \
            f"{what}: tier row of key {k}"
    return len(dc)


# ------------------------------------------ A. table semantics, bit for bit


@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("seed", S.SEEDS)
def test_table_matches_sequential_oracle(seed, variant):
    run = S.OracleRun(variant)
    cpu, hip = run.store, _hip_table(variant)
    refused = 0
    for b_no, keys in enumerate(S.scenario_for(seed, variant)):
        what = f"batch {b_no}"
        resident_before = S.oracle_slots(cpu, keys) >= 0
        want, slots, restored = run.step(b_no, keys)
        got = hip.lookup(_dkeys(keys), train=True).cpu()
        assert torch.equal(_bits(got), _bits(want)), f"{what}: rows"
        _assert_same_table(hip, cpu, what)
        refused += int(((slots < 0) & ~resident_before).sum())
        if variant == "spill":
            for i, emb in restored.items():
                assert torch.equal(got[i], emb), f"{what}: restored row {i}"
            rows = run.stamp(b_no, keys, slots)
            hip.arena[torch.from_numpy(slots).to(_dev())] = rows.to(_dev())
            hip.flush_spill()
            _assert_same_tier(hip, cpu, what)
    assert cpu.evictions >= 500 and len(hip) == len(cpu) == S.CAPACITY
    if variant == "admit":
        assert refused > 100  # otherwise this variant tests nothing
    else:
        assert run.stats["misses"] == 0
    if variant == "spill":
        assert len(cpu.spill) > 0 and run.stats["restored"] > 0
        assert hip.evicted_total == cpu.evictions


@pytest.mark.parametrize("seed", S.SEEDS)
def test_probe_and_import_match_sequential_oracle(seed):
    """The spill-restore front half on its own: store_probe reports exactly
    the oracle's missing keys (and refreshes the ticks of the others, as an
    eval lookup does); store_import lands rows for the missing keys in the
    oracle's slots and logs the oracle's victims with their full rows."""
    from persia_amd.core import hashing

    cpu, hip = S.make_oracle("spill"), _hip_table("spill")
    C = _native()
    n_missing = 0
    for b_no, keys in enumerate(S.table_scenario(seed)):
        what = f"batch {b_no}"
        want_slots = S.oracle_slots(cpu, keys)
        cpu.lookup(S.as_keys(keys), train=False)
        slots = C.store_probe(hip.keys, hip.ticks, _dkeys(keys),
                              hip.next_tick(), hip.no_count).cpu().numpy()
        assert np.array_equal(slots, want_slots), f"{what}: probe"
        _assert_same_table(hip, cpu, f"{what} probed")
        miss = keys[want_slots < 0]
        n_missing += len(miss)
        if not len(miss):
            continue
        signs = hashing.splitmix64_inv(miss)
        inner = torch.stack(
            [S.stamp_row(b_no, k, cpu.row_width) for k in miss]).numpy()
        cpu.import_rows(signs, inner)
        hip.import_rows(signs, inner)
        hip.flush_spill()
        _assert_same_table(hip, cpu, f"{what} imported")
        _assert_same_tier(hip, cpu, what)
    assert n_missing > S.CAPACITY and cpu.evictions >= 500
    assert len(cpu.spill) > 0


def _seeded_pair(n_batches=20):
    cpu, hip = S.make_oracle("plain"), _hip_table("plain")
    batches = S.table_scenario(7, n_batches)
    for keys in batches:
        cpu.lookup(S.as_keys(keys), train=True)
        hip.lookup(_dkeys(keys), train=True)
    _assert_same_table(hip, cpu, "seeded")
    return cpu, hip, batches


def test_eval_lookup_claims_nothing_and_refreshes_hits():
    cpu, hip, batches = _seeded_pair()
    hits = batches[3]
    homes = (hits & np.uint64(S.N_BUCKETS - 1)).astype(np.int64)
    never = np.array([S.window_key(10 ** 6 + i, int(h))
                      for i, h in enumerate(homes)], dtype=np.uint64)
    keys = np.stack([hits, never], axis=1).reshape(-1)
    ticks_before = cpu.ticks.copy()
    want = cpu.lookup(S.as_keys(keys), train=False)
    got = hip.lookup(_dkeys(keys), train=False).cpu()
    assert torch.equal(_bits(got), _bits(want))
    assert (got[1::2] == 0).all() and (got[0::2] != 0).any(dim=1).all()
    _assert_same_table(hip, cpu, "eval")
    assert (cpu.ticks != ticks_before).sum() == len(hits)


@pytest.mark.parametrize("tail", ["sentinel", "real_keys"])
def test_lookup_with_device_count_ignores_the_tail(tail):
    """Keys beyond u_count are never probed or claimed (a real key there
    would land in the table), and their output rows are never written."""
    cpu, hip, _ = _seeded_pair()
    fresh = S.table_scenario(11, 1)[0] + np.uint64(1 << 40)
    n = len(fresh) - 5
    assert n >= 4
    keys = fresh.copy()
    if tail == "sentinel":
        keys[n:] = 0
    want = cpu.lookup(S.as_keys(fresh[:n]), train=True)
    out = torch.full((len(keys), S.TABLE_DIM), 7.0, device=_dev())
    _native().store_lookup(
        hip.keys, hip.ticks, hip.arena, _dkeys(keys), out,
        *hip._lookup_args(True, hip.next_tick()), *hip._no_evict,
        torch.tensor([n], dtype=torch.int64, device=_dev()),
    )
    assert torch.equal(_bits(out[:n].cpu()), _bits(want))
    assert (out[n:] == 7.0).all()
    _assert_same_table(hip, cpu, tail)


# -------------------------------------------- B. overflow: structure only


def test_overflow_structure():
    """40 keys of one home bucket against a 32-slot window, twice.  A peer
    may evict a row claimed at this very tick (probe.h, kOrdered = false), so
    neither the slot of a key nor the row contents are asserted -- only what
    every interleaving guarantees.  All 40 keys sit in one wave, whose lanes
    pick the same first-empty slot in every retry round, so each round admits
    one key: the window fills only if a key may lose once per slot (a limit
    of 16 retries left 16 slots empty and 24 keys missing)."""
    hip = _hip_table("plain")
    home = S.N_BUCKETS - 2  # the window wraps: buckets 62, 63, 0, 1
    window = np.concatenate([
        np.arange(S.BUCKET_SIZE) + ((home + p) % S.N_BUCKETS) * S.BUCKET_SIZE
        for p in range(S.PROBE_BUCKETS)])
    outside = np.setdiff1d(np.arange(S.CAPACITY), window)
    queried = set()
    for batch in range(2):
        keys = np.array([S.window_key(1 + 40 * batch + i, home)
                         for i in range(40)], dtype=np.uint64)
        queried |= set(keys.tolist())
        tick = hip.tick
        rows = hip.lookup(_dkeys(keys), train=True).cpu()
        tkeys = _u64(hip.keys)
        ticks = hip.ticks.cpu().numpy()
        n_occ = int((tkeys[window] != 0).sum())
        n_zero = int((rows == 0).all(dim=1).sum())
        print(f"batch {batch}: {n_occ} of 32 window slots occupied, "
              f"{n_zero} of 40 rows zero")
        assert n_occ == len(window), f"batch {batch}: {n_occ} slots occupied"
        occ = tkeys[tkeys != 0]
        assert len(set(occ.tolist())) == len(occ)
        assert set(occ.tolist()) <= queried
        if batch == 0:
            assert (ticks[window] == tick).all()
        assert n_zero >= 8
        assert (tkeys[outside] == 0).all() and (ticks[outside] == 0).all()
        assert (hip.arena.cpu()[torch.from_numpy(outside)] == 0).all()


# --------------------------------------- C. init, gather and scatter, bitwise


def _init_store(dim, optname, bounds):
    from persia_amd.core.store import HipEmbeddingStore
    from persia_amd.embedding import EmbeddingConfig

    return HipEmbeddingStore(
        dim, 4096, S.mk_init_opt(optname),
        EmbeddingConfig(emb_initialization=bounds), _dev())


def _expected(keys_u64, store, bounds):
    """[n, row_width] rows a fresh claim of each key writes; zero key -> 0."""
    out = np.zeros((len(keys_u64), store.row_width), dtype=np.float32)
    for i, k in enumerate(keys_u64):
        if k != 0:
            out[i] = S.expected_row(k, store.dim, bounds, store.optimizer)
    return torch.from_numpy(out)


def _assert_arena_rows(store, keys_u64, bounds, what):
    """Every key is resident and its whole row -- weights and optimizer state
    columns -- is the seeded init."""
    slots = _native().store_probe(store.keys, store.ticks, _dkeys(keys_u64),
                                  int(store.tick), store.no_count)
    assert (slots >= 0).all(), f"{what}: a key is not resident"
    assert torch.equal(_bits(store.arena[slots].cpu()),
                       _bits(_expected(keys_u64, store, bounds))), what


def _lookup_sums(store, pos_keys_u64, train):
    """The fast path as lookup_local drives it: padded dedup with a device
    count, then store_lookup_sums into a NaN-filled sum buffer.
    -> (sums, uniq[:U] u64, inverse, U, hints)."""
    C = _native()
    keys_t = _dkeys(pos_keys_u64)
    uniq, inverse, perm, ustarts, u_count = C.dedup_padded(keys_t)
    nnz = keys_t.numel()
    sums = torch.full((nnz, store.dim), float("nan"), dtype=torch.float16,
                      device=_dev())
    seg_id = (torch.arange(nnz, device=_dev()) if train
              else torch.empty(0, dtype=torch.int64, device=_dev()))
    hints = C.store_lookup_sums(
        store.keys, store.ticks, store.arena, uniq, perm, ustarts, sums,
        *store._lookup_args(train, store.next_tick()), u_count, seg_id)
    U = int(u_count.item())
    return sums.cpu(), _u64(uniq)[:U], inverse.cpu(), U, hints


@pytest.mark.parametrize("bounds", S.INIT_BOUNDS, ids=["dyadic", "0.01"])
@pytest.mark.parametrize("dim", S.INIT_DIMS)
def test_init_gather_scatter_bitwise(dim, bounds):
    for optname in S.init_opts_for(dim):
        store = _init_store(dim, optname, bounds)
        rng = np.random.default_rng(dim)
        known = np.zeros(0, dtype=np.uint64)
        next_sign = 1

        def batch(U):
            """U unique keys: up to half resident, the rest fresh."""
            nonlocal next_sign
            n_res = min(len(known), U // 2)
            fresh = S.mixed_keys(next_sign, U - n_res)
            next_sign += U - n_res
            keys = np.concatenate([rng.choice(known, n_res, replace=False), fresh])
            return keys[rng.permutation(U)]

        for U in S.INIT_COUNTS:
            what = f"dim {dim} {optname} U {U}"
            # store_lookup_sums: init_scatter (packed dims) / init_scatter2
            uniq = batch(U)
            pos = S.positions_for(uniq, rng)
            sums, got_uniq, inverse, got_U, _ = _lookup_sums(store, pos, True)
            assert got_U == U and np.array_equal(got_uniq, np.sort(uniq))
            rows = _expected(got_uniq, store, bounds)[:, :dim]
            assert torch.equal(_bits(sums), _bits(rows[inverse].half())), \
                f"{what}: sums"
            known = np.union1d(known, uniq)
            _assert_arena_rows(store, uniq, bounds, f"{what}: sums arena")
            # store.lookup, f32 rows: init_gather<float>
            uniq = batch(U)
            got = store.lookup(_dkeys(uniq), train=True).cpu()
            want = _expected(uniq, store, bounds)[:, :dim]
            assert torch.equal(_bits(got), _bits(want)), f"{what}: f32 rows"
            known = np.union1d(known, uniq)
            _assert_arena_rows(store, uniq, bounds, f"{what}: lookup arena")
            # lookup_wire, f16 rows, sentinel entries in between
            uniq = batch(U)
            wire_keys = np.concatenate([uniq, np.zeros(3, dtype=np.uint64)])
            wire_keys = wire_keys[rng.permutation(len(wire_keys))]
            wire = store.lookup_wire(_dkeys(wire_keys), True, torch.float16).cpu()
            want = _expected(wire_keys, store, bounds)[:, :dim]
            assert torch.equal(_bits(wire), _bits(want.half())), f"{what}: wire"
            known = np.union1d(known, uniq)
            _assert_arena_rows(store, uniq, bounds, f"{what}: wire arena")
            real = wire_keys != 0
            f32 = store.lookup(_dkeys(wire_keys[real]), train=False).cpu()
            assert torch.equal(_bits(wire[torch.from_numpy(real)]),
                               _bits(f32.half())), f"{what}: wire vs f32"
        assert len(store) == len(known)  # nothing was evicted on the way

        # eval: missing keys read zero on every path and claim nothing
        keys_before = store.keys.clone()
        for U in (65, 2):
            res = rng.choice(known, U // 2 + 1, replace=False)
            missing = S.mixed_keys(10 ** 9 + U, U // 2)
            uniq = np.concatenate([res, missing])[rng.permutation(len(res) + U // 2)]
            is_missing = torch.from_numpy(np.isin(uniq, missing))
            want = _expected(uniq, store, bounds)[:, :dim]
            want[is_missing] = 0
            got = store.lookup(_dkeys(uniq), train=False).cpu()
            assert torch.equal(_bits(got), _bits(want))
            pos = S.positions_for(uniq, rng)
            sums, got_uniq, inverse, _, hints = _lookup_sums(store, pos, False)
            want = _expected(got_uniq, store, bounds)[:, :dim]
            want[torch.from_numpy(np.isin(got_uniq, missing))] = 0
            assert torch.equal(_bits(sums), _bits(want[inverse].half()))
            assert hints[0].numel() == 0 and hints[1].numel() == 0
        assert torch.equal(store.keys, keys_before)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("dim", [8, 24, 64, 200])
def test_lookup_local_is_the_composition_of_its_steps(dim, train):
    """lookup_local == sign_prep -> dedup_padded -> lookup -> gather, bit for
    bit; its slot hints are what store_probe gives afterwards, its source
    hints what ustarts / perm / seg_id give."""
    C = _native()
    dev = _dev()
    bounds = (-0.01, 0.01)
    fused = _init_store(dim, "adagrad", bounds)
    steps = _init_store(dim, "adagrad", bounds)
    rng = np.random.default_rng(dim)
    B = 43
    spacing = (1 << 56) - 1
    prefixes = torch.from_numpy(
        np.array([1 << 56, 2 << 56, 0], dtype=np.uint64).view(np.int64)).to(dev)
    starts = torch.arange(0, 4 * B, B, dtype=torch.int64, device=dev)
    nnz = 3 * B
    seg_id = torch.arange(nnz, dtype=torch.int64)
    seg_id[::7] = -1  # raw-slot positions carry no gradient row
    no_scale = torch.empty(0, device=dev)
    offs = torch.arange(nnz + 1, device=dev)
    for step in range(2):  # fresh rows, then mostly resident ones
        values = torch.from_numpy(
            rng.integers(0, 60 + 30 * step, size=nnz)).to(dev)
        (sums, uniq, inverse, perm, ustarts, u_count, slot_hint,
         src_hint) = fused.lookup_local(
            values, starts, prefixes, spacing, offs, no_scale,
            seg_id.to(dev) if train else torch.empty(0, dtype=torch.int64,
                                                      device=dev), train)
        keys = C.sign_prep(values, starts, prefixes, spacing)
        d = C.dedup_padded(keys)
        U = int(u_count.item())
        for a, b in zip((uniq, inverse, perm, ustarts[: U + 1], u_count),
                        (d[0], d[1], d[2], d[3][: U + 1], d[4])):
            assert torch.equal(a, b)
        assert 1 < U < nnz
        rows = steps.lookup(d[0][:U], train=train)
        assert torch.equal(_bits(sums), _bits(rows[inverse].half()))
        # the same rows by key (slots of a racing launch are not compared)
        for st in (fused, steps):
            probe = C.store_probe(st.keys, st.ticks, uniq[:U], int(st.tick),
                                  st.no_count)
            if train:
                assert (probe >= 0).all()
                assert torch.equal(
                    _bits(st.arena[probe].cpu()),
                    _bits(_expected(_u64(uniq)[:U], st, bounds)))
            elif step == 0:
                assert (probe < 0).all() and len(st) == 0
        if not train:
            assert slot_hint.numel() == 0 and src_hint.numel() == 0
            assert (sums == 0).all()
            continue
        probe = C.store_probe(fused.keys, fused.ticks, uniq[:U],
                              int(fused.tick), fused.no_count)
        assert torch.equal(slot_hint[:U], probe)
        us, pm = ustarts.cpu(), perm.cpu()
        want_src = torch.tensor([
            int(seg_id[pm[us[u]]]) if us[u + 1] - us[u] == 1 else -1
            for u in range(U)])
        assert torch.equal(src_hint[:U].cpu(), want_src)
        assert (want_src >= 0).any() and (want_src < 0).any()


# ------------------------- D. segment_sum / grad_scatter / grad_scatter_idx

_worst = {}


def _note(kernel, ratio):
    _worst[kernel] = max(_worst.get(kernel, 0.0), ratio)
    print(f"{kernel}: worst err/bound so far {_worst[kernel]:.4g}")


@pytest.mark.parametrize("n_seg", S.RED_COUNTS)
@pytest.mark.parametrize("dim", S.RED_DIMS)
def test_segment_sum_exact(dim, n_seg):
    C = _native()
    for with_scale in (False, True):
        case = S.segment_case(dim, n_seg, with_scale)
        dev = {k: case[k].to(_dev()) for k in ("inverse", "offsets", "scale")}
        for rows in (case["rows"], case["rows"].half()):
            ref, bound = S.segment_reference(rows, case)
            out = C.segment_sum(rows.to(_dev()), dev["inverse"],
                                dev["offsets"], dev["scale"]).cpu()
            assert out.dtype == torch.float16
            what = f"segment_sum dim {dim} n_seg {n_seg} " \
                   f"scale {int(with_scale)} {rows.dtype}"
            _note("segment_sum", _ratio(out, ref, bound, what))
            empty = case["lens"] == 0
            assert (out[empty] == 0).all()


@pytest.mark.parametrize("U", S.RED_COUNTS)
@pytest.mark.parametrize("dim", S.RED_DIMS)
def test_grad_scatter_exact(dim, U):
    C = _native()
    for with_scale in (False, True):
        case = S.scatter_case(dim, U, with_scale)
        dev = {k: case[k].to(_dev())
               for k in ("perm", "ustarts", "seg_id", "scale")}
        gen = torch.Generator().manual_seed(dim * 1000 + U)
        prefill = torch.randn(U, dim, generator=gen) * 0.5
        for gdt in (torch.float16, torch.bfloat16, torch.float32):
            grads = case["grads"].to(gdt)
            g_dev = grads.to(_dev())

            def run(out, accumulate):
                C.grad_scatter(g_dev, dev["perm"], dev["ustarts"],
                               dev["seg_id"], dev["scale"], out, accumulate)
                return out.cpu()

            what = f"grad_scatter dim {dim} U {U} scale {int(with_scale)} {gdt}"
            ref, E, L = S.scatter_reference(grads, case)
            acc0 = run(torch.zeros(U, dim, device=_dev()), 1)
            wrote = run(torch.full((U, dim), float("nan"), device=_dev()), 0)
            # nothing of the NaN rows behind scale == 0 leaks, and write mode
            # is accumulate-into-zeros bit for bit
            assert torch.equal(_bits(acc0), _bits(wrote)), what
            _note("grad_scatter", _ratio(wrote, ref, E, what))
            assert (wrote[L == 0] == 0).all()
            ref, E, _ = S.scatter_reference(grads, case, prefill=prefill)
            acc = run(prefill.to(_dev()), 1)
            _note("grad_scatter", _ratio(acc, ref, E, what + " accumulate"))


@pytest.mark.parametrize("U", S.RED_COUNTS)
@pytest.mark.parametrize("dim", S.RED_DIMS)
def test_grad_scatter_idx_exact(dim, U):
    """The wire variant: out[out_idx[u]] for u below the device-side count.
    Entries beyond the count point at real rows and have empty runs, so
    reading them would zero a checked row; several valid entries point at the
    dummy tail row (not checked: they race for it by design)."""
    C = _native()
    PAD, SPARE, FILL = 7, 5, 7.0
    rng = np.random.default_rng(dim * 1000 + U)
    n_rows = U + SPARE + 1
    dummy = n_rows - 1
    for with_scale in (False, True):
        for counted in (True, False):
            pad = PAD if counted else 0
            case = S.scatter_case(dim, U, with_scale, pad=pad)
            grads = case["grads"].half()
            ref, E, _ = S.scatter_reference(grads, case)
            target = rng.permutation(U + SPARE)[:U]
            to_dummy = np.arange(U) % 9 == 4
            out_idx = np.where(to_dummy, dummy, target)
            kept = ~to_dummy
            tail = np.resize(target[kept], pad)  # real, checked rows
            full_idx = np.concatenate([out_idx, tail])
            count = (torch.tensor([U], dtype=torch.int64, device=_dev())
                     if counted else torch.empty(0, dtype=torch.int64,
                                                 device=_dev()))
            rows_hit = torch.from_numpy(out_idx[kept])
            untouched = np.setdiff1d(np.arange(n_rows - 1), out_idx[kept])
            for odt in (torch.float32, torch.float16):
                out = torch.full((n_rows, dim), FILL, dtype=odt, device=_dev())
                C.grad_scatter_idx(
                    grads.to(_dev()), case["perm"].to(_dev()),
                    case["ustarts"].to(_dev()), case["seg_id"].to(_dev()),
                    case["scale"].to(_dev()),
                    torch.from_numpy(full_idx).to(_dev()), out, count)
                out = out.cpu()
                what = f"grad_scatter_idx dim {dim} U {U} scale " \
                       f"{int(with_scale)} count {int(counted)} {odt}"
                r, e = ref[torch.from_numpy(kept)], E[torch.from_numpy(kept)]
                bound = e if odt == torch.float32 else f16_store_bound(e, r)
                if kept.any():
                    _note("grad_scatter_idx",
                          _ratio(out[rows_hit], r, bound, what))
                assert (out[torch.from_numpy(untouched)] == FILL).all(), what


# ------------------------------------------------------------ E. dedup_padded


@pytest.mark.parametrize("kind", S.DEDUP_KINDS)
@pytest.mark.parametrize("nnz", S.DEDUP_NNZ)
def test_dedup_padded_matches_numpy(nnz, kind):
    from persia_amd.core.engine import _dedup

    C = _native()
    keys = S.dedup_input(nnz, kind)
    want_uniq, want_inv, want_starts, want_perm = S.dedup_reference(keys)
    keys_t = _dkeys(keys)
    uniq, inverse, perm, ustarts, u_count = C.dedup_padded(keys_t)
    assert uniq.shape == inverse.shape == perm.shape == (nnz,)
    assert ustarts.shape == (nnz + 1,) and u_count.shape == (1,)
    U = int(u_count.item())
    assert U == len(want_uniq)
    assert np.array_equal(_u64(uniq)[:U], want_uniq)  # unsigned order
    assert (uniq[U:] == 0).all()
    assert np.array_equal(inverse.cpu().numpy(), want_inv)
    assert np.array_equal(ustarts.cpu().numpy()[: U + 1], want_starts)
    # the radix sort is stable: positions of equal keys stay ascending
    assert np.array_equal(perm.cpu().numpy(), want_perm)
    for other in (C.dedup_keys(keys_t), _dedup(keys_t)):
        o_uniq, o_inv, o_perm, o_starts = other
        assert torch.equal(o_uniq, uniq[:U])
        assert torch.equal(o_inv, inverse)
        assert torch.equal(o_starts, ustarts[: U + 1])
        assert np.array_equal(keys[o_perm.cpu().numpy()], np.sort(keys))


def test_dedup_padded_of_nothing():
    """An empty key tensor has no unique keys: u_count == 0, ustarts == [0].
    The outputs used to be uninitialised memory (the finalize kernel does not
    launch for n == 0), so dirty the allocator's cache first."""
    C = _native()
    empty = torch.empty(0, dtype=torch.int64, device=_dev())
    for _ in range(4):
        dirty = [torch.full((n,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64,
                            device=_dev()) for n in (1, 1, 2, 64)]
        del dirty
        uniq, inverse, perm, ustarts, u_count = C.dedup_padded(empty)
        assert uniq.numel() == inverse.numel() == perm.numel() == 0
        assert u_count.tolist() == [0] and ustarts.tolist() == [0]
        held = (uniq, inverse, perm, ustarts, u_count)  # keep the blocks busy
    del held
