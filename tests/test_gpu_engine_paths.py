"""GPU half of tests/test_engine_paths.py (same helpers, same shapes): the
mixed-group table state against the CPU engine, skip semantics, the forced
distributed path with producer timing on, and spill restore through both
phase-1 callers."""
import numpy as np
import pytest
import torch

import test_engine_paths as P

pytestmark = pytest.mark.gpu

GPU = torch.device("cuda", 0)


# ------------------------------------------- 2. mixed group, table state


@pytest.mark.parametrize("optname", ["adagrad", "adam"])
def test_mixed_group_table_matches_cpu_engine(optname):
    """Sum, sum+sqrt, raw and hashstack slots with variable lengths, driven
    through apply_gradients_base(raw_grads=, loss_scale=4): after 3 steps the
    GPU store holds the CPU engine's signs, rows within the store-update
    tolerance (test_store_update_matches_cpu_oracle: 1e-5 abs and rel)."""
    cpu_eng = P.mk_engine(P.CPU, optname, P.mixed_schema())
    gpu_eng = P.mk_engine(GPU, optname, P.mixed_schema())
    for step in range(P.STEPS):
        tb_c = cpu_eng.process_batch(P.mixed_batch(step))
        tb_g = gpu_eng.process_batch(P.mixed_batch(step))
        gen = torch.Generator().manual_seed(200 + step)
        raw_c = next(p for p in tb_c.payloads if p.is_raw)
        raw_g = next(p for p in tb_g.payloads if p.is_raw)
        assert raw_c.raw_distinct.shape == raw_g.raw_distinct.shape
        g_raw = torch.randn(raw_c.raw_distinct.shape[0] - 1, 16, generator=gen)
        for gc, gg in zip(tb_c._groups, tb_g._groups):
            assert gc.dim == gg.dim and gc.sum_base.shape == gg.sum_base.shape
            g = torch.randn(gc.sum_base.shape, generator=gen).half()
            gc.sum_base.requires_grad_(True)
            gg.sum_base.requires_grad_(True)
            gc.sum_base.grad = g
            gg.sum_base.grad = g.to(GPU)
        cpu_eng.apply_gradients_base(tb_c, raw_grads={"r": g_raw}, loss_scale=4.0)
        gpu_eng.apply_gradients_base(
            tb_g, raw_grads={"r": g_raw.to(GPU)}, loss_scale=4.0
        )
    t_c, t_g = P.table(cpu_eng), P.table(gpu_eng)
    assert t_c.keys() == t_g.keys() == {8, 16}
    for dim in t_c:
        assert np.array_equal(t_c[dim][0], t_g[dim][0]), f"dim {dim}: signs"
        diff = np.abs(t_c[dim][1] - t_g[dim][1]).max()
        print(f"{optname} dim {dim}: rows {t_c[dim][1].shape}, max diff {diff:.3e}")
        assert np.allclose(t_c[dim][1], t_g[dim][1], atol=1e-5, rtol=1e-5), (
            f"dim {dim}: max diff {diff}"
        )


# ---------------------------------------------------------- 3. skip semantics


# single_batch takes the all-single-ID fast path (padded dedup, fused
# update), list_batch the generic one


@pytest.mark.parametrize("mk_batch", [P.single_batch, P.list_batch])
@pytest.mark.parametrize("contract", ["dict", "base"])
def test_skipped_group_leaves_no_trace_gpu(contract, mk_batch):
    P.check_skipped_group_leaves_no_trace(GPU, contract, mk_batch)


@pytest.mark.parametrize("mk_batch", [P.single_batch, P.list_batch])
def test_nan_slot_is_dropped_alone_gpu(mk_batch):
    P.check_nan_slot_is_dropped_alone(GPU, mk_batch)


# ------------------------------------- 4. forced dist vs local, timing on


_PT_BASE = {"n", "batch", "prep", "native", "skip"}
_PT_DIST = {"dedup", "exch", "route", "lkw", "sum"}


def test_forced_dist_matches_local_with_producer_timing():
    """test_forced_dist_path_bitwise_matches_local's scenario with the
    producer timers running on both engines: results stay bit-equal, and the
    per-stage keys appear exactly on the engine whose stages ran."""
    eng_d = P.mk_engine(GPU, "adagrad")
    eng_l = P.mk_engine(GPU, "adagrad")
    eng_d._force_dist = True
    for eng in (eng_d, eng_l):
        eng._prod_timing = True
        eng._pt["skip"] = 0  # no warm-up skip: every batch is timed
    for step in range(P.STEPS):
        batch = P.single_batch(step)
        tb_d = eng_d.process_batch(batch)
        tb_l = eng_l.process_batch(batch)
        for gd, gl in zip(tb_d._groups, tb_l._groups):
            assert gd.a2a_idx is not None and gl.a2a_idx is None
            assert torch.equal(gd.sum_base, gl.sum_base), f"forward, step {step}"
        # 0.125: per-key gradient sums stay exact on the f16 wire
        for eng, tb in ((eng_d, tb_d), (eng_l, tb_l)):
            eng.apply_gradients_base(
                tb,
                sum_base_grads=[
                    torch.full_like(g.sum_base, 0.125) for g in tb._groups
                ],
            )
    assert eng_d.check_a2a_overflow() == 0
    P.assert_tables_equal(P.table(eng_d), P.table(eng_l))
    assert set(eng_d._pt) == _PT_BASE | _PT_DIST
    assert set(eng_l._pt) == _PT_BASE
    for eng in (eng_d, eng_l):
        assert eng._pt["n"] == P.STEPS and eng._pt["skip"] == 0
        assert eng._pt["batch"] >= eng._pt["native"] > 0.0
    assert all(eng_d._pt[k] > 0.0 for k in _PT_DIST)
    assert eng_d._pt["exch"] >= eng_d._pt["route"] + eng_d._pt["lkw"]


# ------------------------------------------------------- 5. spill restore


def _flood_until_spilled(key, store, lookup):
    """Look up fresh 8-id batches until ``key`` lands in the host tier (never
    probing it: a probe refreshes its tick and protects it)."""
    first = 1000
    while key not in store.spill:
        lookup(np.arange(first, first + 8, dtype=np.uint64))
        first += 8
        assert first < 100000, "row never evicted?"


def test_spill_restore_returns_trained_row_engine_and_store():
    """test_spill_roundtrip_gpu's sizes.  A trained row that was evicted to
    the host tier comes back trained — not freshly initialised — through the
    engine's front half (spill_restore on the probe stream) and through a
    plain store.lookup (the inline phase 1)."""
    from persia_amd.core import hashing
    from persia_amd.core.schema import EmbeddingSchema, SlotConfig
    from persia_amd.core.store import BUCKET_SIZE, PROBE_BUCKETS, HipEmbeddingStore
    from persia_amd.embedding import EmbeddingConfig

    dim, cap, bs = 4, BUCKET_SIZE * PROBE_BUCKETS, 8
    eng = P.mk_engine(
        GPU, "adagrad",
        EmbeddingSchema(slots={"s": SlotConfig(name="s", dim=dim)}),
        capacity=cap, spill_capacity=10000,
    )
    plain = HipEmbeddingStore(
        dim, cap, P.mk_opt("adagrad"),
        EmbeddingConfig(emb_initialization=(-0.5, 0.5)), GPU,
        spill_capacity=10000,
    )
    store = eng.stores[dim]

    def eng_lookup(ids):
        return eng.process_batch(P.PersiaBatch(
            [P.IDTypeFeatureWithSingleID("s", ids)],
            labels=[P.Label(np.ones((bs, 1), np.float32))], requires_grad=True,
        ))

    def plain_lookup(ids):
        keys = hashing.splitmix64(np.asarray(ids, dtype=np.uint64))
        return plain.lookup(torch.from_numpy(keys.view(np.int64)).to(GPU), True)

    sevens = np.full(bs, 7, dtype=np.uint64)
    tb = eng_lookup(sevens)
    assert store.spill is not None and tb._groups[0].u_count is not None
    key_t = tb._groups[0].uniq_keys[:1].clone()
    key = int(key_t.cpu().numpy().view(np.uint64)[0])
    init = store.lookup(key_t, train=False).cpu()
    g = torch.full((bs, dim), 2.0, dtype=torch.float16, device=GPU)
    eng.apply_gradients_base(tb, sum_base_grads=[g])
    trained = store.lookup(key_t, train=False).cpu()
    assert not torch.equal(trained, init)

    # the same key in the plain store, trained through update_gradients
    assert torch.equal(plain.lookup(key_t, train=True).cpu(), init)
    plain.update_gradients(key_t, torch.full((1, dim), 2.0, device=GPU))
    trained_plain = plain.lookup(key_t, train=False).cpu()
    assert not torch.equal(trained_plain, init)

    _flood_until_spilled(key, store, eng_lookup)
    _flood_until_spilled(key, plain, plain_lookup)
    assert store.lookup(key_t, train=False).abs().sum().item() == 0.0  # evicted
    tb = eng_lookup(sevens)
    assert torch.equal(tb._groups[0].sum_base.float().cpu(),
                       trained.half().float().expand(bs, dim))
    assert torch.equal(store.lookup(key_t, train=False).cpu(), trained)
    assert torch.equal(plain.lookup(key_t, train=True).cpu(), trained_plain)

