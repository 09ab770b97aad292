"""The native lookup and fused update of raw (sequence) slots against exact
models.

Scenarios and the numpy models (raw_plan_model, raw_gather_model) come from
tests/test_raw_cases_cpu.py, which checks them against raw_embedding_tensors
without a GPU; the twin-store helpers are those of tests/test_gpu_bag_exact.py.

1. raw_plan, exactly: seg_id (cell row, -1 for a truncated position), the sum
   region's cat_offsets / seg_lens, raw_num, and a scale that is 1 bit for bit
   over the raw rows.
2. lookup_local_raw against the existing pieces on a twin store (sign_prep ->
   dedup_padded -> store.lookup -> segment_sum): the raw rows and mask equal
   the model applied to the twin's row bits, the sum region equals
   segment_sum's output, the tables are identical, the hints hold, and a
   second lookup of the same ids reads the updated rows.  One dim per lane
   layout of raw_gather.
3. Misses: a missed id gives a +0 row with mask 1.
4. The engine, PA_RAW_FAST on against off: the path was taken and stays
   sync-free through apply_gradients_base; the model inputs are bitwise equal;
   after 3 steps at loss_scale 4 the signs are equal and the rows within 1e-5
   (the figure of test_mixed_group_table_matches_cpu_engine: the off path sums
   raw gradients with an unordered index_add_); and a twin store driven
   through update_local with the model's seg_id leaves the engine's table bit
   for bit.
5. The dict contract: a None slot and a NaN slot leave their keys' rows alone.
6. TrainCtx end to end, on against off.
7. Which groups take the path, and the pinned host buffer.
"""
import numpy as np
import pytest
import torch

import test_bag_cases_cpu as BC
import test_engine_paths as P
import test_gpu_bag_exact as GB
import test_raw_cases_cpu as RC
from test_gpu_dense_exact import _bits, _dev, _native

pytestmark = pytest.mark.gpu

PREFIXES = (0, 1 << 56, 2 << 56, 3 << 56)
SQRT = (False, True)  # of the S sum slots


def _prefixes(n):
    return torch.tensor(PREFIXES[:n], dtype=torch.int64, device=_dev())


def _flags(S):
    return torch.tensor(list(SQRT[:S]) if any(SQRT[:S]) else [],
                        dtype=torch.int32, device=_dev())


def _meta(S, B, sfs):
    from persia_amd.core.engine import raw_slot_meta

    return torch.from_numpy(raw_slot_meta(S, B, list(sfs))).to(_dev())


def _upload(slots):
    up, nnz, _n, B = GB._upload(slots)
    return up, nnz, B


# ------------------------------------------------------------------ 1. the plan


@pytest.mark.parametrize("S,R,B,kind", RC.CASES)
def test_raw_plan_matches_numpy_model(S, R, B, kind):
    slots, sfs = RC.group_slots(S, R, B, kind), RC.SFS[R]
    up, nnz, _B = _upload(slots)
    n_rows = S * B + B * sum(sfs)
    cat, seg_id, lens, scale, num = _native().raw_plan(
        up[nnz:], S, B, nnz, _flags(S), _meta(S, B, sfs), list(sfs))
    assert np.array_equal(seg_id.cpu().numpy(),
                          RC.raw_plan_model(slots, S, sfs))
    assert np.array_equal(num.cpu().numpy(), RC.raw_num_model(slots, S, sfs))
    if S:
        m_cat, _seg, m_lens, m_scale = BC.plan_model(slots[:S], SQRT[:S])
        assert np.array_equal(cat.cpu().numpy(), m_cat)
        assert np.array_equal(lens.cpu().numpy(), m_lens)
        assert scale.dtype == torch.float32 and scale.numel() == n_rows
        sc = scale.cpu().numpy()
        BC.check_scale(sc[: S * B], m_scale, np.repeat(SQRT[:S], B))
        assert np.array_equal(sc[S * B :], np.ones(n_rows - S * B, np.float32))
    else:
        assert cat.cpu().tolist() == [0] and lens.numel() == 0
        assert scale.numel() == 0  # no sqrt slot: no scale tensor


# ------------------------------------------------------ 2. against a twin store

# (S, R, B, kind): every B, S, R and special shape at least once
LOOKUP_CASES = [(2, 2, 67, "mixed"), (0, 1, 5, "long"), (2, 1, 1, "mixed"),
                (0, 2, 67, "empty_raw"), (2, 2, 5, "all_empty")]


def _lookup(store, up, nnz, S, B, sfs, hints, train, prefixes=None,
            spacing=GB.SPACING):
    if prefixes is None:
        prefixes = _prefixes(S + len(sfs))
    return store.lookup_local_raw(up, nnz, S, B, prefixes, spacing, _flags(S),
                                  _meta(S, B, sfs), list(sfs), hints, train)


def _hint_view(res):
    """lookup_local_raw's results in the order GB._check_hints reads."""
    return (res[0],) + tuple(res[2:13])


def _twin_rows(twin, up, nnz, n_slots, train):
    C = _native()
    keys = C.sign_prep(up[:nnz], up[nnz : nnz + n_slots + 1],
                       _prefixes(n_slots), GB.SPACING)
    d = C.dedup_padded(keys)
    return twin.lookup(d[0], train, u_count=d[4]), d


def _check_against_twin(store, twin, slots, S, sfs, hints, train, what):
    dim = store.dim
    B = len(slots[0][1]) - 1
    up, nnz, _B = _upload(slots)
    res = _lookup(store, up, nnz, S, B, sfs, hints, train)
    base, mask = res[0], res[1]
    n_cells = B * sum(sfs)
    assert base.dtype == mask.dtype == torch.float16
    assert base.shape == (S * B + n_cells, dim) and mask.shape == (n_cells,)
    if nnz == 0:
        assert not base.any() and not mask.any() and int(res[6].item()) == 0
        return res, None
    rows, d = _twin_rows(twin, up, nnz, S + len(sfs), train)
    U = int(res[6].item())
    for got, ref, name in zip(res[2:7], d, ("uniq", "inverse", "perm",
                                            "ustarts", "u_count")):
        if name == "ustarts":  # nnz-padded: the tail is unspecified
            got, ref = got[: U + 1], ref[: U + 1]
        assert torch.equal(got, ref), f"{what}: {name}"
    assert np.array_equal(res[10].cpu().numpy(),
                          RC.raw_plan_model(slots, S, sfs)), f"{what}: seg_id"
    m_rows, m_mask = RC.raw_gather_model(rows.cpu(), res[3].cpu().numpy(),
                                         slots, S, sfs)
    assert torch.equal(_bits(base[S * B :].cpu()), _bits(m_rows)), \
        f"{what}: raw rows"
    assert torch.equal(_bits(mask.cpu()), _bits(m_mask)), f"{what}: mask"
    if S:
        scale = res[12][: S * B].contiguous()  # empty without a sqrt slot
        t_sums = _native().segment_sum(rows, d[1], res[9], scale)
        assert torch.equal(_bits(base[: S * B]), _bits(t_sums)), f"{what}: sums"
    if train and hints:
        GB._check_hints(store, _hint_view(res), what)
    else:
        assert res[7].numel() == 0 and res[8].numel() == 0
    return res, rows


@pytest.mark.parametrize("dim", GB.LOOKUP_DIMS)
def test_lookup_local_raw_matches_twin_and_model(dim):
    for S, R, B, kind in LOOKUP_CASES:
        store, twin = GB._mk_store(dim), GB._mk_store(dim)
        sfs = RC.SFS[R]
        what = f"dim {dim} S {S} R {R} B {B} {kind}"
        slots = RC.group_slots(S, R, B, kind, seed=dim)
        res, rows0 = _check_against_twin(store, twin, slots, S, sfs, True, True,
                                         what + " fresh")
        GB._assert_same_tables(store, twin, what + " after the fresh lookup")
        if rows0 is None:
            assert len(store) == 0
            continue
        # train every row, then look the same ids up again: nothing is fresh
        # and the cells hold the updated rows
        U = int(res[6].item())
        g = torch.randn(U, dim, device=_dev(),
                        generator=torch.Generator(_dev()).manual_seed(dim))
        store.update_gradients(res[2][:U], g)
        twin.update_gradients(res[2][:U], g)
        res2, rows1 = _check_against_twin(store, twin, slots, S, sfs, False,
                                          True, what + " second")
        assert not torch.equal(rows0[:U], rows1[:U])
        if bool(res[1].any()):  # B == 1: the one raw sample may be empty
            assert not torch.equal(res[0][S * B :], res2[0][S * B :])
        # an eval lookup with unseen ids inserts nothing
        keys_before = store.keys.clone()
        unseen = RC.group_slots(S, R, B, kind, seed=dim + 1,
                                vocab=4 * BC.VOCAB)
        res3, rows3 = _check_against_twin(store, twin, unseen, S, sfs, True,
                                           False, what + " eval")
        if B > 1:  # hundreds of ids over four times the vocabulary
            assert bool((rows3[: int(res3[6].item())] == 0).all(dim=1).any())
        assert torch.equal(store.keys, keys_before)
        GB._assert_same_tables(store, twin, what + " at the end")


def test_raw_group_beyond_the_thread_per_position_grid_is_refused():
    store = GB._mk_store(8, capacity=64)
    nnz = 16384 * 256 + 1
    slots = [(np.zeros(nnz, np.uint64), np.array([0, nnz], np.int64))]
    up, _nnz, B = _upload(slots)
    with pytest.raises(RuntimeError, match="4194304"):
        _lookup(store, up, nnz, 0, B, (3,), True, True)
    assert len(store) == 0


# ------------------------------------------------------------------- 3. misses


@pytest.mark.parametrize("admit", [1.0, 0.5])
def test_missed_ids_give_zero_rows_with_mask_one(admit):
    from persia_amd.core.store import BUCKET_SIZE, PROBE_BUCKETS

    dim, S, B, sfs = 8, 1, 8, (4,)
    cap = BUCKET_SIZE * PROBE_BUCKETS
    store = GB._mk_store(dim, capacity=cap, admit=admit)
    ids = GB._ids_of_home_bucket(40, 1, store.n_buckets)
    rng = np.random.default_rng(int(admit * 10))
    pos = np.concatenate([ids, rng.choice(ids, size=10)])
    pos = pos[rng.permutation(len(pos))]
    cuts = np.sort(rng.integers(0, len(pos) + 1, size=2 * B - 1))
    cuts[3] = cuts[2]  # an empty sample at least
    bounds = np.concatenate([[0], cuts, [len(pos)]])
    half = bounds[B]
    slots = [(pos[:half], bounds[: B + 1].astype(np.int64)),
             (pos[half:], (bounds[B:] - half).astype(np.int64))]
    up, nnz, _B = _upload(slots)
    no_prefix = torch.zeros(2, dtype=torch.int64, device=_dev())
    res = _lookup(store, up, nnz, S, B, sfs, True, True, no_prefix, -1)
    base, mask, uniq, inverse = res[0], res[1], res[2], res[3]
    U = int(res[6].item())
    assert U == 40 and res[12].numel() == 0
    sh = GB._check_hints(store, _hint_view(res), f"admit {admit}")
    rows = store.lookup(uniq[:U], train=False)
    resident = ~(rows == 0).all(dim=1).cpu().numpy()
    assert np.array_equal(resident, sh >= 0)
    if admit == 1.0:
        assert resident.sum() == cap  # the window is full, 8 keys overflow
    else:
        assert 5 <= resident.sum() < cap  # about half were refused
    m_rows, m_mask = RC.raw_gather_model(rows.cpu(), inverse.cpu().numpy(),
                                         slots, S, sfs)
    assert torch.equal(_bits(base[S * B :].cpu()), _bits(m_rows))
    assert torch.equal(_bits(mask.cpu()), _bits(m_mask))
    zero_row = (_bits(base[S * B :]) == 0).all(dim=1).cpu()  # +0 everywhere
    n_missed = int((zero_row & (mask.cpu() == 1)).sum())
    print(f"admit {admit}: {int(resident.sum())} of 40 keys resident, "
          f"{n_missed} cells hold a missed id")
    assert n_missed > 0
    assert bool(zero_row[mask.cpu() == 0].all())
    want = BC.f32_bag_loop(rows.cpu().numpy(), inverse.cpu().numpy(),
                           res[9].cpu().numpy())
    assert torch.equal(_bits(base[: S * B].cpu()), _bits(want))


# ------------------------------------------------------------------ 4. engine

RAW_DIMS = (16, 24)  # the groups of RC.raw_schema with a raw slot


def _engine(monkeypatch, raw_fast, optname, schema=None, **gconf):
    monkeypatch.setenv("PA_RAW_FAST", "1" if raw_fast else "0")
    eng = P.mk_engine(_dev(), optname, schema or RC.raw_schema(), **gconf)
    assert eng._raw_fast == raw_fast
    return eng


def _assert_raw_path(tb, taken):
    for g in tb._groups:
        if g.dim not in RAW_DIMS:
            continue
        if taken:
            assert g.u_count is not None and g.u_count.is_cuda
            assert g.slot_hint is not None and g.src_hint is not None
            assert g.raw_mask is not None and g.has_sqrt == (g.dim == 16)
        else:
            assert g.u_count is None and g.slot_hint is None
            assert g.raw_mask is None


def _model_inputs(tb):
    """The tensors prepare_features hands the model, without autograd."""
    out = {}
    for p in tb.payloads:
        if p.raw_rows is not None:
            out[p.name] = torch.cat([p.raw_rows, p.raw_mask], dim=2)
        elif p.is_raw:
            B, sfs = tb.batch_size, p.cfg.sample_fixed_size
            rows = p.raw_distinct.index_select(0, p.raw_index)
            mask = (p.raw_index.view(B, sfs, 1) != 0).half()
            out[p.name] = torch.cat([rows.view(B, sfs, -1), mask], dim=2)
        else:
            out[p.name] = p.sum_tensor
    return out


def _cell_grads(seed, dims):
    """Seeded f16 gradient per slot: (B, dim) for a sum slot, (B*sfs, dim) for
    a raw slot's cells."""
    gen = torch.Generator().manual_seed(seed)
    return {
        n: torch.randn(P.B * (sfs or 1), d, generator=gen).half().to(_dev())
        for n, (d, sfs, _sq) in RC.RAW_SLOTS.items() if d in dims
    }


def _feed_on(tb, grads):
    for g in tb._groups:
        g.sum_base.requires_grad_(True)
        g.sum_base.grad = torch.cat([grads[sc.name] for sc in g.slots])
        assert g.sum_base.grad.shape == g.sum_base.shape


def _feed_off(tb, grads):
    """-> raw_grads as ctx._on_backward builds them from the cell gradient."""
    raw_grads = {}
    for g in tb._groups:
        if g.sum_base is None:  # a group of raw slots only
            continue
        g.sum_base.requires_grad_(True)
        g.sum_base.grad = torch.cat(
            [grads[sc.name] for sc in g.slots if sc.cfg.embedding_summation])
    for p in tb.payloads:
        if not p.is_raw:
            continue
        if p.raw_distinct.shape[0] <= 1:
            raw_grads[p.name] = None
            continue
        grad = torch.zeros_like(p.raw_distinct, dtype=torch.float32)
        nz = p.raw_non_empty_index.view(-1)
        grad.index_add_(0, p.raw_index.view(-1)[nz],
                        grads[p.name].index_select(0, nz).float())
        raw_grads[p.name] = grad[1:, :]
    return raw_grads


def _twin_of(eng, dim, optname):
    from persia_amd.core.store import HipEmbeddingStore

    return HipEmbeddingStore(dim, eng.gconf.capacity, P.mk_opt(optname),
                             eng.hyper, _dev())


@pytest.mark.parametrize("optname", ["adagrad", "adam"])
def test_engine_raw_path_against_generic_and_twin(monkeypatch, optname):
    on = _engine(monkeypatch, True, optname)
    off = _engine(monkeypatch, False, optname)
    twins = {dim: _twin_of(on, dim, optname) for dim in RAW_DIMS}
    for step in range(P.STEPS):
        batch = RC.raw_batch(step)
        grads = _cell_grads(100 + step, (8, 16, 24))
        tb_on, tb_off = on.process_batch(batch), off.process_batch(batch)
        _assert_raw_path(tb_on, True)
        _assert_raw_path(tb_off, False)
        in_on, in_off = _model_inputs(tb_on), _model_inputs(tb_off)
        assert [p.name for p in tb_on.payloads] == list(RC.RAW_NAMES)
        for name, (d, sfs, _sq) in RC.RAW_SLOTS.items():
            want = (P.B, sfs, d + 1) if sfs else (P.B, d)
            assert in_on[name].shape == in_off[name].shape == want, name
            assert torch.equal(_bits(in_on[name].contiguous()),
                               _bits(in_off[name].contiguous())), \
                f"step {step}: model input of {name}"
        for p_on, p_off in zip(tb_on.payloads, tb_off.payloads):
            if p_on.raw_rows is not None:
                assert p_on.raw_distinct is None and p_on.raw_index is None
                assert p_on.raw_non_empty_index is None
                assert torch.equal(p_on.raw_sample_id_num,
                                   p_off.raw_sample_id_num)
        # the twin: the same lookup, then update_local with the engine's dedup
        # tensors, the model's seg_id and the same gradient
        for g in tb_on._groups:
            if g.dim not in RAW_DIMS:
                continue
            names = tuple(sc.name for sc in g.slots)
            plan = on._plans[("raw", g.dim, names, P.B)]
            pin, nnz, B = batch._pinned_cache[("raw", g.dim)]
            twins[g.dim].lookup_local_raw(
                pin.to(_dev()), nnz, plan.S, B, plan.prefixes,
                on._spacing_arg, plan.sqrt_flags, plan.raw_meta, plan.sfs,
                False, True)
            feats = {f.name: f for f in batch.id_type_features}
            slots = [(feats[n].values, feats[n].offsets) for n in names]
            seg_id = torch.from_numpy(
                RC.raw_plan_model(slots, plan.S, plan.sfs)).to(_dev())
            assert torch.equal(g.seg_id, seg_id)
            scale = torch.full((g.sum_base.shape[0],), 0.25, device=_dev())
            if g.dim == 16:
                scale = scale * g.fwd_scale
            twins[g.dim].update_local(
                torch.cat([grads[n] for n in names]), g.perm, g.ustarts,
                seg_id, scale, g.uniq_keys, g.u_count)
        _feed_on(tb_on, grads)
        on.apply_gradients_base(tb_on, loss_scale=4.0)
        off.apply_gradients_base(tb_off, _feed_off(tb_off, grads),
                                 loss_scale=4.0)
        # nobody materialised the group: the count is still on the device
        _assert_raw_path(tb_on, True)
    for dim in RAW_DIMS:
        GB._assert_same_tables(on.stores[dim], twins[dim],
                               f"{optname} dim {dim}: engine against twin")
    untouched = _engine(monkeypatch, True, optname)
    for step in range(P.STEPS):
        untouched.process_batch(RC.raw_batch(step))
    t_un, t_on, t_off = P.table(untouched), P.table(on), P.table(off)
    for dim in (8,) + RAW_DIMS:
        assert P.tables_differ({dim: t_un[dim]}, {dim: t_on[dim]})
    assert t_on.keys() == t_off.keys() == {8, 16, 24}
    for dim in t_on:
        assert np.array_equal(t_on[dim][0], t_off[dim][0]), f"dim {dim}: signs"
        diff = np.abs(t_on[dim][1] - t_off[dim][1]).max()
        print(f"{optname} dim {dim}: rows {t_on[dim][1].shape}, "
              f"max diff on/off {diff:.3e}")
        assert np.allclose(t_on[dim][1], t_off[dim][1], atol=1e-5,
                           rtol=1e-5), f"dim {dim}: max diff {diff}"


# ----------------------------------------------------------- 5. dict contract


def test_dict_contract_none_and_nan_raw_slots_leave_their_rows(monkeypatch):
    """Group 16 through apply_gradients: raw slot r gets None, raw slot q a
    NaN; the rows of their keys keep their bits while the sum slots' rows
    move.  Adagrad: a key that is updated with a zero gradient keeps its
    row."""
    eng = _engine(monkeypatch, True, "adagrad")
    tb = eng.process_batch(RC.raw_batch(0))
    g16 = next(g for g in tb._groups if g.dim == 16)
    store = eng.stores[16]

    def keys_of(name):
        sc = next(sc for sc in g16.slots if sc.name == name)
        s, e = sc.pos_slice
        return g16.uniq_keys[g16.inverse[s:e]].unique()

    keys = {n: keys_of(n) for n in ("a", "b", "r", "q")}
    assert all(k.numel() > 0 for k in keys.values())
    before = {n: store.lookup(k, train=False) for n, k in keys.items()}
    grads = _cell_grads(7, (8, 16, 24))
    grads["r"] = None
    grads["q"] = grads["q"].view(P.B, 4, 16).clone()  # the (B, sfs, dim) form
    grads["q"][3, 1, 5] = float("nan")
    eng.apply_gradients(tb, grads, loss_scale=4.0)
    after = {n: store.lookup(k, train=False) for n, k in keys.items()}
    for n in ("r", "q"):
        assert torch.equal(_bits(before[n]), _bits(after[n])), n
    for n in ("a", "b"):
        assert not torch.equal(before[n], after[n]), n
    # with real gradients the raw slots' rows move too
    tb = eng.process_batch(RC.raw_batch(0))
    eng.apply_gradients(tb, _cell_grads(8, (8, 16, 24)), loss_scale=4.0)
    moved = {n: store.lookup(k, train=False) for n, k in keys.items()}
    for n in ("r", "q"):
        assert not torch.equal(after[n], moved[n]), n


# ------------------------------------------------------------------- 6. ctx


class _SeqModel(torch.nn.Module):
    """One layer over every embedding input, raw (B, sfs, dim+1) included."""

    def __init__(self):
        super().__init__()
        width = sum((d + 1) * sfs if sfs else d
                    for d, sfs, _sq in RC.RAW_SLOTS.values())
        self.lin = torch.nn.Linear(width, 1)

    def forward(self, non_id, embs):
        return self.lin(torch.cat([e.float().flatten(1) for e in embs], dim=1))


def test_train_ctx_end_to_end_on_against_off(monkeypatch):
    from persia_amd.ctx import TrainCtx

    runs = {}
    for raw_fast in (True, False):
        eng = _engine(monkeypatch, raw_fast, "adagrad")
        torch.manual_seed(5)
        model = _SeqModel()
        seen_raw_grads = []
        apply_base = eng.apply_gradients_base

        def spy(tb, raw_grads=None, loss_scale=1.0, _apply=apply_base,
                _seen=seen_raw_grads):
            _seen.append(dict(raw_grads or {}))
            return _apply(tb, raw_grads, loss_scale)

        monkeypatch.setattr(eng, "apply_gradients_base", spy)
        outs = []
        with TrainCtx(
            model=model, engine=eng, device_id=0, mixed_precision=False,
            dense_optimizer=torch.optim.SGD(model.parameters(), lr=0.01),
        ) as ctx:
            for step in range(P.STEPS):
                tb = eng.process_batch(RC.raw_batch(step))
                out, labels = ctx.forward(tb)
                for name, e in zip(RC.RAW_NAMES, ctx.current_batch._emb_cache):
                    assert e[0] == name
                outs.append(out.detach().clone())
                loss = torch.nn.functional.binary_cross_entropy_with_logits(
                    out, labels[0])
                ctx.backward(loss)
                _assert_raw_path(tb, raw_fast)  # still on the fused update
        assert len(seen_raw_grads) == P.STEPS
        if raw_fast:
            assert all(not rg for rg in seen_raw_grads)
        else:
            assert all(set(rg) == {"r", "q", "p"} for rg in seen_raw_grads)
        runs[raw_fast] = (outs, P.table(eng))
    (outs_on, t_on), (outs_off, t_off) = runs[True], runs[False]
    assert outs_on[0].shape == (P.B, 1)
    assert torch.equal(outs_on[0], outs_off[0]), "first-step output"
    untouched = _engine(monkeypatch, True, "adagrad")
    for step in range(P.STEPS):
        untouched.process_batch(RC.raw_batch(step))
    t_un = P.table(untouched)
    for dim in t_on:  # the backward did train every group
        assert P.tables_differ({dim: t_un[dim]}, {dim: t_on[dim]})
    for dim in t_on:
        assert np.array_equal(t_on[dim][0], t_off[dim][0]), f"dim {dim}: signs"
        diff = np.abs(t_on[dim][1] - t_off[dim][1]).max()
        print(f"ctx dim {dim}: max diff on/off {diff:.3e}")
        assert np.allclose(t_on[dim][1], t_off[dim][1], atol=1e-5,
                           rtol=1e-5), f"dim {dim}: max diff {diff}"


def test_inference_lookup_inserts_nothing(monkeypatch):
    """train=0: the same tensors without requires_grad, zeros on a miss."""
    eng = _engine(monkeypatch, True, "adagrad")
    tb = eng.process_batch(RC.raw_batch(0), train=False)
    assert all(g.raw_mask is not None and g.slot_hint is None
               for g in tb._groups if g.dim in RAW_DIMS)
    assert eng.num_resident_rows() == 0
    for p in tb.payloads:
        if p.raw_rows is not None:
            assert not p.raw_rows.any() and not p.raw_rows.requires_grad
            want = torch.arange(p.cfg.sample_fixed_size, device=_dev()) < \
                p.raw_sample_id_num[:, None]
            assert torch.equal(p.raw_mask.squeeze(2), want.half())


# ------------------------------------------------- 7. path choice, host buffer


def test_prepare_host_batch_builds_the_raw_buffer(monkeypatch):
    eng = _engine(monkeypatch, True, "adagrad")
    batch = RC.raw_batch(0)
    eng.prepare_host_batch(batch)
    pins = {k: v for k, v in batch._pinned_cache.items()
            if k[0] in ("raw", "bag")}
    assert set(pins) == {("raw", 16), ("raw", 24), ("bag", 8)}
    assert all(t.is_pinned() for t, _nnz, _B in pins.values())
    tb = eng.process_batch(batch)
    _assert_raw_path(tb, True)
    assert all(batch._pinned_cache[k][0] is v[0] for k, v in pins.items())
    assert set(k for k in batch._pinned_cache if k[0] in ("raw", "bag")) == \
        set(pins)


def test_other_shapes_keep_their_paths(monkeypatch):
    # a raw slot beside a hashstack slot: generic
    eng = _engine(monkeypatch, True, "adagrad", P.mixed_schema())
    batch = P.mixed_batch(0)
    feats = eng._feats_by_dim(batch)
    assert not eng._raw_group(16, feats[16]) and not eng._raw_group(8, feats[8])
    by_dim = {g.dim: g for g in eng.process_batch(batch)._groups}
    assert by_dim[16].u_count is None and by_dim[16].raw_mask is None
    assert by_dim[8].u_count is not None and by_dim[8].has_sqrt is False
    # the raw schema: groups 16 and 24 qualify, the pure bag group keeps its
    # path; a spill tier, PA_FORCE_DIST, PA_RAW_FAST=0 and the CPU device
    # keep them generic
    batch = RC.raw_batch(0)
    eng = _engine(monkeypatch, True, "adagrad")
    feats = eng._feats_by_dim(batch)
    assert eng._raw_group(16, feats[16]) and eng._raw_group(24, feats[24])
    assert not eng._raw_group(8, feats[8]) and eng._bag_group(8, feats[8])
    by_dim = {g.dim: g for g in eng.process_batch(batch)._groups}
    assert by_dim[8].raw_mask is None and by_dim[8].has_sqrt is False
    spill = _engine(monkeypatch, True, "adagrad", spill_capacity=1000)
    monkeypatch.setenv("PA_FORCE_DIST", "1")
    forced = _engine(monkeypatch, True, "adagrad")
    monkeypatch.delenv("PA_FORCE_DIST")
    switched_off = _engine(monkeypatch, False, "adagrad")
    cpu = P.mk_engine(P.CPU, "adagrad", RC.raw_schema())
    assert spill.stores[16].spill is not None and forced._force_dist
    for other in (spill, forced, switched_off, cpu):
        assert not any(other._raw_group(d, f) for d, f in feats.items())
    # an all-single-ID group keeps its static plan
    eng = _engine(monkeypatch, True, "adagrad", P.single_schema())
    tb = eng.process_batch(P.single_batch(0))
    assert all(g.u_count is not None and g.has_sqrt is None
               and g.raw_mask is None for g in tb._groups)
