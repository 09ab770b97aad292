"""Scenario generators and numpy models of tests/test_gpu_raw_exact.py (the
native lookup of raw, i.e. sequence, slots), and the checks that need no GPU.

A raw-path group is S sum slots followed by R raw slots.  Raw slot r has a
``sample_fixed_size`` sfs[r] and owns B*sfs[r] rows of the group's leaf base,
one per cell (sample b, column c), behind the S*B sum segments:

    row(r, b, c) = S*B + sum_{r' < r} B*sfs[r'] + b*sfs[r] + c

* scenarios: the bag scenarios of tests/test_bag_cases_cpu.py (lengths 0..5
  with every length present, so sfs 3 and 4 both truncate and pad), plus a raw
  slot that is entirely empty; "long" puts one 300-id sample into the last raw
  slot.
* ``raw_plan_model``: seg_id of every position.  A sum position goes to its
  segment, a raw position with column c < sfs to its cell row, a truncated one
  (c >= sfs) to -1.
* ``raw_gather_model``: the f16 cell rows and the 0/1 mask from per-unique f32
  rows.  Both models are checked here against ``raw_embedding_tensors``, the
  generic path's builder: rows[b, c] == distinct[index[b*sfs + c]] bit for bit
  and mask == (index != 0).
* the host staging buffer of a sum+raw group and ``raw_slot_meta``.
"""
import numpy as np
import pytest
import torch

from persia_amd.core.schema import EmbeddingSchema, SlotConfig
from persia_amd.ops import reference as REF

import test_bag_cases_cpu as BC
import test_engine_paths as P

# name -> (dim, raw sample_fixed_size or None, sqrt).  Group 16: two sum slots
# (one sqrt) and two raw slots with different sfs; group 24: one raw slot alone
# (S == 0); group 8: a plain bag group.
RAW_SLOTS = {
    "a": (16, None, False), "r": (16, 3, False), "b": (16, None, True),
    "q": (16, 4, False), "p": (24, 1, False), "e": (8, None, False),
}
RAW_NAMES = tuple(RAW_SLOTS)


def raw_schema():
    return EmbeddingSchema(slots={
        n: SlotConfig(name=n, dim=d, sqrt_scaling=sq,
                      embedding_summation=sfs is None,
                      sample_fixed_size=sfs or 10)
        for n, (d, sfs, sq) in RAW_SLOTS.items()
    })


def raw_batch(seed, names=RAW_NAMES, kind="mixed", batch_size=P.B):
    """Lengths 0..5 per sample under the given names (raw slots come before
    sum slots in RAW_NAMES: the engine has to reorder them)."""
    return BC.bag_batch(seed, names, kind, batch_size)


def group_slots(S, R, B, kind="mixed", seed=0, vocab=BC.VOCAB):
    """-> [(values, offsets)] * (S + R), sum slots first.  The kinds of
    BC.bag_slots ("long": one 300-id sample in the last raw slot) and
    "empty_raw": the first raw slot entirely empty."""
    slots = BC.bag_slots(S + R, B, "mixed" if kind == "empty_raw" else kind,
                         seed=seed, vocab=vocab)
    if kind == "empty_raw":
        slots[S] = (np.empty(0, np.uint64), np.zeros(B + 1, np.int64))
    return slots


# --------------------------------------------------------------------- models


def row_bases(S, B, sfs):
    return [S * B + B * sum(sfs[:r]) for r in range(len(sfs))]


def raw_plan_model(slots, S, sfs):
    """seg_id i64[nnz] of a group whose first S slots are sum slots and whose
    other slots are raw with sample_fixed_size sfs[r]."""
    B = len(slots[0][1]) - 1
    parts = [BC.plan_model(slots[:S])[1]] if S else []
    for (values, off), f, base in zip(slots[S:], sfs, row_bases(S, B, sfs)):
        b = np.repeat(np.arange(B, dtype=np.int64), np.diff(off))
        c = np.arange(len(values), dtype=np.int64) - off[b]
        parts.append(np.where(c < f, base + b * f + c, -1))
    return np.concatenate(parts).astype(np.int64)


def raw_num_model(slots, S, sfs):
    return np.concatenate([np.minimum(np.diff(off), f)
                           for (_v, off), f in zip(slots[S:], sfs)])


def raw_gather_model(rows_f32, inverse, slots, S, sfs):
    """rows_f32 [U, dim]: the f32 row of every unique key, zeros for a key the
    table does not hold; inverse i64[nnz] over the whole group.
    -> (rows f16 [sum B*sfs, dim], mask f16 [sum B*sfs]), cells in row order."""
    rows = torch.as_tensor(rows_f32).float()
    inverse = np.asarray(inverse)
    B, dim = len(slots[0][1]) - 1, rows.shape[1]
    starts = np.concatenate([[0], np.cumsum([len(v) for v, _ in slots])])
    out_rows, out_mask = [], []
    for r, f in enumerate(sfs):
        off = slots[S + r][1]
        cells = torch.zeros(B, f, dim, dtype=torch.float16)
        mask = torch.zeros(B, f, dtype=torch.float16)
        for b in range(B):
            n = min(int(off[b + 1] - off[b]), f)
            p0 = starts[S + r] + off[b]
            cells[b, :n] = rows[inverse[p0 : p0 + n]].half()
            mask[b, :n] = 1
        out_rows.append(cells.view(B * f, dim))
        out_mask.append(mask.view(B * f))
    return torch.cat(out_rows), torch.cat(out_mask)


def _bits(t):
    return t.contiguous().view(torch.int16)


# --------------------------------------------------------------------- checks

CASES = [(S, R, B, kind)
         for S in (0, 2) for R in (1, 2) for B in (1, 5, 67)
         for kind in ("mixed", "empty_raw", "long", "all_empty")]
SFS = {1: (3,), 2: (4, 1)}


@pytest.mark.parametrize("S,R,B,kind", CASES)
def test_plan_model_truncates_and_pads(S, R, B, kind):
    """Every kept position's seg_id is its own cell, every dropped one is -1,
    by a plain loop; no two positions share a cell."""
    slots, sfs = group_slots(S, R, B, kind), SFS[R]
    seg_id = raw_plan_model(slots, S, sfs)
    assert len(seg_id) == sum(len(v) for v, _ in slots)
    bases = row_bases(S, B, sfs)
    p = sum(len(v) for v, _ in slots[:S])
    assert (seg_id[:p] >= 0).all() and (seg_id[:p] < S * B).all()
    kept = dropped = 0
    for r, f in enumerate(sfs):
        off = slots[S + r][1]
        for b in range(B):
            for c in range(off[b + 1] - off[b]):
                want = bases[r] + b * f + c if c < f else -1
                assert seg_id[p] == want
                kept, dropped = kept + (c < f), dropped + (c >= f)
                p += 1
    raw_ids = seg_id[seg_id >= S * B]
    assert len(np.unique(raw_ids)) == len(raw_ids) == kept
    assert np.array_equal(raw_num_model(slots, S, sfs).sum(), kept)
    if kind in ("mixed", "long") and B >= 5:
        assert kept and dropped  # sfs 3 and 4 truncate lengths 4 and 5
    if kind == "long":
        assert dropped >= BC.LONG_BAG - max(sfs)


@pytest.mark.parametrize("S,R,B,kind", CASES)
def test_models_match_raw_embedding_tensors(S, R, B, kind):
    """The generic path builds distinct rows and an index per raw slot and the
    consumer index-selects; the models give the same bits directly."""
    slots, sfs, dim = group_slots(S, R, B, kind, seed=1), SFS[R], 6
    keys = np.concatenate(
        [v + np.uint64(1000 * i) for i, (v, _) in enumerate(slots)])
    uniq, inverse = np.unique(keys, return_inverse=True)
    rng = np.random.default_rng(len(keys))
    rows = torch.from_numpy(
        rng.standard_normal((len(uniq), dim)).astype(np.float32))
    rows[::7] = 0.0  # keys the table does not hold
    got_rows, got_mask = raw_gather_model(rows, inverse, slots, S, sfs)
    seg_id = raw_plan_model(slots, S, sfs)
    starts = np.concatenate([[0], np.cumsum([len(v) for v, _ in slots])])
    cell0 = 0
    for r, f in enumerate(sfs):
        s, e = starts[S + r], starts[S + r + 1]
        slot_uniq, slot_inv = torch.unique(
            torch.from_numpy(inverse[s:e]), sorted=True, return_inverse=True)
        distinct, index, non_empty, num = REF.raw_embedding_tensors(
            rows[slot_uniq], slot_inv, torch.from_numpy(slots[S + r][1]), f,
            1.0, torch.float16)
        want = distinct.index_select(0, index)
        n = B * f
        assert torch.equal(_bits(got_rows[cell0 : cell0 + n]), _bits(want))
        assert torch.equal(got_mask[cell0 : cell0 + n], (index != 0).half())
        # the plan sends exactly the non-empty cells a position
        cells = seg_id[s:e][seg_id[s:e] >= 0] - (S * B + cell0)
        assert np.array_equal(np.sort(cells), non_empty.numpy())
        assert np.array_equal(
            raw_num_model(slots, S, sfs)[r * B : (r + 1) * B], num.numpy())
        cell0 += n
    assert cell0 == got_rows.shape[0] == got_mask.numel()


def test_raw_slot_meta_on_a_hand_case():
    from persia_amd.core.engine import raw_slot_meta

    assert raw_slot_meta(2, 5, [3, 4, 1]).tolist() == [10, 25, 45, 3, 4, 1]
    assert raw_slot_meta(0, 7, [2]).tolist() == [0, 2]
    assert raw_slot_meta(2, 5, [3, 4, 1]).dtype == np.int64
    assert row_bases(2, 5, [3, 4, 1]) == [10, 25, 45]


def test_host_buffer_of_a_sum_and_raw_group():
    """Sum slots first, then raw slots, each part in its incoming order; one
    buffer in pack_bag_buffer's layout under the key ("raw", dim)."""
    from persia_amd.core.engine import pack_bag_buffer

    eng = P.mk_engine(P.CPU, "adagrad", raw_schema())
    batch = raw_batch(0)
    feats = eng._feats_by_dim(batch)[16]
    assert [f.name for f in feats] == ["a", "r", "b", "q"]
    ordered = eng._sums_first(feats)
    assert [f.name for f in ordered] == ["a", "b", "r", "q"]
    t, nnz, B = eng._bag_host_buffer(batch, 16, ordered, kind="raw")
    assert ("raw", 16) in batch._pinned_cache
    assert ("bag", 16) not in batch._pinned_cache
    assert eng._bag_host_buffer(batch, 16, ordered, kind="raw")[0] is t
    ref, ref_nnz, ref_B = pack_bag_buffer(ordered)
    assert (nnz, B) == (ref_nnz, ref_B) == (sum(len(f.values) for f in feats),
                                            P.B)
    assert np.array_equal(t.numpy(), ref)
    n_slots = 4
    starts = t.numpy()[nnz : nnz + n_slots + 1]
    assert starts.tolist() == np.concatenate(
        [[0], np.cumsum([len(f.values) for f in ordered])]).tolist()
    offs = t.numpy()[nnz + n_slots + 1 :].reshape(n_slots, B + 1)
    for i, f in enumerate(ordered):
        assert np.array_equal(offs[i], f.offsets)


def test_cpu_engine_never_takes_the_raw_path():
    eng = P.mk_engine(P.CPU, "adagrad", raw_schema())
    batch = raw_batch(0)
    assert eng._raw_fast
    for dim, feats in eng._feats_by_dim(batch).items():
        assert not eng._raw_group(dim, feats)
    tb = eng.process_batch(batch)
    assert all(g.u_count is None and g.raw_mask is None for g in tb._groups)
    raw = [p for p in tb.payloads if p.is_raw]
    assert [p.name for p in raw] == ["r", "q", "p"]
    assert all(p.raw_rows is None and p.raw_distinct is not None for p in raw)


def test_raw_fast_knob_is_read_at_construction(monkeypatch):
    monkeypatch.setenv("PA_RAW_FAST", "0")
    assert not P.mk_engine(P.CPU, "adagrad", raw_schema())._raw_fast
