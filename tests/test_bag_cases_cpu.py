"""Scenario generators, models and bounds of tests/test_gpu_bag_exact.py (the
native lookup of multi-ID sum slots), and the checks that need no GPU.

* bag scenarios: per slot a CSR (values, offsets) with bag lengths 0..5, and
  the special shapes -- a slot that is entirely empty, one 300-id bag, every
  bag empty.
* ``plan_model``: what bag_plan computes, in numpy.  Segment s*B+b is sample
  b of slot s.
* ``bag_reference``: the f64 sum of the SAME row bits and the per-element
  bound, in the vocabulary of tests/test_gpu_sparse_exact.py section D.  L is
  the number of addends of a segment, S the sum of their absolute values,
  scale the exact 1/sqrt(max(L, 1)) of a sqrt slot (1 elsewhere):

      E = (L + 1) 2^-23 scale S      L adds and the scale multiply, a full
                                     f32 ulp each
        + 2 * 2^-23 scale S          sqrt slots: 2 ulp of rsqrtf, the figure
                                     of tests/test_update_cases_cpu.py
      then the f16 store: E + 2^-11 (|ref| + E) + 2^-25

  Here a plain f32 loop is held to the bound, and a loop that drops one
  addend or ignores the scale is shown to break it.
* the host staging buffer ``pack_bag_buffer``: layout, the per-batch cache,
  and a ValueError for each kind of bad offsets.
"""
import numpy as np
import pytest
import torch

from persia_amd.embedding.data import (
    IDTypeFeature, Label, PersiaBatch, _FlatIDFeature,
)

import test_engine_paths as P
from test_gpu_dense_exact import EPS32, f16_store_bound

VOCAB = 300
MAX_LEN = 5
LONG_BAG = 300
RSQRT_ULPS = 2  # tests/test_update_cases_cpu.py


# ------------------------------------------------------------------ scenarios


def _rng(*tag):
    seed = 0
    for t in tag:
        seed = seed * 1000003 + int(t)
    return np.random.default_rng(seed)


def bag_slots(S, B, kind="mixed", seed=0, vocab=VOCAB):
    """-> [(values u64[n_s], offsets i64[B+1])] * S.

    kind: "mixed"       lengths 0..5, some bags empty
          "empty_slot"  the same, one slot (the middle one) entirely empty
          "long"        the same, one 300-id bag in the last slot
          "all_empty"   nnz == 0
          "single"      one id per sample (a single-ID slot is a bag of 1)"""
    rng = _rng(7, S, B, seed, ("mixed", "empty_slot", "long", "all_empty",
                               "single").index(kind))
    out = []
    for s in range(S):
        lens = rng.integers(0, MAX_LEN + 1, size=B)
        if B >= MAX_LEN + 1:
            lens[: MAX_LEN + 1] = np.arange(MAX_LEN + 1)  # every length occurs
            lens = lens[rng.permutation(B)]
        if kind == "all_empty" or (kind == "empty_slot" and s == S // 2):
            lens[:] = 0
        if kind == "single":
            lens[:] = 1
        if kind == "long" and s == S - 1:
            lens[B // 2] = LONG_BAG
        offsets = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        values = rng.integers(0, vocab, size=int(offsets[-1]), dtype=np.uint64)
        out.append((values, offsets))
    return out


def bag_feats(slots, names=None):
    names = names or [f"s{i}" for i in range(len(slots))]
    return [_FlatIDFeature(n, v, o) for n, (v, o) in zip(names, slots)]


# ---------------------------------------------------------------- plan model


def plan_model(slots, sqrt_flags=None):
    """numpy model of bag_plan -> (cat_offsets i64[S*B+1], seg_id i64[nnz],
    seg_lens f32[S*B], seg_scale f64[S*B] exact, or None without a sqrt
    slot)."""
    S, B = len(slots), len(slots[0][1]) - 1
    starts = np.concatenate([[0], np.cumsum([len(v) for v, _ in slots])])
    cat = np.concatenate(
        [starts[s] + slots[s][1][:-1] for s in range(S)] + [starts[-1:]]
    ).astype(np.int64)
    lens = np.diff(cat)
    seg_id = np.repeat(np.arange(S * B, dtype=np.int64), lens)
    scale = None
    if sqrt_flags is not None and any(sqrt_flags):
        scale = np.where(
            np.repeat(np.asarray(sqrt_flags, dtype=bool), B),
            1.0 / np.sqrt(np.maximum(lens, 1).astype(np.float64)), 1.0,
        )
    return cat, seg_id, lens.astype(np.float32), scale


def check_scale(got_f32, exact_f64, sqrt_seg):
    """The device's scale against the exact one: 1 bit for bit on a plain
    slot, within 2 ulp of rsqrtf on a sqrt slot."""
    got = np.asarray(got_f32, dtype=np.float64)
    assert np.array_equal(got[~sqrt_seg], np.ones((~sqrt_seg).sum()))
    err = np.abs(got[sqrt_seg] - exact_f64[sqrt_seg])
    assert (err <= RSQRT_ULPS * EPS32 * exact_f64[sqrt_seg]).all()


# ------------------------------------------------------- reference and bound


def bag_reference(rows, inverse, cat_offsets, sqrt_seg=None):
    """rows f32 [U, dim] (a row of zeros: the key contributes nothing),
    inverse i64[nnz], cat_offsets i64[n_seg+1], sqrt_seg bool[n_seg] or None.
    -> (ref f64 [n_seg, dim], bound f64 [n_seg, dim])."""
    rows = torch.as_tensor(rows)
    inverse = torch.as_tensor(inverse)
    cat = torch.as_tensor(cat_offsets)
    n_seg, dim = cat.numel() - 1, rows.shape[1]
    lens = cat[1:] - cat[:-1]
    seg = torch.repeat_interleave(torch.arange(n_seg), lens)
    g = rows.double()[inverse]
    ref = torch.zeros(n_seg, dim, dtype=torch.float64)
    S = torch.zeros_like(ref)
    ref.index_add_(0, seg, g)
    S.index_add_(0, seg, g.abs())
    L = lens.double()[:, None]
    ulps = L + 1
    if sqrt_seg is not None:
        sq = torch.as_tensor(sqrt_seg)[:, None]
        sc = torch.where(sq, L.clamp_min(1.0).rsqrt(), torch.ones_like(L))
        ref, S = ref * sc, S * sc
        ulps = ulps + RSQRT_ULPS * sq.double()
    E = ulps * EPS32 * S
    return ref, f16_store_bound(E, ref)


def f32_bag_loop(rows, inverse, cat_offsets, scale=None, drop_last=False):
    """What bag_sum does, in plain numpy f32: adds in position order from +0,
    one multiply by the f32 scale, the f16 store."""
    r = np.asarray(rows, dtype=np.float32)
    inv, off = np.asarray(inverse), np.asarray(cat_offsets)
    n_seg = len(off) - 1
    out = np.zeros((n_seg, r.shape[1]), dtype=np.float32)
    for s in range(n_seg):
        acc = np.zeros(r.shape[1], dtype=np.float32)
        for k in range(off[s], off[s + 1] - int(drop_last)):
            acc = acc + r[inv[k]]
        out[s] = acc * (np.float32(1) if scale is None else np.float32(scale[s]))
    return torch.from_numpy(out).half()


def worst(got, ref, bound):
    err = (got.double() - ref).abs()
    return (err / bound.clamp_min(1e-300)).max().item()


def _loop_case(dim, kind):
    slots = bag_slots(3, 37, kind, seed=dim)
    cat, seg_id, _lens, scale = plan_model(slots, (False, True, True))
    nnz = len(seg_id)
    rng = _rng(9, dim)
    n_rows = 50
    rows = (rng.standard_normal((n_rows, dim)) * 0.5 + 0.05).astype(np.float32)
    inverse = rng.integers(0, n_rows, size=nnz)
    sqrt_seg = np.repeat([False, True, True], 37)
    return rows, inverse, cat, scale, sqrt_seg


@pytest.mark.parametrize("kind", ["mixed", "long"])
@pytest.mark.parametrize("dim", (8, 24, 64, 96, 200))
def test_bag_bound_fits_f32_and_rejects_wrong_loops(dim, kind):
    rows, inverse, cat, scale, sqrt_seg = _loop_case(dim, kind)
    ref, bound = bag_reference(rows, inverse, cat, sqrt_seg)
    s32 = scale.astype(np.float32)
    good = worst(f32_bag_loop(rows, inverse, cat, s32), ref, bound)
    dropped = worst(f32_bag_loop(rows, inverse, cat, s32, drop_last=True),
                    ref, bound)
    unscaled = worst(f32_bag_loop(rows, inverse, cat, None), ref, bound)
    print(f"bag dim {dim} {kind}: err/bound {good:.3g}, last addend dropped "
          f"{dropped:.3g}, scale ignored {unscaled:.3g}")
    assert good <= 1.0 < 10.0 < min(dropped, unscaled)


def test_plan_model_on_a_hand_case():
    """Two slots, B = 3: slot 0 has bags [2, 0, 1], slot 1 is empty."""
    slots = [(np.array([5, 6, 7], np.uint64), np.array([0, 2, 2, 3])),
             (np.empty(0, np.uint64), np.array([0, 0, 0, 0]))]
    cat, seg_id, lens, scale = plan_model(slots, (True, False))
    assert cat.tolist() == [0, 2, 2, 3, 3, 3, 3]
    assert seg_id.tolist() == [0, 0, 2]
    assert lens.tolist() == [2, 0, 1, 0, 0, 0]
    assert np.allclose(scale, [2 ** -0.5, 1, 1, 1, 1, 1])
    assert plan_model(slots, (False, False))[3] is None


# --------------------------------------------------------- the staging buffer


def test_pack_bag_buffer_layout():
    from persia_amd.core.engine import pack_bag_buffer

    for kind in ("mixed", "empty_slot", "long", "all_empty", "single"):
        slots = bag_slots(3, 5, kind)
        buf, nnz, B = pack_bag_buffer(bag_feats(slots))
        S = len(slots)
        assert buf.dtype == np.int64 and B == 5
        assert nnz == sum(len(v) for v, _ in slots)
        assert len(buf) == nnz + S + 1 + S * (B + 1)
        values = np.concatenate([v for v, _ in slots]).view(np.int64)
        assert np.array_equal(buf[:nnz], values)
        starts = np.concatenate([[0], np.cumsum([len(v) for v, _ in slots])])
        assert np.array_equal(buf[nnz : nnz + S + 1], starts)
        offs = buf[nnz + S + 1 :].reshape(S, B + 1)
        for s in range(S):
            assert np.array_equal(offs[s], slots[s][1])  # relative to the slot


def test_pack_bag_buffer_writes_into_the_callers_array():
    from persia_amd.core.engine import pack_bag_buffer

    made = []

    def alloc(n):
        made.append(np.full(n, -7, dtype=np.int64))
        return made[0]

    buf, nnz, _B = pack_bag_buffer(bag_feats(bag_slots(2, 4)), alloc)
    assert buf is made[0] and len(made) == 1 and (buf[nnz:] >= 0).all()


def _bad(kind):
    values = np.arange(6, dtype=np.uint64)
    good = np.array([0, 2, 2, 6], dtype=np.int64)
    other = _FlatIDFeature("ok", values, good)
    offsets = {
        "first_not_zero": np.array([1, 2, 2, 6]),
        "decreasing": np.array([0, 3, 2, 6]),
        "last_short": np.array([0, 2, 2, 5]),
        "last_long": np.array([0, 2, 2, 7]),
        "other_batch_size": np.array([0, 2, 6]),
    }[kind].astype(np.int64)
    return [other, _FlatIDFeature("bad", values, offsets)]


@pytest.mark.parametrize("kind", ["first_not_zero", "decreasing", "last_short",
                                  "last_long", "other_batch_size"])
def test_pack_bag_buffer_rejects_bad_offsets(kind):
    from persia_amd.core.engine import pack_bag_buffer

    pack_bag_buffer(_bad(kind)[:1])  # the companion slot alone is fine
    with pytest.raises(ValueError, match="bad"):
        pack_bag_buffer(_bad(kind))


def bag_batch(seed, names=("a", "b"), kind="mixed", batch_size=P.B):
    """A PersiaBatch of bag slots (lengths 0..5) under the given slot names."""
    slots = bag_slots(len(names), batch_size, kind, seed=seed)
    feats = [
        IDTypeFeature(n, [v[o[b] : o[b + 1]] for b in range(batch_size)])
        for n, (v, o) in zip(names, slots)
    ]
    return PersiaBatch(
        feats, labels=[Label(np.ones((batch_size, 1), np.float32))],
        requires_grad=True,
    )


def test_host_buffer_is_built_once_per_batch_and_group():
    eng = P.mk_engine(P.CPU, "adagrad")
    batch = bag_batch(0, ("a", "b"))
    feats = eng._feats_by_dim(batch)[8]
    first = eng._bag_host_buffer(batch, 8, feats)
    again = eng._bag_host_buffer(batch, 8, feats)
    assert again[0] is first[0] and again[1:] == first[1:]
    assert ("bag", 8) in batch._pinned_cache
    t, nnz, B = first
    assert t.dtype == torch.int64 and B == P.B
    from persia_amd.core.engine import pack_bag_buffer

    ref, ref_nnz, _ = pack_bag_buffer(feats)
    assert nnz == ref_nnz and np.array_equal(t.numpy(), ref)
    other = bag_batch(1, ("a", "b"))
    assert eng._bag_host_buffer(other, 8, eng._feats_by_dim(other)[8])[0] is not t


def test_cpu_engine_never_takes_the_bag_path():
    eng = P.mk_engine(P.CPU, "adagrad")
    batch = bag_batch(0, ("a", "b"))
    assert eng._bag_fast and not eng._bag_group(8, eng._feats_by_dim(batch)[8])
    tb = eng.process_batch(batch)
    assert all(g.u_count is None and g.has_sqrt is None for g in tb._groups)
