"""Cases and models of tests/test_gpu_stack_exact.py (the native bag lookup of
sum slots with hashstack rounds), and the checks that need no GPU.

* cases: the bag shapes of tests/test_bag_cases_cpu.py (S in {1, 3}, B in
  {1, 5, 67}, kinds mixed / empty_slot / long / all_empty) with per-slot
  rounds from {0, 1, 2, 3} over 64 buckets and a vocabulary of 300, so the ids
  of one bag collide inside a round; a prefix-0 slot beside prefixed ones; and
  a four-slot shape with two single-ID slots, one of them stacked.
* the expected keys are ``test_route_cases_cpu.sign_prep_model`` (held there
  to EmbeddingEngine._prepare_slot_keys), the expected plan is
  ``test_bag_cases_cpu.plan_model`` on the expanded offsets.
* ``pack_stack_bag_buffer``: the layout on a hand case, today's bytes for an
  unstacked group, a ValueError for each kind of bad offsets, rounds and
  bucket count, and the per-batch cache.
* ``index_model``: the kernel's index arithmetic in numpy -- from an output
  position q its slot, sample, round and input id -- and ``keys_from_index``,
  the keys that follow from it.  They reproduce sign_prep_model on every
  case, so the GPU file only has to compare the kernel with them; an
  id-major layout (the rounds of one id adjacent) is shown to be rejected.
* the CPU engine never takes the bag path for a stacked group.
"""
import functools

import numpy as np
import pytest
import torch

from persia_amd.core import hashing
from persia_amd.core.engine import pack_bag_buffer, pack_stack_bag_buffer
from persia_amd.embedding.data import _FlatIDFeature

import test_bag_cases_cpu as BC
import test_engine_paths as P
import test_route_cases_cpu as RC

SIZE = 64  # buckets per round: 300 ids fold onto 64, bags collide
SPACING = RC.SPACING
ROUNDS_S1 = ((1,), (2,), (3,))  # by B
ROUNDS_S3 = ((2, 0, 3), (0, 1, 2), (3, 2, 1))
SHAPES = [(S, B) for S in (1, 3) for B in (1, 5, 67)]
KINDS = ("mixed", "empty_slot", "long", "all_empty")


def _prefix(i, S):
    """Slot 0 of a several-slot group has no prefix, beside prefixed ones."""
    return 0 if (i == 0 and S > 1) else (i + 1) << 56


@functools.lru_cache(maxsize=None)
def stack_case(S, B, kind):
    """-> [RC.PrepSlot] * S: BC.bag_slots with rounds, bucket count, prefix."""
    rounds = (ROUNDS_S1 if S == 1 else ROUNDS_S3)[(1, 5, 67).index(B)]
    return [
        RC.PrepSlot(f"s{i}", v, o, r, SIZE if r else 1, _prefix(i, S))
        for i, ((v, o), r) in enumerate(zip(BC.bag_slots(S, B, kind), rounds))
    ]


@functools.lru_cache(maxsize=None)
def single_case(B):
    """Four slots: a bag, a stacked single-ID slot, a stacked bag without a
    prefix, an unstacked single-ID slot."""
    bags = BC.bag_slots(2, B, "mixed", seed=3)
    singles = BC.bag_slots(2, B, "single", seed=4)
    parts = [(bags[0], 0, 1 << 56), (singles[0], 2, 2 << 56),
             (bags[1], 3, 0), (singles[1], 0, 3 << 56)]
    return [RC.PrepSlot(f"s{i}", v, o, r, SIZE if r else 1, p)
            for i, ((v, o), r, p) in enumerate(parts)]


def all_cases():
    out = [((S, B, kind), stack_case(S, B, kind))
           for S, B in SHAPES for kind in KINDS]
    out += [(("single", B), single_case(B)) for B in (5, 67)]
    return out


CASE_IDS = ["-".join(str(x) for x in tag) for tag, _ in all_cases()]


def feats_of(slots):
    return [_FlatIDFeature(s.name, s.values, s.offsets) for s in slots]


def rounds_of(slots):
    return [s.rounds for s in slots], [s.size for s in slots]


def expanded(slots):
    """The slots as bags of the expanded position space, for BC.plan_model:
    [(placeholder values of the expanded length, offsets * max(R, 1))]."""
    return [(np.zeros(len(s.values) * max(s.rounds, 1), np.uint64),
             np.asarray(s.offsets) * max(s.rounds, 1)) for s in slots]


def pack(slots, alloc=None):
    return pack_stack_bag_buffer(feats_of(slots), *rounds_of(slots), alloc)


def split(buf, nnz_in, S, B):
    """-> (values u64, slot_starts, offsets [S, B+1], in_starts)."""
    plan = nnz_in + S + 1 + S * (B + 1)
    assert len(buf) == plan + S + 1
    return (buf[:nnz_in].view(np.uint64), buf[nnz_in : nnz_in + S + 1],
            buf[nnz_in + S + 1 : plan].reshape(S, B + 1), buf[plan:])


# ------------------------------------------------------------- index model


def index_model(buf, nnz_in, nnz_out, S, B, rounds, id_major=False):
    """What one thread of the sign-prep kernel derives from its output
    position q -> (slot, sample, round, index into values), each i64[nnz_out].
    Slot: the last s with slot_starts[s] <= q.  Sample of a stacked slot: the
    last b < B with E[b] <= p, p = q - slot_starts[s]; then len =
    (E[b+1] - E[b]) / R, t = p - E[b], r = t / len, id E[b]/R + t % len.
    ``id_major`` is the wrong layout r = t % R, id E[b]/R + t / R."""
    _values, starts, offs, in_starts = split(buf, nnz_in, S, B)
    q = np.arange(nnz_out, dtype=np.int64)
    slot = np.searchsorted(starts[:S], q, side="right") - 1
    p = q - starts[slot]
    sample = np.zeros(nnz_out, dtype=np.int64)
    rnd = np.zeros(nnz_out, dtype=np.int64)
    src = in_starts[slot] + p
    for s in range(S):
        R = rounds[s]
        m = slot == s
        if not m.any():
            continue
        E = offs[s]
        b = np.searchsorted(E[:B], p[m], side="right") - 1
        if R == 0:  # the kernel does not look for it; bag_plan does
            sample[m] = b
            continue
        ln = (E[b + 1] - E[b]) // R
        t = p[m] - E[b]
        assert (ln >= 1).all()
        sample[m] = b
        if id_major:
            rnd[m], src[m] = t % R, in_starts[s] + E[b] // R + t // R
        else:
            rnd[m], src[m] = t // ln, in_starts[s] + E[b] // R + t % ln
    return slot, sample, rnd, src


def keys_from_index(buf, nnz_in, slots, slot, rnd, src):
    """The mixed key of every output position: round ``rnd`` of the id at
    ``src`` (splitmix64 iterated rnd+1 times on the raw id, folded into the
    round's buckets), then the prefix fold, the mix and the empty-key remap."""
    values = buf[:nnz_in].view(np.uint64)
    out = np.empty(len(slot), dtype=np.uint64)
    for s, ps in enumerate(slots):
        m = slot == s
        v = values[src[m]]
        if ps.rounds:
            stacked = hashing.hash_stack(v, ps.rounds, ps.size)
            v = stacked[rnd[m], np.arange(len(v))]
        out[m] = RC._mix_slot(v, ps.prefix)
    return out


@pytest.mark.parametrize("tag,slots", all_cases(), ids=CASE_IDS)
def test_index_model_reproduces_sign_prep_model(tag, slots):
    S, B = len(slots), len(slots[0].offsets) - 1
    buf, nnz_in, nnz_out, _B = pack(slots)
    rounds, _sizes = rounds_of(slots)
    want = RC.sign_prep_model(slots)
    assert len(want) == nnz_out
    assert nnz_out == sum(len(s.values) * max(s.rounds, 1) for s in slots)
    slot, sample, rnd, src = index_model(buf, nnz_in, nnz_out, S, B, rounds)
    got = keys_from_index(buf, nnz_in, slots, slot, rnd, src)
    assert np.array_equal(got, want)
    # the position belongs to the segment bag_plan gives it
    _cat, seg_id, _lens, _scale = BC.plan_model(expanded(slots))
    assert np.array_equal(slot * B + sample, seg_id)
    assert (src >= 0).all() and (src < max(nnz_in, 1)).all()
    for s, ps in enumerate(slots):
        assert (rnd[slot == s] < max(ps.rounds, 1)).all()
    # every id is read once per round
    if nnz_out:
        assert np.array_equal(
            np.bincount(src, minlength=nnz_in),
            np.repeat([max(s.rounds, 1) for s in slots],
                      [len(s.values) for s in slots]))
    if any(s.rounds > 1 and np.diff(s.offsets).max(initial=0) > 1
           for s in slots):
        slot, _sample, rnd, src = index_model(buf, nnz_in, nnz_out, S, B,
                                              rounds, id_major=True)
        wrong = keys_from_index(buf, nnz_in, slots, slot, rnd, src)
        assert not np.array_equal(wrong, want)


def test_cases_collide_and_cover_the_rounds():
    seen = set()
    for _tag, slots in all_cases():
        seen |= {s.rounds for s in slots}
    assert seen == {0, 1, 2, 3}
    slots = stack_case(3, 67, "long")
    model = RC.sign_prep_model(slots)
    buf, nnz_in, nnz_out, B = pack(slots)
    _v, starts, offs, _in = split(buf, nnz_in, 3, 67)
    # slot 0 has 3 rounds: inside the bags, ids of one round collide (several
    # positions of one segment with one key), and a key of round 0 never
    # equals one of round 1 (disjoint bucket ranges)
    collided = 0
    for b in range(67):
        lo, hi = starts[0] + offs[0][b], starts[0] + offs[0][b + 1]
        n = (hi - lo) // 3
        r0, r1 = model[lo : lo + n], model[lo + n : lo + 2 * n]
        ids = slots[0].values[slots[0].offsets[b] : slots[0].offsets[b + 1]]
        collided += len(np.unique(ids)) - len(np.unique(r0))
        assert not set(r0.tolist()) & set(r1.tolist())
    assert collided > 0
    prefixes = [s.prefix for s in slots]
    assert prefixes[0] == 0 and all(prefixes[1:])
    assert [np.diff(s.offsets).max() for s in single_case(5)][1::2] == [1, 1]


# --------------------------------------------------------- the staging buffer


def test_stack_buffer_on_a_hand_case():
    """Two slots, B = 3.  Slot 0: bags [2, 0, 1], 2 rounds; slot 1: bags
    [1, 1, 0], none."""
    feats = [_FlatIDFeature("x", np.array([5, 6, 7], np.uint64),
                            np.array([0, 2, 2, 3])),
             _FlatIDFeature("y", np.array([8, 9], np.uint64),
                            np.array([0, 1, 2, 2]))]
    buf, nnz_in, nnz_out, B = pack_stack_bag_buffer(feats, [2, 0], [64, 1])
    assert (nnz_in, nnz_out, B) == (5, 8, 3) and buf.dtype == np.int64
    assert buf.tolist() == [5, 6, 7, 8, 9,        # the ids as they came
                            0, 6, 8,              # expanded slot starts
                            0, 4, 4, 6,           # slot 0: offsets * 2
                            0, 1, 2, 2,           # slot 1: its own
                            0, 3, 5]              # slot starts in values
    slots = [RC.PrepSlot("x", feats[0].values, feats[0].offsets, 2, 64, 0),
             RC.PrepSlot("y", feats[1].values, feats[1].offsets, 0, 1, 0)]
    slot, sample, rnd, src = index_model(buf, 5, 8, 2, 3, [2, 0])
    assert slot.tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    assert sample.tolist() == [0, 0, 0, 0, 2, 2, 0, 1]
    assert rnd.tolist() == [0, 0, 1, 1, 0, 1, 0, 0]  # round-major in a span
    assert src.tolist() == [0, 1, 0, 1, 2, 2, 3, 4]
    assert np.array_equal(keys_from_index(buf, 5, slots, slot, rnd, src),
                          RC.sign_prep_model(slots))


@pytest.mark.parametrize("kind", KINDS + ("single",))
def test_unstacked_group_yields_todays_bytes(kind):
    feats = BC.bag_feats(BC.bag_slots(3, 5, kind))
    want, nnz, B = pack_bag_buffer(feats)
    got, nnz_in, nnz_out, got_B = pack_stack_bag_buffer(
        feats, [0, 0, 0], [1, 1, 1])
    assert got.tobytes() == want.tobytes() and got.dtype == want.dtype
    assert (nnz_in, nnz_out, got_B) == (nnz, nnz, B)


@pytest.mark.parametrize("tag,slots", all_cases(), ids=CASE_IDS)
def test_stack_buffer_layout(tag, slots):
    S, B = len(slots), len(slots[0].offsets) - 1
    buf, nnz_in, nnz_out, got_B = pack(slots)
    assert got_B == B and nnz_in == sum(len(s.values) for s in slots)
    values, starts, offs, in_starts = split(buf, nnz_in, S, B)
    assert np.array_equal(values, np.concatenate([s.values for s in slots]))
    args = RC.prep_kernel_args(slots)  # what _group_keys uploads
    assert np.array_equal(starts, args["out_starts"])
    assert np.array_equal(in_starts, args["in_starts"])
    assert np.array_equal(offs.reshape(-1), args["all_offs"])
    assert nnz_out == args["n_out"]
    # slot_starts ‖ offsets is pack_bag_buffer's plan of the expanded bags
    ref, ref_nnz, _ = pack_bag_buffer(BC.bag_feats(expanded(slots)))
    assert ref_nnz == nnz_out
    assert np.array_equal(buf[nnz_in : len(buf) - (S + 1)], ref[ref_nnz:])


def test_stack_buffer_writes_into_the_callers_array():
    made = []

    def alloc(n):
        made.append(np.full(n, -7, dtype=np.int64))
        return made[0]

    buf, nnz_in, _out, _B = pack(stack_case(3, 5, "mixed"), alloc)
    assert buf is made[0] and len(made) == 1 and (buf[nnz_in:] >= 0).all()


@pytest.mark.parametrize("kind", ["first_not_zero", "decreasing", "last_short",
                                  "last_long", "other_batch_size"])
def test_stack_buffer_rejects_bad_offsets(kind):
    pack_stack_bag_buffer(BC._bad(kind)[:1], [2], [SIZE])
    for rounds in ([2, 2], [0, 2], [2, 0]):
        with pytest.raises(ValueError, match="bad"):
            pack_stack_bag_buffer(BC._bad(kind), rounds, [SIZE, SIZE])


def test_stack_buffer_rejects_bad_rounds_and_sizes():
    feats = BC.bag_feats(BC.bag_slots(2, 4))
    pack_stack_bag_buffer(feats, [2, 0], [1, 0])  # size of an unstacked slot
    with pytest.raises(ValueError, match="s1.*-1 hashstack rounds"):
        pack_stack_bag_buffer(feats, [2, -1], [SIZE, SIZE])
    with pytest.raises(ValueError, match="s0.*embedding_size 0"):
        pack_stack_bag_buffer(feats, [2, 0], [0, SIZE])
    with pytest.raises(ValueError, match="s1.*embedding_size -3"):
        pack_stack_bag_buffer(feats, [0, 1], [SIZE, -3])
    with pytest.raises(ValueError, match="2 slots"):
        pack_stack_bag_buffer(feats, [2], [SIZE])
    with pytest.raises(ValueError, match="2 slots"):
        pack_stack_bag_buffer(feats, [2, 0], [SIZE, SIZE, SIZE])


# ------------------------------------------------------------------ the engine

NAMES = tuple(P.SINGLE_SLOTS)  # a, b: dim 8; c, d: dim 16


def stack_schema(sqrt=False):
    """Pure-sum slots in two dim-groups: a plain and b stacked (bags), c
    stacked and d plain (both fed one id per sample).  ``sqrt``: b scales by
    1/sqrt of its expanded length."""
    from persia_amd.core.schema import (EmbeddingSchema, HashStackConfig,
                                        SlotConfig)

    def stack(r):
        return HashStackConfig(hash_stack_rounds=r, embedding_size=SIZE)

    return EmbeddingSchema(slots={
        "a": SlotConfig(name="a", dim=8),
        "b": SlotConfig(name="b", dim=8, hash_stack_config=stack(2),
                        sqrt_scaling=sqrt),
        "c": SlotConfig(name="c", dim=16, hash_stack_config=stack(3)),
        "d": SlotConfig(name="d", dim=16),
    })


def stack_batch(seed):
    """a, b: bags of 0..5 ids; c, d: one id per sample."""
    batch = BC.bag_batch(seed, NAMES)
    feats = {f.name: f for f in batch.id_type_features}
    for f in P.single_batch(seed).id_type_features:
        if f.name in ("c", "d"):
            feats[f.name] = f
    batch.id_type_features = [feats[n] for n in NAMES]
    return batch


def test_host_buffer_is_built_once_per_batch_and_group():
    eng = P.mk_engine(P.CPU, "adagrad", stack_schema())
    batch = stack_batch(0)
    by_dim = eng._feats_by_dim(batch)
    for dim, rounds, sizes in ((8, [0, 2], [1, SIZE]), (16, [3, 0], [SIZE, 1])):
        feats = by_dim[dim]
        first = eng._stack_host_buffer(batch, dim, feats)
        again = eng._stack_host_buffer(batch, dim, feats)
        assert again[0] is first[0] and again[1:] == first[1:]
        t, nnz_in, nnz_out, B = batch._pinned_cache[("bag", dim)]
        assert t is first[0] and t.dtype == torch.int64 and B == P.B
        ref, r_in, r_out, _ = pack_stack_bag_buffer(feats, rounds, sizes)
        assert (nnz_in, nnz_out) == (r_in, r_out) and r_out > r_in
        assert np.array_equal(t.numpy(), ref)
    assert set(batch._pinned_cache) == {("bag", 8), ("bag", 16)}
    other = stack_batch(1)
    assert eng._stack_host_buffer(other, 8, eng._feats_by_dim(other)[8])[0] \
        is not batch._pinned_cache[("bag", 8)][0]
    # an unstacked group: today's buffer and tuple under the same key
    plain = P.mk_engine(P.CPU, "adagrad")
    batch = BC.bag_batch(0, ("a", "b"))
    feats = plain._feats_by_dim(batch)[8]
    t, nnz_in, nnz_out, B = plain._stack_host_buffer(batch, 8, feats)
    assert batch._pinned_cache[("bag", 8)] == (t, nnz_in, B)
    assert nnz_in == nnz_out and plain._bag_host_buffer(batch, 8, feats)[0] is t


def test_cpu_engine_never_takes_the_bag_path():
    eng = P.mk_engine(P.CPU, "adagrad", stack_schema())
    batch = stack_batch(0)
    assert eng._bag_fast
    for dim, feats in eng._feats_by_dim(batch).items():
        assert not eng._bag_group(dim, feats)
        assert not eng._all_single_sum(feats)
    tb = eng.process_batch(batch)
    assert all(g.u_count is None and g.has_sqrt is None for g in tb._groups)
    assert not getattr(batch, "_pinned_cache", None)
    # positions and offsets of the generic group are the expanded ones
    g8 = {g.dim: g for g in tb._groups}[8]
    n_a = len(batch.id_type_features[0].values)
    n_b = len(batch.id_type_features[1].values)
    assert [sc.pos_slice for sc in g8.slots] == [(0, n_a), (n_a, n_a + 2 * n_b)]
    assert torch.equal(
        g8.slots[1].seg_offsets,
        torch.from_numpy(batch.id_type_features[1].offsets * 2))
