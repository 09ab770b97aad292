"""The embedding engine: dedup → route → lookup → postprocess → backward.

This is the MI355X-native collapse of three reference tiers into one
per-GPU object:

* nn-worker forward/backward engines (rust/persia-core/src/forward.rs,
  backward.rs) — prefetch pipeline, staleness, H2D/D2H;
* embedding worker (embedding_worker_service/mod.rs) — dedup, sharding,
  summation/raw postprocess, gradient merge;
* embedding parameter server (embedding_parameter_service/mod.rs) — the
  sharded table + sparse optimizers.

Per batch (one dim-group):
  1. sign prep: hashstack folding + feature-group prefix + splitmix64 mix
     (the mixed key is both the dedup sort key and the shard router);
  2. dedup: radix sort + unique over the *whole batch* (all slots at once —
     the reference dedups per-slot per-worker with CPU hashmaps);
  3. route: contiguous range-partition of the sorted unique keys by owner
     rank, RCCL all_to_all_single over xGMI for keys, then rows (f16 wire,
     like the reference's f16 EmbeddingBatch wire format);
  4. owner-side: set-associative HBM hash-table probe/insert (HIP kernel);
  5. postprocess: fused gather + segment-sum into per-slot (B, dim) f16
     tensors, or raw distinct+index tensors (exact reference contract);
  6. backward: reverse — segment grad scatter, all_to_all, fused
     optimizer update on the owner shard.
"""
import contextlib
import functools
import os
import queue
import threading
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from persia_amd.core import hashing
from persia_amd.core.comm import DistContext
from persia_amd.core.schema import EmbeddingSchema, GlobalConfig, SlotConfig
from persia_amd.core.store import make_store
from persia_amd.embedding import EmbeddingConfig
from persia_amd.embedding.data import PersiaBatch
from persia_amd.embedding.optim import Optimizer
from persia_amd.logger import get_default_logger
from persia_amd.ops import reference as R

_logger = get_default_logger("persia_amd.engine")

_FLIP = -(2 ** 63)  # XOR with sign bit: signed sort order == unsigned order
_NO_STREAM = contextlib.nullcontext()  # stands in for torch.cuda.stream(...)


def _roctx_range(name):
    """Method decorator: named roctx range (rocprofv3 --marker-trace) when
    the engine runs with PA_ROCTX=1; a bare call otherwise."""

    def deco(fn):
        @functools.wraps(fn)
        def wrap(self, *a, **k):
            if not getattr(self, "_roctx", False):
                return fn(self, *a, **k)
            torch.cuda.nvtx.range_push(name)
            try:
                return fn(self, *a, **k)
            finally:
                torch.cuda.nvtx.range_pop()
        return wrap
    return deco


def _update_entry(fn):
    """Decorator of the two public gradient entry points: advances
    ``_update_counter`` once per call, samples the host-side issue+wait time
    of the whole push into ``update_gradient_time_cost_sec`` (the reference's
    gauge, mod.rs:83-100) every PA_METRICS_EVERY calls, and opens the
    ``persia:update`` roctx range under PA_ROCTX=1."""

    @functools.wraps(fn)
    def wrap(self, *a, **k):
        self._update_counter += 1
        sample = (
            self.metrics_enabled
            and self._update_counter % self._metrics_every
            == 1 % self._metrics_every
        )
        if not (sample or self._roctx):
            return fn(self, *a, **k)
        if self._roctx:
            torch.cuda.nvtx.range_push("persia:update")
        t0 = time.perf_counter()
        try:
            return fn(self, *a, **k)
        finally:
            if sample:
                self.metrics.update_gradient_time_cost_sec.set(
                    time.perf_counter() - t0
                )
            if self._roctx:
                torch.cuda.nvtx.range_pop()

    return wrap


def _sqrt_scale(sqrt_mask: torch.Tensor, seg_lens: torch.Tensor) -> torch.Tensor:
    """Per-segment 1/sqrt(len) of the sqrt-scaling sum slots (1 elsewhere):
    the forward sum and its gradient carry the same factor."""
    return torch.where(
        sqrt_mask, seg_lens.clamp(min=1.0).rsqrt(), torch.ones_like(seg_lens)
    )


def _owner_of_keys(keys: torch.Tensor, world_size: int) -> torch.Tensor:
    """Monotone range-partition of u64 bit-pattern keys (int64 tensors) to
    ranks — same math as hashing.owner_of."""
    hi = (keys >> 32) & 0xFFFFFFFF
    return (hi * world_size) >> 32


def _dedup(keys_t: torch.Tensor):
    """Sort-based dedup of u64-bit-pattern keys.

    -> (uniq [U] ascending in u64 order, inverse [nnz] pos->uniq idx,
        perm [nnz] sort permutation, ustarts [U+1] uniq boundaries in sorted
        order).  perm/ustarts drive the ordered (deterministic, atomic-free)
        gradient scatter kernel: a unique key's positions are contiguous in
        sort order.  torch.sort on GPU is a hipCUB radix sort.
    """
    dev = keys_t.device
    nnz = keys_t.numel()
    if nnz == 0:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return z, z, z, torch.zeros(1, dtype=torch.int64, device=dev)
    flipped = keys_t ^ _FLIP  # signed sort order == unsigned key order
    svals, perm = torch.sort(flipped)
    neq = torch.ones(nnz, dtype=torch.bool, device=dev)
    neq[1:] = svals[1:] != svals[:-1]
    inv_sorted = torch.cumsum(neq, 0) - 1
    inverse = torch.empty(nnz, dtype=torch.int64, device=dev)
    inverse[perm] = inv_sorted
    uniq = svals[neq] ^ _FLIP
    ustarts = torch.cat(
        [
            torch.nonzero(neq, as_tuple=False).view(-1),
            torch.tensor([nnz], dtype=torch.int64, device=dev),
        ]
    )
    return uniq, inverse, perm, ustarts


def pack_bag_buffer(feats, alloc=None) -> Tuple[np.ndarray, int, int]:
    """The host staging buffer of a bag group (sum slots with any number of
    ids per sample), one i64 array

        values[nnz] ‖ slot_starts[S+1] ‖ offsets[S, B+1]

    with each slot's offsets relative to its own start.  -> (buffer, nnz, B).
    ``alloc(n)`` supplies the writable i64[n] array (pinned memory on the
    GPU path).

    Each slot's offsets are checked here, once: batches arrive over the byte
    wire and the device kernels index with these values.  ValueError unless
    every slot has the same B, and its offsets start at 0, never decrease
    and end at ``len(values)``."""
    S = len(feats)
    B = _check_bag_offsets(feats)
    lens = [len(f.values) for f in feats]
    nnz = int(sum(lens))
    total = nnz + (S + 1) + S * (B + 1)
    buf = np.empty(total, dtype=np.int64) if alloc is None else alloc(total)
    pos = 0
    for f, n in zip(feats, lens):
        buf[pos : pos + n] = np.asarray(f.values, dtype=np.uint64).view(np.int64)
        pos += n
    buf[nnz] = 0
    np.cumsum(lens, out=buf[nnz + 1 : nnz + S + 1])
    buf[nnz + S + 1 :].reshape(S, B + 1)[:] = [f.offsets for f in feats]
    return buf, nnz, B


def _check_bag_offsets(feats) -> int:
    """pack_bag_buffer's checks of every slot's offsets -> B."""
    B = len(feats[0].offsets) - 1
    for f in feats:
        offs = np.asarray(f.offsets)
        if offs.ndim != 1 or len(offs) - 1 != B or B < 0:
            raise ValueError(
                f"slot {f.name}: {len(offs) - 1} samples, the group has {B}"
            )
        if offs[0] != 0:
            raise ValueError(f"slot {f.name}: offsets start at {offs[0]}, not 0")
        if B and bool((offs[1:] < offs[:-1]).any()):
            raise ValueError(f"slot {f.name}: offsets decrease")
        if offs[-1] != len(f.values):
            raise ValueError(
                f"slot {f.name}: offsets end at {offs[-1]}, "
                f"the slot has {len(f.values)} ids"
            )
    return B


def pack_stack_bag_buffer(
    feats, rounds, sizes, alloc=None
) -> Tuple[np.ndarray, int, int, int]:
    """The host staging buffer of a bag group with hashstack slots.  Slot s
    has ``rounds[s]`` hashstack rounds (0: none) over ``sizes[s]`` buckets
    (its ``embedding_size``); each of its ids becomes ``rounds[s]`` positions
    inside its sample's span, so the slot's offsets grow by that factor.  One
    i64 array

        values[nnz_in] ‖ slot_starts[S+1] ‖ offsets[S, B+1] ‖ in_starts[S+1]

    ``values`` are the ids as they came: the expansion and the hashing run on
    the device (sign_prep_bags).  ``slot_starts`` and ``offsets`` are in the
    expanded position space (a stacked slot's offsets times its rounds,
    relative to the slot's start), so ``slot_starts ‖ offsets`` is the plan
    of pack_bag_buffer over ``nnz_out`` positions; ``in_starts`` are the
    slots' starts in ``values``.  -> (buffer, nnz_in, nnz_out, B).

    The offsets are checked as pack_bag_buffer checks them.  ValueError also
    for a negative round count and for a stacked slot of fewer than one
    bucket.  Without a stacked slot the buffer is pack_bag_buffer's, byte for
    byte, and nnz_out == nnz_in."""
    S = len(feats)
    if len(rounds) != S or len(sizes) != S:
        raise ValueError(
            f"{S} slots, {len(rounds)} round counts and {len(sizes)} sizes"
        )
    for f, r, size in zip(feats, rounds, sizes):
        if r < 0:
            raise ValueError(f"slot {f.name}: {r} hashstack rounds")
        if r > 0 and size < 1:
            raise ValueError(
                f"slot {f.name}: hashstack embedding_size {size}, below 1"
            )
    if not any(rounds):
        buf, nnz, B = pack_bag_buffer(feats, alloc)
        return buf, nnz, nnz, B
    B = _check_bag_offsets(feats)
    lens = [len(f.values) for f in feats]
    grow = [max(int(r), 1) for r in rounds]
    nnz_in = int(sum(lens))
    nnz_out = int(sum(n * g for n, g in zip(lens, grow)))
    total = nnz_in + 2 * (S + 1) + S * (B + 1)
    buf = np.empty(total, dtype=np.int64) if alloc is None else alloc(total)
    pos = 0
    for f, n in zip(feats, lens):
        buf[pos : pos + n] = np.asarray(f.values, dtype=np.uint64).view(np.int64)
        pos += n
    starts = buf[nnz_in : nnz_in + S + 1]
    starts[0] = 0
    np.cumsum([n * g for n, g in zip(lens, grow)], out=starts[1:])
    offs = buf[nnz_in + S + 1 : total - (S + 1)].reshape(S, B + 1)
    for s, (f, g) in enumerate(zip(feats, grow)):
        offs[s] = np.asarray(f.offsets, dtype=np.int64) * g
    in_starts = buf[total - (S + 1) :]
    in_starts[0] = 0
    np.cumsum(lens, out=in_starts[1:])
    return buf, nnz_in, nnz_out, B


def _stack_config(cfgs) -> Tuple[List[int], List[int]]:
    """Per slot: hashstack rounds (0: none) and the bucket count of a stacked
    slot (1 elsewhere, as _group_keys passes it)."""
    rounds = [int(c.hash_stack_rounds) for c in cfgs]
    sizes = [
        int(c.hash_stack_config.embedding_size) if r > 0 else 1
        for c, r in zip(cfgs, rounds)
    ]
    return rounds, sizes


def raw_slot_meta(S: int, B: int, sfs: List[int]) -> np.ndarray:
    """Where the raw slots of a raw-path group sit in its leaf base, as the
    native lookup takes it: i64 ``row_base[R] ‖ sfs[R]``.  The base holds the
    S*B sum segments first, then per raw slot its B*sfs cell rows
    (sample-major), so ``row_base[r] = S*B + sum_{r' < r} B*sfs[r']``."""
    bases = S * B + B * np.concatenate([[0], np.cumsum(sfs[:-1])])
    return np.concatenate([bases, sfs]).astype(np.int64)


@dataclass
class SlotPayload:
    """What the dense side consumes for one slot (reference
    FeatureEmbeddingBatch, persia-common/src/lib.rs:85-113).

    A raw slot comes under one of two contracts.  The generic path fills
    ``raw_distinct`` / ``raw_index`` / ``raw_non_empty_index`` (the
    reference's distinct rows and index tensors; the consumer index-selects).
    The native raw path fills ``raw_rows`` / ``raw_mask`` instead, the
    fixed-size tensor itself, and leaves those three ``None``: it never builds
    per-slot distinct rows."""

    name: str
    cfg: SlotConfig
    sum_tensor: Optional[torch.Tensor] = None  # [B, dim] f16
    raw_distinct: Optional[torch.Tensor] = None  # [U_slot+1, dim] f16, row0 pad
    raw_index: Optional[torch.Tensor] = None  # [B*sfs] i64
    raw_non_empty_index: Optional[torch.Tensor] = None
    raw_sample_id_num: Optional[torch.Tensor] = None  # [B] i64 min(len, sfs)
    # native raw path: views of the group's leaf base and mask
    raw_rows: Optional[torch.Tensor] = None  # [B, sfs, dim] f16
    raw_mask: Optional[torch.Tensor] = None  # [B, sfs, 1] f16, 1 = holds an id

    @property
    def is_raw(self) -> bool:
        return self.raw_distinct is not None or self.raw_rows is not None


@dataclass
class _SlotCtx:
    name: str
    cfg: SlotConfig
    pos_slice: Tuple[int, int]  # slice of group position space
    seg_offsets: torch.Tensor  # [B+1] per-slot CSR (into its own positions)
    sum_seg_base: int = -1  # sum slots: base index in the group segment space
    slot_uniq_global: Optional[torch.Tensor] = None  # raw slots: local->global uniq
    slot_inverse: Optional[torch.Tensor] = None  # raw slots: pos->local distinct
    # native raw path: the slot's B*raw_sfs cell rows start at raw_row_base of
    # the group's leaf base (raw_sfs 0: not a raw-path slot)
    raw_row_base: int = -1
    raw_sfs: int = 0


@dataclass
class _GroupCtx:
    dim: int
    uniq_keys: torch.Tensor  # [U] int64 (u64 bit pattern); fast path: [nnz]
    #   padded with the true count ONLY in u_count (device) — sync-free dedup
    inverse: torch.Tensor  # [nnz] i64
    perm: torch.Tensor  # [nnz] sort permutation (ordered grad scatter)
    ustarts: torch.Tensor  # [U+1] unique boundaries in sorted order
    u_count: Optional[torch.Tensor] = None  # [1] i64 device unique count
    # update hints of the one-call lookup (None on every other path), [nnz]
    # i64, valid below u_count: the slot each unique key was given, and the
    # gradient row of a key with a single position (-1: none)
    slot_hint: Optional[torch.Tensor] = None
    src_hint: Optional[torch.Tensor] = None
    slots: List[_SlotCtx] = field(default_factory=list)
    # fused sum-slot segment space (sum slots occupy positions [0, sum_end))
    cat_offsets: Optional[torch.Tensor] = None  # [n_sum_segs+1]
    seg_id: Optional[torch.Tensor] = None  # [nnz]: pos -> group seg idx, -1 raw
    seg_lens: Optional[torch.Tensor] = None  # [n_sum_segs] f32
    sqrt_mask: Optional[torch.Tensor] = None  # [n_sum_segs] bool
    sum_base: Optional[torch.Tensor] = None  # [n_sum_segs, dim] f16 fused output
    n_sum_slots: int = 0
    # bag path only: whether a sqrt-scaling slot exists (host bool; None on
    # the other paths: not known without reading sqrt_mask back) and the
    # forward's per-segment scale [n_sum_segs] f32, empty = all ones
    has_sqrt: Optional[bool] = None
    fwd_scale: Optional[torch.Tensor] = None
    # native raw path only: sum_base is the whole leaf base, the n_sum_slots
    # sum slots' segments first, then every raw slot's cell rows; seg_id sends
    # a raw position to its cell row and fwd_scale (if any) covers all rows
    raw_mask: Optional[torch.Tensor] = None  # [base rows - n_sum_segs] f16
    raw_num: Optional[torch.Tensor] = None  # [R*B] i64 min(len, sfs)
    send_counts: Optional[List[int]] = None
    recv_counts: Optional[List[int]] = None
    # capacity-padded even-a2a fast path (sync-free distributed lookup):
    a2a_plan: Optional["_GroupPlan"] = None
    a2a_idx: Optional[torch.Tensor] = None  # [len(uniq)] uniq -> send-slot map
    a2a_recv_keys: Optional[torch.Tensor] = None  # [world*cap] owner-side keys
    a2a_owner_dedup: Optional[tuple] = None  # GPU: dedup_padded(recv_keys)


class _GroupPlan:
    """Static per-(group, batch-size) device constants for the all-single-ID
    fast path (the DLRM shape: every slot one id per sample).  Everything here
    is shape-derived, so one plan serves every batch of that shape."""

    def __init__(self, dim: int, cfgs: List[SlotConfig], B: int,
                 device: torch.device):
        S = len(cfgs)
        self.dim = dim
        self.names = tuple(c.name for c in cfgs)
        self.B = B
        self.S = S
        prefixes_np = np.array([c.index_prefix for c in cfgs], dtype=np.uint64)
        self.slot_starts = torch.arange(0, (S + 1) * B, B, dtype=torch.int64,
                                        device=device)
        self.prefixes = torch.from_numpy(prefixes_np.view(np.int64)).to(device)
        self.cat_offsets = torch.arange(S * B + 1, dtype=torch.int64, device=device)
        self.seg_id = torch.arange(S * B, dtype=torch.int64, device=device)
        self.empty_scale = torch.empty(0, dtype=torch.float32, device=device)
        # padded-a2a constants (attached lazily by EmbeddingEngine._a2a_setup)
        self.a2a_world: Optional[int] = None
        self.a2a_cap: Optional[int] = None
        self.a2a_ar: Optional[torch.Tensor] = None  # arange(nnz)
        self.a2a_ones: Optional[torch.Tensor] = None  # ones(nnz) count weights
        self.owner_seg_id: Optional[torch.Tensor] = None  # arange(world*cap)


class _BagPlan:
    """Static per-(group, batch-size) device constants of the bag path (sum
    slots with any number of ids per sample).  The positions vary per batch
    and come with the upload; only what the slot configs fix lives here.
    ``rounds`` / ``sizes`` are the slots' hashstack rounds (0: none) and
    bucket counts on the host, ``stack_dev`` the same as device tensors for
    the sign-prep kernel; all three None for a group without a stacked
    slot."""

    def __init__(self, dim: int, cfgs: List[SlotConfig], B: int,
                 device: torch.device):
        self.dim = dim
        self.B = B
        self.S = len(cfgs)
        self.rounds = self.sizes = self.stack_dev = None
        rounds, sizes = _stack_config(cfgs)
        if any(rounds):
            self.rounds, self.sizes = rounds, sizes
            self.stack_dev = (
                torch.tensor(rounds, dtype=torch.int32, device=device),
                torch.tensor(sizes, dtype=torch.int64, device=device),
            )
        prefixes_np = np.array([c.index_prefix for c in cfgs], dtype=np.uint64)
        self.prefixes = torch.from_numpy(prefixes_np.view(np.int64)).to(device)
        sqrt = [bool(c.sqrt_scaling) for c in cfgs]
        self.has_sqrt = any(sqrt)
        # i32[S] for bag_plan; empty = no sqrt slot, no scale tensor at all
        self.sqrt_flags = torch.tensor(
            sqrt if self.has_sqrt else [], dtype=torch.int32, device=device
        )
        self.sqrt_mask = torch.tensor(
            sqrt, dtype=torch.bool, device=device
        ).repeat_interleave(B)


class _RawPlan:
    """Static per-(group, batch-size) constants of the native raw path: S sum
    slots, then R raw slots (``cfgs`` in that order).  Prefixes of all slots,
    sqrt flags of the sum slots, and per raw slot its ``sample_fixed_size``
    and the first row of its cells in the leaf base (raw_slot_meta)."""

    def __init__(self, dim: int, cfgs: List[SlotConfig], B: int,
                 device: torch.device):
        self.dim = dim
        self.B = B
        sums = [c for c in cfgs if c.embedding_summation]
        self.S = S = len(sums)
        prefixes_np = np.array([c.index_prefix for c in cfgs], dtype=np.uint64)
        self.prefixes = torch.from_numpy(prefixes_np.view(np.int64)).to(device)
        sqrt = [bool(c.sqrt_scaling) for c in sums]
        self.has_sqrt = any(sqrt)
        self.sqrt_flags = torch.tensor(
            sqrt if self.has_sqrt else [], dtype=torch.int32, device=device
        )
        self.sqrt_mask = torch.tensor(
            sqrt, dtype=torch.bool, device=device
        ).repeat_interleave(B)
        self.sfs = [int(c.sample_fixed_size) for c in cfgs[S:]]
        meta = raw_slot_meta(S, B, self.sfs)
        self.row_bases = [int(x) for x in meta[: len(self.sfs)]]
        self.raw_meta = torch.from_numpy(meta).to(device)


class _SplitSlots(torch.autograd.Function):
    """Split a group's fused sum tensor into per-slot views with ONE backward
    op: autograd's native per-view SliceBackward would zero-fill and add a
    full-base-sized buffer per slot (2×n_slots kernels per step).  ``rows``
    is each slot's row count: B for a sum slot, B*sfs for a raw-path slot."""

    @staticmethod
    def forward(ctx, base: torch.Tensor, rows: Tuple[int, ...]):
        ctx.rows, ctx.dim = rows, base.shape[1]
        ctx.dev, ctx.dtype = base.device, base.dtype
        return base.split(list(rows), dim=0)

    @staticmethod
    def backward(ctx, *grads):
        parts = [
            g
            if g is not None
            else torch.zeros(n, ctx.dim, dtype=ctx.dtype, device=ctx.dev)
            for g, n in zip(grads, ctx.rows)
        ]
        return torch.cat(parts, dim=0), None


def _raw_path_payload(group: _GroupCtx, r: int, B: int) -> SlotPayload:
    """The payload of raw slot r of a raw-path group: views of the group's
    leaf base and mask."""
    sc = group.slots[group.n_sum_slots + r]
    n, dim = B * sc.raw_sfs, group.dim
    r0 = sc.raw_row_base
    m0 = r0 - group.n_sum_slots * B
    return SlotPayload(
        name=sc.name, cfg=sc.cfg,
        raw_rows=group.sum_base[r0 : r0 + n].view(B, sc.raw_sfs, dim),
        raw_mask=group.raw_mask[m0 : m0 + n].view(B, sc.raw_sfs, 1),
        raw_sample_id_num=group.raw_num[r * B : (r + 1) * B],
    )


class PersiaTrainingBatch:
    """Device-side batch ready for the dense model (reference
    PersiaTrainingBatch, persia-core/src/forward.rs:256-331)."""

    def __init__(self):
        self._payloads: List[SlotPayload] = []
        # fast-path groups whose SlotPayloads have not been built yet:
        # (group, slot_names, B).  The flagship loop reads group.sum_base
        # directly (enable_training_views / bench graph path), so building
        # ~2*n_slots python objects per batch in the pipeline thread is
        # wasted work unless someone actually asks for .payloads.
        self._lazy_sum_groups: List[Tuple["_GroupCtx", List[str], int]] = []
        self._order: Optional[Dict[str, int]] = None
        self._sorted: bool = False
        self.non_id_type_tensors: List[torch.Tensor] = []
        self.label_tensors: List[torch.Tensor] = []
        self.batch_size: int = 0
        self.requires_grad: bool = True
        self.meta: Optional[bytes] = None
        self.batch_id: Optional[int] = None
        self._groups: List[_GroupCtx] = []
        self._engine: Optional["EmbeddingEngine"] = None

    @property
    def payloads(self) -> List[SlotPayload]:
        """Per-slot payloads in the original id_type_features order
        (materialized on first access)."""
        if self._lazy_sum_groups:
            for group, _names, B in self._lazy_sum_groups:
                sums = group.sum_base
                for i, sc in enumerate(group.slots):
                    if sc.raw_sfs:
                        self._payloads.append(
                            _raw_path_payload(group, i - group.n_sum_slots, B)
                        )
                        continue
                    self._payloads.append(
                        SlotPayload(name=sc.name, cfg=sc.cfg,
                                    sum_tensor=sums[i * B : (i + 1) * B])
                    )
            self._lazy_sum_groups.clear()
            self._sorted = False
        if not self._sorted:
            if self._order is not None:
                self._payloads.sort(key=lambda p: self._order[p.name])
            self._sorted = True
        return self._payloads

    def enable_training_views(self) -> Dict[str, torch.Tensor]:
        """Mark each group's sum base requires_grad and return fresh per-slot
        views connected to it (autograd accumulates into ``sum_base.grad`` —
        consumed by ``EmbeddingEngine.apply_gradients_base``).  A raw-path
        slot's view is its ``(B, sfs, dim)`` rows, off the same backward
        node."""
        views: Dict[str, torch.Tensor] = {}
        B = self.batch_size
        for group in self._groups:
            if group.sum_base is None:
                continue
            group.sum_base.requires_grad_(True)
            in_base = [
                sc for sc in group.slots
                if sc.cfg.embedding_summation or sc.raw_sfs
            ]
            parts = _SplitSlots.apply(
                group.sum_base, tuple(B * (sc.raw_sfs or 1) for sc in in_base)
            )
            for sc, part in zip(in_base, parts):
                if sc.raw_sfs:
                    part = part.view(B, sc.raw_sfs, group.dim)
                views[sc.name] = part
        return views

    def training_embeddings(self) -> List[torch.Tensor]:
        """payload-ordered embedding tensors for a manual train loop."""
        views = self.enable_training_views()
        return [views.get(p.name, p.sum_tensor) for p in self.payloads]

    def record_stream(self, stream: "torch.cuda.Stream") -> None:
        """Tag every device tensor produced on the lookup stream as in-use by
        ``stream`` so the caching allocator cannot recycle the memory for new
        lookup-stream allocations while consumer kernels still read it
        (mandatory for cross-stream tensor hand-off)."""
        for t in self._device_tensors():
            t.record_stream(stream)

    def _device_tensors(self):
        for t in self.non_id_type_tensors + self.label_tensors:
            if t.is_cuda:
                yield t
        for g in self._groups:
            a2a_owner = g.a2a_owner_dedup or ()
            for t in (g.uniq_keys, g.inverse, g.perm, g.ustarts, g.u_count,
                      g.slot_hint, g.src_hint, g.sum_base, g.cat_offsets,
                      g.seg_id, g.seg_lens, g.fwd_scale, g.raw_mask, g.raw_num,
                      g.sqrt_mask, g.a2a_idx, g.a2a_recv_keys, *a2a_owner):
                if t is not None and t.is_cuda:
                    yield t
            for sc in g.slots:
                for t in (sc.seg_offsets, sc.slot_uniq_global, sc.slot_inverse):
                    if t is not None and t.is_cuda:
                        yield t
        # lazy groups hold only payloads that are views of group tensors (no
        # per-payload device tensors), so iterating the eagerly-built list is
        # sufficient and avoids materializing payloads in the pipeline thread
        for p in self._payloads:
            for t in (p.raw_distinct, p.raw_index, p.raw_non_empty_index,
                      p.raw_sample_id_num):
                if t is not None and t.is_cuda:
                    yield t


class EmbeddingEngine:
    def __init__(
        self,
        schema: EmbeddingSchema,
        hyper: EmbeddingConfig,
        optimizer: Optional[Optimizer],
        gconf: GlobalConfig,
        device: torch.device,
        dist_ctx: Optional[DistContext] = None,
        wire_dtype: torch.dtype = torch.float16,
    ):
        self.schema = schema
        self.hyper = hyper
        self.optimizer = optimizer
        self.gconf = gconf
        self.device = device
        self.dist = dist_ctx or DistContext.from_default_group()
        # Lookups are issued from the pipeline THREAD and gradient pushes from
        # the main thread; each needs its OWN communicator so cross-thread
        # interleaving can't reorder collectives across ranks (NCCL requires
        # identical issue order per communicator on every rank).
        self.dist_grad = (
            DistContext.new_sparse_group() if self.dist.distributed else self.dist
        )
        self.wire_dtype = wire_dtype
        # group slots by dim (slots of one dim share one store + one a2a)
        self.groups: Dict[int, List[SlotConfig]] = {}
        for name in schema.slot_names():
            cfg = schema.get_slot(name)
            self.groups.setdefault(cfg.dim, []).append(cfg)
        if optimizer is None:
            from persia_amd.embedding.optim import SGD

            optimizer = SGD(lr=0.0)
            self.optimizer = optimizer
        self.stores = {
            dim: make_store(
                dim, gconf.capacity, optimizer, hyper, device, gconf.spill_capacity
            )
            for dim in self.groups
        }
        self.skipped_grad_signs = 0
        self.nan_grad_batches = 0
        self._plans = {}
        self._empty_scale = torch.empty(0, dtype=torch.float32, device=device)
        # lookup_local's seg_id argument when no update hints are wanted
        self._no_seg = torch.empty(0, dtype=torch.int64, device=device)
        spacing = schema.feature_spacing
        self._spacing_arg = spacing if spacing < (1 << 63) else -1
        self.model_manager_status = "Idle"
        self.model_manager_progress = 0.0
        self._prod_timing = os.environ.get("PA_PROD_TIMING", "0") == "1"
        self._prod_timing_live = True  # cleared while the warm-up skip runs
        # timers skip the first batches: one-time ATen kernel-module loads
        # (~hundreds of ms) otherwise dominate the averages
        self._pt = {"prep": 0.0, "native": 0.0, "batch": 0.0, "n": 0,
                    "skip": 20}
        # fused distributed path (capacity-padded even a2a, sync-free);
        # PA_FUSED_DIST=0 falls back to the exact two-phase counts exchange,
        # PA_FORCE_DIST=1 exercises the padded machinery at world_size=1
        # (copy in place of the collectives) for single-GPU tests/profiling
        self._fused_dist = os.environ.get("PA_FUSED_DIST", "1") == "1"
        self._force_dist = os.environ.get("PA_FORCE_DIST", "0") == "1"
        # PA_UPDATE_HINTS (default on): the fused local update takes the
        # lookup's slot/source hints; 0 asks for and passes none (A/B switch,
        # same results)
        self._update_hints = os.environ.get("PA_UPDATE_HINTS", "1") != "0"
        # PA_BAG_FAST (default on): single-GPU dim-groups of sum slots with
        # several ids per sample or with hashstack rounds take the one-call
        # native bag lookup; 0 sends them down the generic path (A/B switch,
        # same results)
        self._bag_fast = os.environ.get("PA_BAG_FAST", "1") != "0"
        # PA_RAW_FAST (default on): single-GPU dim-groups with raw (sequence)
        # slots and no hashstack take the one-call native raw lookup; 0 sends
        # them down the generic path (A/B switch)
        self._raw_fast = os.environ.get("PA_RAW_FAST", "1") != "0"
        # PA_ROCTX=1: named roctx ranges around the pipeline stages for
        # rocprofv3 --marker-trace (torch.cuda.nvtx IS roctx on ROCm);
        # off by default so the hot loop never pays the marker calls
        self._roctx = os.environ.get("PA_ROCTX", "0") == "1"
        self._a2a_overflow = torch.zeros(1, dtype=torch.int64, device=device)
        from persia_amd.core.metrics import EngineMetrics

        self.metrics_enabled = bool(gconf.enable_metrics)
        self.metrics = EngineMetrics(self.metrics_enabled)
        # hot-path observability: sampled every PA_METRICS_EVERY batches so
        # the flagship loop never pays for timers/copies it does not use;
        # GPU-side values (event timings, device counters) are harvested one
        # sample late through pinned async copies — no stream syncs
        self._metrics_every = max(1, int(os.environ.get("PA_METRICS_EVERY", "64")))
        self._batch_counter = 0
        self._update_counter = 0
        self._pending_metric = None
        self._skipped_last = (0, 0)
        self._evicted_last = 0
        self.monitor = None
        if self.metrics_enabled:
            from persia_amd.core.monitor import DistinctIdMonitor

            self.monitor = DistinctIdMonitor()
        self.incremental = None
        if gconf.enable_incremental_update:
            # config-driven (reference inc-update lib.rs:79-120: the train
            # side starts the manager from the global config)
            self.enable_incremental_update(
                gconf.incremental_dir, gconf.incremental_buffer_size
            )

    def enable_incremental_update(self, dst_dir: str,
                                  buffer_size: int = 1_000_000):
        """Attach an incremental-update dumper: every gradient update's
        touched signs are recorded automatically and packets flush when the
        dedup buffer fills (reference inc-update lib.rs:178-312)."""
        from persia_amd.core.incremental import IncrementalUpdateDumper

        self.incremental = IncrementalUpdateDumper(self, dst_dir, buffer_size)
        return self.incremental

    @functools.cached_property
    def _C(self):
        """The HIP extension, imported on first use: CPU-only hosts import
        this module (and run the CPU engine) without it."""
        from persia_amd.ops import native

        return native()

    def _tick(self, key: str, t0: float) -> float:
        """Producer timing (PA_PROD_TIMING=1, callers test ``_prod_timing``):
        add the time since ``t0`` to ``_pt[key]`` unless the warm-up skip is
        still running; -> now, the next stage's ``t0``."""
        now = time.perf_counter()
        if self._prod_timing_live:
            self._pt[key] = self._pt.get(key, 0.0) + (now - t0)
        return now

    @staticmethod
    def _materialize_group(group: "_GroupCtx") -> "_GroupCtx":
        """Resolve a padded sync-free dedup group (fast path: uniq/ustarts are
        nnz-padded, true count on-device) to exact host shapes.  Costs one
        stream sync — only rare paths (raw grads, f32/large-dim fallback,
        skipped-grad groups) need it; the fused kernels read the count from
        the device."""
        if group.u_count is None:
            return group
        U = int(group.u_count.item())
        group.uniq_keys = group.uniq_keys.narrow(0, 0, U)
        group.ustarts = group.ustarts.narrow(0, 0, U + 1)
        group.u_count = None
        return group

    # ------------------------------------------------------------- sign prep

    def _prepare_slot_keys(self, feat) -> Tuple[np.ndarray, np.ndarray]:
        """raw uint64 ids -> prepared (mixed keys u64[nnz'], offsets i64[B+1]).
        Applies hashstack folding then feature-group prefix then splitmix64
        (reference: mod.rs:348-429 + sign_to_shard hashing)."""
        cfg = self.schema.get_slot(feat.name)
        values, offsets = feat.values, feat.offsets
        rounds = cfg.hash_stack_rounds
        if rounds > 0:
            stacked = hashing.hash_stack(
                values, rounds, cfg.hash_stack_config.embedding_size
            )  # (rounds, nnz)
            # per-sample segments repeat each position `rounds` times;
            # interleave position-major so each sample's span stays contiguous:
            # new position layout = for each sample, [r0 ids..., r1 ids..., ...]
            B = len(offsets) - 1
            lens = offsets[1:] - offsets[:-1]
            new_vals = np.empty(len(values) * rounds, dtype=np.uint64)
            new_offsets = np.zeros(B + 1, dtype=np.int64)
            np.cumsum(lens * rounds, out=new_offsets[1:])
            for r in range(rounds):
                for b in range(B):
                    s, e = offsets[b], offsets[b + 1]
                    dst = new_offsets[b] + r * (e - s)
                    new_vals[dst : dst + (e - s)] = stacked[r, s:e]
            values, offsets = new_vals, new_offsets
        signs = hashing.apply_prefix(values, cfg.index_prefix, self.schema.feature_spacing)
        keys = hashing.splitmix64(signs)
        keys[keys == np.uint64(0)] = np.uint64(0xD1B54A32D192ED03)
        return keys, offsets

    # ---------------------------------------------------------------- lookup

    def _exchange_rows(self, group: _GroupCtx, train: bool) -> torch.Tensor:
        """uniq keys -> rows [U, dim] (wire dtype on GPU path, f32 on CPU)."""
        store = self.stores[group.dim]
        if not self.dist.distributed:
            rows = store.lookup(group.uniq_keys, train, u_count=group.u_count)
            return rows
        owner = _owner_of_keys(group.uniq_keys, self.dist.world_size)
        send_counts = torch.bincount(owner, minlength=self.dist.world_size).tolist()
        recv_counts = self.dist.all_to_all_lengths(send_counts, self.device)
        group.send_counts, group.recv_counts = send_counts, recv_counts
        recv_keys = self.dist.all_to_all(group.uniq_keys, send_counts, recv_counts)
        rows_local = store.lookup(recv_keys, train).to(self.wire_dtype)
        rows = self.dist.all_to_all(rows_local, recv_counts, send_counts)
        return rows

    # ------------------------------------- padded even-a2a (fused distributed)

    def _a2a_setup(self, plan: "_GroupPlan") -> Tuple[int, int]:
        """One-time per-plan constants for the capacity-padded a2a.

        Every rank sends each peer a fixed ``cap``-row bucket (padding key 0 =
        "no entry"), so the variable per-destination counts NEVER reach the
        host — no ``.tolist()`` syncs in the hot loop (the reference's RPC
        naturally carried lengths; RCCL ``all_to_all_single`` with even splits
        is the xGMI-native equivalent).  Keys are hash-mixed ⇒ per-owner
        counts concentrate at nnz/world (binomial, σ≈√(nnz/world)); the slack
        of max(512, per/8) puts overflow beyond ~20σ.  A one-time allreduce
        verifies all ranks agree on nnz (weak scaling keeps shapes equal)."""
        if plan.a2a_cap is not None:
            return plan.a2a_world, plan.a2a_cap
        world = self.dist.world_size
        nnz = plan.S * plan.B
        if world > 1:
            lo, hi = self.dist.allreduce_int_minmax(nnz)
            if lo != hi:
                raise RuntimeError(
                    f"padded-a2a fast path needs equal per-rank batch shapes "
                    f"(nnz min {lo} != max {hi}); set PA_FUSED_DIST=0"
                )
            per = max(1, nnz // world)
            cap = per + max(512, per // 8)
        else:
            cap = nnz  # forced single-rank exercise: exact fit
        plan.a2a_world = world
        plan.a2a_cap = cap
        plan.a2a_ar = torch.arange(nnz, dtype=torch.int64, device=self.device)
        plan.a2a_ones = torch.ones(nnz, dtype=torch.int64, device=self.device)
        plan.owner_seg_id = torch.arange(
            world * cap, dtype=torch.int64, device=self.device
        )
        return world, cap

    def _a2a_route(self, plan: "_GroupPlan", uniq: torch.Tensor,
                   u_count: Optional[torch.Tensor]):
        """uniq (sorted, possibly nnz-padded with key 0) -> (send_keys
        [world*cap + 1] with per-owner buckets zero-padded, idx [len(uniq)]
        mapping each unique to its send slot; invalid/overflow -> the dummy
        tail slot).  Pure device ops — sync-free."""
        world, cap = plan.a2a_world, plan.a2a_cap
        if self.device.type == "cuda":
            # fused route: one bounds kernel (the owner partition of the
            # sorted keys is a range partition -> binary searches) + one
            # packed scatter — replaces the ~10-dispatch torch chain below
            # (measured 0.51 ms/batch of producer issue time)
            return self._C.a2a_route(
                uniq,
                u_count if u_count is not None
                else self.stores[plan.dim].no_count,
                world, cap, self._a2a_overflow,
            )
        n = uniq.numel()
        ar = plan.a2a_ar[:n]
        owner = _owner_of_keys(uniq, world)
        if u_count is not None:
            # padding tail (key 0) routes to the invalid bucket `world`
            owner = torch.where(ar < u_count, owner,
                                torch.full_like(owner, world))
        # NOT torch.bincount: its CUDA kernel sizes the histogram via
        # input.max().item() — a hidden device sync that would stall the
        # producer thread behind the whole lookup-stream backlog
        counts = torch.zeros(world + 1, dtype=torch.int64, device=uniq.device)
        counts.scatter_add_(0, owner, plan.a2a_ones[:n])
        starts = torch.cumsum(counts, 0) - counts
        pos = ar - starts.gather(0, owner)
        dummy = world * cap
        bad = (owner >= world) | (pos >= cap)
        idx = torch.where(bad, torch.full_like(pos, dummy), owner * cap + pos)
        send = torch.zeros(dummy + 1, dtype=torch.int64, device=uniq.device)
        send.scatter_(0, idx, uniq)
        # dropped keys, the unit the native route counts in
        self._a2a_overflow.add_((counts[:world] - cap).clamp(min=0).sum())
        return send, idx

    @_roctx_range("persia:a2a_exchange")
    def _a2a_exchange_fwd(self, plan: "_GroupPlan", group: _GroupCtx,
                          train: bool):
        """Padded forward exchange: route keys -> even a2a -> owner lookup in
        wire dtype -> even a2a back.  Returns (rows_full [world*cap+1, dim]
        with a zero dummy tail row, idx).  Fills group.a2a_* for backward."""
        world, cap = self._a2a_setup(plan)
        timing = self._prod_timing
        if timing:
            t = time.perf_counter()
        send_keys, idx = self._a2a_route(plan, group.uniq_keys, group.u_count)
        comm = self.dist
        if world > 1:
            recv_keys = comm.all_to_all_even(send_keys[: world * cap])
        else:
            recv_keys = send_keys[: world * cap].clone()
        if timing:
            t = self._tick("route", t)
        store = self.stores[group.dim]
        rows_local = store.lookup_wire(recv_keys, train, self.wire_dtype)
        if timing:
            self._tick("lkw", t)
        rows_full = torch.empty(
            world * cap + 1, group.dim, dtype=rows_local.dtype,
            device=self.device,
        )
        if world > 1:
            comm.all_to_all_even(rows_local, out=rows_full[: world * cap])
        else:
            rows_full[: world * cap].copy_(rows_local)
        rows_full[world * cap].zero_()
        group.a2a_plan = plan
        group.a2a_idx = idx
        group.a2a_recv_keys = recv_keys
        if train and self.device.type == "cuda":
            # owner-side dedup for the backward merge, issued HERE so the
            # sort overlaps the dense step on the pipeline stream (the fused
            # a2a_route freed the producer budget this costs);
            # _a2a_backward_native falls back lazily if absent (infer skips)
            group.a2a_owner_dedup = tuple(self._C.dedup_padded(recv_keys))
        return rows_full, idx

    def check_a2a_overflow(self) -> int:
        """Keys dropped so far because their per-owner bucket was over `cap`
        (they went to the dummy slot: rows read as zeros, grads discarded);
        the same unit on the native and the CPU route.  Non-zero means the
        slack heuristic failed — syncs the device."""
        return int(self._a2a_overflow.sum().item())

    # ---------------------------------------------------------- forward path

    @_roctx_range("persia:process_batch")
    def process_batch(self, batch: PersiaBatch, train: Optional[bool] = None) -> PersiaTrainingBatch:
        if self._prod_timing:
            # timers skip the first batches (see _pt in __init__)
            self._prod_timing_live = self._pt["skip"] <= 0
            if not self._prod_timing_live:
                self._pt["skip"] -= 1
            _tb0 = time.perf_counter()
        self._batch_counter += 1
        sample = (
            self.metrics_enabled
            and self._batch_counter % self._metrics_every == 1 % self._metrics_every
        )
        if sample:
            _ms_t0 = time.perf_counter()
            _ms_ev0 = None
            if self.device.type == "cuda":
                _ms_ev0 = torch.cuda.Event(enable_timing=True)
                _ms_ev0.record()
        train = batch.requires_grad if train is None else train
        if self.gconf.job_type == "infer":
            train = False
        out = PersiaTrainingBatch()
        out.batch_size = batch.batch_size
        out.requires_grad = batch.requires_grad
        out.meta = batch.meta
        out.batch_id = batch.batch_id
        out._engine = self

        for i, x in enumerate(batch.non_id_type_features):
            out.non_id_type_tensors.append(
                self._upload_aux(batch, ("nid", i), x.data)
            )
        for i, x in enumerate(batch.labels):
            out.label_tensors.append(self._upload_aux(batch, ("lab", i), x.data))

        for dim, feats in self._feats_by_dim(batch).items():
            out._groups.append(self._process_group(dim, feats, out, train, batch))
        # keep payloads in the original id_type_features order (applied
        # lazily when .payloads is first materialized)
        out._order = {f.name: i for i, f in enumerate(batch.id_type_features)}
        out._sorted = False
        if sample:
            self._record_lookup_metrics(batch, out, _ms_t0, _ms_ev0)
        if self._prod_timing and self._prod_timing_live:
            self._tick("batch", _tb0)
            self._pt["n"] += 1
        return out

    def _record_lookup_metrics(self, batch, out, t0: float, ev0) -> None:
        """Sampled hot-path observability (reference worker/PS gauges,
        embedding_worker_service/mod.rs:83-100, parameter mod.rs:27-79).
        Device-side values are harvested one sample late (events/pinned
        copies complete by then) so this never synchronizes a stream."""
        m = self.metrics
        # host producer time of this batch (prep + kernel issue + any waits)
        m.lookup_preprocess_time_cost_sec.set(time.perf_counter() - t0)
        # distinct-id estimates from the raw host-side id arrays
        # (reference monitor.rs:29-114 samples the same point: pre-dedup ids)
        if self.monitor is not None:
            for feat in batch.id_type_features:
                vals = getattr(feat, "values", None)
                if vals is not None and len(vals):
                    self.monitor.observe(feat.name, vals)
            for name, est in self.monitor.estimates().items():
                m.distinct_id_estimate.labels(name).set(est)
        # unique-indices rate: exact on CPU; via the deferred u_count pinned
        # copy on GPU (padded dedup keeps U device-side)
        nnz = sum(
            len(getattr(f, "values", ())) for f in batch.id_type_features
        )
        # harvest the PREVIOUS sample's deferred device-side values
        pend = self._pending_metric
        self._pending_metric = None
        if pend is not None:
            ev_a, ev_b, ucnt_pin, skip_pin, p_nnz, done = pend
            if done.query():
                if ev_a is not None and ev_b is not None:
                    try:
                        m.lookup_hashmap_time_cost_sec.set(
                            ev_a.elapsed_time(ev_b) / 1e3
                        )
                    except Exception:
                        pass
                if ucnt_pin is not None and p_nnz:
                    m.batch_unique_indices_rate.set(
                        float(ucnt_pin.item()) / p_nnz
                    )
                if skip_pin is not None:
                    miss, nan = int(skip_pin[0].item()), int(skip_pin[1].item())
                    lm, ln = self._skipped_last
                    if miss > lm:
                        m.gradient_id_miss_count.inc(miss - lm)
                    if nan > ln:
                        m.nan_grad_skipped.inc(nan - ln)
                    self._skipped_last = (miss, nan)
        if self.device.type == "cuda":
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record()
            ucnt_pin = None
            for g in out._groups:
                if g.u_count is not None:
                    ucnt_pin = torch.empty(1, dtype=torch.int64, pin_memory=True)
                    ucnt_pin.copy_(g.u_count, non_blocking=True)
                    break
                # exact dedup: U known host-side without a sync
                m.batch_unique_indices_rate.set(
                    g.uniq_keys.numel() / max(1, nnz)
                )
            skip_pin = None
            skipped = next(iter(self.stores.values())).skip_counters()
            if skipped is not None:
                skip_pin = torch.empty(2, dtype=torch.int32, pin_memory=True)
                skip_pin.copy_(skipped, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            self._pending_metric = (ev0, ev1, ucnt_pin, skip_pin, nnz, done)
        else:
            U = sum(g.uniq_keys.numel() for g in out._groups)
            m.batch_unique_indices_rate.set(U / max(1, nnz))
            m.nan_grad_skipped.inc(0)
        # eviction counter (host-side total maintained by the spill drain)
        ev_tot = sum(
            getattr(s, "evicted_total", 0) for s in self.stores.values()
        )
        if ev_tot > self._evicted_last:
            m.evicted_count.inc(ev_tot - self._evicted_last)
            self._evicted_last = ev_tot

    def prepare_host_batch(self, batch: PersiaBatch) -> None:
        """Build a batch's pinned staging buffers host-side, without touching
        the GPU streams.  The first visit of a batch otherwise pays
        hipHostMalloc + copy inside the pipeline thread — ms-scale when the
        host is still reclaiming a prior process's pinned pages, which
        dominates short timed runs.  Idempotent; safe to call from the data
        producer (the reference allocates its pinned pools at startup for the
        same reason, cuda/pinned_memory_pool.rs)."""
        if self.device.type != "cuda":
            return
        pc = getattr(batch, "_pinned_cache", None)
        if pc is None:
            pc = batch._pinned_cache = {}
        for kind, items in (("nid", batch.non_id_type_features),
                            ("lab", batch.labels)):
            for i, x in enumerate(items):
                if (kind, i) not in pc:
                    pc[(kind, i)] = self._pin_array(x.data)
        for dim, feats in self._feats_by_dim(batch).items():
            if self._all_single_sum(feats):
                if dim not in pc:
                    pc[dim] = self._pin_values(feats)
            elif self._bag_group(dim, feats):
                self._stack_host_buffer(batch, dim, feats)
            elif self._raw_group(dim, feats):
                self._bag_host_buffer(
                    batch, dim, self._sums_first(feats), kind="raw"
                )

    def _feats_by_dim(self, batch: PersiaBatch) -> Dict[int, List]:
        """A batch's id features by dim-group (one store + one a2a each)."""
        by_dim: Dict[int, List] = {}
        for feat in batch.id_type_features:
            by_dim.setdefault(self.schema.get_slot(feat.name).dim, []).append(feat)
        return by_dim

    @staticmethod
    def _pin_array(arr: np.ndarray) -> torch.Tensor:
        src = torch.from_numpy(np.ascontiguousarray(arr))
        t = torch.empty_like(src, pin_memory=True)
        t.copy_(src)
        return t

    def _upload_aux(self, batch, cache_key, arr: np.ndarray) -> torch.Tensor:
        """Dense-feature/label upload: pageable H2D stalls the pipeline
        thread ~0.1-0.2ms per batch, so stage through a per-batch pinned
        buffer (repeat visits are a pure async copy)."""
        if self.device.type != "cuda":
            return torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)
        pc = getattr(batch, "_pinned_cache", None)
        if pc is None:
            pc = batch._pinned_cache = {}
        t = pc.get(cache_key)
        if t is None:
            t = pc[cache_key] = self._pin_array(arr)
        return t.to(self.device, non_blocking=True)

    def _pin_values(self, feats) -> torch.Tensor:
        """A group's raw ids, concatenated into a fresh pinned i64 buffer."""
        values_np = np.concatenate([f.values for f in feats])
        pin = torch.empty(len(values_np), dtype=torch.int64, pin_memory=True)
        pin.numpy()[:] = values_np.view(np.int64)
        return pin

    def _upload_group(self, dim: int, feats, batch) -> torch.Tensor:
        """One async H2D of a fast-path group's raw ids through the batch's
        pinned staging (allocated once per PersiaBatch, like a loader-side
        pinned pool: repeat visits are a pure async copy; pageable uploads
        stall the lookup thread ~0.2ms/batch)."""
        pcache = getattr(batch, "_pinned_cache", None)
        if pcache is None:
            pcache = batch._pinned_cache = {}
        pin = pcache.get(dim)
        if pin is None:
            pin = pcache[dim] = self._pin_values(feats)
        return pin.to(self.device, non_blocking=True)

    def _all_single_sum(self, feats) -> bool:
        """The fast-path shape (flagship DLRM): every feature carries one id
        per sample and is a sum slot without hashstack."""
        get_slot = self.schema.get_slot
        for f in feats:
            if not getattr(f, "is_single", False):
                return False
            cfg = get_slot(f.name)
            if not cfg.embedding_summation or cfg.hash_stack_rounds != 0:
                return False
        return True

    def _bag_group(self, dim: int, feats) -> bool:
        """The bag-path shape: a single-GPU native group (the one-call
        condition of _process_group_fast) of sum slots, at least one of them
        with several ids per sample or with hashstack rounds (each id of such
        a slot becomes ``rounds`` positions: a bag even when the feature
        carries one id per sample), and PA_BAG_FAST on.  All-single-ID groups
        without a stacked slot keep their own path and its static plan; a
        group with a raw slot is never a bag group."""
        if not (self._bag_fast and self._one_call(dim)):
            return False
        get_slot = self.schema.get_slot
        stacked = False
        for f in feats:
            cfg = get_slot(f.name)
            if not cfg.embedding_summation or cfg.hash_stack_rounds < 0:
                return False
            stacked = stacked or cfg.hash_stack_rounds > 0
        return stacked or not all(
            getattr(f, "is_single", False) for f in feats
        )

    def _one_call(self, dim: int) -> bool:
        """A group of this dim can be looked up in one native call: CUDA
        device, a store with the fused entry points, not distributed (nor
        PA_FORCE_DIST), no spill tier."""
        store = self.stores[dim]
        return (
            self.device.type == "cuda"
            and store.fused_native
            and not (self.dist.distributed or self._force_dist)
            and store.spill is None
        )

    def _raw_group(self, dim: int, feats) -> bool:
        """The raw-path shape: a one-call group (_one_call) with at least one
        raw slot, no slot (sum or raw) with hashstack rounds, and PA_RAW_FAST
        on.  Its sum slots ride along, single-ID or bags."""
        if not (self._raw_fast and self._one_call(dim)):
            return False
        cfgs = [self.schema.get_slot(f.name) for f in feats]
        return any(not c.embedding_summation for c in cfgs) and all(
            c.hash_stack_rounds == 0 for c in cfgs
        )

    def _sums_first(self, feats) -> List:
        """A group's features, sum slots first, then raw slots; each part in
        its incoming order."""
        return sorted(
            feats,
            key=lambda f: not self.schema.get_slot(f.name).embedding_summation,
        )

    def _bag_host_buffer(self, batch, dim: int, feats, kind: str = "bag"):
        """A bag group's staging buffer (pack_bag_buffer), built and checked
        once per (batch, dim-group) and kept in the batch's pinned cache under
        ``(kind, dim)``: -> (i64 tensor, nnz, B).  Pinned on the GPU path."""
        pc = getattr(batch, "_pinned_cache", None)
        if pc is None:
            pc = batch._pinned_cache = {}
        hit = pc.get((kind, dim))
        if hit is None:
            made = []

            def alloc(n: int) -> np.ndarray:
                made.append(torch.empty(
                    n, dtype=torch.int64,
                    pin_memory=self.device.type == "cuda",
                ))
                return made[0].numpy()

            _buf, nnz, B = pack_bag_buffer(feats, alloc)
            hit = pc[(kind, dim)] = (made[0], nnz, B)
        return hit

    def _stack_host_buffer(self, batch, dim: int, feats):
        """The staging buffer of a bag group that may hold hashstack slots,
        -> (i64 tensor, nnz_in, nnz_out, B).  Without a stacked slot it is
        _bag_host_buffer's (nnz_out == nnz_in); with one it is
        pack_stack_bag_buffer's, built, checked and cached the same way under
        the same ``("bag", dim)``, the two counts in the cached tuple."""
        rounds, sizes = _stack_config(
            [self.schema.get_slot(f.name) for f in feats]
        )
        if not any(rounds):
            pin, nnz, B = self._bag_host_buffer(batch, dim, feats)
            return pin, nnz, nnz, B
        pc = getattr(batch, "_pinned_cache", None)
        if pc is None:
            pc = batch._pinned_cache = {}
        hit = pc.get(("bag", dim))
        if hit is None:
            made = []

            def alloc(n: int) -> np.ndarray:
                made.append(torch.empty(
                    n, dtype=torch.int64,
                    pin_memory=self.device.type == "cuda",
                ))
                return made[0].numpy()

            _buf, nnz_in, nnz_out, B = pack_stack_bag_buffer(
                feats, rounds, sizes, alloc
            )
            hit = pc[("bag", dim)] = (made[0], nnz_in, nnz_out, B)
        return hit

    def _padded_a2a(self, store) -> bool:
        """Rows travel over the capacity-padded even a2a (not the two-phase
        counts exchange): distributed, or PA_FORCE_DIST at one rank, with
        PA_FUSED_DIST on and no spill tier."""
        return (
            (self.dist.distributed or self._force_dist)
            and self._fused_dist
            and store.spill is None
        )

    def _plan(self, dim: int, names: Tuple[str, ...], B: int) -> _GroupPlan:
        plan = self._plans.get((dim, names, B))
        if plan is None:
            cfgs = [self.schema.get_slot(n) for n in names]
            plan = self._plans[(dim, names, B)] = _GroupPlan(
                dim, cfgs, B, self.device
            )
        return plan

    def _process_group_fast(self, dim: int, feats, out: PersiaTrainingBatch,
                            train: bool, batch: PersiaBatch) -> _GroupCtx:
        """All-single-ID sum-slot fast path on a static device-side plan:
        upload -> keys -> dedup -> rows -> sums -> group, ~15 kernel launches.
        Three variants replace stages of that chain: one native call for all
        of it, the front half on the spill probe stream, rows over the padded
        a2a."""
        timing = self._prod_timing
        if timing:
            t0 = time.perf_counter()
        C = self._C
        B = len(feats[0].values)
        plan = self._plan(dim, tuple(f.name for f in feats), B)
        slot_ctxs = [
            _SlotCtx(
                name=f.name, cfg=self.schema.get_slot(f.name),
                pos_slice=(i * B, (i + 1) * B), seg_offsets=None,
                sum_seg_base=i * B,
            )
            for i, f in enumerate(feats)
        ]
        store = self.stores[dim]
        dist = self.dist.distributed
        one_call = not (dist or self._force_dist or store.spill is not None)
        padded = not one_call and self._padded_a2a(store)
        if one_call:
            # upload..sums in ONE native call (C++ drives sign prep, dedup,
            # probe/insert, gather and the fused segment-sum)
            if timing:
                t0 = self._tick("prep", t0)
            (sums, uniq, inverse, perm, ustarts, u_count, slot_hint,
             src_hint) = store.lookup_local(
                self._upload_group(dim, feats, batch), plan.slot_starts,
                plan.prefixes, self._spacing_arg, plan.cat_offsets,
                plan.empty_scale,
                plan.seg_id if train and self._update_hints else self._no_seg,
                train,
            )
        else:
            # spill tier (single GPU, training): upload..dedup plus the
            # restore of spilled rows run on a dedicated probe stream, so the
            # miss-mask readback in spill_restore waits only for this batch's
            # tiny probe work, not the lookup stream's multi-batch backlog
            # (the dcn-spill ~1.9 ms/batch producer stall)
            ps = cur = None
            if store.spill is not None and not dist and train:
                ps, cur = store.probe_stream, torch.cuda.current_stream()
            with torch.cuda.stream(ps) if ps is not None else _NO_STREAM:
                vals_t = self._upload_group(dim, feats, batch)
                keys_t = C.sign_prep(
                    vals_t, plan.slot_starts, plan.prefixes, self._spacing_arg
                )
                if padded or not dist:
                    # sync-free padded dedup: the fused distributed exchange
                    # and the single-GPU store read the unique count on-device
                    uniq, inverse, perm, ustarts, u_count = C.dedup_padded(keys_t)
                else:
                    uniq, inverse, perm, ustarts = _dedup(keys_t)
                    u_count = None
                if ps is not None:
                    store.spill_restore(uniq, u_count)
            if ps is not None:
                cur.wait_stream(ps)
                for x in (vals_t, uniq, inverse, perm, ustarts, u_count):
                    x.record_stream(cur)
        group = _GroupCtx(
            dim=dim, uniq_keys=uniq, inverse=inverse, perm=perm,
            ustarts=ustarts, u_count=u_count, slots=slot_ctxs,
            cat_offsets=plan.cat_offsets, seg_id=plan.seg_id,
            n_sum_slots=plan.S,
        )
        if one_call:
            if slot_hint.numel():  # both empty when none were asked for
                group.slot_hint, group.src_hint = slot_hint, src_hint
        if padded:
            # rows over the capacity-padded even a2a (no host count syncs
            # anywhere); the unpack gather is composed into `inverse` so
            # segment_sum reads the recv buffer directly — no [nnz, dim] rows
            if timing:
                t = self._tick("dedup", t0)
            rows_full, idx = self._a2a_exchange_fwd(plan, group, train)
            if timing:
                t = self._tick("exch", t)
            sums = C.segment_sum(
                rows_full, idx.gather(0, inverse), plan.cat_offsets,
                plan.empty_scale,
            )
            if timing:
                self._tick("sum", t)
        elif not one_call:
            rows = self._exchange_rows(group, train)
            sums = C.segment_sum(
                rows.contiguous(), inverse, plan.cat_offsets, plan.empty_scale
            )
        group.sum_base = sums
        # SlotPayload construction is deferred: consumers on the fused path
        # read group.sum_base directly (~2*n_slots python objects per batch)
        out._lazy_sum_groups.append((group, [sc.name for sc in slot_ctxs], B))
        if timing and (one_call or padded):
            self._tick("native", t0)
        return group

    def _process_group_bags(self, dim: int, feats, out: PersiaTrainingBatch,
                            train: bool, batch: PersiaBatch) -> _GroupCtx:
        """Bag path: sum slots with any number of ids per sample (a single-ID
        slot is a bag of length 1, a slot of R hashstack rounds a bag of R
        positions per id), single GPU.  One async upload of the unexpanded
        values and the offsets, one native call for sign prep (with the
        hashstack expansion), padded dedup, the segment plan, probe/insert
        and the sums read straight from the arena.  No host sync between the
        upload and the return.  The group it leaves is what the generic path
        leaves, positions and offsets in the expanded space, with the unique
        count on the device."""
        timing = self._prod_timing
        if timing:
            t0 = time.perf_counter()
        pin, nnz_in, nnz, B = self._stack_host_buffer(batch, dim, feats)
        names = tuple(f.name for f in feats)
        plan = self._plans.get(("bag", dim, names, B))
        if plan is None:
            plan = self._plans[("bag", dim, names, B)] = _BagPlan(
                dim, [self.schema.get_slot(n) for n in names], B, self.device
            )
        S = plan.S
        upload = pin.to(self.device, non_blocking=True)
        if timing:
            t0 = self._tick("prep", t0)
        (sums, uniq, inverse, perm, ustarts, u_count, slot_hint, src_hint,
         cat_offsets, seg_id, seg_lens, fwd_scale) = self.stores[
            dim
        ].lookup_local_bags(
            upload, nnz_in, S, B, plan.prefixes, self._spacing_arg,
            plan.sqrt_flags, train and self._update_hints, train,
            rounds=plan.rounds, sizes=plan.sizes, nnz_out=nnz,
            stack_dev=plan.stack_dev,
        )
        # per-slot views of the upload: positions on the host, offsets on
        # the device (both in the expanded space of a stacked group)
        starts = pin.numpy()[nnz_in : nnz_in + S + 1]
        offsets = upload[
            nnz_in + S + 1 : nnz_in + S + 1 + S * (B + 1)
        ].view(S, B + 1)
        slot_ctxs = [
            _SlotCtx(
                name=f.name, cfg=self.schema.get_slot(f.name),
                pos_slice=(int(starts[i]), int(starts[i + 1])),
                seg_offsets=offsets[i], sum_seg_base=i * B,
            )
            for i, f in enumerate(feats)
        ]
        group = _GroupCtx(
            dim=dim, uniq_keys=uniq, inverse=inverse, perm=perm,
            ustarts=ustarts, u_count=u_count, slots=slot_ctxs,
            cat_offsets=cat_offsets, seg_id=seg_id, seg_lens=seg_lens,
            sqrt_mask=plan.sqrt_mask, sum_base=sums, n_sum_slots=S,
            has_sqrt=plan.has_sqrt, fwd_scale=fwd_scale,
        )
        if slot_hint.numel():  # both empty when none were asked for
            group.slot_hint, group.src_hint = slot_hint, src_hint
        out._lazy_sum_groups.append((group, list(names), B))
        if timing:
            self._tick("native", t0)
        return group

    def _process_group_raw(self, dim: int, feats, out: PersiaTrainingBatch,
                           train: bool, batch: PersiaBatch) -> _GroupCtx:
        """Raw path: a single-GPU group with raw (sequence) slots, whose sum
        slots (single-ID or bags) ride along.  The bag path's upload over all
        the slots, sum slots first, and one native call that also writes each
        raw slot's fixed-size ``(B, sfs, dim)`` rows and mask straight from
        the arena.  No host sync.  ``sum_base`` of the group it leaves is the
        whole leaf base: the sum segments, then every raw slot's cell rows,
        which ``seg_id`` sends the raw positions to (-1 past sfs), so
        ``update_local`` takes the group as it takes a bag group."""
        timing = self._prod_timing
        if timing:
            t0 = time.perf_counter()
        feats = self._sums_first(feats)
        pin, nnz, B = self._bag_host_buffer(batch, dim, feats, kind="raw")
        names = tuple(f.name for f in feats)
        plan = self._plans.get(("raw", dim, names, B))
        if plan is None:
            plan = self._plans[("raw", dim, names, B)] = _RawPlan(
                dim, [self.schema.get_slot(n) for n in names], B, self.device
            )
        S, n_slots = plan.S, len(feats)
        upload = pin.to(self.device, non_blocking=True)
        if timing:
            t0 = self._tick("prep", t0)
        (base, mask, uniq, inverse, perm, ustarts, u_count, slot_hint,
         src_hint, cat_offsets, seg_id, seg_lens, fwd_scale,
         raw_num) = self.stores[dim].lookup_local_raw(
            upload, nnz, S, B, plan.prefixes, self._spacing_arg,
            plan.sqrt_flags, plan.raw_meta, plan.sfs,
            train and self._update_hints, train,
        )
        starts = pin.numpy()[nnz : nnz + n_slots + 1]
        offsets = upload[nnz + n_slots + 1 :].view(n_slots, B + 1)
        slot_ctxs = []
        for i, f in enumerate(feats):
            sc = _SlotCtx(
                name=f.name, cfg=self.schema.get_slot(f.name),
                pos_slice=(int(starts[i]), int(starts[i + 1])),
                seg_offsets=offsets[i],
            )
            if i < S:
                sc.sum_seg_base = i * B
            else:
                sc.raw_row_base = plan.row_bases[i - S]
                sc.raw_sfs = plan.sfs[i - S]
            slot_ctxs.append(sc)
        group = _GroupCtx(
            dim=dim, uniq_keys=uniq, inverse=inverse, perm=perm,
            ustarts=ustarts, u_count=u_count, slots=slot_ctxs,
            cat_offsets=cat_offsets, seg_id=seg_id, seg_lens=seg_lens,
            sqrt_mask=plan.sqrt_mask, sum_base=base, n_sum_slots=S,
            has_sqrt=plan.has_sqrt, fwd_scale=fwd_scale, raw_mask=mask,
            raw_num=raw_num,
        )
        if slot_hint.numel():  # both empty when none were asked for
            group.slot_hint, group.src_hint = slot_hint, src_hint
        out._lazy_sum_groups.append((group, list(names), B))
        if timing:
            self._tick("native", t0)
        return group

    def _process_group(self, dim: int, feats, out: PersiaTrainingBatch, train: bool,
                       batch: PersiaBatch) -> _GroupCtx:
        native = self.device.type == "cuda"
        fast_shape = self._all_single_sum(feats)
        if native and fast_shape:
            return self._process_group_fast(dim, feats, out, train, batch)
        if self._bag_group(dim, feats):
            return self._process_group_bags(dim, feats, out, train, batch)
        if self._raw_group(dim, feats):
            return self._process_group_raw(dim, feats, out, train, batch)
        # sum slots first so they occupy a contiguous prefix of the position
        # space (one fused segment-sum launch for the whole group)
        feats = sorted(
            feats, key=lambda f: 0 if self.schema.get_slot(f.name).embedding_summation else 1
        )
        keys_t, slot_ctxs = self._group_keys(feats, gpu_prep=native)
        uniq_keys, inverse, perm, ustarts = _dedup(keys_t)
        group = _GroupCtx(
            dim=dim, uniq_keys=uniq_keys, inverse=inverse, perm=perm,
            ustarts=ustarts, slots=slot_ctxs,
        )
        if not native and fast_shape and self._padded_a2a(self.stores[dim]):
            # CPU mirror of the GPU fused distributed path: same capacity-padded
            # even-a2a routing math, exact (unpadded) dedup — this is what the
            # gloo multi-process tests exercise so the 8-GPU driver run's code
            # path has CPU coverage
            plan = self._plan(
                dim, tuple(sc.name for sc in slot_ctxs), out.batch_size
            )
            rows_full, idx = self._a2a_exchange_fwd(plan, group, train)
            rows = rows_full[idx]
        else:
            rows = self._exchange_rows(group, train)  # [U, dim]
        self._sum_payloads(group, rows, out)
        self._raw_payloads(group, rows, out)
        return group

    def _group_keys(self, feats, gpu_prep: bool):
        """Generic path, stage 1: -> (mixed keys i64[nnz'] on the device in
        slot order, one _SlotCtx per feature with its position slice and
        per-sample offsets).  CPU: sign prep on the host; GPU: raw ids are
        uploaded and hashstack expansion + prefix + mix run in one kernel."""
        dev = self.device
        key_arrays = []
        offset_arrays = []
        slot_ctxs: List[_SlotCtx] = []
        in_lens: List[int] = []      # uploaded (pre-expansion) lengths
        rounds_list: List[int] = []  # hashstack rounds per slot (GPU prep)
        sizes_list: List[int] = []
        pos = 0  # OUTPUT (post-hashstack-expansion) position space
        for feat in feats:
            cfg = self.schema.get_slot(feat.name)
            r = cfg.hash_stack_rounds
            if gpu_prep:
                # expanded seg offsets are exactly offsets*r (every segment
                # grows by the same factor)
                keys = feat.values
                offsets = feat.offsets * r if r > 0 else feat.offsets
                out_len = len(keys) * max(r, 1)
            else:
                keys, offsets = self._prepare_slot_keys(feat)
                out_len = len(keys)
            key_arrays.append(keys)
            offset_arrays.append(offsets)
            in_lens.append(len(keys))
            rounds_list.append(r if gpu_prep else 0)
            sizes_list.append(
                cfg.hash_stack_config.embedding_size if r > 0 else 1
            )
            slot_ctxs.append(
                _SlotCtx(name=feat.name, cfg=cfg, pos_slice=(pos, pos + out_len),
                         seg_offsets=None)
            )
            pos += out_len

        all_keys = np.concatenate(key_arrays) if key_arrays else np.empty(0, np.uint64)
        # single H2D upload of the whole group's values + all offsets
        keys_t = torch.from_numpy(all_keys.view(np.int64)).to(dev, non_blocking=False)
        all_offs = np.concatenate(offset_arrays or [np.zeros(1, np.int64)])
        all_offs_t = torch.from_numpy(all_offs).to(dev)
        o0 = 0
        for sc, offs in zip(slot_ctxs, offset_arrays):
            sc.seg_offsets = all_offs_t[o0 : o0 + len(offs)]
            o0 += len(offs)
        if not gpu_prep:
            return keys_t, slot_ctxs
        out_starts = torch.tensor(
            [sc.pos_slice[0] for sc in slot_ctxs] + [pos],
            dtype=torch.int64, device=dev,
        )
        prefixes = torch.from_numpy(
            np.array([sc.cfg.index_prefix for sc in slot_ctxs], dtype=np.uint64)
            .view(np.int64)
        ).to(dev)
        if not any(rounds_list):
            return self._C.sign_prep(
                keys_t, out_starts, prefixes, self._spacing_arg
            ), slot_ctxs
        in_starts = torch.from_numpy(
            np.concatenate([[0], np.cumsum(in_lens)]).astype(np.int64)
        ).to(dev)
        off_starts = torch.from_numpy(
            np.concatenate(
                [[0], np.cumsum([len(o) for o in offset_arrays])]
            ).astype(np.int64)
        ).to(dev)
        keys_t = self._C.sign_prep_stack(
            keys_t, in_starts, out_starts, prefixes,
            torch.tensor(rounds_list, dtype=torch.int32, device=dev),
            torch.tensor(sizes_list, dtype=torch.int64, device=dev),
            off_starts, all_offs_t, self._spacing_arg, pos,
        )
        return keys_t, slot_ctxs

    def _sum_payloads(self, group: _GroupCtx, rows: torch.Tensor,
                      out: PersiaTrainingBatch) -> None:
        """Generic path: fused postprocess of the group's sum slots (one
        segment-sum over their contiguous position prefix) into
        ``group.sum_base`` and one sum payload per slot."""
        sum_slots = [sc for sc in group.slots if sc.cfg.embedding_summation]
        if not sum_slots:
            return
        dev = self.device
        base = 0
        offs_parts, sqrt_parts = [], []
        for sc in sum_slots:
            s, _e = sc.pos_slice
            sc.sum_seg_base = base
            nseg = sc.seg_offsets.numel() - 1
            offs_parts.append(sc.seg_offsets[:-1] + s)
            sqrt_parts.append(
                torch.full((nseg,), bool(sc.cfg.sqrt_scaling), dtype=torch.bool, device=dev)
            )
            base += nseg
        sum_end = sum_slots[-1].pos_slice[1]
        cat_offsets = torch.cat(
            offs_parts + [torch.tensor([sum_end], dtype=torch.int64, device=dev)]
        )
        group.cat_offsets = cat_offsets
        group.sqrt_mask = torch.cat(sqrt_parts)
        seg_counts = cat_offsets[1:] - cat_offsets[:-1]
        group.seg_lens = seg_counts.float()
        seg_id = torch.full(
            (group.inverse.numel(),), -1, dtype=torch.int64, device=dev
        )
        seg_id[:sum_end] = torch.repeat_interleave(
            torch.arange(base, dtype=torch.int64, device=dev), seg_counts
        )
        group.seg_id = seg_id
        fwd_scale = _sqrt_scale(group.sqrt_mask, group.seg_lens)
        if dev.type == "cuda":
            sums = self._C.segment_sum(
                rows.contiguous(), group.inverse, cat_offsets, fwd_scale
            )
        else:
            sums = (
                R.segment_sum_rows(
                    rows, group.inverse[:sum_end], cat_offsets, False, torch.float32
                )
                * fwd_scale.unsqueeze(1)
            ).to(torch.float16)
        group.sum_base = sums
        group.n_sum_slots = len(sum_slots)
        b0 = 0
        for sc in sum_slots:
            nseg = sc.seg_offsets.numel() - 1
            out._payloads.append(
                SlotPayload(name=sc.name, cfg=sc.cfg, sum_tensor=sums[b0 : b0 + nseg])
            )
            b0 += nseg

    def _raw_payloads(self, group: _GroupCtx, rows: torch.Tensor,
                      out: PersiaTrainingBatch) -> None:
        """Generic path: raw slots (torch on both backends: not in the
        flagship loop) -> distinct rows + index tensors per slot."""
        for sc in group.slots:
            if sc.cfg.embedding_summation:
                continue
            s, e = sc.pos_slice
            slot_uniq, slot_inv = torch.unique(
                group.inverse[s:e], sorted=True, return_inverse=True
            )
            sc.slot_uniq_global = slot_uniq
            sc.slot_inverse = slot_inv
            scale = 1.0
            rounds = sc.cfg.hash_stack_rounds
            if sc.cfg.sqrt_scaling and rounds > 1:
                scale = 1.0 / float(np.sqrt(rounds))
            distinct, index, non_empty, num = R.raw_embedding_tensors(
                rows[slot_uniq], slot_inv, sc.seg_offsets, sc.cfg.sample_fixed_size,
                scale, torch.float16,
            )
            out._payloads.append(
                SlotPayload(
                    name=sc.name, cfg=sc.cfg, raw_distinct=distinct, raw_index=index,
                    raw_non_empty_index=non_empty, raw_sample_id_num=num,
                )
            )

    # --------------------------------------------------------- backward path

    def _seg_scale(self, group: _GroupCtx, loss_scale: float,
                   skip: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-segment gradient scale of a group's sum slots: 1/loss_scale,
        times the sqrt-scaling factor, zeroed where ``skip`` (bool per
        segment: a NaN slot's segments).  The empty tensor means all ones.
        A ``skip`` caller builds the tensor anyway, so only the others pay
        the ``any()`` readback that can spare it; a bag group knows on the
        host whether it has a sqrt slot and reuses the forward's scale
        tensor, so it never reads anything back.  For a raw-path group the
        scale covers every row of the leaf base, the raw cells included (the
        update indexes it by gradient row)."""
        mask = group.sqrt_mask
        if group.has_sqrt is not None:
            has_sqrt = group.has_sqrt
        else:
            has_sqrt = mask is not None and (
                skip is not None or bool(mask.any())
            )
        if skip is None and loss_scale == 1.0 and not has_sqrt:
            return self._empty_scale
        n_rows = (
            group.sum_base.shape[0] if group.raw_mask is not None
            else group.cat_offsets.numel() - 1
        )
        scale = torch.full((n_rows,), 1.0 / loss_scale, device=self.device)
        if has_sqrt:
            sqrt_scale = group.fwd_scale
            if sqrt_scale is None:
                sqrt_scale = _sqrt_scale(mask, group.seg_lens)
            scale = scale * sqrt_scale
        if skip is not None:
            scale = torch.where(skip, torch.zeros_like(scale), scale)
        return scale

    def _nan_slot(self, sc: _SlotCtx, g: torch.Tensor) -> bool:
        """Host-side NaN filter of one slot's gradient (reference
        mod.rs:731-746: skip the whole slot)."""
        if not bool(torch.isnan(g).any()):
            return False
        self.nan_grad_batches += 1
        _logger.warning(f"nan found in gradient update of {sc.name}, skipping")
        return True

    def _add_raw_grads(self, group: _GroupCtx, grads, loss_scale: float,
                       buf: torch.Tensor) -> bool:
        """Accumulate the raw slots' (U_slot, dim) gradients (the index_add_
        de-dup output of ctx._on_backward) into the per-unique buffer;
        -> whether any slot contributed."""
        added = False
        for sc in group.slots:
            if sc.cfg.embedding_summation or sc.raw_sfs:
                continue  # raw-path slots ride in the group's base
            g = grads.get(sc.name)
            if g is None or self._nan_slot(sc, g):
                continue
            gf = g.float()
            if loss_scale != 1.0:
                gf = gf / loss_scale
            rounds = sc.cfg.hash_stack_rounds
            if sc.cfg.sqrt_scaling and rounds > 0:
                gf = gf / float(np.sqrt(rounds))
            buf.index_add_(0, sc.slot_uniq_global, gf)
            added = True
        return added

    @_update_entry
    def apply_gradients(
        self,
        training_batch: PersiaTrainingBatch,
        grads: Dict[str, Optional[torch.Tensor]],
        loss_scale: float = 1.0,
    ) -> None:
        """grads: slot name -> grad tensor ((B,dim) f16 for sum slots,
        (U_slot, dim) f32 for raw slots — the contract of ctx._on_backward,
        reference persia/ctx.py:926-1005) or None (skipped).  A raw-path slot
        (``SlotPayload.raw_rows``) takes the gradient of its rows instead,
        (B, sfs, dim) or (B*sfs, dim) f16, and is handled as the sum slots
        are."""
        self._apply_slot_grads(training_batch, grads, loss_scale)

    def _apply_slot_grads(self, training_batch, grads, loss_scale) -> None:
        native = self.device.type == "cuda"
        B = training_batch.batch_size
        for group in training_batch._groups:
            self._materialize_group(group)  # generic path needs exact U
            U = group.uniq_keys.numel()
            buf = torch.zeros(U, group.dim, dtype=torch.float32, device=self.device)
            sum_slots = [
                sc for sc in group.slots
                if (sc.cfg.embedding_summation or sc.raw_sfs)
                and grads.get(sc.name) is not None
            ]
            # no sum-slot grads at all: no fused launch, so a fully skipped
            # group never applies a zero-gradient optimizer step (reference
            # skip-the-slot semantics, mod.rs:731-746)
            any_grad = False
            if native and sum_slots:
                # fused ordered scatter over ALL sum slots in one launch.
                # Per-slot NaN skip without a host sync: zero the slot's
                # per-segment scale via a device flag and sanitize the grads
                # (NaN*0 would still be NaN); a None slot is a skipped one.
                g_parts, flag_parts = [], []
                for sc in group.slots:
                    if not (sc.cfg.embedding_summation or sc.raw_sfs):
                        continue
                    n = B * (sc.raw_sfs or 1)  # the slot's rows of the base
                    g = grads.get(sc.name)
                    if g is None:
                        g = torch.zeros(n, group.dim, dtype=torch.float16, device=self.device)
                        flag = torch.ones((), dtype=torch.bool, device=self.device)
                    else:
                        flag = torch.isnan(g).any()
                    g_parts.append(g.to(torch.float16).reshape(n, group.dim))
                    flag_parts.append(flag.expand(n))
                scale = self._seg_scale(group, loss_scale, skip=torch.cat(flag_parts))
                self._C.grad_scatter(
                    torch.nan_to_num(torch.cat(g_parts, dim=0)).contiguous(),
                    group.perm, group.ustarts, group.seg_id, scale.contiguous(),
                    buf, 1,
                )
                any_grad = True  # kernels launched regardless (no host sync)
            elif not native:
                for sc in sum_slots:
                    g = grads[sc.name]
                    if self._nan_slot(sc, g):
                        continue
                    any_grad = True
                    s, e = sc.pos_slice
                    buf += R.segment_grad_scatter(
                        g, group.inverse[s:e], sc.seg_offsets, U,
                        scale_factor=loss_scale, sqrt_scaling=sc.cfg.sqrt_scaling,
                    )
            if self._add_raw_grads(group, grads, loss_scale, buf) or any_grad:
                self._route_and_update(group, buf)

    def _a2a_backward_native(self, group: _GroupCtx, gbase: torch.Tensor,
                             seg_scale: torch.Tensor, store) -> None:
        """GPU fused distributed backward: per-uniq ordered grad reduction
        written directly into the padded a2a send layout (f16 wire), even
        all-to-all on the grad communicator, then owner-side fused
        dedup+scatter+optimizer.  No [U, dim] buffer, no host syncs."""
        plan = group.a2a_plan
        world, cap = plan.a2a_world, plan.a2a_cap
        send_g = torch.empty(
            world * cap + 1, group.dim, dtype=torch.float16, device=self.device
        )
        self._C.grad_scatter_idx(
            gbase.contiguous(), group.perm, group.ustarts, group.seg_id,
            seg_scale, group.a2a_idx, send_g,
            group.u_count if group.u_count is not None else store.no_count,
        )
        if world > 1:
            recv_g = self.dist_grad.all_to_all_even(send_g[: world * cap])
        else:
            recv_g = send_g[: world * cap]
        # positions whose recv key is 0 (bucket padding) were never written:
        # scatter_update skips them on the key, before reading the grads
        if group.a2a_owner_dedup is None:
            group.a2a_owner_dedup = tuple(
                self._C.dedup_padded(group.a2a_recv_keys)
            )
        ou, _oinv, operm, oustarts, ou_count = group.a2a_owner_dedup
        store.scatter_update(
            ou, recv_g, operm, oustarts, plan.owner_seg_id, ou_count
        )
        if self.incremental is not None:
            # owner-side recording: this rank's shard's touched signs
            self.incremental.record_keys(ou, ou_count)

    def _store_update(self, store, keys: torch.Tensor, grads: torch.Tensor) -> None:
        """One optimizer application per key on this rank's shard."""
        self.skipped_grad_signs += store.update_gradients(keys, grads)
        if self.incremental is not None:
            self.incremental.record_keys(keys)

    def _owner_merge_update(self, store, keys_recv: torch.Tensor,
                            grads_recv: torch.Tensor) -> None:
        """Owner side of a gradient exchange: merge duplicate keys across
        source ranks into ONE optimizer application per sign (the reference
        applies each rank's RPC sequentially under a per-sign lock — summing
        first is the synchronous-equivalent, deterministic, and race-free on
        GPU)."""
        uniq_f, inv = torch.unique(keys_recv ^ _FLIP, sorted=True, return_inverse=True)
        merged = torch.zeros(
            uniq_f.numel(), store.dim, dtype=torch.float32, device=self.device
        )
        merged.index_add_(0, inv, grads_recv.float())
        self._store_update(store, uniq_f ^ _FLIP, merged)

    def _route_and_update_padded(self, group: _GroupCtx, buf: torch.Tensor) -> None:
        """CPU mirror of the padded backward (the gloo-tested twin of
        _a2a_backward_native): pack per-uniq grads into the fixed bucket
        layout, even a2a, owner-side merge (same semantics as
        _route_and_update)."""
        plan = group.a2a_plan
        world, cap = plan.a2a_world, plan.a2a_cap
        send_g = torch.zeros(
            world * cap + 1, group.dim, dtype=self.wire_dtype,
            device=self.device,
        )
        # buf is exact [U, dim] (a materialized group); idx may be nnz-padded
        # — its first U entries are the valid uniques
        send_g.index_copy_(
            0, group.a2a_idx[: buf.shape[0]], buf.to(self.wire_dtype)
        )
        if world > 1:
            recv_g = self.dist_grad.all_to_all_even(send_g[: world * cap])
        else:
            recv_g = send_g[: world * cap]
        rk = group.a2a_recv_keys
        m = rk != 0
        if bool(m.any()):
            self._owner_merge_update(self.stores[group.dim], rk[m], recv_g[m])

    def _route_and_update(self, group: _GroupCtx, buf: torch.Tensor) -> None:
        store = self.stores[group.dim]
        if group.a2a_idx is not None:
            return self._route_and_update_padded(group, buf)
        if not self.dist.distributed:
            return self._store_update(store, group.uniq_keys, buf)
        comm = self.dist_grad  # main-thread communicator (see __init__)
        send_counts, recv_counts = group.send_counts, group.recv_counts
        if send_counts is None:
            owner = _owner_of_keys(group.uniq_keys, comm.world_size)
            send_counts = torch.bincount(owner, minlength=comm.world_size).tolist()
            recv_counts = comm.all_to_all_lengths(send_counts, self.device)
        keys_recv = comm.all_to_all(group.uniq_keys, send_counts, recv_counts)
        grads_recv = comm.all_to_all(
            buf.to(self.wire_dtype), send_counts, recv_counts
        )
        self._owner_merge_update(store, keys_recv, grads_recv)

    @_update_entry
    def apply_gradients_base(
        self,
        training_batch: PersiaTrainingBatch,
        raw_grads: Optional[Dict[str, Optional[torch.Tensor]]] = None,
        loss_scale: float = 1.0,
        sum_base_grads: Optional[List[torch.Tensor]] = None,
    ) -> None:
        """Backward fast path: sum-slot gradients are read directly from
        ``group.sum_base.grad`` (the per-group base tensor that
        ``prepare_features`` marked requires_grad) or ``sum_base_grads[i]``,
        so there is no per-slot cat/NaN-reduce cascade — one ordered scatter
        per group.

        ``raw_grads``: slot name -> (U_slot, dim) f32 for raw slots (the
        index_add_ de-dup output of ctx._on_backward)."""
        groups = training_batch._groups
        if sum_base_grads is None:
            sum_base_grads = [
                g.sum_base.grad if g.sum_base is not None else None
                for g in groups
            ]
        if self.device.type != "cuda":
            # CPU: slice each base into the per-slot dict contract
            grads: Dict[str, Optional[torch.Tensor]] = dict(raw_grads or {})
            B = training_batch.batch_size
            for group, gbase in zip(groups, sum_base_grads):
                b0 = 0
                for sc in group.slots:
                    if sc.cfg.embedding_summation:
                        grads[sc.name] = (
                            gbase[b0 : b0 + B] if gbase is not None else None
                        )
                        b0 += B
            return self._apply_slot_grads(training_batch, grads, loss_scale)

        for group, gbase in zip(groups, sum_base_grads):
            if gbase is None and not raw_grads:
                # no sum-base grad and no raw grads: skip the group (a
                # zero-grad optimizer application would still move Adam /
                # Adagrad state — reference skips the slot instead)
                continue
            store = self.stores[group.dim]
            if gbase is not None:
                # NaN gradients flow on and are skipped ROW-wise by the
                # update kernels — no isnan pass here
                seg_scale = self._seg_scale(group, loss_scale)
                if store.fused_native and not raw_grads:
                    if (
                        group.a2a_idx is not None
                        and self.wire_dtype == torch.float16
                    ):
                        # fused distributed backward: zero host syncs
                        self._a2a_backward_native(group, gbase, seg_scale, store)
                        continue
                    if not self.dist.distributed:
                        # fused native backward: scatter + optimizer in one call
                        store.update_local(
                            gbase, group.perm, group.ustarts, group.seg_id,
                            seg_scale, group.uniq_keys, group.u_count,
                            group.slot_hint, group.src_hint,
                        )
                        if self.incremental is not None:
                            self.incremental.record_keys(
                                group.uniq_keys, group.u_count
                            )
                        continue
            self._materialize_group(group)
            U = group.uniq_keys.numel()
            if gbase is not None:
                buf = torch.empty(
                    U, group.dim, dtype=torch.float32, device=self.device
                )
                self._C.grad_scatter(
                    gbase.contiguous(), group.perm, group.ustarts,
                    group.seg_id, seg_scale, buf, 0,
                )
            else:
                buf = torch.zeros(
                    U, group.dim, dtype=torch.float32, device=self.device
                )
            if raw_grads:  # raw slots add on top (buf fully written above)
                self._add_raw_grads(group, raw_grads, loss_scale, buf)
            self._route_and_update(group, buf)

    # ------------------------------------------------------------ checkpoint

    # checkpoint status machine (reference model-manager lib.rs:63-69:
    # {Dumping(progress) | Loading(progress) | Idle | Failed})
    def _set_status(self, status: str, progress: float = 0.0):
        self.model_manager_status = status
        self.model_manager_progress = progress

    def dump(self, dst_dir: str, blocking: bool = True) -> None:
        from persia_amd.core.checkpoint import dump_embedding

        def run():
            try:
                dump_embedding(self, dst_dir)
                self._set_status("Idle", 100.0)
            except Exception as e:
                _logger.error(f"embedding dump failed: {e}")
                self._set_status("Failed")
                if blocking:
                    raise

        # status set BEFORE the worker starts: a wait_for_emb_dumping issued
        # right after a non-blocking dump must never observe a stale 'Idle'
        self._set_status("Dumping", 0.0)
        if blocking:
            run()
        else:
            threading.Thread(target=run, daemon=True, name="persia-ckpt-dump").start()

    def load(self, src_dir: str, blocking: bool = True) -> None:
        from persia_amd.core.checkpoint import load_embedding

        def run():
            try:
                load_embedding(self, src_dir)
                self._set_status("Idle", 100.0)
            except Exception as e:
                _logger.error(f"embedding load failed: {e}")
                self._set_status("Failed")
                if blocking:
                    raise

        self._set_status("Loading", 0.0)  # before the thread (see dump)
        if blocking:
            run()
        else:
            threading.Thread(target=run, daemon=True, name="persia-ckpt-load").start()

    def wait_for_emb_dumping(self, timeout: float = 600.0) -> None:
        """Poll until the dump completes (reference rpc.rs:211-241)."""
        import time as _time

        t0 = _time.time()
        while getattr(self, "model_manager_status", "Idle") == "Dumping":
            if _time.time() - t0 > timeout:
                raise TimeoutError("embedding dump did not finish")
            _time.sleep(0.05)
        if getattr(self, "model_manager_status", "Idle") == "Failed":
            raise RuntimeError("embedding dump failed")

    def wait_for_emb_loading(self, timeout: float = 600.0) -> None:
        import time as _time

        t0 = _time.time()
        while getattr(self, "model_manager_status", "Idle") == "Loading":
            if _time.time() - t0 > timeout:
                raise TimeoutError("embedding load did not finish")
            _time.sleep(0.05)
        if getattr(self, "model_manager_status", "Idle") == "Failed":
            raise RuntimeError("embedding load failed")

    def num_resident_rows(self) -> int:
        return sum(len(s) for s in self.stores.values())


class ForwardPipeline:
    """Async prefetch with bounded staleness (reference ForwardImpl,
    forward.rs:470-528: input channel → lookup workers gated by a staleness
    Semaphore → output channel; the permit is released when the batch's
    gradients have been pushed — backward.rs:341-343)."""

    def __init__(self, engine: EmbeddingEngine, staleness: int = 8, out_buffer: int = 8,
                 reorder: bool = False):
        self.engine = engine
        self.staleness = max(1, staleness)
        # reproducible mode with several data loaders: process batches in
        # batch_id order via a min-heap (reference PerisaDataOrderManager,
        # forward.rs:396-468)
        self.reorder = reorder
        self._heap: list = []
        self._next_id = 0
        self._sem = threading.Semaphore(self.staleness)
        self._in: "queue.Queue" = queue.Queue(maxsize=max(2, out_buffer))
        self._out: "queue.Queue" = queue.Queue(maxsize=max(2, out_buffer))
        self._thread: Optional[threading.Thread] = None
        self._stop = threading.Event()
        self._exc: Optional[BaseException] = None
        self.inflight = 0  # lookups ahead of their gradient push (staleness)
        self.prod_s = 0.0  # cumulative producer-thread process_batch seconds
        self.prod_n = 0

    def start(self):
        if self._thread is None:
            self._thread = threading.Thread(target=self._run, daemon=True, name="persia-forward")
            self._thread.start()

    def _run(self):
        # On GPU, lookups run on a dedicated HIP stream so the sparse pipeline
        # overlaps the dense fwd/bwd on the default stream.  A fresh thread
        # defaults to device 0 — bind it to this rank's GPU first.
        stream = None
        if self.engine.device.type == "cuda":
            torch.cuda.set_device(self.engine.device)
            # PA_SPARSE_PRIORITY=-1 raises the lookup stream's scheduling
            # priority: on presets where the sparse stream is the critical
            # path (spill/dim-8 tables) the dense replay otherwise starves it
            prio = int(os.environ.get("PA_SPARSE_PRIORITY", "0"))
            stream = torch.cuda.Stream(device=self.engine.device, priority=prio)
        import heapq

        pending_eof = False
        while not self._stop.is_set():
            item = None
            if self.reorder and self._heap and self._heap[0][0] == self._next_id:
                item = heapq.heappop(self._heap)[1]
                self._next_id += 1
            else:
                try:
                    got = self._in.get(timeout=0.1)
                except queue.Empty:
                    if pending_eof and not self._heap:
                        self._out.put(None)
                        break
                    continue
                if got is None:
                    if self.reorder and self._heap:
                        pending_eof = True  # drain the heap first
                        continue
                    self._out.put(None)
                    break
                if self.reorder and got.batch_id is not None:
                    if got.batch_id != self._next_id:
                        heapq.heappush(self._heap, (got.batch_id, got))
                        continue
                    self._next_id += 1
                item = got
            self._sem.acquire()
            self.inflight += 1
            if self.engine.metrics_enabled:
                self.engine.metrics.staleness.set(self.inflight)
            try:
                t0 = time.perf_counter()
                if stream is not None:
                    with torch.cuda.stream(stream):
                        tb = self.engine.process_batch(item)
                    ev = torch.cuda.Event()
                    ev.record(stream)
                    tb._ready_event = ev
                else:
                    tb = self.engine.process_batch(item)
                # host-side producer cost (kernel issue + any CPU work);
                # excludes GPU completion — see `prod_n`/`prod_s` for the avg
                self.prod_s += time.perf_counter() - t0
                self.prod_n += 1
                self._out.put(tb)
            except BaseException as e:  # propagate to consumer
                self._exc = e
                self._out.put(None)
                break

    def put(self, batch: PersiaBatch):
        self.start()
        self._in.put(batch)
        if self.engine.metrics_enabled:
            self.engine.metrics.num_pending_batches.set(self._in.qsize())

    def finish(self):
        self.start()
        self._in.put(None)

    def get(self, timeout: Optional[float] = None) -> Optional[PersiaTrainingBatch]:
        tb = self._out.get(timeout=timeout)
        if tb is None and self._exc is not None:
            raise self._exc
        if tb is not None and getattr(tb, "_ready_event", None) is not None:
            cur = torch.cuda.current_stream()
            cur.wait_event(tb._ready_event)
            tb.record_stream(cur)
        return tb

    def release_permit(self):
        """Called after the batch's gradients were applied (or the batch was
        dropped) — the staleness window slides."""
        self.inflight = max(0, self.inflight - 1)
        self._sem.release()

    def stop(self):
        """Deterministic shutdown: wake and join the worker so no background
        thread is inside a HIP call at interpreter teardown."""
        self._stop.set()
        self._sem.release()  # unblock a worker waiting on the staleness gate
        try:
            self._in.put_nowait(None)
        except queue.Full:
            pass
        if self._thread is not None:
            self._thread.join(timeout=5.0)
            self._thread = None
