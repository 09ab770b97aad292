"""The embedding store: one shard of the (conceptually trillion-row) table.

Re-architecture of the reference parameter-server storage stack
(`persia-embedding-holder`: Sharded<EvictionMap<u64, HashMapEmbeddingEntry>>,
LRU via ArrayLinkedList — rust/persia-embedding-holder/src/lib.rs:28-64) as a
GPU-friendly **set-associative hash table**:

* keys:  ``uint64[n_slots]``   — splitmix64-mixed signs (bijective, so the
  mixed key IS the hash; 0 = empty sentinel)
* ticks: ``uint32[n_slots]``   — last-access batch counter (approximate LRU:
  evict the min-tick slot of the probe window when full)
* arena: ``float32[n_slots, row_width]`` — row = [emb(dim) | opt_state]
  (same logical layout as the reference's HashMapEmbeddingEntry.inner)

Buckets of ``BUCKET_SIZE`` slots; probing scans ``PROBE_BUCKETS`` consecutive
buckets.  Eviction is bounded-window LRU instead of the reference's global
linked-list LRU — O(1), no global state, GPU-parallel.

Two implementations with identical semantics:
* :class:`CpuEmbeddingStore` — numpy/torch sequential model (the oracle;
  also the CPU execution backend).
* :class:`HipEmbeddingStore` — HBM-resident, HIP kernels via persia_amd._C.
"""
from typing import Iterator, List, Optional, Tuple

import numpy as np
import torch

from persia_amd.core import hashing
from persia_amd.embedding import EmbeddingConfig
from persia_amd.embedding.optim import Adagrad, Adam, Ftrl, Optimizer, SGD

BUCKET_SIZE = 8
PROBE_BUCKETS = 4
EMPTY_KEY = np.uint64(0)
_ZERO_REMAP = np.uint64(0xD1B54A32D192ED03)  # mixed-key 0 is remapped here


def _floor_pow2(x: int) -> int:
    """Largest power of two <= x (capacity is a BUDGET: never round up —
    a ceil on a 2.6e9-row request would double a 128 GB arena)."""
    p = 1
    while (p << 1) <= x:
        p <<= 1
    return p


def _u01_from_u64(u: np.ndarray) -> np.ndarray:
    """Uniform [0,1) from the top 24 bits — must match csrc/common.h."""
    return (u >> np.uint64(40)).astype(np.float64) * (1.0 / (1 << 24))


def row_init(sign: int, dim: int, lo: float, hi: float) -> np.ndarray:
    """Deterministic per-sign bounded-uniform init (reference seeds SmallRng
    by sign — emb_entry.rs:35; we use splitmix64 streams, same both CPU/HIP)."""
    seed = hashing.init_seed_for(np.array([sign], dtype=np.uint64))[0]
    cols = np.arange(1, dim + 1, dtype=np.uint64)
    u = hashing.splitmix64(np.uint64(seed) ^ cols)
    return (lo + (hi - lo) * _u01_from_u64(u)).astype(np.float32)


class HostTier:
    """Host-DRAM spill tier: rows evicted from the HBM table park here and
    come back on their next lookup (exclusive cache: a fetch removes the
    entry, an eviction re-inserts the freshest copy).  Bounded LRU.

    Replaces the reference's remote-CPU parameter servers as the capacity
    extension beyond HBM (BASELINE config 4: 1e11-row tables)."""

    def __init__(self, capacity: int, row_width: int):
        from collections import OrderedDict

        self.capacity = capacity
        self.row_width = row_width
        self._map: "OrderedDict[int, np.ndarray]" = OrderedDict()

    def __len__(self) -> int:
        return len(self._map)

    def insert(self, keys: np.ndarray, rows: np.ndarray) -> None:
        for i, k in enumerate(keys):
            k = int(k)
            if k in self._map:
                self._map.move_to_end(k)
            self._map[k] = rows[i].copy()
        while len(self._map) > self.capacity:
            self._map.popitem(last=False)

    def fetch(self, keys: np.ndarray):
        """-> (rows f32 [k, row_width], found bool [k]); found entries are
        removed (they move to the HBM tier)."""
        rows = np.zeros((len(keys), self.row_width), dtype=np.float32)
        found = np.zeros(len(keys), dtype=bool)
        for i, k in enumerate(keys):
            row = self._map.pop(int(k), None)
            if row is not None:
                rows[i] = row
                found[i] = True
        return rows, found

    def __contains__(self, key) -> bool:
        return int(key) in self._map

    def export(self):
        """-> (keys u64 [n], rows f32 [n, row_width]) for checkpointing."""
        n = len(self._map)
        keys = np.fromiter(self._map.keys(), dtype=np.uint64, count=n)
        rows = (
            np.stack(list(self._map.values()))
            if n
            else np.zeros((0, self.row_width), dtype=np.float32)
        )
        return keys, rows.astype(np.float32)


class NativeHostTier:
    """C++ host spill tier (csrc/engine.cpp NativeHostTier) behind the same
    numpy interface as :class:`HostTier` — the python dict loops were the
    dominant producer-thread cost of spill-heavy configs."""

    def __init__(self, capacity: int, row_width: int):
        from persia_amd.ops import native

        self.capacity = capacity
        self.row_width = row_width
        self._impl = native().HostTier(capacity, row_width)

    def __len__(self) -> int:
        return int(self._impl.size())

    def insert(self, keys: np.ndarray, rows: np.ndarray) -> None:
        self._impl.insert(
            torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)),
            torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)),
        )

    def fetch(self, keys: np.ndarray):
        rows, found = self._impl.fetch(
            torch.from_numpy(np.ascontiguousarray(keys).view(np.int64))
        )
        return rows.numpy(), found.numpy()

    def __contains__(self, key) -> bool:
        return bool(self._impl.contains(int(np.int64(np.uint64(key)))))

    def export(self):
        keys, rows = self._impl.export_all()
        return keys.numpy().view(np.uint64), rows.numpy()



def _adapt_row_width(inner: np.ndarray, row_width: int,
                     state_init: float = 0.0) -> np.ndarray:
    """Adapt checkpoint rows to this store's row width: an infer-role store
    (no optimizer state) truncates the dumped opt-state columns; a train
    store loading an optimizer-less dump re-initializes the state columns
    (reference infer PS keeps whatever inner was dumped and slices the emb
    prefix on lookup — mod.rs:231-251; adapting at import keeps our fixed
    arena layout)."""
    cur = inner.shape[1]
    if cur == row_width:
        return inner
    if cur > row_width:
        return np.ascontiguousarray(inner[:, :row_width])
    out = np.full((inner.shape[0], row_width), state_init, dtype=np.float32)
    out[:, :cur] = inner
    return out


class EmbeddingStoreBase:
    """One rank's shard for one dim-group of slots."""

    # True where the backend has the fused entry points the engine's
    # sync-free paths call: lookup_local, lookup_local_bags, lookup_local_raw,
    # update_local, scatter_update
    fused_native = False

    def __init__(
        self,
        dim: int,
        capacity: int,
        optimizer: Optimizer,
        hyper: EmbeddingConfig,
        device: torch.device,
        spill_capacity: int = 0,
    ):
        self.dim = dim
        self.optimizer = optimizer
        self.hyper = hyper
        self.device = device
        self.opt_space = optimizer.require_space(dim)
        self.row_width = dim + self.opt_space
        self.n_buckets = _floor_pow2(max(1, capacity // BUCKET_SIZE))
        self.n_slots = self.n_buckets * BUCKET_SIZE
        self.tick = 1  # current batch counter (0 reserved)
        # tick allocation may be hit from the pipeline thread (lookups) and
        # the main thread (updates, incremental exports) concurrently
        self._tick_lock = __import__("threading").Lock()
        self.spill = HostTier(spill_capacity, self.row_width) if spill_capacity > 0 else None
        # Adam per-group beta powers (persia-common optim.rs:147-216); kept
        # per-store and stepped once per update call (all slot-groups in a
        # store receive every update batch in this architecture).
        if isinstance(optimizer, Adam):
            self.beta1_power = optimizer.betas[0]
            self.beta2_power = optimizer.betas[1]

    def __len__(self) -> int:
        raise NotImplementedError

    def lookup(self, keys: torch.Tensor, train: bool,
               u_count: Optional[torch.Tensor] = None) -> torch.Tensor:
        """keys: int64[n] (mixed u64 bit pattern) -> rows float32[n, dim].
        train=True inserts on miss (admit-gated, seeded init);
        train=False returns zeros on miss (reference parameter
        mod.rs:231-251).  ``u_count``: HIP-only padded-prefix length."""
        raise NotImplementedError

    def update_gradients(self, keys: torch.Tensor, grads: torch.Tensor) -> int:
        """Apply the sparse optimizer to rows addressed by keys; skip keys no
        longer resident. Returns number skipped."""
        raise NotImplementedError

    def lookup_wire(self, keys: torch.Tensor, train: bool,
                    wire_dtype: torch.dtype) -> torch.Tensor:
        """Owner-side lookup for the padded a2a exchange: ``keys`` may contain
        the empty-key sentinel 0 (bucket padding) — those entries are silently
        skipped (zeros out, no insert).  Rows come back in the WIRE dtype so
        they go straight onto the xGMI all-to-all."""
        raise NotImplementedError

    def export_rows(self) -> Tuple[np.ndarray, np.ndarray]:
        """-> (signs u64[n], inner f32[n, row_width]) of every resident row."""
        raise NotImplementedError

    def import_rows(self, signs: np.ndarray, inner: np.ndarray) -> None:
        raise NotImplementedError

    def export_chunks(
        self, chunk_rows: int
    ) -> Iterator[Tuple[np.ndarray, np.ndarray]]:
        """Stream ``export_rows()`` as (signs, inner) pieces of at most
        ``chunk_rows`` records, in the same order.  A piece is only valid
        until the generator is advanced (backends may reuse staging
        buffers); copy it to keep it.  This default slices one whole-table
        export; the HIP backend streams in bounded memory."""
        chunk_rows = max(1, int(chunk_rows))
        signs, inner = self.export_rows()
        for lo in range(0, len(signs), chunk_rows):
            yield signs[lo:lo + chunk_rows], inner[lo:lo + chunk_rows]

    def import_chunk(self, signs: np.ndarray, inner: np.ndarray) -> None:
        """Insert one chunk of a streamed load (own tick per chunk)."""
        self.import_rows(np.asarray(signs), np.asarray(inner))

    def finish_import(self) -> int:
        """End of a streamed load: number of rows offered to ``import_chunk``
        since the last call that found no slot and were dropped (0 where the
        backend does not count)."""
        return 0

    def clear(self) -> None:
        raise NotImplementedError

    def next_tick(self) -> int:
        with self._tick_lock:
            t = self.tick
            self.tick += 1
        return t

    def export_keys(self, signs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """Export rows for specific signs: (found_signs, inner[found]).
        Presence comes from the table probe (NOT a rows==0 heuristic — an
        all-zero row is a legitimate value), without insert-on-miss and
        without consuming a tick.  Used by the incremental-update dumper;
        may run concurrently with training — a row mutated mid-read yields a
        mixed old/new row, which the bounded-staleness freshness contract
        tolerates (the reference holds per-sign locks instead)."""
        raise NotImplementedError

    def skip_counters(self) -> Optional[torch.Tensor]:
        """Device-side i32[2] (missing-key, NaN-row) update skip counters for
        the metrics harvest, or None where skips are returned host-side."""
        return None

    def _spill_export(self):
        """Host-tier rows for checkpointing (spilled rows are table state)."""
        if self.spill is None or len(self.spill) == 0:
            return None
        keys, rows = self.spill.export()
        return hashing.splitmix64_inv(keys), rows

    def _adam_step_powers(self):
        o = self.optimizer
        if isinstance(o, Adam):
            b1p, b2p = self.beta1_power, self.beta2_power
            self.beta1_power *= o.betas[0]
            self.beta2_power *= o.betas[1]
            return b1p, b2p
        return None


class CpuEmbeddingStore(EmbeddingStoreBase):
    """Sequential oracle + CPU execution backend."""

    def __init__(self, dim, capacity, optimizer, hyper, device=torch.device("cpu"),
                 spill_capacity: int = 0):
        super().__init__(dim, capacity, optimizer, hyper, device, spill_capacity)
        self.keys = np.zeros(self.n_slots, dtype=np.uint64)
        self.ticks = np.zeros(self.n_slots, dtype=np.uint32)
        self.arena = torch.zeros(self.n_slots, self.row_width, dtype=torch.float32)
        self._count = 0

    def __len__(self) -> int:
        return self._count

    # -- probing ------------------------------------------------------------
    def _probe(self, k: np.uint64) -> int:
        """Find slot of key k, or -1."""
        mask = np.uint64(self.n_buckets - 1)
        b0 = int(k & mask)
        for p in range(PROBE_BUCKETS):
            base = ((b0 + p) % self.n_buckets) * BUCKET_SIZE
            for s in range(BUCKET_SIZE):
                if self.keys[base + s] == k:
                    return base + s
        return -1

    def _probe_or_claim(self, k: np.uint64, tick: int) -> Tuple[int, bool]:
        """-> (slot, is_new). Claims an empty slot, else evicts the min-tick
        slot of the probe window; rows touched at the CURRENT tick are never
        victims (same rule as the HIP kernel, so concurrent claims within a
        batch cannot evict each other). slot=-1 = overflow miss."""
        mask = np.uint64(self.n_buckets - 1)
        b0 = int(k & mask)
        empty = -1
        victim, victim_tick = -1, None
        for p in range(PROBE_BUCKETS):
            base = ((b0 + p) % self.n_buckets) * BUCKET_SIZE
            for s in range(BUCKET_SIZE):
                i = base + s
                ki = self.keys[i]
                if ki == k:
                    return i, False
                if ki == EMPTY_KEY:
                    if empty < 0:
                        empty = i
                elif self.ticks[i] != tick and (
                    victim_tick is None or self.ticks[i] < victim_tick
                ):
                    victim, victim_tick = i, self.ticks[i]
        if empty >= 0:
            self.keys[empty] = k
            self.ticks[empty] = tick
            self._count += 1
            return empty, True
        if victim < 0:
            return -1, False  # whole window is current-tick: overflow
        if self.spill is not None:  # save the victim row to the host tier
            self.spill.insert(
                np.array([self.keys[victim]], dtype=np.uint64),
                self.arena[victim].numpy().reshape(1, -1),
            )
        self.keys[victim] = k  # evict (bounded-window LRU)
        self.ticks[victim] = tick
        return victim, True

    def _init_row(self, slot: int, k: np.uint64) -> None:
        sign = int(hashing.splitmix64_inv(np.array([k], dtype=np.uint64))[0])
        lo, hi = self.hyper.emb_initialization
        emb = row_init(sign, self.dim, lo, hi)
        row = torch.zeros(self.row_width, dtype=torch.float32)
        row[: self.dim] = torch.from_numpy(emb)
        if self.opt_space:
            row[self.dim :] = self.optimizer.state_init(self.dim)
        self.arena[slot] = row

    def _admitted(self, k: np.uint64, tick: int) -> bool:
        if self.hyper.admit_probability >= 1.0:
            return True
        u = hashing.splitmix64(np.array([k ^ np.uint64(tick)], dtype=np.uint64))
        return float(_u01_from_u64(u)[0]) < self.hyper.admit_probability

    # -- public ops ---------------------------------------------------------
    def lookup(self, keys: torch.Tensor, train: bool,
               u_count: Optional[torch.Tensor] = None) -> torch.Tensor:
        assert u_count is None, "padded lookup is a HIP-path feature"
        tick = self.next_tick()
        k_np = keys.cpu().numpy().view(np.uint64).copy()
        k_np[k_np == EMPTY_KEY] = _ZERO_REMAP
        out = torch.zeros(len(k_np), self.dim, dtype=torch.float32)
        for i, k in enumerate(k_np):
            if train:
                if self._admitted(k, tick) or self._probe(k) >= 0:
                    slot, is_new = self._probe_or_claim(k, tick)
                    if slot < 0:
                        continue  # overflow miss: zeros
                    if is_new:
                        restored = False
                        if self.spill is not None:
                            rows, found = self.spill.fetch(np.array([k], dtype=np.uint64))
                            if found[0]:
                                self.arena[slot] = torch.from_numpy(rows[0])
                                restored = True
                        if not restored:
                            self._init_row(slot, k)
                    self.ticks[slot] = tick
                    out[i] = self.arena[slot, : self.dim]
            else:
                slot = self._probe(k)
                if slot >= 0:
                    self.ticks[slot] = tick
                    out[i] = self.arena[slot, : self.dim]
        return out

    def lookup_wire(self, keys: torch.Tensor, train: bool,
                    wire_dtype: torch.dtype) -> torch.Tensor:
        out = torch.zeros(keys.numel(), self.dim, dtype=torch.float32)
        m = keys != 0
        if bool(m.any()):
            out[m] = self.lookup(keys[m], train)
        else:
            self.next_tick()  # tick parity with the non-empty case
        return out.to(wire_dtype)

    def update_gradients(self, keys: torch.Tensor, grads: torch.Tensor) -> int:
        powers = self._adam_step_powers()
        k_np = keys.cpu().numpy().view(np.uint64).copy()
        k_np[k_np == EMPTY_KEY] = _ZERO_REMAP
        slots = np.array([self._probe(k) for k in k_np], dtype=np.int64)
        present = slots >= 0
        # row-level NaN skip (same semantics as the HIP update kernel)
        nan_rows = torch.isnan(grads.float()).any(dim=1).cpu().numpy()
        present = present & ~nan_rows
        skipped = int((slots < 0).sum())
        if present.sum() == 0:
            return skipped
        idx = torch.from_numpy(slots[present])
        g = grads.float().cpu()[torch.from_numpy(np.nonzero(present)[0])]
        rows = self.arena[idx]  # copy [n, row_width]
        emb = rows[:, : self.dim]
        from persia_amd.ops import reference as R

        o = self.optimizer
        wb = self.hyper.weight_bound
        if isinstance(o, SGD):
            R.sgd_update(emb, g, o.lr, o.weight_decay, wb)
        elif isinstance(o, Adagrad):
            accum = rows[:, self.dim :] if not o.vectorwise_shared else rows[:, self.dim : self.dim + 1]
            R.adagrad_update(
                emb, accum, g, o.lr, o.g_square_momentum, o.eps, wb, o.vectorwise_shared
            )
        elif isinstance(o, Adam):
            m = rows[:, self.dim : 2 * self.dim]
            v = rows[:, 2 * self.dim :]
            b1p, b2p = powers
            R.adam_update(emb, m, v, g, b1p, b2p, o.lr, o.betas[0], o.betas[1], o.eps, wb)
        elif isinstance(o, Ftrl):
            z = rows[:, self.dim : 2 * self.dim]
            n = rows[:, 2 * self.dim :]
            R.ftrl_update(emb, z, n, g, o.lr, o.beta, o.l1, o.l2, wb)
        else:
            raise ValueError(f"unknown optimizer {o.kind}")
        self.arena[idx] = rows
        return skipped

    def export_keys(self, signs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        ks = hashing.splitmix64(signs.astype(np.uint64))
        ks[ks == EMPTY_KEY] = _ZERO_REMAP
        slots = np.array([self._probe(k) for k in ks], dtype=np.int64)
        found = slots >= 0
        inner = self.arena[torch.from_numpy(slots[found])].numpy().copy()
        return signs[found], inner

    def export_rows(self) -> Tuple[np.ndarray, np.ndarray]:
        occ = np.nonzero(self.keys != EMPTY_KEY)[0]
        signs = hashing.splitmix64_inv(self.keys[occ])
        inner = self.arena[torch.from_numpy(occ)].numpy()
        sp = self._spill_export()
        if sp is not None:
            signs = np.concatenate([signs, sp[0]])
            inner = np.concatenate([inner, sp[1]])
        return signs, inner

    def import_rows(self, signs: np.ndarray, inner: np.ndarray) -> None:
        inner = _adapt_row_width(
            inner, self.row_width, float(self.optimizer.state_init(self.dim))
        )
        ks = hashing.splitmix64(signs.astype(np.uint64))
        ks[ks == EMPTY_KEY] = _ZERO_REMAP
        tick = self.next_tick()
        for i, k in enumerate(ks):
            slot, _ = self._probe_or_claim(k, tick)
            if slot < 0:
                continue  # shard over capacity: drop (bounded table)
            self.arena[slot] = torch.from_numpy(inner[i].astype(np.float32))
            self.ticks[slot] = tick

    def clear(self) -> None:
        self.keys[:] = EMPTY_KEY
        self.ticks[:] = 0
        self.arena.zero_()
        self._count = 0


class HipEmbeddingStore(EmbeddingStoreBase):
    """HBM-resident shard driven by HIP kernels (persia_amd._C).

    All state lives in torch CUDA tensors (allocated through the caching
    allocator so it coexists with the dense model); kernels mutate them in
    place."""

    fused_native = True

    def __init__(self, dim, capacity, optimizer, hyper, device, spill_capacity: int = 0):
        super().__init__(dim, capacity, optimizer, hyper, device, spill_capacity)
        from persia_amd.ops import native

        self._C = native()
        assert device.type == "cuda"
        if self.spill is not None:
            # native spill tier: same LRU semantics, no python dict loops
            self.spill = NativeHostTier(spill_capacity, self.row_width)
        self.keys = torch.zeros(self.n_slots, dtype=torch.int64, device=device)
        self.ticks = torch.zeros(self.n_slots, dtype=torch.int32, device=device)
        self.arena = torch.zeros(
            self.n_slots, self.row_width, dtype=torch.float32, device=device
        )
        self._skipped = torch.zeros(2, dtype=torch.int32, device=device)  # miss, nan
        self._opt_code = {"sgd": 0, "adagrad": 1, "adam": 2, "ftrl": 3}[optimizer.kind]
        self._probe_stream: Optional[torch.cuda.Stream] = None
        self._restore_tick: Optional[int] = None
        self._ckpt_stream: Optional[torch.cuda.Stream] = None
        # streamed-load accounting: rows offered (host) vs rows landed (device)
        self._imported = torch.zeros(1, dtype=torch.int64, device=device)
        self._import_offered = 0
        self.evicted_total = 0  # host-side eviction count (spill drains)
        # "argument absent" sentinels of the native calls: no device-side
        # unique count (keys are exact), no per-segment scale (all ones), no
        # eviction log (no spill tier)
        self.no_count = torch.empty(0, dtype=torch.int64, device=device)
        self._no_scale = torch.empty(0, dtype=torch.float32, device=device)
        self._no_evict = (
            self.no_count,
            torch.empty(0, dtype=torch.int32, device=device),
            self._no_scale,
        )

    def _evict_buffers(self, n: int):
        if self.spill is None:
            return self._no_evict
        return (
            torch.zeros(n, dtype=torch.int64, device=self.device),
            torch.zeros(1, dtype=torch.int32, device=self.device),
            torch.empty(n, self.row_width, dtype=torch.float32, device=self.device),
        )

    def _drain_evictions(self, ev):
        """Deferred: stash this batch's eviction log with an async count
        readback; the NEXT lookup drains it (avoids a device sync per batch —
        an evicted key re-looked-up within that one-batch window re-inits,
        which bounded-window LRU makes a cold-key non-event)."""
        keys_t, count_t, rows_t = ev
        if keys_t.numel() == 0:
            return
        self._drain_pending()
        cnt_pin = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        cnt_pin.copy_(count_t, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._pending_evict = (keys_t, rows_t, cnt_pin, done)

    def _drain_pending(self):
        pend = getattr(self, "_pending_evict", None)
        if pend is None:
            return
        self._pending_evict = None
        keys_t, rows_t, cnt_pin, done = pend
        done.synchronize()
        cnt = int(cnt_pin.item())
        if cnt == 0:
            return
        self.evicted_total += cnt
        keys_np = keys_t[:cnt].cpu().numpy().view(np.uint64)
        rows_np = rows_t[:cnt].cpu().numpy()
        self.spill.insert(keys_np, rows_np)

    def flush_spill(self):
        """Drain any stashed eviction log (checkpoint/export paths)."""
        if self.spill is not None:
            self._drain_pending()

    def _opt_params(self):
        o = self.optimizer
        if isinstance(o, SGD):
            return [o.lr, o.weight_decay, 0.0, 0.0, 0.0, 0.0]
        if isinstance(o, Adagrad):
            return [
                o.lr,
                o.g_square_momentum,
                o.eps,
                1.0 if o.vectorwise_shared else 0.0,
                0.0,
                0.0,
            ]
        if isinstance(o, Adam):
            return [o.lr, o.betas[0], o.betas[1], o.eps, 0.0, 0.0]
        if isinstance(o, Ftrl):
            return [o.lr, o.beta, o.l1, o.l2, 0.0, 0.0]
        raise ValueError(o.kind)

    def _lookup_args(self, train: bool, tick: int):
        """The argument run every native lookup shares (after the table
        tensors): dim, train, tick, init range, admit probability, optimizer
        state init and width."""
        lo, hi = self.hyper.emb_initialization
        return (
            self.dim, int(train), tick, float(lo), float(hi),
            float(self.hyper.admit_probability),
            float(self.optimizer.state_init(self.dim)), self.opt_space,
        )

    def _update_args(self):
        """The argument run every native update shares: dim, optimizer code
        and params, Adam beta powers, weight bound, skip counters.  Steps the
        Adam powers, so it is called exactly once per update call."""
        powers = self._adam_step_powers()
        b1p, b2p = powers if powers else (0.0, 0.0)
        return (
            self.dim, self._opt_code, self._opt_params(), float(b1p),
            float(b2p), float(self.hyper.weight_bound), self._skipped,
        )

    def __len__(self) -> int:
        return int((self.keys != 0).sum().item())

    @property
    def probe_stream(self) -> "torch.cuda.Stream":
        """Side stream for the spill-restore front half: its backlog is only
        this batch's tiny probe work, so the miss-mask readback does not wait
        for the lookup stream's multi-batch queue (the dcn-spill producer
        stall — profiles/README round-1 finding)."""
        if self._probe_stream is None:
            self._probe_stream = torch.cuda.Stream(device=self.device)
        return self._probe_stream

    def spill_restore(self, keys: torch.Tensor,
                      u_count: Optional[torch.Tensor] = None) -> None:
        """Phase 1 of a training lookup with a spill tier, split out so the
        engine can run it on ``probe_stream``: probe for missing-but-spilled
        rows, fetch them from the host tier and import into HBM.  The
        following ``lookup`` call reuses this tick and skips its own phase 1.

        Probes may race in-flight inserts/evictions on the lookup stream;
        both races degrade to a cold-key re-init or a no-op fetch — the
        bounded-staleness tolerance the table already guarantees."""
        tick = self.next_tick()
        self._restore_tick = tick
        if not len(self.spill) or keys.numel() == 0:
            return
        self._drain_pending()
        # the log holds the imports' evictions only; drained at once
        ev = self._spill_phase1(
            keys, tick, u_count if u_count is not None else self.no_count, 0
        )
        if ev is not None:
            self._drain_evictions(ev)

    def _spill_phase1(self, keys: torch.Tensor, tick: int, uc: torch.Tensor,
                      log_rows: int):
        """Probe ``keys``, fetch the misses from the host tier and import the
        found rows into HBM.  -> the eviction log the import wrote (sized
        ``log_rows`` + rows imported: imports can evict too), or None when
        nothing was imported.  The ``keys[slots < 0]`` readback syncs only the
        caller's stream."""
        slots = self._C.store_probe(self.keys, self.ticks, keys, tick, uc)
        miss_keys = keys[slots < 0]
        if not miss_keys.numel():
            return None
        miss_np = miss_keys.cpu().numpy().view(np.uint64)
        rows, found = self.spill.fetch(miss_np)
        if not found.any():
            return None
        ev = self._evict_buffers(log_rows + int(found.sum()))
        found_keys = torch.from_numpy(
            miss_np[found].view(np.int64).copy()
        ).to(self.device)
        rows_t = torch.from_numpy(rows[found]).to(self.device)
        self._C.store_import(
            self.keys, self.ticks, self.arena, found_keys, rows_t, tick, *ev
        )
        return ev

    def lookup(
        self, keys: torch.Tensor, train: bool,
        u_count: Optional[torch.Tensor] = None,
    ) -> torch.Tensor:
        """``u_count``: optional device-side i64[1] valid-prefix length for
        nnz-padded ``keys`` (sync-free dedup) — the padding tail is the
        empty-key sentinel and is never probed or claimed."""
        restored = self._restore_tick is not None
        if restored:
            tick = self._restore_tick
            self._restore_tick = None
        else:
            tick = self.next_tick()
        n = keys.numel()
        uc = u_count if u_count is not None else self.no_count
        ev = self._no_evict
        if self.spill is not None and train and n:
            self._drain_pending()
            ev = self._evict_buffers(n)
            if not restored and len(self.spill):
                # spill phase 1 inline (engine did not pre-restore): one log
                # for the imports' and the lookup's evictions, drained below
                ev = self._spill_phase1(keys, tick, uc, n) or ev
        out = torch.empty(n, self.dim, dtype=torch.float32, device=self.device)
        self._C.store_lookup(
            self.keys, self.ticks, self.arena, keys, out,
            *self._lookup_args(train, tick), *ev, uc,
        )
        self._drain_evictions(ev)
        return out

    def lookup_wire(self, keys: torch.Tensor, train: bool,
                    wire_dtype: torch.dtype) -> torch.Tensor:
        """Padded-a2a owner lookup: key 0 entries (bucket padding) return
        zeros and never claim slots (kernel-level skip); output is the wire
        dtype directly (fused f16 cast in init_gather).

        ``keys`` is the receive buffer as it arrives and may repeat a key
        (once per source rank that asked for it): every occurrence returns the
        same row, and a key new to the table is claimed once and initialized
        before any occurrence is read (training runs the init in a launch of
        its own ahead of the gather; an eval lookup claims nothing and pays
        nothing for this)."""
        out = torch.empty(
            keys.numel(), self.dim, dtype=wire_dtype, device=self.device
        )
        self._C.store_lookup(
            self.keys, self.ticks, self.arena, keys, out,
            *self._lookup_args(train, self.next_tick()), *self._no_evict,
            self.no_count,
        )
        return out

    def lookup_local(self, values: torch.Tensor, slot_starts: torch.Tensor,
                     prefixes: torch.Tensor, spacing_arg: int,
                     cat_offsets: torch.Tensor, seg_scale: torch.Tensor,
                     seg_id: torch.Tensor, train: bool):
        """The whole single-GPU lookup of an all-single-ID sum group in one
        native call: sign prep, padded dedup, probe/insert, gather and the
        fused segment sum over the uploaded raw ``values``.
        -> (sums, uniq, inverse, perm, ustarts, u_count, slot_hint, src_hint).
        The last two are the update hints ``update_local`` takes back: per
        unique key the slot the probe gave it, and through ``seg_id`` the
        gradient row of a key with one position (-1: none)."""
        return self._C.lookup_local(
            values, slot_starts, prefixes, spacing_arg, cat_offsets, seg_scale,
            seg_id, self.keys, self.ticks, self.arena,
            *self._lookup_args(train, self.next_tick()),
        )

    def lookup_local_bags(self, upload: torch.Tensor, nnz: int, S: int,
                          B: int, prefixes: torch.Tensor, spacing_arg: int,
                          sqrt_flags: torch.Tensor, hints: bool, train: bool,
                          rounds=None, sizes=None, nnz_out: Optional[int] = None,
                          stack_dev=None):
        """The whole single-GPU lookup of a bag group (sum slots with any
        number of ids per sample) in one native call.  ``upload`` is the
        group's device buffer ``values[nnz] ‖ slot_starts[S+1] ‖
        offsets[S, B+1]`` (engine ``pack_bag_buffer``); ``sqrt_flags`` i32[S]
        marks the sqrt-scaling slots, empty when there is none.
        -> (sums, uniq, inverse, perm, ustarts, u_count, slot_hint, src_hint,
        cat_offsets, seg_id, seg_lens, seg_scale): ``lookup_local``'s results
        and the group's segment plan.  ``seg_scale`` is empty (all ones)
        without a sqrt slot; the hints are empty unless ``hints`` and
        ``train``.

        A group with hashstack slots passes ``rounds`` and ``sizes`` (host
        sequences of S ints: the slots' ``hash_stack_rounds``, 0 for none,
        and ``embedding_size``) and ``nnz_out``, the number of expanded
        positions.  ``upload`` is then engine ``pack_stack_bag_buffer``'s,
        ``values[nnz] ‖ slot_starts[S+1] ‖ offsets[S, B+1] ‖ in_starts[S+1]``
        with the ids unexpanded and the plan in the expanded space, and the
        results are sized by ``nnz_out``.  ``stack_dev`` is the pair of device
        tensors (rounds i32[S], sizes i64[S]) of the same values, which a
        caller with a static plan builds once; without it they are uploaded
        here.  Everything is checked on the host, before any launch."""
        if rounds is None:
            return self._C.lookup_local_bags(
                upload, nnz, S, B, prefixes, spacing_arg, sqrt_flags,
                int(hints), self.keys, self.ticks, self.arena,
                *self._lookup_args(train, self.next_tick()),
            )
        rounds, sizes = [int(r) for r in rounds], [int(z) for z in sizes]
        if len(rounds) != S or len(sizes) != S:
            raise ValueError(
                f"lookup_local_bags: {S} slots, {len(rounds)} round counts "
                f"and {len(sizes)} sizes"
            )
        if nnz_out is None:
            raise ValueError("lookup_local_bags: rounds without nnz_out")
        if not any(r > 1 for r in rounds) and nnz_out != nnz:
            # no slot expands: the position count is the id count
            raise ValueError(
                f"lookup_local_bags: {nnz_out} positions from {nnz} ids, "
                f"no slot has more than one round"
            )
        if stack_dev is None:
            stack_dev = (
                torch.tensor(rounds, dtype=torch.int32, device=upload.device),
                torch.tensor(sizes, dtype=torch.int64, device=upload.device),
            )
        return self._C.lookup_local_bags_stack(
            upload, nnz, nnz_out, S, B, prefixes, spacing_arg, sqrt_flags,
            stack_dev[0], stack_dev[1], rounds, sizes, int(hints),
            self.keys, self.ticks, self.arena,
            *self._lookup_args(train, self.next_tick()),
        )

    def lookup_local_raw(self, upload: torch.Tensor, nnz: int, S: int, B: int,
                         prefixes: torch.Tensor, spacing_arg: int,
                         sqrt_flags: torch.Tensor, raw_meta: torch.Tensor,
                         sfs: List[int], hints: bool, train: bool):
        """The whole single-GPU lookup of a group with raw (sequence) slots in
        one native call: ``S`` sum slots first (single-ID or bags), then one
        raw slot per entry of ``sfs`` (its ``sample_fixed_size``).  ``upload``
        is ``lookup_local_bags``' buffer over all the slots; ``raw_meta`` is
        the device i64 ``row_base[R] ‖ sfs[R]`` (engine ``raw_slot_meta``).
        -> (base, mask, uniq, inverse, perm, ustarts, u_count, slot_hint,
        src_hint, cat_offsets, seg_id, seg_lens, seg_scale, raw_num).
        ``base`` f16 ``[S*B + sum B*sfs, dim]`` holds the sums, then each raw
        slot's cell rows sample-major; ``mask`` f16 ``[sum B*sfs]`` is 1 where
        a cell holds an id (a missing row included).  ``seg_id`` sends a
        position to its gradient row in ``base``, -1 for a truncated one;
        ``seg_scale`` covers ``base``'s rows or is empty without a sqrt slot;
        ``raw_num`` i64 ``[R*B]`` is ``min(len, sfs)``."""
        return self._C.lookup_local_raw(
            upload, nnz, S, B, prefixes, spacing_arg, sqrt_flags, raw_meta,
            list(sfs), int(hints), self.keys, self.ticks, self.arena,
            *self._lookup_args(train, self.next_tick()),
        )

    def update_local(self, gbase, perm, ustarts, seg_id, seg_scale, uniq,
                     u_count: Optional[torch.Tensor],
                     slot_hint: Optional[torch.Tensor] = None,
                     src_hint: Optional[torch.Tensor] = None) -> None:
        """Fused local backward: ordered per-unique reduction of the segment
        gradients ``gbase`` and the optimizer step, in one call.  The hints
        (``lookup_local``, both or neither) only shorten the kernel's
        dependent loads; the result is the same bits without them."""
        hinted = slot_hint is not None and src_hint is not None
        self._C.update_local(
            gbase.contiguous(), perm, ustarts, seg_id, seg_scale, uniq,
            self.keys, self.ticks, self.arena, *self._update_args(),
            u_count if u_count is not None else self.no_count,
            slot_hint if hinted else self.no_count,
            src_hint if hinted else self.no_count,
        )

    def scatter_update(self, uniq, grads, perm, ustarts, seg_id,
                       u_count: torch.Tensor) -> None:
        """Owner-side fused backward of the padded a2a: reduce the received
        per-position ``grads`` per unique key and apply the optimizer.
        Positions whose key is 0 (bucket padding) are skipped on the key."""
        self._C.scatter_update(
            self.keys, self.ticks, self.arena, uniq, grads, perm, ustarts,
            seg_id, self._no_scale, *self._update_args(), u_count,
        )

    def update_gradients(self, keys: torch.Tensor, grads: torch.Tensor) -> int:
        self._C.store_update(
            self.keys, self.ticks, self.arena, keys,
            grads.float().contiguous(), *self._update_args(),
        )
        return 0  # skipped count is accumulated device-side (no hot-path sync)

    def skip_counters(self) -> torch.Tensor:
        return self._skipped

    def skipped_count(self) -> int:
        return int(self._skipped[0].item())

    def nan_row_count(self) -> int:
        return int(self._skipped[1].item())

    def export_keys(self, signs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        ks = hashing.splitmix64(signs.astype(np.uint64))
        ks[ks == EMPTY_KEY] = _ZERO_REMAP
        keys_t = torch.from_numpy(ks.view(np.int64)).to(self.device)
        slots = self._C.store_probe(
            self.keys, self.ticks, keys_t, self.tick, self.no_count
        )
        found = slots >= 0
        inner = self.arena[slots[found]].cpu().numpy()
        found_np = found.cpu().numpy()
        out_signs, out_inner = signs[found_np], inner
        if self.spill is not None and (~found_np).any():
            # a touched sign may have been evicted to the host tier between
            # update and flush; fetch + re-insert (peek) keeps it resident
            self.flush_spill()
            miss, miss_ks = signs[~found_np], ks[~found_np]
            rows, sp_found = self.spill.fetch(miss_ks)
            if sp_found.any():
                self.spill.insert(miss_ks[sp_found], rows[sp_found])
                out_signs = np.concatenate([out_signs, miss[sp_found]])
                out_inner = np.concatenate([out_inner, rows[sp_found]])
        return out_signs, out_inner

    def export_rows(self) -> Tuple[np.ndarray, np.ndarray]:
        self.flush_spill()
        occ = torch.nonzero(self.keys != 0, as_tuple=False).view(-1)
        keys = self.keys[occ].cpu().numpy().view(np.uint64)
        signs = hashing.splitmix64_inv(keys)
        inner = self.arena[occ].cpu().numpy()
        sp = self._spill_export()
        if sp is not None:
            signs = np.concatenate([signs, sp[0]])
            inner = np.concatenate([inner, sp[1]])
        return signs, inner

    def import_rows(self, signs: np.ndarray, inner: np.ndarray) -> None:
        inner = _adapt_row_width(
            inner, self.row_width, float(self.optimizer.state_init(self.dim))
        )
        ks = hashing.splitmix64(signs.astype(np.uint64))
        ks[ks == EMPTY_KEY] = _ZERO_REMAP
        keys_t = torch.from_numpy(ks.view(np.int64)).to(self.device)
        rows_t = torch.from_numpy(np.ascontiguousarray(inner, dtype=np.float32)).to(
            self.device
        )
        tick = self.next_tick()
        ev = self._evict_buffers(keys_t.numel())
        self._C.store_import(
            self.keys, self.ticks, self.arena, keys_t, rows_t, tick, *ev
        )
        self._drain_evictions(ev)

    @property
    def ckpt_stream(self) -> "torch.cuda.Stream":
        """Dedicated stream of the streaming dump, so a non-blocking dump
        does not queue behind (or in front of) the training stream's work."""
        if self._ckpt_stream is None:
            self._ckpt_stream = torch.cuda.Stream(device=self.device)
        return self._ckpt_stream

    def export_chunks(
        self, chunk_rows: int
    ) -> Iterator[Tuple[np.ndarray, np.ndarray]]:
        """Bounded-memory export in ``export_rows()`` order: slot windows of
        ``chunk_rows`` slots are compacted on the device
        (csrc/checkpoint.hip) into two staging buffers and copied, ``count``
        rows each, into two pinned host buffers; the spill tier follows.
        While the consumer handles window k, window k+1 is already compacted
        and on its way to the host.  Yields views of the pinned buffers,
        valid until the generator is advanced."""
        chunk_rows = max(1, int(chunk_rows))
        self.flush_spill()
        cap = min(chunk_rows, self.n_slots)
        n_win = (self.n_slots + cap - 1) // cap
        st = self.ckpt_stream
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(st):
            st.wait_event(ready)  # table state as of the caller's stream
            dev = [
                (
                    torch.empty(cap, dtype=torch.int64, device=self.device),
                    torch.empty(cap, self.row_width, dtype=torch.float32,
                                device=self.device),
                    torch.empty(1, dtype=torch.int32, device=self.device),
                )
                for _ in range(2)
            ]
        pin = [
            (
                torch.empty(cap, dtype=torch.int64, pin_memory=True),
                torch.empty(cap, self.row_width, dtype=torch.float32,
                            pin_memory=True),
                torch.empty(1, dtype=torch.int32, pin_memory=True),
            )
            for _ in range(2)
        ]
        counted = [torch.cuda.Event() for _ in range(2)]
        copied = [torch.cuda.Event() for _ in range(2)]

        def stage(k: int) -> int:
            """Queue window k (compaction, count readback, then the copy of
            exactly ``count`` rows); returns its count."""
            b = k % 2
            d_signs, d_rows, d_count = dev[b]
            p_signs, p_rows, p_count = pin[b]
            with torch.cuda.stream(st):
                self._C.store_export_window(
                    self.keys, self.arena, k * cap,
                    min(self.n_slots, (k + 1) * cap), d_signs, d_rows, d_count,
                )
                p_count.copy_(d_count, non_blocking=True)
                counted[b].record(st)
                counted[b].synchronize()
                c = int(p_count.item())
                if c:
                    p_signs[:c].copy_(d_signs[:c], non_blocking=True)
                    p_rows[:c].copy_(d_rows[:c], non_blocking=True)
                copied[b].record(st)
            return c

        c = stage(0)
        for k in range(n_win):
            c_next = stage(k + 1) if k + 1 < n_win else 0
            b = k % 2
            copied[b].synchronize()
            if c:
                yield (
                    pin[b][0][:c].numpy().view(np.uint64),
                    pin[b][1][:c].numpy(),
                )
            c = c_next
        sp = self.spill.export() if self.spill is not None and len(self.spill) else None
        if sp is not None:
            sp_keys, sp_rows = sp
            for lo in range(0, len(sp_keys), chunk_rows):
                yield (
                    hashing.splitmix64_inv(sp_keys[lo:lo + chunk_rows]),
                    sp_rows[lo:lo + chunk_rows],
                )

    def import_chunk(self, signs: np.ndarray, inner: np.ndarray) -> None:
        """One chunk of a streamed load: staged through pinned memory; the
        sign mixing, the slot claim, the eviction log and the row-width
        adaptation all run in ``store_import_signs``."""
        n = len(signs)
        if n == 0:
            return
        assert inner.shape[0] == n and inner.shape[1] > 0
        p_signs = torch.empty(n, dtype=torch.int64, pin_memory=True)
        p_rows = torch.empty(n, inner.shape[1], dtype=torch.float32, pin_memory=True)
        np.copyto(p_signs.numpy().view(np.uint64), signs, casting="same_kind")
        np.copyto(p_rows.numpy(), inner, casting="same_kind")
        signs_t = p_signs.to(self.device, non_blocking=True)
        rows_t = p_rows.to(self.device, non_blocking=True)
        tick = self.next_tick()
        ev = self._evict_buffers(n)
        self._C.store_import_signs(
            self.keys, self.ticks, self.arena, signs_t, rows_t, tick,
            float(self.optimizer.state_init(self.dim)), *ev, self._imported,
        )
        self._import_offered += n
        self._drain_evictions(ev)

    def finish_import(self) -> int:
        if self._import_offered == 0:
            return 0
        dropped = self._import_offered - int(self._imported.item())
        self._import_offered = 0
        self._imported.zero_()
        return dropped

    def clear(self) -> None:
        self.keys.zero_()
        self.ticks.zero_()
        self.arena.zero_()


def make_store(
    dim: int,
    capacity: int,
    optimizer: Optimizer,
    hyper: EmbeddingConfig,
    device: torch.device,
    spill_capacity: int = 0,
) -> EmbeddingStoreBase:
    if device.type == "cuda":
        return HipEmbeddingStore(dim, capacity, optimizer, hyper, device, spill_capacity)
    return CpuEmbeddingStore(dim, capacity, optimizer, hyper, device, spill_capacity)
