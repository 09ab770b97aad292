// persia_amd HIP kernels (gfx950 / CDNA4, wave64).
//
// MI355X-native replacements for the reference's CPU hot loops:
//  * set-associative HBM hash table  <- EvictionMap LRU + per-sign locks
//    (rust/persia-embedding-holder/src/eviction_map.rs,
//     embedding_parameter_service/mod.rs:162-262)
//  * fused gather + segment-sum      <- add_assign_avx2 summation
//    (embedding_worker_service/mod.rs:486-629, persia-simd lib.rs:4-18)
//  * ordered gradient scatter        <- per-sign HashMap grad accumulation
//    (embedding_worker_service/mod.rs:782-814)
//  * fused row-wise sparse optimizers + weight bound
//    (persia-simd lib.rs:21-251, exact-math variants)
//
// Layout: keys u64[n_slots] (0 = empty), ticks u32[n_slots], arena
// f32[n_slots, row_width], row = [emb(dim) | opt_state].  Buckets of 8
// slots (one 64B cache line of keys); probe scans 4 consecutive buckets.
//
// Concurrency contract (matches the engine's stream discipline):
//  * keys within one lookup/update call are unique (deduped upstream), with
//    one exception: the wire lookup (store_lookup with f16 rows) takes the
//    padded all-to-all receive buffer as it arrives, `world` sorted buckets
//    that repeat a key once per source rank and carry the empty key as
//    padding.  probe_claim gives every occurrence of a key the same slot and
//    is_new to exactly one of them; the claimed rows are initialized in a
//    launch that precedes the gather launch, so every occurrence reads the
//    initialized row.  The owner-side update dedups the buffer first;
//  * lookup calls are serialized on one stream (ForwardPipeline);
//  * an update may overlap a lookup; claims use atomicCAS on the key word,
//    so the only hazard is an eviction racing an in-flight update of the
//    evicted row — bounded-staleness noise the PERSIA algorithm tolerates
//    (SURVEY §7 hard part 2); it cannot corrupt the table structure.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hipcub/hipcub.hpp>

#include "common.h"
#include "optim.h"
#include "probe.h"

using ull = unsigned long long;

namespace {

// Column ownership of one lane.  Dims that divide the wave pack G = 64/dim
// keys (or segments) per wave: lane -> key `sub`, the single column c0.
// Every other dim gives the whole wave to one key: columns c0 = lane,
// lane + 64, ...  `st` is both the column stride and the subgroup width.
struct PaLanes {
  int G, sub, c0, st;
};
__device__ __forceinline__ PaLanes pa_lanes(int lane, int dim) {
  PaLanes l;
  l.G = (dim < PA_WAVE && (PA_WAVE % dim) == 0) ? PA_WAVE / dim : 1;
  l.sub = (l.G > 1) ? lane / dim : 0;
  l.c0 = (l.G > 1) ? lane % dim : lane;
  l.st = (l.G > 1) ? dim : PA_WAVE;
  return l;
}

// Seeded init of a freshly claimed row: emb columns from the sign's seed
// (bit-identical to core/store.py row_init), optimizer state to state_init.
__device__ __forceinline__ void pa_init_row(float* row, ull key,
                                            int dim, int row_width, double lo,
                                            double hi, float state_init,
                                            int c0, int st) {
  const uint64_t seed = pa_init_seed(pa_splitmix64_inv((uint64_t)key));
  for (int c = c0; c < dim; c += st) row[c] = pa_init_val(seed, c, lo, hi);
  for (int c = dim + c0; c < row_width; c += st) row[c] = state_init;
}

// ---------------------------------------------------------------- store probe

// Find the slot holding key k, or -1.  Bucket loads hit one cache line.
__device__ __forceinline__ long long probe_find(const ull* __restrict__ keys,
                                                int64_t n_buckets, ull k) {
  const int64_t mask = n_buckets - 1;
  int64_t b = (int64_t)(k & (ull)mask);
  for (int p = 0; p < PA_PROBE_BUCKETS; ++p) {
    const int64_t base = ((b + p) & mask) * PA_BUCKET_SIZE;
#pragma unroll
    for (int s = 0; s < PA_BUCKET_SIZE; ++s) {
      if (keys[base + s] == k) return base + s;
    }
  }
  return -1;
}

// Update hint of one unique key (see scatter_update_multi_kernel): the
// gradient row of its only position, or -1 when the key has several
// positions or that position belongs to a raw slot — the update then walks
// ustarts/perm/seg_id as it does without hints.
__device__ __forceinline__ long long pa_src_hint(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ seg_id,
    int64_t lo_p, int64_t hi_p) {
  if (hi_p - lo_p != 1) return -1;
  const int64_t s = seg_id[perm[lo_p]];
  return s >= 0 ? (long long)s : -1;
}

// Eviction log (host-DRAM spill tier): a claim that evicts appends the
// victim's key to evict_keys and remembers the log index so init_gather can
// copy the victim ROW out before overwriting it — the engine drains the log
// into the host tier (SURVEY §7.7 spill design).
__global__ void probe_claim_kernel(ull* __restrict__ table_keys,
                                   unsigned* __restrict__ ticks,
                                   const ull* __restrict__ query,
                                   int64_t n, int64_t n_buckets, int train,
                                   unsigned tick, float admit_prob,
                                   long long* __restrict__ out_slot,
                                   int* __restrict__ out_new,
                                   ull* __restrict__ evict_keys,
                                   int* __restrict__ evict_count,
                                   long long* __restrict__ out_evict_idx,
                                   const long long* __restrict__ n_dev,
                                   const int64_t* __restrict__ ustarts,
                                   const int64_t* __restrict__ perm,
                                   const int64_t* __restrict__ seg_id,
                                   long long* __restrict__ src_hint) {
  // n_dev: device-side element count (padded-dedup path — the true unique
  // count is produced on-GPU so the host never synchronizes); n is the
  // grid-sizing upper bound
  if (n_dev) n = *n_dev;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ull k = query[i];
  // src_hint (optional, with ustarts/perm/seg_id): this thread's key is
  // unique key i of a dedup, so its source hint rides along — three small
  // loads that overlap the probe
  if (src_hint)
    src_hint[i] = pa_src_hint(perm, seg_id, ustarts[i], ustarts[i + 1]);
  if (k == PA_EMPTY_KEY) {
    // a2a padding sentinel (distributed recv buffers): never probed — the
    // empty key would match every free slot
    out_slot[i] = -1;
    out_new[i] = 0;
    if (out_evict_idx) out_evict_idx[i] = -1;
    return;
  }
  long long slot;
  int is_new = 0;
  ull victim = 0;
  if (train) {
    bool admitted = true;
    if (admit_prob < 1.0f) {
      // stochastic admission re-rolled per tick (store.py _admitted)
      const double u = pa_u01(pa_splitmix64(k ^ (ull)tick));
      admitted = u < (double)admit_prob;
    }
    if (admitted) {
      slot = probe_claim(table_keys, ticks, n_buckets, k, tick, &is_new,
                         evict_keys ? &victim : nullptr);
    } else {
      slot = probe_find(table_keys, n_buckets, k);
    }
  } else {
    slot = probe_find(table_keys, n_buckets, k);
  }
  if (slot >= 0) ticks[slot] = tick;
  out_slot[i] = slot;
  out_new[i] = is_new;
  long long eidx = -1;
  if (evict_keys && victim != 0) {
    eidx = (long long)atomicAdd(evict_count, 1);
    evict_keys[eidx] = victim;
  }
  if (out_evict_idx) out_evict_idx[i] = eidx;
}

// one wave per key: init freshly claimed rows, then gather emb -> out.
// OutT = f32 (local path) or f16 (distributed wire: the gathered rows go
// straight onto the xGMI all-to-all, so the wire cast is fused here).
//
// INIT and GATHER select the two halves.  Unique keys take both in one
// launch: the wave that initializes a row is the only one that reads it.  A
// wire buffer repeats keys across its buckets, and only one occurrence of a
// fresh key is the claimer (is_new), so a training wire lookup runs
// <INIT, !GATHER> and then <!INIT, GATHER>: the launch boundary orders every
// init before every read, whichever occurrence claimed.
__device__ __forceinline__ void pa_store_out(float v, float* p) { *p = v; }
__device__ __forceinline__ void pa_store_out(float v, __half* p) {
  *p = __float2half(v);
}
template <typename OutT, bool INIT, bool GATHER>
__global__ void init_gather_kernel(float* __restrict__ arena,
                                   const ull* __restrict__ query,
                                   const long long* __restrict__ slots,
                                   const int* __restrict__ is_new,
                                   OutT* __restrict__ out, int64_t n, int dim,
                                   int row_width, double lo, double hi,
                                   float state_init,
                                   const long long* __restrict__ evict_idx,
                                   float* __restrict__ evict_rows,
                                   const long long* __restrict__ n_dev) {
  if (n_dev) n = *n_dev;
  const int wave = threadIdx.x / PA_WAVE;
  const int lane = threadIdx.x % PA_WAVE;
  const int waves_per_block = blockDim.x / PA_WAVE;
  const PaLanes L = pa_lanes(lane, dim);
  const int c0 = L.c0, st = L.st;
  const int64_t n_waveitems = (n + L.G - 1) / L.G;
  for (int64_t w = (int64_t)blockIdx.x * waves_per_block + wave;
       w < n_waveitems; w += (int64_t)gridDim.x * waves_per_block) {
    const int64_t i = w * L.G + L.sub;
    if (i >= n) continue;
    const long long slot = slots[i];
    OutT* dst = out + i * dim;
    if (slot < 0) {
      if (GATHER)
        for (int c = c0; c < dim; c += st) pa_store_out(0.0f, dst + c);
      continue;
    }
    float* row = arena + (int64_t)slot * row_width;
    if (INIT && is_new[i]) {
      if (evict_rows && evict_idx[i] >= 0) {
        // spill: save the victim's full row before overwriting it
        float* spill = evict_rows + evict_idx[i] * row_width;
        for (int c = c0; c < row_width; c += st) spill[c] = row[c];
      }
      pa_init_row(row, query[i], dim, row_width, lo, hi, state_init, c0, st);
    }
    if (GATHER)
      for (int c = c0; c < dim; c += st) pa_store_out(row[c], dst + c);
  }
}

// init + DIRECT f16 scatter to the per-position sum rows (fast-path variant
// of init_gather_kernel: the all-single-ID path has exactly one id per
// segment, so segment p's sum IS the row of the unique key at sorted
// position p — writing sums[perm[p]] straight from the arena skips the
// [nnz, dim] f32 rows round-trip that segment_sum would re-read).
__global__ void init_scatter_kernel(float* __restrict__ arena,
                                    const ull* __restrict__ query,
                                    const long long* __restrict__ slots,
                                    const int* __restrict__ is_new,
                                    const int64_t* __restrict__ perm,
                                    const int64_t* __restrict__ ustarts,
                                    __half* __restrict__ sums, int64_t n,
                                    int dim, int row_width, double lo,
                                    double hi, float state_init,
                                    const long long* __restrict__ n_dev) {
  if (n_dev) n = *n_dev;
  const int wave = threadIdx.x / PA_WAVE;
  const int lane = threadIdx.x % PA_WAVE;
  const int waves_per_block = blockDim.x / PA_WAVE;
  const PaLanes L = pa_lanes(lane, dim);
  const int c0 = L.c0, st = L.st;
  const int64_t n_waveitems = (n + L.G - 1) / L.G;
  for (int64_t w = (int64_t)blockIdx.x * waves_per_block + wave;
       w < n_waveitems; w += (int64_t)gridDim.x * waves_per_block) {
    const int64_t i = w * L.G + L.sub;
    if (i >= n) continue;
    const long long slot = slots[i];
    const int64_t lo_p = ustarts[i], hi_p = ustarts[i + 1];
    if (slot < 0) {
      for (int64_t p = lo_p; p < hi_p; ++p) {
        __half* dst = sums + perm[p] * dim;
        for (int c = c0; c < dim; c += st) dst[c] = __float2half(0.0f);
      }
      continue;
    }
    float* row = arena + (int64_t)slot * row_width;
    if (is_new[i])
      pa_init_row(row, query[i], dim, row_width, lo, hi, state_init, c0, st);
    for (int64_t p = lo_p; p < hi_p; ++p) {
      __half* dst = sums + perm[p] * dim;
      for (int c = c0; c < dim; c += st) dst[c] = __float2half(row[c]);
    }
  }
}

// Dual-key init/scatter for full-wave dims (see scatter_update_multi_kernel
// for the rationale: the slots->arena->sums chain is latency-bound on random
// row granules; two independent keys per wave double the in-flight loads).
// The rare fresh-init path falls back to per-key sequential work.
__global__ void init_scatter2_kernel(float* __restrict__ arena,
                                     const ull* __restrict__ query,
                                     const long long* __restrict__ slots,
                                     const int* __restrict__ is_new,
                                     const int64_t* __restrict__ perm,
                                     const int64_t* __restrict__ ustarts,
                                     __half* __restrict__ sums, int64_t n,
                                     int dim, int row_width, double lo,
                                     double hi, float state_init,
                                     const long long* __restrict__ n_dev) {
  if (n_dev) n = *n_dev;
  const int wave = threadIdx.x / PA_WAVE;
  const int lane = threadIdx.x % PA_WAVE;
  const int waves_per_block = blockDim.x / PA_WAVE;
  const int64_t n_waveitems = (n + 1) / 2;
  for (int64_t w = (int64_t)blockIdx.x * waves_per_block + wave;
       w < n_waveitems; w += (int64_t)gridDim.x * waves_per_block) {
    const int64_t iA = w * 2, iB = w * 2 + 1;
    const bool okB0 = iB < n;
    const long long slotA = slots[iA];
    const long long slotB = okB0 ? slots[iB] : -1;
    // fresh rows: seeded init first (rare in steady state)
    if (is_new[iA] && slotA >= 0)
      pa_init_row(arena + (int64_t)slotA * row_width, query[iA], dim,
                  row_width, lo, hi, state_init, lane, PA_WAVE);
    if (okB0 && is_new[iB] && slotB >= 0)
      pa_init_row(arena + (int64_t)slotB * row_width, query[iB], dim,
                  row_width, lo, hi, state_init, lane, PA_WAVE);
    const int64_t loA = ustarts[iA], hiA = ustarts[iA + 1];
    const int64_t loB = okB0 ? ustarts[iB] : 0;
    const int64_t hiB = okB0 ? ustarts[iB + 1] : 0;
    const float* rowA = slotA >= 0 ? arena + (int64_t)slotA * row_width : nullptr;
    const float* rowB = slotB >= 0 ? arena + (int64_t)slotB * row_width : nullptr;
    if (hiA - loA == 1 && hiB - loB == 1) {  // common single-position case
      __half* dstA = sums + perm[loA] * dim;
      __half* dstB = sums + perm[loB] * dim;
      for (int c = lane; c < dim; c += PA_WAVE) {
        const float vA = rowA ? rowA[c] : 0.0f;
        const float vB = rowB ? rowB[c] : 0.0f;
        dstA[c] = __float2half(vA);
        dstB[c] = __float2half(vB);
      }
    } else {
      for (int64_t p = loA; p < hiA; ++p) {
        __half* dst = sums + perm[p] * dim;
        for (int c = lane; c < dim; c += PA_WAVE)
          dst[c] = __float2half(rowA ? rowA[c] : 0.0f);
      }
      for (int64_t p = loB; p < hiB; ++p) {
        __half* dst = sums + perm[p] * dim;
        for (int c = lane; c < dim; c += PA_WAVE)
          dst[c] = __float2half(rowB ? rowB[c] : 0.0f);
      }
    }
  }
}

// ------------------------------------------------------------- sparse update

// one wave per key: probe (lane-parallel over the 32-slot window) + fused
// row-wise optimizer + weight bound.
// opt / p0..p3: see PaOptArgs (optim.h).  FTRL (opt 3) is an instantiation of
// its own, chosen by the launcher: as one more arm next to the others it cost
// the SGD/Adagrad/Adam code registers and a wave per SIMD.
template <bool FTRL>
__global__ void update_kernel(ull* __restrict__ table_keys,
                              unsigned* __restrict__ ticks,
                              float* __restrict__ arena,
                              const ull* __restrict__ query,
                              const float* __restrict__ grads, int64_t n,
                              int dim, int row_width, int64_t n_buckets,
                              int opt, float p0, float p1, float p2, float p3,
                              float b1_power, float b2_power,
                              float weight_bound,
                              int* __restrict__ skipped) {
  const int wave = threadIdx.x / PA_WAVE;
  const int lane = threadIdx.x % PA_WAVE;
  const int waves_per_block = blockDim.x / PA_WAVE;
  const int64_t mask = n_buckets - 1;
  const PaOptArgs oa =
      pa_opt_args(opt, p0, p1, p2, p3, b1_power, b2_power, weight_bound);
  for (int64_t i = (int64_t)blockIdx.x * waves_per_block + wave; i < n;
       i += (int64_t)gridDim.x * waves_per_block) {
    const ull k = query[i];
    if (k == PA_EMPTY_KEY) continue;  // a2a padding: silent skip
    // lane-parallel probe: lanes 0..31 each inspect one slot of the window
    long long slot = -1;
    const int64_t b = (int64_t)(k & (ull)mask);
    if (lane < PA_PROBE_BUCKETS * PA_BUCKET_SIZE) {
      const int p = lane / PA_BUCKET_SIZE;
      const int s = lane % PA_BUCKET_SIZE;
      const int64_t j = ((b + p) & mask) * PA_BUCKET_SIZE + s;
      if (table_keys[j] == k) slot = j;
    }
    const unsigned long long found = __ballot(slot >= 0);
    if (found == 0) {
      if (lane == 0) atomicAdd(&skipped[0], 1);
      continue;
    }
    const int src = __ffsll((long long)found) - 1;
    slot = __shfl(slot, src);
    float* row = arena + (int64_t)slot * row_width;
    const float* g = grads + i * dim;
    // row-level NaN skip (finer-grained than the reference's per-slot skip,
    // mod.rs:731-746: a NaN gradient never touches the table)
    bool has_nan = false;
    for (int c = lane; c < dim; c += PA_WAVE) has_nan |= isnan(g[c]);
    if (__ballot(has_nan) != 0) {
      if (lane == 0) atomicAdd(&skipped[1], 1);
      continue;
    }
    if constexpr (FTRL) {
      for (int c = lane; c < dim; c += PA_WAVE) {
        const PaFtrlRow r =
            pa_ftrl(oa, row[c], row[dim + c], row[2 * dim + c], g[c]);
        row[c] = r.w;
        row[dim + c] = r.z;
        row[2 * dim + c] = r.n;
      }
    } else if (opt == 0) {  // SGD
      for (int c = lane; c < dim; c += PA_WAVE)
        row[c] = pa_sgd(oa, row[c], g[c]);
    } else if (opt == 1) {  // Adagrad
      if (pa_adagrad_shared(oa)) {
        // shared scalar accumulator at row[dim]
        const float acc = row[dim];
        float gsq = 0.0f;
        for (int c = lane; c < dim; c += PA_WAVE) {
          row[c] = pa_adagrad_w(oa, row[c], acc, g[c]);
          gsq += g[c] * g[c];
        }
#pragma unroll
        for (int off = PA_WAVE / 2; off > 0; off >>= 1)
          gsq += __shfl_down(gsq, off);
        if (lane == 0) row[dim] = pa_adagrad_shared_acc(oa, acc, gsq, dim);
      } else {
        for (int c = lane; c < dim; c += PA_WAVE) {
          const float acc = row[dim + c];
          row[c] = pa_adagrad_w(oa, row[c], acc, g[c]);
          row[dim + c] = pa_adagrad_acc(oa, acc, g[c]);
        }
      }
    } else if (opt == 2) {  // Adam
      for (int c = lane; c < dim; c += PA_WAVE) {
        const float m = pa_adam_m<true>(oa, row[dim + c], g[c]);
        const float v = pa_adam_v<true>(oa, row[2 * dim + c], g[c]);
        row[c] = pa_adam_w(oa, row[c], m, v);
        row[dim + c] = m;
        row[2 * dim + c] = v;
      }
    }
  }
}

// ------------------------------------------------------------------ sign prep

// raw ids -> routed keys: fold into the slot's feature-group prefix space
// (indices_add_prefix, mod.rs:403-429) then splitmix64-mix (the mixed key is
// the dedup sort key AND the shard router).  Slot of position i found by
// binary search over slot_starts (S is small).
__global__ void sign_prep_kernel(const ull* __restrict__ values,
                                 const int64_t* __restrict__ slot_starts,
                                 const ull* __restrict__ prefixes, int n_slots,
                                 ull spacing, ull* __restrict__ out,
                                 int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = n_slots;  // find slot: slot_starts[s] <= i < slot_starts[s+1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (i >= slot_starts[mid]) lo = mid; else hi = mid;
  }
  const ull prefix = prefixes[lo];
  ull sign = values[i];
  if (prefix != 0) sign = sign % spacing + prefix;
  ull k = pa_splitmix64(sign);
  if (k == PA_EMPTY_KEY) k = 0xD1B54A32D192ED03ull;  // empty-sentinel remap
  out[i] = k;
}

// sign prep with hashstack expansion (reference
// indices_to_hashstack_indices, embedding_worker_service/mod.rs:348-400):
// each raw id of a slot with hash_stack_rounds=R becomes R bucketed ids
// (round r: iterate splitmix64, fold into [r*size,(r+1)*size)), laid out
// position-major per sample ([r0 ids..., r1 ids...] inside each sample's
// span) to match the CPU path bit-for-bit.  One thread per INPUT id writes
// its R outputs; slots with R==0 pass through the plain prefix+mix path.
__global__ void sign_prep_stack_kernel(
    const ull* __restrict__ values, const int64_t* __restrict__ in_starts,
    const int64_t* __restrict__ out_starts, const ull* __restrict__ prefixes,
    const int* __restrict__ rounds, const int64_t* __restrict__ sizes,
    const int64_t* __restrict__ off_starts,
    const int64_t* __restrict__ all_offs,  // EXPANDED per-slot seg offsets
    int n_slots, ull spacing, ull* __restrict__ out, int64_t n_in) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_in) return;
  int lo = 0, hi = n_slots;  // find slot: in_starts[s] <= i < in_starts[s+1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (i >= in_starts[mid]) lo = mid; else hi = mid;
  }
  const int s = lo;
  const ull prefix = prefixes[s];
  const int R = rounds[s];
  if (R == 0) {
    ull sign = values[i];
    if (prefix != 0) sign = sign % spacing + prefix;
    ull k = pa_splitmix64(sign);
    if (k == PA_EMPTY_KEY) k = 0xD1B54A32D192ED03ull;
    out[out_starts[s] + (i - in_starts[s])] = k;
    return;
  }
  const int64_t j = i - in_starts[s];  // slot-local input position
  // sample b: expanded offsets E[b] = off[b]*R, so E[b] <= j*R < E[b+1]
  const int64_t* E = all_offs + off_starts[s];
  const int64_t nE = off_starts[s + 1] - off_starts[s];
  const int64_t key = j * (int64_t)R;
  int64_t blo = 0, bhi = nE - 1;
  while (bhi - blo > 1) {
    const int64_t mid = (blo + bhi) >> 1;
    if (key >= E[mid]) blo = mid; else bhi = mid;
  }
  const int64_t seg_lo = E[blo] / R, seg_hi = E[blo + 1] / R;
  const int64_t base = out_starts[s] + E[blo];
  const int64_t size = sizes[s];
  ull h = values[i];
  for (int r = 0; r < R; ++r) {
    h = pa_splitmix64(h);
    ull sign = h % (ull)size + (ull)((int64_t)r * size);
    if (prefix != 0) sign = sign % spacing + prefix;
    ull k = pa_splitmix64(sign);
    if (k == PA_EMPTY_KEY) k = 0xD1B54A32D192ED03ull;
    out[base + (int64_t)r * (seg_hi - seg_lo) + (j - seg_lo)] = k;
  }
}

// sign prep of a bag group with hashstack slots, straight from the group's one
// upload (engine pack_stack_bag_buffer):
//   values[nnz_in] ‖ slot_starts[S+1] ‖ offsets[S, B+1] ‖ in_starts[S+1]
// slot_starts and offsets are in the EXPANDED position space (a slot of R
// rounds has offsets*R; they are bag_plan_kernel's `plan`), in_starts are the
// slots' starts in `values`.  Keys and layout are sign_prep_stack_kernel's,
// round-major inside each sample's span.  One thread per OUTPUT position q,
// so the stores are coalesced and no thread writes R strided keys: with
// t = q - E[b] inside sample b of expanded span [E[b], E[b+1]) and
// len = (E[b+1] - E[b]) / R, the round is r = t / len and the id is
// values[in_start + E[b]/R + t % len]; the thread iterates splitmix64 r+1
// times on it (R(R+1)/2 mixes per id against R of the thread-per-id form:
// ALU work beside two binary searches).  Slots with R == 0 take the plain
// prefix+mix path.  The host builder has checked the offsets; rounds that
// disagree with them give wrong keys, never a read outside `values` (len, r
// and the id index are clamped).
__global__ void sign_prep_bags_kernel(
    const ull* __restrict__ values, const int64_t* __restrict__ slot_starts,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ in_starts,
    const ull* __restrict__ prefixes, const int* __restrict__ rounds,
    const int64_t* __restrict__ sizes, int n_slots, int64_t B, ull spacing,
    ull* __restrict__ out, int64_t n_in, int64_t n_out) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_out) return;
  int lo = 0, hi = n_slots;  // slot_starts[s] <= q < slot_starts[s+1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (q >= slot_starts[mid]) lo = mid; else hi = mid;
  }
  const int s = lo;
  const ull prefix = prefixes[s];
  const int R = rounds[s];
  const int64_t p = q - slot_starts[s];  // slot-local output position
  int64_t src = p;
  int r = 0;
  if (R > 0) {
    const int64_t* E = offsets + (int64_t)s * (B + 1);
    int64_t blo = 0, bhi = B;  // E[blo] <= p < E[blo + 1]
    while (bhi - blo > 1) {
      const int64_t mid = (blo + bhi) >> 1;
      if (p >= E[mid]) blo = mid; else bhi = mid;
    }
    const int64_t e0 = E[blo];
    int64_t len = (E[blo + 1] - e0) / R;
    if (len < 1) len = 1;
    const int64_t t = p - e0;
    const int64_t rr = t / len;
    r = rr < R ? (int)rr : R - 1;
    src = e0 / R + t % len;
  }
  src += in_starts[s];
  if (src < 0) src = 0;
  if (src >= n_in) src = n_in - 1;  // n_out > 0 implies n_in > 0
  ull sign = values[src];
  if (R > 0) {
    const ull size = (ull)sizes[s];
    ull h = sign;
    for (int i = 0; i <= r; ++i) h = pa_splitmix64(h);
    sign = h % size + (ull)r * size;
  }
  if (prefix != 0) sign = sign % spacing + prefix;
  ull k = pa_splitmix64(sign);
  if (k == PA_EMPTY_KEY) k = 0xD1B54A32D192ED03ull;
  out[q] = k;
}

// ------------------------------------------------------- padded a2a routing
// The owner partition of the SORTED uniq keys is a range partition (owner =
// (hi32*world)>>32 is monotone in the key), so per-owner segment starts are
// world binary searches — one tiny kernel — and the pack is one grid-stride
// scatter.  Replaces a ~10-dispatch torch chain that cost the producer
// thread ~0.5 ms/batch of issue time.
__global__ void a2a_bounds_kernel(const ull* __restrict__ uniq,
                                  const long long* __restrict__ n_dev,
                                  long long n_pad, int world,
                                  long long* __restrict__ starts) {
  const long long n = n_dev ? *n_dev : n_pad;
  const int r = threadIdx.x;
  if (r > world) return;
  if (r == 0) { starts[0] = 0; return; }
  if (r == world) { starts[world] = n; return; }
  // smallest key with owner >= r: hi32 >= ceil(r * 2^32 / world)
  const ull hi_min =
      (ull)((((unsigned __int128)r << 32) + (ull)world - 1) / (ull)world);
  const ull thresh = hi_min << 32;
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (uniq[mid] < thresh) lo = mid + 1; else hi = mid;
  }
  starts[r] = lo;
}

__global__ void a2a_scatter_kernel(const ull* __restrict__ uniq,
                                   const long long* __restrict__ n_dev,
                                   long long n_pad,
                                   const long long* __restrict__ starts,
                                   int world, long long cap,
                                   ull* __restrict__ send,
                                   int64_t* __restrict__ idx,
                                   long long* __restrict__ overflow) {
  const long long n = n_dev ? *n_dev : n_pad;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pad) return;
  const long long dummy = (long long)world * cap;
  if (i >= n) {  // dedup padding tail
    idx[i] = dummy;
    return;
  }
  const ull k = uniq[i];
  const int o = (int)(((k >> 32) * (ull)world) >> 32);
  const long long pos = i - starts[o];
  long long d = dummy;
  if (pos < cap) {
    d = (long long)o * cap + pos;
    send[d] = k;
  } else {
    atomicAdd((unsigned long long*)overflow, 1ull);
  }
  idx[i] = d;
}

__global__ void iota_i64_kernel(int64_t* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = i;
}

// flags[i] = (sorted[i] != sorted[i-1]); flags[0] = 1  (boundary marks for
// the rank scan — replaces a ones+slice+ne op chain)
__global__ void neq_flags_kernel(const ull* __restrict__ sorted,
                                 bool* __restrict__ flags, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flags[i] = (i == 0) || (sorted[i] != sorted[i - 1]);
}

// Fixed-shape dedup epilogue: after sort + neq + rank=cumsum(neq)-1 (all
// shape-static ATen ops), ONE pass finalizes inverse/uniq/ustarts into
// nnz-padded buffers and writes the true unique count to a device scalar —
// the host never learns U, so the whole lookup issues without a single
// synchronization (the probe/gather/update kernels read U from n_dev).
__global__ void dedup_finalize_kernel(
    const ull* __restrict__ svals_flipped, const int64_t* __restrict__ perm,
    const bool* __restrict__ neq, const int64_t* __restrict__ rank,
    int64_t n, ull flip, int64_t* __restrict__ inverse,
    ull* __restrict__ uniq, int64_t* __restrict__ ustarts,
    long long* __restrict__ u_count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rank[i];
  inverse[perm[i]] = r;
  if (neq[i]) {
    uniq[r] = svals_flipped[i] ^ flip;
    ustarts[r] = i;
  }
  if (i == n - 1) {
    u_count[0] = r + 1;
    ustarts[r + 1] = n;
  }
}

// --------------------------------------------------------------- import rows

__global__ void import_kernel(ull* __restrict__ table_keys,
                              unsigned* __restrict__ ticks,
                              float* __restrict__ arena,
                              const ull* __restrict__ query,
                              const float* __restrict__ rows, int64_t n,
                              int row_width, int64_t n_buckets, unsigned tick,
                              ull* __restrict__ evict_keys,
                              int* __restrict__ evict_count,
                              float* __restrict__ evict_rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int is_new;
  ull victim = 0;
  const long long slot =
      probe_claim(table_keys, ticks, n_buckets, query[i], tick, &is_new,
                  evict_keys ? &victim : nullptr);
  if (slot < 0) return;
  ticks[slot] = tick;
  float* dst = arena + (int64_t)slot * row_width;
  if (evict_keys && victim != 0) {
    const long long eidx = (long long)atomicAdd(evict_count, 1);
    evict_keys[eidx] = victim;
    float* spill = evict_rows + eidx * row_width;
    for (int c = 0; c < row_width; ++c) spill[c] = dst[c];
  }
  const float* src = rows + i * row_width;
  for (int c = 0; c < row_width; ++c) dst[c] = src[c];
}

// ----------------------------------------------------- fused gather + seg-sum

// out[s, :] = seg_scale[s] * sum_{k in [off[s], off[s+1])} rows[inverse[k], :]
// One wave per segment (all sum-slots of a dim-group in ONE launch);
// f32 accumulate; f16 store (reference wire dtype, persia-common lib.rs:88-99).
// Small dims pack 64/dim segments per wave (sub-wave groups) so dim-8
// tables still use all lanes; large dims stride as before.
template <typename RowT>
__global__ void segment_sum_kernel(const RowT* __restrict__ rows,
                                   const int64_t* __restrict__ inverse,
                                   const int64_t* __restrict__ seg_offsets,
                                   const float* __restrict__ seg_scale,
                                   __half* __restrict__ out, int64_t n_seg,
                                   int dim) {
  const int wave = threadIdx.x / PA_WAVE;
  const int lane = threadIdx.x % PA_WAVE;
  const int waves_per_block = blockDim.x / PA_WAVE;
  const PaLanes L = pa_lanes(lane, dim);
  const int64_t n_waveitems = (n_seg + L.G - 1) / L.G;
  for (int64_t w = (int64_t)blockIdx.x * waves_per_block + wave;
       w < n_waveitems; w += (int64_t)gridDim.x * waves_per_block) {
    const int64_t s = w * L.G + L.sub;
    if (s >= n_seg) continue;
    const int64_t lo = seg_offsets[s], hi = seg_offsets[s + 1];
    const float scale = seg_scale ? seg_scale[s] : 1.0f;
    __half* dst = out + s * dim;
    for (int c = L.c0; c < dim; c += L.st) {
      float acc = 0.0f;
      for (int64_t k = lo; k < hi; ++k) {
        acc += pa_to_float(rows[inverse[k] * dim + c]);
      }
      dst[c] = __float2half(acc * scale);
    }
  }
}

// ------------------------------------------------ bag (multi-ID) sum lookup

// Segment plan of a bag group, from the uploaded per-slot CSR.  `plan` is
// slot_starts[S+R+1] followed by offsets[S+R, B+1] (each slot's offsets
// relative to its start; the host builder has checked them: first 0,
// non-decreasing, last == the slot's length).  The first S slots are sum
// slots: segment s*B+b is sample b of slot s.
//   cat_offsets[s*B+b] = slot_starts[s] + offsets[s][b]
//   cat_offsets[S*B]   = slot_starts[S]   (nnz without raw slots)
//   seg_id[p]          = segment of position p
//   seg_lens[seg]      = (float)len
//   seg_scale[seg]     = sqrt slot ? rsqrtf(max(len, 1)) : 1   (optional)
// Thread i serves segment i and position i.  A position finds its slot and
// sample by binary search (the last start <= p: empty slots and empty bags
// repeat a start, and the position belongs behind them).
//
// The R slots behind them are raw (sequence) slots, R = 0 for a pure bag
// group.  raw_meta is row_base[R] followed by sfs[R]: raw slot r owns the
// B*sfs[r] rows from row_base[r] on, one per cell (sample b, column c), in
// the group's gradient-row space of n_rows rows (sum segments first).  A raw
// position with column c = q - offsets[b] feeds cell row_base + b*sfs + c, or
// nothing (-1) when it is truncated (c >= sfs); a cell is a segment of at
// most one position.
//   seg_id[p]          = c < sfs ? row_base[r] + b*sfs[r] + c : -1
//   seg_scale[row]     = 1 over the raw rows (the update indexes it by row)
//   raw_num[r*B+b]     = min(len, sfs[r])
__global__ void bag_plan_kernel(const int64_t* __restrict__ plan,
                                const int* __restrict__ sqrt_flags, int S,
                                int64_t B, int64_t nnz,
                                int64_t* __restrict__ cat_offsets,
                                int64_t* __restrict__ seg_id,
                                float* __restrict__ seg_lens,
                                float* __restrict__ seg_scale, int R,
                                const int64_t* __restrict__ raw_meta,
                                int64_t n_rows,
                                int64_t* __restrict__ raw_num) {
  const int64_t n_seg = (int64_t)S * B;
  const int64_t n_raw = (int64_t)R * B;
  const int64_t n_head = (R ? n_rows : n_seg) + 1;  // n_rows >= n_seg + n_raw
  const int64_t n = n_head > nnz ? n_head : nnz;
  const int64_t* slot_starts = plan;
  const int64_t* offsets = plan + S + R + 1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n_seg) {
      const int64_t s = i / B, b = i % B;
      const int64_t* off = offsets + s * (B + 1);
      const int64_t len = off[b + 1] - off[b];
      cat_offsets[i] = slot_starts[s] + off[b];
      seg_lens[i] = (float)len;
      if (seg_scale)
        seg_scale[i] =
            sqrt_flags[s] ? rsqrtf(fmaxf((float)len, 1.0f)) : 1.0f;
    } else {
      if (i == n_seg) cat_offsets[i] = slot_starts[S];
      if (seg_scale && i < n_rows) seg_scale[i] = 1.0f;
    }
    if (i < n_raw) {
      const int64_t r = i / B, b = i % B;
      const int64_t* off = offsets + (S + r) * (B + 1);
      const int64_t len = off[b + 1] - off[b], sfs = raw_meta[R + r];
      raw_num[i] = len < sfs ? len : sfs;
    }
    if (i < nnz) {
      int lo = 0, hi = S + R;  // slot_starts[lo] <= i < slot_starts[lo + 1]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (i >= slot_starts[mid]) lo = mid; else hi = mid;
      }
      const int64_t* off = offsets + (int64_t)lo * (B + 1);
      const int64_t q = i - slot_starts[lo];
      int64_t blo = 0, bhi = B;  // off[blo] <= q < off[blo + 1]
      while (bhi - blo > 1) {
        const int64_t mid = (blo + bhi) >> 1;
        if (q >= off[mid]) blo = mid; else bhi = mid;
      }
      if (lo < S) {
        seg_id[i] = (int64_t)lo * B + blo;
      } else {
        const int64_t c = q - off[blo], sfs = raw_meta[R + lo - S];
        seg_id[i] = c < sfs ? raw_meta[lo - S] + blo * sfs + c : -1;
      }
    }
  }
}

// out[s, c] = f16( (sum_{k in [off[s], off[s+1])} row(k)[c]) * scale[s] ),
// row(k) = arena[slots[inverse[k]]]; a slot < 0 (miss, not admitted) adds
// nothing.  segment_sum_kernel reading the arena: same lane layout, and the
// adds run in position order in f32 from +0, so the bits equal a gather into
// a [U, dim] buffer followed by segment_sum (a skipped row is that path's
// +0 row: the accumulator is never -0, so adding +0 leaves it).
//
// inverse -> slots -> arena row is three dependent loads per addend on random
// row granules (the latency chain of scatter_update_multi_kernel and
// init_scatter2_kernel).  Addends go in groups of PA_BAG_DEPTH: all index
// loads, then all slot loads, then all row loads are issued before the first
// add.  Every load of a group is unconditional (a position past the bag's
// end re-reads the bag's last one, a missing row reads row 0, and the value
// is replaced by +0 afterwards), so no branch separates the loads and the
// compiler keeps them in flight together.  A lane holds T columns
// (c0 + t*st) of the row per pass; dims above T*64 take further passes.
#define PA_BAG_DEPTH 4
template <int T>
__global__ void bag_sum_kernel(const float* __restrict__ arena,
                               const long long* __restrict__ slots,
                               const int64_t* __restrict__ inverse,
                               const int64_t* __restrict__ seg_offsets,
                               const float* __restrict__ seg_scale,
                               __half* __restrict__ out, int64_t n_seg,
                               int dim, int row_width) {
  const int wave = threadIdx.x / PA_WAVE;
  const int lane = threadIdx.x % PA_WAVE;
  const int waves_per_block = blockDim.x / PA_WAVE;
  const PaLanes L = pa_lanes(lane, dim);
  const int64_t n_waveitems = (n_seg + L.G - 1) / L.G;
  for (int64_t w = (int64_t)blockIdx.x * waves_per_block + wave;
       w < n_waveitems; w += (int64_t)gridDim.x * waves_per_block) {
    const int64_t s = w * L.G + L.sub;
    if (s >= n_seg) continue;
    const int64_t lo = seg_offsets[s], hi = seg_offsets[s + 1];
    const float scale = seg_scale ? seg_scale[s] : 1.0f;
    __half* dst = out + s * dim;
    for (int cb = L.c0; cb < dim; cb += T * L.st) {
      int col[T];  // a column past dim re-reads cb; it is never stored
#pragma unroll
      for (int t = 0; t < T; ++t)
        col[t] = (cb + t * L.st < dim) ? cb + t * L.st : cb;
      float acc[T];
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = 0.0f;
      for (int64_t k = lo; k < hi; k += PA_BAG_DEPTH) {
        int64_t u[PA_BAG_DEPTH];
        long long sl[PA_BAG_DEPTH];
        float v[PA_BAG_DEPTH][T];
#pragma unroll
        for (int j = 0; j < PA_BAG_DEPTH; ++j)
          u[j] = inverse[(k + j < hi) ? k + j : hi - 1];
#pragma unroll
        for (int j = 0; j < PA_BAG_DEPTH; ++j) sl[j] = slots[u[j]];
#pragma unroll
        for (int j = 0; j < PA_BAG_DEPTH; ++j) {
          const float* row =
              arena + (int64_t)(sl[j] >= 0 ? sl[j] : 0) * row_width;
#pragma unroll
          for (int t = 0; t < T; ++t) v[j][t] = row[col[t]];
        }
#pragma unroll
        for (int j = 0; j < PA_BAG_DEPTH; ++j) {
          const bool live = (k + j < hi) && sl[j] >= 0;
#pragma unroll
          for (int t = 0; t < T; ++t) acc[t] += live ? v[j][t] : 0.0f;
        }
      }
#pragma unroll
      for (int t = 0; t < T; ++t)
        if (cb + t * L.st < dim)
          dst[cb + t * L.st] = __float2half(acc[t] * scale);
    }
  }
}

// ------------------------------------------------ raw (sequence) slot gather

// The fixed-size tensor of the raw slots of a group, straight from the arena.
// Cell (r, b, c) is row row_base[r] + b*sfs[r] + c of `out` (the group's leaf
// base, sum rows first) and entry row - S*B of `mask`; with len the length of
// sample b in slot r,
//   c < len : f16(arena[slots[inverse[start_r + off[b] + c]]]), mask 1; a
//             slot < 0 (miss, not admitted) gives a +0 row, the mask stays 1
//   c >= len: +0 row, mask 0
// `plan` and raw_meta are bag_plan_kernel's.  A wave item is one chunk of
// G * PA_RAW_DEPTH consecutive cells of one sample (G = 64/dim cells side by
// side for the dims pa_lanes packs): items are numbered slot-major, then
// sample, then chunk, so a wave finds its slot by walking the R chunk counts.
//
// bag_sum_kernel's load chain with one addend per cell: the index, slot and
// row loads of a lane's PA_RAW_DEPTH cells are issued level by level, all
// unconditional (an absent cell re-reads position 0, a missing row reads row
// 0, and the value is replaced by +0), before the first store.  The kernel
// walks cells, not unique keys, so it never reads the unique count.  The
// caller launches it only when the group has at least one id, in blocks of
// 256 threads (the launch bound keeps the 8-column instantiation out of
// scratch).
#define PA_RAW_DEPTH 4
template <int T>
__global__ void __launch_bounds__(256) raw_gather_kernel(const float* __restrict__ arena,
                                  const long long* __restrict__ slots,
                                  const int64_t* __restrict__ inverse,
                                  const int64_t* __restrict__ plan,
                                  const int64_t* __restrict__ raw_meta,
                                  __half* __restrict__ out,
                                  __half* __restrict__ mask, int S, int R,
                                  int64_t B, int64_t n_rows, unsigned n_items,
                                  int dim, int row_width) {
  const int wave = threadIdx.x / PA_WAVE;
  const int lane = threadIdx.x % PA_WAVE;
  const int waves_per_block = blockDim.x / PA_WAVE;
  const PaLanes L = pa_lanes(lane, dim);
  const unsigned CH = (unsigned)L.G * PA_RAW_DEPTH;  // cells per wave item
  const int64_t* slot_starts = plan;
  const int64_t* offsets = plan + S + R + 1;
  const int64_t n_sum_rows = (int64_t)S * B;
  for (unsigned w = blockIdx.x * waves_per_block + wave; w < n_items;
       w += gridDim.x * waves_per_block) {
    int r = 0;
    unsigned rem = w;
    int64_t sfs = raw_meta[R];
    unsigned nch = ((unsigned)sfs + CH - 1) / CH;  // chunks per sample
    while (r < R - 1 && rem >= (unsigned)B * nch) {
      rem -= (unsigned)B * nch;
      ++r;
      sfs = raw_meta[R + r];
      nch = ((unsigned)sfs + CH - 1) / CH;
    }
    const int64_t b = rem / nch;
    if (b >= B) continue;
    const int64_t c_base = (int64_t)(rem % nch) * CH;
    const int64_t* off = offsets + (int64_t)(S + r) * (B + 1);
    const int64_t p0 = slot_starts[S + r] + off[b];
    const int64_t len = off[b + 1] - off[b];
    const int64_t row0 = raw_meta[r] + b * sfs;  // cell (r, b, 0)
    int64_t c[PA_RAW_DEPTH];
    bool present[PA_RAW_DEPTH];
#pragma unroll
    for (int j = 0; j < PA_RAW_DEPTH; ++j) {
      c[j] = c_base + j * L.G + L.sub;
      present[j] = c[j] < len && c[j] < sfs;
    }
    for (int cb = L.c0; cb < dim; cb += T * L.st) {
      int col[T];  // a column past dim re-reads cb; it is never stored
#pragma unroll
      for (int t = 0; t < T; ++t)
        col[t] = (cb + t * L.st < dim) ? cb + t * L.st : cb;
      int64_t u[PA_RAW_DEPTH];
      long long sl[PA_RAW_DEPTH];
      float v[PA_RAW_DEPTH][T];
#pragma unroll
      for (int j = 0; j < PA_RAW_DEPTH; ++j)
        u[j] = inverse[present[j] ? p0 + c[j] : 0];
#pragma unroll
      for (int j = 0; j < PA_RAW_DEPTH; ++j) sl[j] = slots[u[j]];
#pragma unroll
      for (int j = 0; j < PA_RAW_DEPTH; ++j) {
        const float* row =
            arena + (int64_t)(sl[j] >= 0 ? sl[j] : 0) * row_width;
#pragma unroll
        for (int t = 0; t < T; ++t) v[j][t] = row[col[t]];
      }
#pragma unroll
      for (int j = 0; j < PA_RAW_DEPTH; ++j) {
        const int64_t cell = row0 + c[j];
        if (c[j] >= sfs || cell < n_sum_rows || cell >= n_rows) continue;
        const bool live = present[j] && sl[j] >= 0;
        __half* dst = out + cell * dim;
#pragma unroll
        for (int t = 0; t < T; ++t)
          if (cb + t * L.st < dim)
            dst[cb + t * L.st] = __float2half(live ? v[j][t] : 0.0f);
        if (cb == 0)  // the lane that holds column 0, on its first pass
          mask[cell - n_sum_rows] = __float2half(present[j] ? 1.0f : 0.0f);
      }
    }
  }
}

// --------------------------------------------------- ordered gradient scatter

// out[u, :] += sum_{p in [ustart[u], ustart[u+1])} grads[seg_id[perm[p]], :]
//              * seg_scale[seg_id[perm[p]]]
// One wave per unique sign — deterministic (ordered), atomic-free: the
// positions of a unique key are contiguous in sort order.  Positions with
// seg_id < 0 (raw-slot positions, handled by a separate indexed add) are
// skipped.
template <typename GradT, bool ACCUMULATE>
__global__ void grad_scatter_kernel(const GradT* __restrict__ grads,
                                    const int64_t* __restrict__ perm,
                                    const int64_t* __restrict__ ustarts,
                                    const int64_t* __restrict__ seg_id,
                                    const float* __restrict__ seg_scale,
                                    float* __restrict__ out, int64_t n_unique,
                                    int dim) {
  const int wave = threadIdx.x / PA_WAVE;
  const int lane = threadIdx.x % PA_WAVE;
  const int waves_per_block = blockDim.x / PA_WAVE;
  for (int64_t u = (int64_t)blockIdx.x * waves_per_block + wave; u < n_unique;
       u += (int64_t)gridDim.x * waves_per_block) {
    const int64_t lo = ustarts[u], hi = ustarts[u + 1];
    float* dst = out + u * dim;
    for (int c = lane; c < dim; c += PA_WAVE) {
      float acc[1] = {0.0f};
      pa_reduce_positions<1>(acc, grads, perm, seg_id, seg_scale, lo, hi, dim, c,
                          PA_WAVE);
      if (ACCUMULATE) dst[c] += acc[0]; else dst[c] = acc[0];
    }
  }
}

// Indexed wire variant: out[out_idx[u], :] = acc in the WIRE dtype — packs
// each unique key's reduced gradient straight into the a2a send buffer
// (layout [world, cap] by owner rank), skipping both the [U, dim] f32
// intermediate and a separate pack pass.  n_unique comes from n_dev (padded
// sync-free dedup); invalid/overflowed entries point at the dummy tail row.
// Small dims pack 64/dim keys per wave (sub-wave groups).
template <typename OutT>
__global__ void grad_scatter_idx_kernel(
    const __half* __restrict__ grads, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ ustarts, const int64_t* __restrict__ seg_id,
    const float* __restrict__ seg_scale, const int64_t* __restrict__ out_idx,
    OutT* __restrict__ out, int64_t n_unique, int dim,
    const long long* __restrict__ n_dev) {
  if (n_dev) n_unique = *n_dev;
  const int wave = threadIdx.x / PA_WAVE;
  const int lane = threadIdx.x % PA_WAVE;
  const int waves_per_block = blockDim.x / PA_WAVE;
  const PaLanes L = pa_lanes(lane, dim);
  const int64_t n_waveitems = (n_unique + L.G - 1) / L.G;
  for (int64_t w = (int64_t)blockIdx.x * waves_per_block + wave;
       w < n_waveitems; w += (int64_t)gridDim.x * waves_per_block) {
    const int64_t u = w * L.G + L.sub;
    if (u >= n_unique) continue;
    const int64_t lo = ustarts[u], hi = ustarts[u + 1];
    OutT* dst = out + out_idx[u] * dim;
    for (int c = L.c0; c < dim; c += L.st) {
      float acc[1] = {0.0f};
      pa_reduce_positions<1>(acc, grads, perm, seg_id, seg_scale, lo, hi, dim, c,
                          L.st);
      pa_store_out(acc[0], dst + c);
    }
  }
}

// ------------------------------------------- fused scatter + optimizer update

// One wave per unique sign: reduce its gradient from the per-segment grads
// (ordered, via the sort permutation) straight into registers, probe the
// table, and apply the optimizer — no intermediate [U, dim] buffer.
// Supports dim <= 8*PA_WAVE (register-resident grad row).
template <bool HINTS, bool FTRL>
__global__ void scatter_update_kernel(
    ull* __restrict__ table_keys, unsigned* __restrict__ ticks,
    float* __restrict__ arena, const ull* __restrict__ uniq,
    const __half* __restrict__ grads, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ ustarts, const int64_t* __restrict__ seg_id,
    const float* __restrict__ seg_scale, int64_t n, int dim, int row_width,
    int64_t n_buckets, int opt, float p0, float p1, float p2, float p3,
    float b1_power, float b2_power, float weight_bound,
    int* __restrict__ skipped, const long long* __restrict__ n_dev,
    const long long* __restrict__ slot_hint,
    const long long* __restrict__ src_hint, int64_t n_slots, int64_t n_src) {
  if (n_dev) n = *n_dev;
  const int wave = threadIdx.x / PA_WAVE;
  const int lane = threadIdx.x % PA_WAVE;
  const int waves_per_block = blockDim.x / PA_WAVE;
  const int64_t mask = n_buckets - 1;
  const PaOptArgs oa =
      pa_opt_args(opt, p0, p1, p2, p3, b1_power, b2_power, weight_bound);
  // small dims pack 64/dim keys per wave (sub-wave groups)
  const PaLanes L = pa_lanes(lane, dim);
  const int G = L.G, sub = L.sub, c0 = L.c0, st = L.st;
  const int sg = L.st;  // subgroup width
  const ull sg_mask = (sg >= 64) ? ~0ull : ((1ull << sg) - 1ull);
  const int64_t n_waveitems = (n + G - 1) / G;
  constexpr int WINDOW = PA_PROBE_BUCKETS * PA_BUCKET_SIZE;
  for (int64_t w = (int64_t)blockIdx.x * waves_per_block + wave;
       w < n_waveitems; w += (int64_t)gridDim.x * waves_per_block) {
    const int64_t u = w * G + sub;
    const ull k = (u < n) ? uniq[u] : 0;
    // empty key = a2a padding: silent skip (the empty key would match every
    // free table slot in the probe)
    const bool active = (u < n) && (k != PA_EMPTY_KEY);
    // update hints (see scatter_update_multi_kernel): the key verify, the
    // gradient row and its scale load straight off the hints, none waiting
    // on another.  An absent or out-of-range hint is no hint; a slot hint
    // that fails the verify falls back to the window probe, a key without a
    // source hint to the ustarts/perm/seg_id walk.
    long long sh = -1, sr = -1;
    if (HINTS && active) {
      sh = slot_hint[u];
      sr = src_hint[u];
    }
    if (sh < 0 || sh >= n_slots) sh = -1;
    if (sr < 0 || sr >= n_src) sr = -1;
    ull kv = PA_EMPTY_KEY;
    if (sh >= 0) kv = table_keys[sh];
    float hsc = 0.0f;
    __half hg[8];
    if (sr >= 0) {
      hsc = seg_scale ? seg_scale[sr] : 1.0f;
      const __half* g = grads + (int64_t)sr * dim;
#pragma unroll
      for (int t = 0; t < 8; ++t)
        if (c0 + t * st < dim) hg[t] = g[c0 + t * st];
    }
    long long slot = (sh >= 0 && kv == k) ? sh : -1;
    // subgroup-parallel probe over the 32-slot window
    if (active && slot < 0) {
      const int64_t b = (int64_t)(k & (ull)mask);
      for (int it = 0; it * sg + c0 < WINDOW; ++it) {
        const int widx = it * sg + c0;
        const int p = widx / PA_BUCKET_SIZE;
        const int s = widx % PA_BUCKET_SIZE;
        const int64_t j = ((b + p) & mask) * PA_BUCKET_SIZE + s;
        if (table_keys[j] == k) slot = j;
      }
    }
    const unsigned long long found = __ballot(slot >= 0);
    const unsigned long long sub_found = (found >> (sub * sg)) & sg_mask;
    bool ok = active;
    if (ok && sub_found == 0) {
      if (c0 == 0) atomicAdd(&skipped[0], 1);
      ok = false;
    }
    if (ok)
      slot = __shfl(slot, sub * sg + __ffsll((long long)sub_found) - 1);
    // ordered gradient reduction into registers
    float acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = 0.0f;
    if (ok) {
      if (sr >= 0) {
        // pa_reduce_positions over the key's one position
        if (hsc != 0.0f) {
#pragma unroll
          for (int t = 0; t < 8; ++t)
            if (c0 + t * st < dim) acc[t] += __half2float(hg[t]) * hsc;
        }
      } else {
        pa_reduce_positions<8>(acc, grads, perm, seg_id, seg_scale, ustarts[u],
                               ustarts[u + 1], dim, c0, st);
      }
    }
    bool has_nan = false;
    if (ok)
      for (int t = 0, c = c0; c < dim; c += st, ++t) has_nan |= isnan(acc[t]);
    const unsigned long long nanb = __ballot(has_nan);
    if (ok && ((nanb >> (sub * sg)) & sg_mask) != 0) {
      if (c0 == 0) atomicAdd(&skipped[1], 1);
      ok = false;
    }
    if (!ok) continue;
    float* row = arena + (int64_t)slot * row_width;
    // nontemporal arena traffic: each row is touched exactly once per step
    // and this kernel overlaps the dense graph on another stream — keeping
    // ~0.5 GB/step of one-shot data out of L2 leaves it to the GEMMs
    if constexpr (FTRL) {
      for (int t = 0, c = c0; c < dim; c += st, ++t) {
        const float z0 = __builtin_nontemporal_load(&row[dim + c]);
        const float n0 = __builtin_nontemporal_load(&row[2 * dim + c]);
        const float w0 = __builtin_nontemporal_load(&row[c]);
        const PaFtrlRow r = pa_ftrl(oa, w0, z0, n0, acc[t]);
        __builtin_nontemporal_store(r.w, &row[c]);
        __builtin_nontemporal_store(r.z, &row[dim + c]);
        __builtin_nontemporal_store(r.n, &row[2 * dim + c]);
      }
    } else if (opt == 0) {  // SGD
      for (int t = 0, c = c0; c < dim; c += st, ++t) {
        const float w0 = __builtin_nontemporal_load(&row[c]);
        __builtin_nontemporal_store(pa_sgd(oa, w0, acc[t]), &row[c]);
      }
    } else if (opt == 1) {  // Adagrad
      if (pa_adagrad_shared(oa)) {
        const float a0 = row[dim];
        float gsq = 0.0f;
        for (int t = 0, c = c0; c < dim; c += st, ++t) {
          const float w0 = __builtin_nontemporal_load(&row[c]);
          __builtin_nontemporal_store(pa_adagrad_w(oa, w0, a0, acc[t]), &row[c]);
          gsq += acc[t] * acc[t];
        }
        for (int off = sg / 2; off > 0; off >>= 1)
          gsq += __shfl_down(gsq, off, sg);
        if (c0 == 0) row[dim] = pa_adagrad_shared_acc(oa, a0, gsq, dim);
      } else {
        for (int t = 0, c = c0; c < dim; c += st, ++t) {
          const float a0 = __builtin_nontemporal_load(&row[dim + c]);
          const float w0 = __builtin_nontemporal_load(&row[c]);
          __builtin_nontemporal_store(pa_adagrad_w(oa, w0, a0, acc[t]), &row[c]);
          __builtin_nontemporal_store(pa_adagrad_acc<true>(oa, a0, acc[t]),
                                      &row[dim + c]);
        }
      }
    } else if (opt == 2) {  // Adam
      for (int t = 0, c = c0; c < dim; c += st, ++t) {
        const float m = pa_adam_m(
            oa, __builtin_nontemporal_load(&row[dim + c]), acc[t]);
        const float v = pa_adam_v(
            oa, __builtin_nontemporal_load(&row[2 * dim + c]), acc[t]);
        const float w0 = __builtin_nontemporal_load(&row[c]);
        __builtin_nontemporal_store(pa_adam_w(oa, w0, m, v), &row[c]);
        __builtin_nontemporal_store(m, &row[dim + c]);
        __builtin_nontemporal_store(v, &row[2 * dim + c]);
      }
    }
  }
}

// Per-key register vector of the multi-key kernels below.
template <int T>
using PaAccVec = float __attribute__((ext_vector_type(T)));

// Arena rows reach the helpers below through per-key pointer arrays; the
// explicit global address space keeps their loads and stores global ones
// (the compiler otherwise falls back to flat addressing for them).
using PaGlobalF = __attribute__((address_space(1))) float;

// The arena values of Q rows held in registers between their load and the
// optimizer step: weights, up to two per-column state vectors, and the
// vectorwise-shared Adagrad scalar.  Lane `lane` owns columns lane + t*64.
template <int Q, int T>
struct PaRowRegs {
  PaAccVec<T> w0[Q], s1[Q], s2[Q];
  float a0[Q];
};

// nontemporal arena traffic: each row is touched exactly once per step and
// the kernel overlaps the dense graph on another stream — keeping ~0.5
// GB/step of one-shot data out of L2 leaves it to the GEMMs
template <int Q, int T, bool FTRL>
__device__ __forceinline__ void pa_load_rows(PaRowRegs<Q, T>& r,
                                             const PaOptArgs& oa,
                                             const bool (&ok)[Q],
                                             float* const (&rows)[Q], int dim,
                                             int lane) {
  PaGlobalF* rowk[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) rowk[q] = (PaGlobalF*)rows[q];
  const bool shared = !FTRL && oa.opt == 1 && pa_adagrad_shared(oa);
#pragma unroll
  for (int q = 0; q < Q; ++q)
    r.a0[q] = (shared && ok[q]) ? rowk[q][dim] : 0.0f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int c = lane + t * PA_WAVE;
    if (c >= dim) continue;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      if (!ok[q]) continue;
      if (FTRL || (oa.opt != 0 && !shared))
        r.s1[q][t] = __builtin_nontemporal_load(&rowk[q][dim + c]);
      if (FTRL || oa.opt == 2)
        r.s2[q][t] = __builtin_nontemporal_load(&rowk[q][2 * dim + c]);
      r.w0[q][t] = __builtin_nontemporal_load(&rowk[q][c]);
    }
  }
}

// Optimizer step of Q loaded rows (pa_load_rows) and their stores.
template <int Q, int T, bool FTRL>
__device__ __forceinline__ void pa_step_rows(const PaRowRegs<Q, T>& r,
                                             const PaOptArgs& oa,
                                             const bool (&ok)[Q],
                                             float* const (&rows)[Q],
                                             const PaAccVec<T> (&acc)[Q],
                                             int dim, int lane) {
  PaGlobalF* rowk[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) rowk[q] = (PaGlobalF*)rows[q];
  if constexpr (FTRL) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int c = lane + t * PA_WAVE;
      if (c >= dim) continue;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (!ok[q]) continue;
        const PaFtrlRow n =
            pa_ftrl(oa, r.w0[q][t], r.s1[q][t], r.s2[q][t], acc[q][t]);
        __builtin_nontemporal_store(n.w, &rowk[q][c]);
        __builtin_nontemporal_store(n.z, &rowk[q][dim + c]);
        __builtin_nontemporal_store(n.n, &rowk[q][2 * dim + c]);
      }
    }
  } else if (oa.opt == 0) {  // SGD
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int c = lane + t * PA_WAVE;
      if (c >= dim) continue;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (!ok[q]) continue;
        __builtin_nontemporal_store(pa_sgd(oa, r.w0[q][t], acc[q][t]),
                                    &rowk[q][c]);
      }
    }
  } else if (oa.opt == 1) {  // Adagrad
    if (pa_adagrad_shared(oa)) {
      float gsq[Q] = {};
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int c = lane + t * PA_WAVE;
        if (c >= dim) continue;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          if (!ok[q]) continue;
          __builtin_nontemporal_store(
              pa_adagrad_w(oa, r.w0[q][t], r.a0[q], acc[q][t]), &rowk[q][c]);
          gsq[q] += acc[q][t] * acc[q][t];
        }
      }
#pragma unroll
      for (int off = PA_WAVE / 2; off > 0; off >>= 1)
#pragma unroll
        for (int q = 0; q < Q; ++q) gsq[q] += __shfl_down(gsq[q], off);
      if (lane == 0)
#pragma unroll
        for (int q = 0; q < Q; ++q)
          if (ok[q])
            rowk[q][dim] = pa_adagrad_shared_acc(oa, r.a0[q], gsq[q], dim);
    } else {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int c = lane + t * PA_WAVE;
        if (c >= dim) continue;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          if (!ok[q]) continue;
          __builtin_nontemporal_store(
              pa_adagrad_w(oa, r.w0[q][t], r.s1[q][t], acc[q][t]),
              &rowk[q][c]);
          __builtin_nontemporal_store(
              pa_adagrad_acc(oa, r.s1[q][t], acc[q][t]), &rowk[q][dim + c]);
        }
      }
    }
  } else if (oa.opt == 2) {  // Adam
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int c = lane + t * PA_WAVE;
      if (c >= dim) continue;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (!ok[q]) continue;
        const float m = pa_adam_m(oa, r.s1[q][t], acc[q][t]);
        const float v = pa_adam_v(oa, r.s2[q][t], acc[q][t]);
        __builtin_nontemporal_store(pa_adam_w(oa, r.w0[q][t], m, v),
                                    &rowk[q][c]);
        __builtin_nontemporal_store(m, &rowk[q][dim + c]);
        __builtin_nontemporal_store(v, &rowk[q][2 * dim + c]);
      }
    }
  }
}

// The unhinted form of the same step: per column, load the values of all Q
// keys, then do the dependent math and store.  Nothing is held across
// columns, which keeps the kernel without hints at its register budget.
template <int Q, int T, bool FTRL>
__device__ __forceinline__ void pa_update_rows(const PaOptArgs& oa,
                                               const bool (&ok)[Q],
                                               float* const (&rowk)[Q],
                                               const PaAccVec<T> (&acc)[Q],
                                               int dim, int lane) {
  const int opt = oa.opt;
  // every branch below loads for all Q keys before the dependent math
  if constexpr (FTRL) {
    for (int t = 0, c = lane; c < dim; c += PA_WAVE, ++t) {
      float w0[Q], z0[Q], n0[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        z0[q] = ok[q] ? __builtin_nontemporal_load(&rowk[q][dim + c]) : 0.0f;
        n0[q] = ok[q] ? __builtin_nontemporal_load(&rowk[q][2 * dim + c]) : 0.0f;
        w0[q] = ok[q] ? __builtin_nontemporal_load(&rowk[q][c]) : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (!ok[q]) continue;
        const PaFtrlRow r = pa_ftrl(oa, w0[q], z0[q], n0[q], acc[q][t]);
        __builtin_nontemporal_store(r.w, &rowk[q][c]);
        __builtin_nontemporal_store(r.z, &rowk[q][dim + c]);
        __builtin_nontemporal_store(r.n, &rowk[q][2 * dim + c]);
      }
    }
  } else if (opt == 0) {  // SGD
    for (int t = 0, c = lane; c < dim; c += PA_WAVE, ++t) {
      float w0[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q)
        w0[q] = ok[q] ? __builtin_nontemporal_load(&rowk[q][c]) : 0.0f;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (!ok[q]) continue;
        __builtin_nontemporal_store(pa_sgd(oa, w0[q], acc[q][t]), &rowk[q][c]);
      }
    }
  } else if (opt == 1) {  // Adagrad
    if (pa_adagrad_shared(oa)) {
      float a0[Q], gsq[Q] = {};
#pragma unroll
      for (int q = 0; q < Q; ++q) a0[q] = ok[q] ? rowk[q][dim] : 0.0f;
      for (int t = 0, c = lane; c < dim; c += PA_WAVE, ++t) {
        float w0[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q)
          w0[q] = ok[q] ? __builtin_nontemporal_load(&rowk[q][c]) : 0.0f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          if (!ok[q]) continue;
          __builtin_nontemporal_store(
              pa_adagrad_w(oa, w0[q], a0[q], acc[q][t]), &rowk[q][c]);
          gsq[q] += acc[q][t] * acc[q][t];
        }
      }
#pragma unroll
      for (int off = PA_WAVE / 2; off > 0; off >>= 1)
#pragma unroll
        for (int q = 0; q < Q; ++q) gsq[q] += __shfl_down(gsq[q], off);
      if (lane == 0)
#pragma unroll
        for (int q = 0; q < Q; ++q)
          if (ok[q])
            rowk[q][dim] = pa_adagrad_shared_acc(oa, a0[q], gsq[q], dim);
    } else {
      for (int t = 0, c = lane; c < dim; c += PA_WAVE, ++t) {
        float w0[Q], a0[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          a0[q] = ok[q] ? __builtin_nontemporal_load(&rowk[q][dim + c]) : 0.0f;
          w0[q] = ok[q] ? __builtin_nontemporal_load(&rowk[q][c]) : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          if (!ok[q]) continue;
          __builtin_nontemporal_store(
              pa_adagrad_w(oa, w0[q], a0[q], acc[q][t]), &rowk[q][c]);
          __builtin_nontemporal_store(pa_adagrad_acc(oa, a0[q], acc[q][t]),
                                      &rowk[q][dim + c]);
        }
      }
    }
  } else if (opt == 2) {  // Adam
    for (int t = 0, c = lane; c < dim; c += PA_WAVE, ++t) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (!ok[q]) continue;
        const float m = pa_adam_m(
            oa, __builtin_nontemporal_load(&rowk[q][dim + c]), acc[q][t]);
        const float v = pa_adam_v(
            oa, __builtin_nontemporal_load(&rowk[q][2 * dim + c]), acc[q][t]);
        const float w0 = __builtin_nontemporal_load(&rowk[q][c]);
        __builtin_nontemporal_store(pa_adam_w(oa, w0, m, v), &rowk[q][c]);
        __builtin_nontemporal_store(m, &rowk[q][dim + c]);
        __builtin_nontemporal_store(v, &rowk[q][2 * dim + c]);
      }
    }
  }
}

// Multi-key variant for full-wave dims: one wave updates Q unique keys with
// interleaved loads — the single-key kernel is latency-bound on its probe ->
// grads -> arena dependent chain (random 1-2 KB row granules), so Q
// independent in-flight chains per wave buy memory-level parallelism the
// scheduler can't extract across grid-stride iterations (ballots/shfl block
// software pipelining).  Q = 4 for dim <= 128, Q = 2 for dim <= 256: the
// register-resident gradient is acc[Q][8/Q] either way.  Probe: 64/Q lanes
// per key, each lane scans Q/2 of the 32 window slots; after it the whole
// wave works on every key.  All per-key loops unroll over the constexpr Q so
// the per-key arrays stay in registers.
//
// Update hints (slot_hint/src_hint, both or neither) shorten that chain.
// The lookup of the same batch already knew each key's slot and, for a key
// with one position, its gradient row.  A wave whose Q keys all carry
// in-range hints issues the key verify, the gradient rows, their scales and
// the arena rows straight off the hints, none waiting on another; it keeps
// what it loaded only if every table_keys[slot] still holds its key (a later
// lookup may have evicted the row and reused the slot), and never stores a
// row it did not verify.  Any other wave takes the probe and the
// ustarts/perm/seg_id walk below, as every wave does without hints.  The
// hinted wave is a special case of the all-single branch and computes the
// same expressions, so the results are the same bits.
template <int Q, bool HINTS, bool FTRL>
__global__ void scatter_update_multi_kernel(
    ull* __restrict__ table_keys, unsigned* __restrict__ ticks,
    float* __restrict__ arena, const ull* __restrict__ uniq,
    const __half* __restrict__ grads, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ ustarts, const int64_t* __restrict__ seg_id,
    const float* __restrict__ seg_scale, int64_t n, int dim, int row_width,
    int64_t n_buckets, int opt, float p0, float p1, float p2, float p3,
    float b1_power, float b2_power, float weight_bound,
    int* __restrict__ skipped, const long long* __restrict__ n_dev,
    const long long* __restrict__ slot_hint,
    const long long* __restrict__ src_hint, int64_t n_slots, int64_t n_src) {
  static_assert(Q == 2 || Q == 4, "two or four keys per wave");
  constexpr int WINDOW = PA_PROBE_BUCKETS * PA_BUCKET_SIZE;  // 32
  constexpr int PL = PA_WAVE / Q;   // probe lanes per key
  constexpr int WS = WINDOW / PL;   // window slots per probe lane
  constexpr int T = 8 / Q;          // columns per lane per key
  constexpr ull PL_MASK = (1ull << PL) - 1ull;
  if (n_dev) n = *n_dev;
  const int wave = threadIdx.x / PA_WAVE;
  const int lane = threadIdx.x % PA_WAVE;
  const int waves_per_block = blockDim.x / PA_WAVE;
  const int64_t mask = n_buckets - 1;
  const PaOptArgs oa =
      pa_opt_args(opt, p0, p1, p2, p3, b1_power, b2_power, weight_bound);
  const int kq = lane / PL;
  const int widx = lane % PL;
  const int64_t n_waveitems = (n + Q - 1) / Q;
  for (int64_t w = (int64_t)blockIdx.x * waves_per_block + wave;
       w < n_waveitems; w += (int64_t)gridDim.x * waves_per_block) {
    const int64_t u = w * Q + kq;
    const ull k = (u < n) ? uniq[u] : 0;
    const bool active = (u < n) && (k != PA_EMPTY_KEY);
    bool ok[Q];
    float* rowk[Q];
    // one register vector per key: a [Q][T] array is a single stack object
    // whose runtime column index t costs more registers than Q small ones
    PaAccVec<T> acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0f;
    PaRowRegs<Q, T> rows;  // HINTS only
    bool hinted = false;
    if constexpr (HINTS) {
      const long long sh = active ? slot_hint[u] : -1;
      const long long sr = active ? src_hint[u] : -1;
      const bool usable = sh >= 0 && sh < n_slots && sr >= 0 && sr < n_src;
      if (__ballot(usable) == ~0ull) {
        const ull kv = table_keys[sh];
        float scq[Q];
        __half graw[Q][T];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const long long shq = __shfl(sh, PL * q);
          const long long srq = __shfl(sr, PL * q);
          ok[q] = true;
          rowk[q] = arena + (int64_t)shq * row_width;
          scq[q] = seg_scale ? seg_scale[srq] : 1.0f;
          const __half* g = grads + (int64_t)srq * dim;
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const int c = lane + t * PA_WAVE;
            if (c < dim) graw[q][t] = g[c];
          }
        }
        pa_load_rows<Q, T, FTRL>(rows, oa, ok, rowk, dim, lane);
        if (__ballot(kv == k) == ~0ull) {
          hinted = true;
          // the all-single expressions below, bit for bit
#pragma unroll
          for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int t = 0; t < T; ++t)
              if (lane + t * PA_WAVE < dim)
                acc[q][t] = (scq[q] != 0.0f)
                                ? scq[q] * __half2float(graw[q][t])
                                : 0.0f;
        }
      }
    }
    if (!hinted) {
      long long slot = -1;
      if (active) {
        const int64_t b = (int64_t)(k & (ull)mask);
#pragma unroll
        for (int h = 0; h < WS; ++h) {
          const int wi = widx + h * PL;
          const int p = wi / PA_BUCKET_SIZE;
          const int s = wi % PA_BUCKET_SIZE;
          const int64_t j = ((b + p) & mask) * PA_BUCKET_SIZE + s;
          if (table_keys[j] == k) slot = j;
        }
      }
      const unsigned long long found = __ballot(slot >= 0);
      const unsigned long long nonzero = __ballot(k != PA_EMPTY_KEY);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const unsigned fq = (unsigned)((found >> (PL * q)) & PL_MASK);
        // empty-key (a2a padding) entries skip silently, not as misses
        ok[q] = (w * Q + q) < n && (nonzero >> (PL * q) & 1ull);
        if (ok[q] && fq == 0) {
          if (lane == 0) atomicAdd(&skipped[0], 1);
          ok[q] = false;
        }
        const long long slotq =
            ok[q] ? __shfl(slot, PL * q + __ffs(fq) - 1) : -1;
        rowk[q] = ok[q] ? arena + (int64_t)slotq * row_width : nullptr;
      }
      // gradient accumulation (whole wave per key; the interleaved
      // single-position fast path is the overwhelmingly common case)
      int64_t lop[Q], hip[Q];
      bool all_single = true;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        lop[q] = ok[q] ? ustarts[w * Q + q] : 0;
        hip[q] = ok[q] ? ustarts[w * Q + q + 1] : 0;
        all_single = all_single && ok[q] && hip[q] - lop[q] == 1;
      }
      if (all_single) {
        // same rule as pa_reduce_positions: seg_id < 0 or scale 0 leaves the
        // key's acc at 0 without multiplying its gradient (uniform per key)
        const __half* gq[Q];
        float scq[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const int64_t s = seg_id[perm[lop[q]]];
          scq[q] = (s >= 0) ? (seg_scale ? seg_scale[s] : 1.0f) : 0.0f;
          gq[q] = grads + (s >= 0 ? s : 0) * dim;
        }
        for (int t = 0, c = lane; c < dim; c += PA_WAVE, ++t) {
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            const float g = __half2float(gq[q][c]);
            acc[q][t] = (scq[q] != 0.0f) ? scq[q] * g : 0.0f;
          }
        }
      } else {
#pragma unroll
        for (int q = 0; q < Q; ++q)
          if (ok[q])
            pa_reduce_positions<T>(acc[q], grads, perm, seg_id, seg_scale,
                                   lop[q], hip[q], dim, lane, PA_WAVE);
      }
    }
    // a NaN row is counted and left untouched (a hinted wave drops what it
    // loaded for it)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      bool has_nan = false;
      for (int t = 0, c = lane; c < dim; c += PA_WAVE, ++t)
        has_nan |= isnan(acc[q][t]);
      if (ok[q] && __ballot(has_nan) != 0) {
        if (lane == 0) atomicAdd(&skipped[1], 1);
        ok[q] = false;
      }
    }
    bool any_ok = false;
#pragma unroll
    for (int q = 0; q < Q; ++q) any_ok = any_ok || ok[q];
    if (!any_ok) continue;
    if constexpr (HINTS) {
      // the rows of all Q keys are loaded before the dependent math
      if (!hinted) pa_load_rows<Q, T, FTRL>(rows, oa, ok, rowk, dim, lane);
      pa_step_rows<Q, T, FTRL>(rows, oa, ok, rowk, acc, dim, lane);
    } else {
      pa_update_rows<Q, T, FTRL>(oa, ok, rowk, acc, dim, lane);
    }
  }
}

inline int n_blocks_for(int64_t work_items, int per_block) {
  int64_t b = (work_items + per_block - 1) / per_block;
  // >> 256 CUs needed to fill the chip; cap and grid-stride beyond
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

// ============================================================ torch bindings

static hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// optional tensor arguments arrive empty when absent
static const long long* count_or_null(const torch::Tensor& u_count) {
  return u_count.numel() ? (const long long*)u_count.data_ptr<int64_t>()
                         : nullptr;
}
static const float* scale_or_null(const torch::Tensor& seg_scale) {
  return seg_scale.numel() ? seg_scale.data_ptr<float>() : nullptr;
}

// u64 radix sort-pairs (keys ascending in UNSIGNED order — exactly the
// dedup/owner-range order; torch.sort would need the sign-flip trick AND
// runs a merge sort with a slow index-iota setup: ~3x the time)
std::vector<torch::Tensor> sort_pairs_u64(torch::Tensor keys) {
  const int64_t n = keys.numel();
  auto opts = torch::TensorOptions().dtype(torch::kInt64).device(keys.device());
  auto iota = torch::empty({n}, opts);
  auto sorted = torch::empty_like(keys);
  auto perm = torch::empty({n}, opts);
  if (n == 0) return {sorted, perm};
  hipStream_t st = cur_stream();
  hipLaunchKernelGGL(iota_i64_kernel, dim3(n_blocks_for(n, 256)), dim3(256),
                     0, st, iota.data_ptr<int64_t>(), n);
  size_t temp_bytes = 0;
  hipcub::DeviceRadixSort::SortPairs(
      nullptr, temp_bytes, (const ull*)keys.data_ptr<int64_t>(),
      (ull*)sorted.data_ptr<int64_t>(),
      (const long long*)iota.data_ptr<int64_t>(),
      (long long*)perm.data_ptr<int64_t>(), n, 0, 64, st);
  auto temp = torch::empty(
      {(int64_t)temp_bytes},
      torch::TensorOptions().dtype(torch::kUInt8).device(keys.device()));
  hipcub::DeviceRadixSort::SortPairs(
      temp.data_ptr(), temp_bytes, (const ull*)keys.data_ptr<int64_t>(),
      (ull*)sorted.data_ptr<int64_t>(),
      (const long long*)iota.data_ptr<int64_t>(),
      (long long*)perm.data_ptr<int64_t>(), n, 0, 64, st);
  return {sorted, perm};
}

torch::Tensor neq_flags(torch::Tensor sorted) {
  const int64_t n = sorted.numel();
  auto flags = torch::empty(
      {n}, torch::TensorOptions().dtype(torch::kBool).device(sorted.device()));
  if (n == 0) return flags;
  hipLaunchKernelGGL(neq_flags_kernel, dim3(n_blocks_for(n, 256)), dim3(256),
                     0, cur_stream(), (const ull*)sorted.data_ptr<int64_t>(),
                     flags.data_ptr<bool>(), n);
  return flags;
}


void store_lookup(torch::Tensor table_keys, torch::Tensor ticks,
                  torch::Tensor arena, torch::Tensor query, torch::Tensor out,
                  int64_t dim, int64_t train, int64_t tick, double lo,
                  double hi, double admit_prob, double state_init,
                  int64_t opt_space, torch::Tensor evict_keys,
                  torch::Tensor evict_count, torch::Tensor evict_rows,
                  torch::Tensor u_count) {
  const int64_t n = query.numel();
  if (n == 0) return;
  const int64_t n_buckets = table_keys.numel() / PA_BUCKET_SIZE;
  const int row_width = (int)(dim + opt_space);
  const bool spill = evict_keys.numel() > 0;
  const long long* n_dev = count_or_null(u_count);
  auto opts = torch::TensorOptions().dtype(torch::kInt64).device(query.device());
  auto slots = torch::empty({n}, opts);
  auto is_new = torch::empty({n}, opts.dtype(torch::kInt32));
  torch::Tensor evict_idx;
  if (spill) evict_idx = torch::empty({n}, opts);
  hipStream_t st = cur_stream();
  hipLaunchKernelGGL(probe_claim_kernel, dim3(n_blocks_for(n, 256)), dim3(256),
                     0, st, (ull*)table_keys.data_ptr<int64_t>(),
                     (unsigned*)ticks.data_ptr<int32_t>(),
                     (const ull*)query.data_ptr<int64_t>(), n, n_buckets,
                     (int)train, (unsigned)tick, (float)admit_prob,
                     (long long*)slots.data_ptr<int64_t>(),
                     is_new.data_ptr<int32_t>(),
                     spill ? (ull*)evict_keys.data_ptr<int64_t>() : nullptr,
                     spill ? evict_count.data_ptr<int32_t>() : nullptr,
                     spill ? (long long*)evict_idx.data_ptr<int64_t>() : nullptr,
                     n_dev, nullptr, nullptr, nullptr, nullptr);
  auto launch = [&](auto kernel, auto* out_ptr) {
    hipLaunchKernelGGL(kernel, dim3(n_blocks_for(n, 4)), dim3(256), 0, st,
                       arena.data_ptr<float>(),
                       (const ull*)query.data_ptr<int64_t>(),
                       (const long long*)slots.data_ptr<int64_t>(),
                       is_new.data_ptr<int32_t>(), out_ptr, n, (int)dim,
                       row_width, lo, hi, (float)state_init,
                       spill ? (const long long*)evict_idx.data_ptr<int64_t>() : nullptr,
                       spill ? evict_rows.data_ptr<float>() : nullptr, n_dev);
  };
  if (out.scalar_type() == torch::kFloat16) {
    // f16 out: distributed wire path (rows go straight onto the a2a).  The
    // query may repeat a key, so a training lookup initializes every claimed
    // row in a launch of its own before any row is read (see
    // init_gather_kernel); an eval lookup claims nothing and only gathers.
    __half* o = (__half*)out.data_ptr<at::Half>();
    if (train) launch(init_gather_kernel<__half, true, false>, o);
    launch(init_gather_kernel<__half, false, true>, o);
  } else {
    launch(init_gather_kernel<float, true, true>, out.data_ptr<float>());
  }
}

// fast-path lookup: probe/claim + fused init/f16-scatter to sum rows
// (single-ID groups only — no spill; see init_scatter_kernel)
//
// Returns the update hints {slot_hint, src_hint} (nnz-padded i64; entries at
// or beyond the unique count are unspecified): the slot probe_claim gave each
// unique key (-1: miss or not admitted) and, when seg_id is given, the
// gradient row of a key with one position (pa_src_hint).  Without seg_id
// (eval lookups, hints switched off) no hints are computed and both are empty.
std::vector<torch::Tensor> store_lookup_sums(
    torch::Tensor table_keys, torch::Tensor ticks, torch::Tensor arena,
    torch::Tensor query, torch::Tensor perm, torch::Tensor ustarts,
    torch::Tensor sums, int64_t dim, int64_t train, int64_t tick, double lo,
    double hi, double admit_prob, double state_init, int64_t opt_space,
    torch::Tensor u_count, torch::Tensor seg_id) {
  const int64_t n = query.numel();
  auto opts = torch::TensorOptions().dtype(torch::kInt64).device(query.device());
  auto slots = torch::empty({n}, opts);
  const bool hints = seg_id.numel() > 0;
  auto src_hint = torch::empty({hints ? n : 0}, opts);
  if (n == 0) return {src_hint, src_hint};
  TORCH_CHECK(!hints || seg_id.numel() >= perm.numel(),
              "store_lookup_sums: seg_id shorter than perm");
  TORCH_CHECK(!hints || ustarts.numel() > n,
              "store_lookup_sums: ustarts shorter than query + 1");
  const int64_t* seg_ptr = hints ? seg_id.data_ptr<int64_t>() : nullptr;
  long long* src_ptr =
      hints ? (long long*)src_hint.data_ptr<int64_t>() : nullptr;
  const int64_t n_buckets = table_keys.numel() / PA_BUCKET_SIZE;
  const int row_width = (int)(dim + opt_space);
  const long long* n_dev = count_or_null(u_count);
  auto is_new = torch::empty({n}, opts.dtype(torch::kInt32));
  hipStream_t st = cur_stream();
  hipLaunchKernelGGL(probe_claim_kernel, dim3(n_blocks_for(n, 256)), dim3(256),
                     0, st, (ull*)table_keys.data_ptr<int64_t>(),
                     (unsigned*)ticks.data_ptr<int32_t>(),
                     (const ull*)query.data_ptr<int64_t>(), n, n_buckets,
                     (int)train, (unsigned)tick, (float)admit_prob,
                     (long long*)slots.data_ptr<int64_t>(),
                     is_new.data_ptr<int32_t>(), nullptr, nullptr, nullptr,
                     n_dev, hints ? ustarts.data_ptr<int64_t>() : nullptr,
                     hints ? perm.data_ptr<int64_t>() : nullptr, seg_ptr,
                     src_ptr);
  const bool dual = !(dim < PA_WAVE && (PA_WAVE % dim) == 0);
  if (dual) {
    hipLaunchKernelGGL(init_scatter2_kernel,
                       dim3(n_blocks_for((n + 1) / 2, 4)), dim3(256), 0, st,
                       arena.data_ptr<float>(),
                       (const ull*)query.data_ptr<int64_t>(),
                       (const long long*)slots.data_ptr<int64_t>(),
                       is_new.data_ptr<int32_t>(), perm.data_ptr<int64_t>(),
                       ustarts.data_ptr<int64_t>(),
                       (__half*)sums.data_ptr<at::Half>(), n, (int)dim,
                       row_width, lo, hi, (float)state_init, n_dev);
  } else {
    hipLaunchKernelGGL(init_scatter_kernel, dim3(n_blocks_for(n, 4)),
                       dim3(256), 0, st, arena.data_ptr<float>(),
                       (const ull*)query.data_ptr<int64_t>(),
                       (const long long*)slots.data_ptr<int64_t>(),
                       is_new.data_ptr<int32_t>(), perm.data_ptr<int64_t>(),
                       ustarts.data_ptr<int64_t>(),
                       (__half*)sums.data_ptr<at::Half>(), n, (int)dim,
                       row_width, lo, hi, (float)state_init, n_dev);
  }
  if (!hints) return {src_hint, src_hint};  // slots was a temporary
  return {slots, src_hint};
}

// Launch of bag_plan_kernel for S sum slots followed by R raw slots (R = 0: a
// pure bag group; raw_meta and n_rows are then unused).
// -> {cat_offsets i64[S*B+1], seg_id i64[nnz], seg_lens f32[S*B], seg_scale
//     f32[S*B], [n_rows] with raw slots, or empty (all ones) without a sqrt
//     slot, raw_num i64[R*B]}
static std::vector<torch::Tensor> plan_launch(
    const torch::Tensor& plan, int64_t S, int64_t R, int64_t B, int64_t nnz,
    const torch::Tensor& sqrt_flags, const torch::Tensor& raw_meta,
    int64_t n_rows) {
  const bool scaled = sqrt_flags.numel() > 0;
  auto opts = torch::TensorOptions().dtype(torch::kInt64).device(plan.device());
  const int64_t n_seg = S * B;
  auto cat_offsets = torch::empty({n_seg + 1}, opts);
  auto seg_id = torch::empty({nnz}, opts);
  auto seg_lens = torch::empty({n_seg}, opts.dtype(torch::kFloat32));
  auto seg_scale = torch::empty({scaled ? (R ? n_rows : n_seg) : 0},
                                opts.dtype(torch::kFloat32));
  auto raw_num = torch::empty({R * B}, opts);
  // >= 1: no empty launch
  const int64_t n = std::max((R ? n_rows : n_seg) + 1, nnz);
  hipLaunchKernelGGL(bag_plan_kernel, dim3(n_blocks_for(n, 256)), dim3(256), 0,
                     cur_stream(), plan.data_ptr<int64_t>(),
                     scaled ? sqrt_flags.data_ptr<int32_t>() : nullptr, (int)S,
                     B, nnz, cat_offsets.data_ptr<int64_t>(),
                     seg_id.data_ptr<int64_t>(), seg_lens.data_ptr<float>(),
                     scaled ? seg_scale.data_ptr<float>() : nullptr, (int)R,
                     R ? raw_meta.data_ptr<int64_t>() : nullptr, n_rows,
                     raw_num.data_ptr<int64_t>());
  return {cat_offsets, seg_id, seg_lens, seg_scale, raw_num};
}

// Segment plan of a bag group (bag_plan_kernel).  `plan` is the uploaded
// slot_starts[S+1] ‖ offsets[S, B+1]; sqrt_flags i32[S] marks the sqrt-scaling
// slots and is empty when the group has none.
// -> {cat_offsets i64[S*B+1], seg_id i64[nnz], seg_lens f32[S*B],
//     seg_scale f32[S*B], or empty (all ones) without a sqrt slot}
std::vector<torch::Tensor> bag_plan(torch::Tensor plan, int64_t S, int64_t B,
                                    int64_t nnz, torch::Tensor sqrt_flags) {
  TORCH_CHECK(S >= 1 && B >= 0 && nnz >= 0, "bag_plan: bad shape");
  TORCH_CHECK(plan.scalar_type() == torch::kInt64 && plan.is_contiguous() &&
                  plan.numel() == S + 1 + S * (B + 1),
              "bag_plan: plan must be i64[S+1 + S*(B+1)]");
  TORCH_CHECK(!sqrt_flags.numel() ||
                  (sqrt_flags.scalar_type() == torch::kInt32 &&
                   sqrt_flags.numel() == S),
              "bag_plan: sqrt_flags must be i32[S]");
  auto p = plan_launch(plan, S, 0, B, nnz, sqrt_flags, sqrt_flags, 0);
  p.pop_back();
  return p;
}

// Rows of the leaf base of a raw group: the S*B sum segments, then B*sfs[r]
// cell rows per raw slot.
static int64_t raw_group_rows(int64_t S, int64_t B,
                              const std::vector<int64_t>& sfs) {
  int64_t n = S * B;
  for (int64_t f : sfs) n += B * f;
  return n;
}

// Plan of a raw group: S sum slots, then R = sfs.size() raw (sequence) slots
// with sample_fixed_size sfs[r] (see bag_plan_kernel).  `plan` is the uploaded
// slot_starts[S+R+1] ‖ offsets[S+R, B+1]; raw_meta is the device copy of
// row_base[R] ‖ sfs[R], row_base[r] = S*B + sum_{r' < r} B*sfs[r'].
// -> bag_plan's four tensors, seg_scale sized by the base's rows (1 over the
//    raw rows), and raw_num i64[R*B] = min(len, sfs)
std::vector<torch::Tensor> raw_plan(torch::Tensor plan, int64_t S, int64_t B,
                                    int64_t nnz, torch::Tensor sqrt_flags,
                                    torch::Tensor raw_meta,
                                    std::vector<int64_t> sfs) {
  const int64_t R = (int64_t)sfs.size();
  TORCH_CHECK(S >= 0 && R >= 1 && B >= 0 && nnz >= 0, "raw_plan: bad shape");
  for (int64_t f : sfs)
    TORCH_CHECK(f >= 1, "raw_plan: sample_fixed_size must be positive");
  TORCH_CHECK(plan.scalar_type() == torch::kInt64 && plan.is_contiguous() &&
                  plan.numel() == S + R + 1 + (S + R) * (B + 1),
              "raw_plan: plan must be i64[S+R+1 + (S+R)*(B+1)]");
  TORCH_CHECK(!sqrt_flags.numel() ||
                  (sqrt_flags.scalar_type() == torch::kInt32 &&
                   sqrt_flags.numel() == S),
              "raw_plan: sqrt_flags must be i32[S]");
  TORCH_CHECK(raw_meta.scalar_type() == torch::kInt64 &&
                  raw_meta.is_contiguous() && raw_meta.numel() == 2 * R &&
                  raw_meta.device() == plan.device(),
              "raw_plan: raw_meta must be i64[2R] on the plan's device");
  return plan_launch(plan, S, R, B, nnz, sqrt_flags, raw_meta,
                     raw_group_rows(S, B, sfs));
}

// The raw slots of a group behind its sum slots, for lookup_unique_sums.
struct RawPart {
  const torch::Tensor& plan;      // slot_starts ‖ offsets of all S+R slots
  const torch::Tensor& raw_meta;  // row_base[R] ‖ sfs[R], device
  const std::vector<int64_t>& sfs;
  int64_t S, B;
  torch::Tensor& base;  // f16 [n_rows, dim], sums first
  torch::Tensor& mask;  // f16 [n_rows - S*B]
};

// Lookup over the unique keys of a dedup: probe/claim, a launch that only
// initializes the freshly claimed rows (training), then the segment sums read
// straight from the arena (bag_sum_kernel) — no [U, dim] row buffer — and,
// with `raw`, the raw slots' cells (raw_gather_kernel).  The init launch
// precedes the reading launches because a fresh row is read by every segment
// and cell that holds its key, not by the wave that claimed it.
// Returns the update hints {slot_hint, src_hint} as store_lookup_sums does:
// both empty unless seg_id is given.
static std::vector<torch::Tensor> lookup_unique_sums(
    torch::Tensor table_keys, torch::Tensor ticks, torch::Tensor arena,
    torch::Tensor query, torch::Tensor inverse, torch::Tensor perm,
    torch::Tensor ustarts, torch::Tensor cat_offsets, torch::Tensor seg_scale,
    torch::Tensor sums, int64_t dim, int64_t train, int64_t tick, double lo,
    double hi, double admit_prob, double state_init, int64_t opt_space,
    torch::Tensor u_count, torch::Tensor seg_id, const RawPart* raw) {
  const int64_t n = query.numel();
  const int64_t n_seg = cat_offsets.numel() - 1;
  auto opts = torch::TensorOptions().dtype(torch::kInt64).device(query.device());
  const bool hints = seg_id.numel() > 0;
  auto src_hint = torch::empty({hints ? n : 0}, opts);
  TORCH_CHECK(inverse.numel() == n && perm.numel() == n && ustarts.numel() > n,
              "store_lookup_bags: dedup tensors do not match the query");
  TORCH_CHECK(sums.size(0) == n_seg && sums.size(1) == dim &&
                  sums.is_contiguous(),
              "store_lookup_bags: sums must be [n_seg, dim]");
  TORCH_CHECK(!seg_scale.numel() || seg_scale.numel() >= n_seg,
              "store_lookup_bags: seg_scale must be empty or [n_seg]");
  TORCH_CHECK(!hints || seg_id.numel() >= n,
              "store_lookup_bags: seg_id shorter than perm");
  if (n == 0) {  // every bag empty: nothing to probe, the sums are zeros
    sums.zero_();
    if (raw) {
      raw->base.zero_();
      raw->mask.zero_();
    }
    return {src_hint, src_hint};
  }
  auto slots = torch::empty({n}, opts);
  auto is_new = torch::empty({n}, opts.dtype(torch::kInt32));
  const int64_t n_buckets = table_keys.numel() / PA_BUCKET_SIZE;
  const int row_width = (int)(dim + opt_space);
  const long long* n_dev = count_or_null(u_count);
  hipStream_t st = cur_stream();
  hipLaunchKernelGGL(probe_claim_kernel, dim3(n_blocks_for(n, 256)), dim3(256),
                     0, st, (ull*)table_keys.data_ptr<int64_t>(),
                     (unsigned*)ticks.data_ptr<int32_t>(),
                     (const ull*)query.data_ptr<int64_t>(), n, n_buckets,
                     (int)train, (unsigned)tick, (float)admit_prob,
                     (long long*)slots.data_ptr<int64_t>(),
                     is_new.data_ptr<int32_t>(), nullptr, nullptr, nullptr,
                     n_dev, hints ? ustarts.data_ptr<int64_t>() : nullptr,
                     hints ? perm.data_ptr<int64_t>() : nullptr,
                     hints ? seg_id.data_ptr<int64_t>() : nullptr,
                     hints ? (long long*)src_hint.data_ptr<int64_t>() : nullptr);
  if (train)  // an eval lookup claims nothing: nothing to initialize
    hipLaunchKernelGGL((init_gather_kernel<float, true, false>),
                       dim3(n_blocks_for(n, 4)), dim3(256), 0, st,
                       arena.data_ptr<float>(),
                       (const ull*)query.data_ptr<int64_t>(),
                       (const long long*)slots.data_ptr<int64_t>(),
                       is_new.data_ptr<int32_t>(), (float*)nullptr, n,
                       (int)dim, row_width, lo, hi, (float)state_init, nullptr,
                       nullptr, n_dev);
  const bool packed = dim < PA_WAVE && (PA_WAVE % dim) == 0;
  if (n_seg > 0) {
    const dim3 grid(n_blocks_for(n_seg, 4)), block(256);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, block, 0, st, arena.data_ptr<float>(),
                         (const long long*)slots.data_ptr<int64_t>(),
                         inverse.data_ptr<int64_t>(),
                         cat_offsets.data_ptr<int64_t>(),
                         scale_or_null(seg_scale),
                         (__half*)sums.data_ptr<at::Half>(), n_seg, (int)dim,
                         row_width);
    };
    // columns a lane holds per pass: the whole row up to dim 512
    if (packed || dim <= PA_WAVE) launch(bag_sum_kernel<1>);
    else if (dim <= 2 * PA_WAVE) launch(bag_sum_kernel<2>);
    else if (dim <= 4 * PA_WAVE) launch(bag_sum_kernel<4>);
    else launch(bag_sum_kernel<8>);
  }
  if (raw) {
    // wave items: per raw slot, B samples times the chunks of one sample
    const int64_t chunk = (packed ? PA_WAVE / dim : 1) * PA_RAW_DEPTH;
    int64_t n_items = 0;
    for (int64_t f : raw->sfs) n_items += raw->B * ((f + chunk - 1) / chunk);
    if (n_items > 0) {
      auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(
            kernel, dim3(n_blocks_for(n_items, 4)), dim3(256), 0, st,
            arena.data_ptr<float>(),
            (const long long*)slots.data_ptr<int64_t>(),
            inverse.data_ptr<int64_t>(), raw->plan.data_ptr<int64_t>(),
            raw->raw_meta.data_ptr<int64_t>(),
            (__half*)raw->base.data_ptr<at::Half>(),
            (__half*)raw->mask.data_ptr<at::Half>(), (int)raw->S,
            (int)raw->sfs.size(), raw->B, raw->base.size(0),
            (unsigned)n_items, (int)dim, row_width);
      };
      if (packed || dim <= PA_WAVE) launch(raw_gather_kernel<1>);
      else if (dim <= 2 * PA_WAVE) launch(raw_gather_kernel<2>);
      else if (dim <= 4 * PA_WAVE) launch(raw_gather_kernel<4>);
      else launch(raw_gather_kernel<8>);
    }
  }
  if (!hints) return {src_hint, src_hint};  // slots was a temporary
  return {slots, src_hint};
}

// Bag lookup over the unique keys of a dedup (lookup_unique_sums without raw
// slots).
std::vector<torch::Tensor> store_lookup_bags(
    torch::Tensor table_keys, torch::Tensor ticks, torch::Tensor arena,
    torch::Tensor query, torch::Tensor inverse, torch::Tensor perm,
    torch::Tensor ustarts, torch::Tensor cat_offsets, torch::Tensor seg_scale,
    torch::Tensor sums, int64_t dim, int64_t train, int64_t tick, double lo,
    double hi, double admit_prob, double state_init, int64_t opt_space,
    torch::Tensor u_count, torch::Tensor seg_id) {
  TORCH_CHECK(!seg_scale.numel() ||
                  seg_scale.numel() == cat_offsets.numel() - 1,
              "store_lookup_bags: seg_scale must be empty or [n_seg]");
  return lookup_unique_sums(table_keys, ticks, arena, query, inverse, perm,
                            ustarts, cat_offsets, seg_scale, sums, dim, train,
                            tick, lo, hi, admit_prob, state_init, opt_space,
                            u_count, seg_id, nullptr);
}

// Lookup of a raw group over the unique keys of its dedup: S sum slots as
// store_lookup_bags, then the R = sfs.size() raw slots' cells into the rows
// of `base` behind the S*B sums and into `mask` (raw_gather_kernel).  `plan`,
// raw_meta and sfs are raw_plan's; seg_scale is empty or covers base's rows.
std::vector<torch::Tensor> store_lookup_raw(
    torch::Tensor table_keys, torch::Tensor ticks, torch::Tensor arena,
    torch::Tensor query, torch::Tensor inverse, torch::Tensor perm,
    torch::Tensor ustarts, torch::Tensor cat_offsets, torch::Tensor seg_scale,
    torch::Tensor plan, torch::Tensor raw_meta, std::vector<int64_t> sfs,
    int64_t S, int64_t B, torch::Tensor base, torch::Tensor mask, int64_t dim,
    int64_t train, int64_t tick, double lo, double hi, double admit_prob,
    double state_init, int64_t opt_space, torch::Tensor u_count,
    torch::Tensor seg_id) {
  const int64_t R = (int64_t)sfs.size();
  const int64_t n_rows = raw_group_rows(S, B, sfs);
  TORCH_CHECK(S >= 0 && R >= 1 && B >= 0 && cat_offsets.numel() - 1 == S * B,
              "store_lookup_raw: bad shape");
  for (int64_t f : sfs)
    TORCH_CHECK(f >= 1, "store_lookup_raw: sample_fixed_size must be positive");
  // raw_gather numbers its wave items and cells with 32 bits
  TORCH_CHECK(n_rows < ((int64_t)1 << 31), "store_lookup_raw: ", n_rows,
              " rows in one group");
  TORCH_CHECK(plan.scalar_type() == torch::kInt64 && plan.is_contiguous() &&
                  plan.numel() == S + R + 1 + (S + R) * (B + 1),
              "store_lookup_raw: plan must be i64[S+R+1 + (S+R)*(B+1)]");
  TORCH_CHECK(raw_meta.scalar_type() == torch::kInt64 &&
                  raw_meta.is_contiguous() && raw_meta.numel() == 2 * R,
              "store_lookup_raw: raw_meta must be i64[2R]");
  TORCH_CHECK(base.scalar_type() == torch::kFloat16 && base.is_contiguous() &&
                  base.dim() == 2 && base.size(0) == n_rows &&
                  base.size(1) == dim,
              "store_lookup_raw: base must be f16 [S*B + sum B*sfs, dim]");
  TORCH_CHECK(mask.scalar_type() == torch::kFloat16 && mask.is_contiguous() &&
                  mask.numel() == n_rows - S * B,
              "store_lookup_raw: mask must be f16 [sum B*sfs]");
  TORCH_CHECK(!seg_scale.numel() || seg_scale.numel() == n_rows,
              "store_lookup_raw: seg_scale must be empty or cover base's rows");
  RawPart raw{plan, raw_meta, sfs, S, B, base, mask};
  return lookup_unique_sums(table_keys, ticks, arena, query, inverse, perm,
                            ustarts, cat_offsets, seg_scale,
                            base.narrow(0, 0, S * B), dim, train, tick, lo, hi,
                            admit_prob, state_init, opt_space, u_count, seg_id,
                            &raw);
}

torch::Tensor store_probe(torch::Tensor table_keys, torch::Tensor ticks,
                          torch::Tensor query, int64_t tick,
                          torch::Tensor u_count) {
  const int64_t n = query.numel();
  auto opts = torch::TensorOptions().dtype(torch::kInt64).device(query.device());
  // padded queries: slots defaults to 0 ("found") beyond the device count so
  // the padding never reads as missing
  auto slots = u_count.numel() ? torch::zeros({n}, opts) : torch::empty({n}, opts);
  if (n == 0) return slots;
  auto is_new = torch::empty({n}, opts.dtype(torch::kInt32));
  const int64_t n_buckets = table_keys.numel() / PA_BUCKET_SIZE;
  hipLaunchKernelGGL(probe_claim_kernel, dim3(n_blocks_for(n, 256)), dim3(256),
                     0, cur_stream(), (ull*)table_keys.data_ptr<int64_t>(),
                     (unsigned*)ticks.data_ptr<int32_t>(),
                     (const ull*)query.data_ptr<int64_t>(), n, n_buckets,
                     /*train=*/0, (unsigned)tick, 1.0f,
                     (long long*)slots.data_ptr<int64_t>(),
                     is_new.data_ptr<int32_t>(), nullptr, nullptr, nullptr,
                     count_or_null(u_count), nullptr, nullptr, nullptr,
                     nullptr);
  return slots;
}

void store_update(torch::Tensor table_keys, torch::Tensor ticks,
                  torch::Tensor arena, torch::Tensor query,
                  torch::Tensor grads, int64_t dim, int64_t opt,
                  std::vector<double> params, double b1_power,
                  double b2_power, double weight_bound,
                  torch::Tensor skipped /* persistent i32[2]: miss, nan */) {
  TORCH_CHECK(opt >= 0 && opt <= 3, "store_update: unknown optimizer code ",
              opt, " (0 SGD, 1 Adagrad, 2 Adam, 3 FTRL)");
  const int64_t n = query.numel();
  if (n == 0) return;
  const int64_t n_buckets = table_keys.numel() / PA_BUCKET_SIZE;
  const int row_width = (int)arena.size(1);
  TORCH_CHECK(opt < 2 || row_width >= 3 * dim,
              "store_update: Adam/FTRL rows hold 3*dim floats");
  hipStream_t st = cur_stream();
  auto kernel = opt == 3 ? update_kernel<true> : update_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(n_blocks_for(n, 4)), dim3(256), 0, st,
                     (ull*)table_keys.data_ptr<int64_t>(),
                     (unsigned*)ticks.data_ptr<int32_t>(),
                     arena.data_ptr<float>(),
                     (const ull*)query.data_ptr<int64_t>(),
                     grads.data_ptr<float>(), n, (int)dim, row_width,
                     n_buckets, (int)opt, (float)params[0], (float)params[1],
                     (float)params[2], (float)params[3], (float)b1_power,
                     (float)b2_power, (float)weight_bound,
                     skipped.data_ptr<int32_t>());
}

void store_import(torch::Tensor table_keys, torch::Tensor ticks,
                  torch::Tensor arena, torch::Tensor query, torch::Tensor rows,
                  int64_t tick, torch::Tensor evict_keys,
                  torch::Tensor evict_count, torch::Tensor evict_rows) {
  const int64_t n = query.numel();
  if (n == 0) return;
  const int64_t n_buckets = table_keys.numel() / PA_BUCKET_SIZE;
  const bool spill = evict_keys.numel() > 0;
  hipLaunchKernelGGL(import_kernel, dim3(n_blocks_for(n, 256)), dim3(256), 0,
                     cur_stream(), (ull*)table_keys.data_ptr<int64_t>(),
                     (unsigned*)ticks.data_ptr<int32_t>(),
                     arena.data_ptr<float>(),
                     (const ull*)query.data_ptr<int64_t>(),
                     rows.data_ptr<float>(), n, (int)rows.size(1), n_buckets,
                     (unsigned)tick,
                     spill ? (ull*)evict_keys.data_ptr<int64_t>() : nullptr,
                     spill ? evict_count.data_ptr<int32_t>() : nullptr,
                     spill ? evict_rows.data_ptr<float>() : nullptr);
}

torch::Tensor segment_sum(torch::Tensor rows, torch::Tensor inverse,
                          torch::Tensor seg_offsets, torch::Tensor seg_scale) {
  const int64_t n_seg = seg_offsets.numel() - 1;
  const int64_t dim = rows.size(1);
  auto out = torch::empty(
      {n_seg, dim},
      torch::TensorOptions().dtype(torch::kFloat16).device(rows.device()));
  if (n_seg == 0) return out;
  const float* scale_ptr = scale_or_null(seg_scale);
  hipStream_t st = cur_stream();
  const dim3 grid(n_blocks_for(n_seg, 4)), block(256);
  if (rows.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(segment_sum_kernel<float>, grid, block, 0, st,
                       rows.data_ptr<float>(), inverse.data_ptr<int64_t>(),
                       seg_offsets.data_ptr<int64_t>(), scale_ptr,
                       (__half*)out.data_ptr<at::Half>(), n_seg, (int)dim);
  } else if (rows.scalar_type() == torch::kFloat16) {
    hipLaunchKernelGGL(segment_sum_kernel<__half>, grid, block, 0, st,
                       (const __half*)rows.data_ptr<at::Half>(),
                       inverse.data_ptr<int64_t>(),
                       seg_offsets.data_ptr<int64_t>(), scale_ptr,
                       (__half*)out.data_ptr<at::Half>(), n_seg, (int)dim);
  } else {
    TORCH_CHECK(false, "segment_sum: rows must be f32 or f16");
  }
  return out;
}

void grad_scatter(torch::Tensor grads, torch::Tensor perm,
                  torch::Tensor ustarts, torch::Tensor seg_id,
                  torch::Tensor seg_scale, torch::Tensor out,
                  int64_t accumulate) {
  const int64_t n_unique = ustarts.numel() - 1;
  const int64_t dim = out.size(1);
  if (n_unique == 0) return;
  hipStream_t st = cur_stream();
  const dim3 grid(n_blocks_for(n_unique, 4)), block(256);
  const float* scale_ptr = scale_or_null(seg_scale);
#define PA_GS(T, ACC)                                                         \
  hipLaunchKernelGGL((grad_scatter_kernel<T, ACC>), grid, block, 0, st,       \
                     (const T*)grads.data_ptr(), perm.data_ptr<int64_t>(),    \
                     ustarts.data_ptr<int64_t>(), seg_id.data_ptr<int64_t>(), \
                     scale_ptr, out.data_ptr<float>(),                        \
                     n_unique, (int)dim)
  if (grads.scalar_type() == torch::kFloat16) {
    if (accumulate) PA_GS(__half, true); else PA_GS(__half, false);
  } else if (grads.scalar_type() == torch::kFloat32) {
    if (accumulate) PA_GS(float, true); else PA_GS(float, false);
  } else if (grads.scalar_type() == torch::kBFloat16) {
    if (accumulate) PA_GS(__hip_bfloat16, true); else PA_GS(__hip_bfloat16, false);
  } else {
    TORCH_CHECK(false, "grad_scatter: grads must be f16/bf16/f32");
  }
#undef PA_GS
}

void grad_scatter_idx(torch::Tensor grads, torch::Tensor perm,
                      torch::Tensor ustarts, torch::Tensor seg_id,
                      torch::Tensor seg_scale, torch::Tensor out_idx,
                      torch::Tensor out, torch::Tensor u_count) {
  const int64_t n_unique = out_idx.numel();  // padded upper bound
  const int64_t dim = out.size(1);
  if (n_unique == 0) return;
  TORCH_CHECK(grads.scalar_type() == torch::kFloat16,
              "grad_scatter_idx: f16 grads");
  hipStream_t st = cur_stream();
  const dim3 grid(n_blocks_for(n_unique, 4)), block(256);
  const float* scale_ptr = scale_or_null(seg_scale);
  const long long* n_dev = count_or_null(u_count);
  if (out.scalar_type() == torch::kFloat16) {
    hipLaunchKernelGGL(grad_scatter_idx_kernel<__half>, grid, block, 0, st,
                       (const __half*)grads.data_ptr<at::Half>(),
                       perm.data_ptr<int64_t>(), ustarts.data_ptr<int64_t>(),
                       seg_id.data_ptr<int64_t>(), scale_ptr,
                       out_idx.data_ptr<int64_t>(),
                       (__half*)out.data_ptr<at::Half>(), n_unique, (int)dim,
                       n_dev);
  } else if (out.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(grad_scatter_idx_kernel<float>, grid, block, 0, st,
                       (const __half*)grads.data_ptr<at::Half>(),
                       perm.data_ptr<int64_t>(), ustarts.data_ptr<int64_t>(),
                       seg_id.data_ptr<int64_t>(), scale_ptr,
                       out_idx.data_ptr<int64_t>(),
                       out.data_ptr<float>(), n_unique, (int)dim, n_dev);
  } else {
    TORCH_CHECK(false, "grad_scatter_idx: out must be f16/f32");
  }
}

void scatter_update(torch::Tensor table_keys, torch::Tensor ticks,
                    torch::Tensor arena, torch::Tensor uniq,
                    torch::Tensor grads, torch::Tensor perm,
                    torch::Tensor ustarts, torch::Tensor seg_id,
                    torch::Tensor seg_scale, int64_t dim, int64_t opt,
                    std::vector<double> params, double b1_power,
                    double b2_power, double weight_bound,
                    torch::Tensor skipped, torch::Tensor u_count,
                    torch::Tensor slot_hint, torch::Tensor src_hint) {
  TORCH_CHECK(opt >= 0 && opt <= 3, "scatter_update: unknown optimizer code ",
              opt, " (0 SGD, 1 Adagrad, 2 Adam, 3 FTRL)");
  const int64_t n = uniq.numel();
  if (n == 0) return;
  TORCH_CHECK(grads.scalar_type() == torch::kFloat16, "scatter_update: f16 grads");
  TORCH_CHECK(dim <= 8 * PA_WAVE, "scatter_update: dim too large");
  // update hints (store_lookup_sums): both or neither, one per entry of uniq
  const bool hints = slot_hint.numel() > 0;
  TORCH_CHECK(!hints || (slot_hint.numel() >= n && src_hint.numel() >= n),
              "scatter_update: hints shorter than uniq");
  TORCH_CHECK(!hints || (slot_hint.scalar_type() == torch::kInt64 &&
                         src_hint.scalar_type() == torch::kInt64 &&
                         slot_hint.device() == uniq.device() &&
                         src_hint.device() == uniq.device() &&
                         slot_hint.is_contiguous() && src_hint.is_contiguous()),
              "scatter_update: hints must be contiguous int64 on uniq's device");
  // the hinted kernels read seg_scale[src] for any src < grads.size(0)
  TORCH_CHECK(!hints || seg_scale.numel() == 0 ||
                  seg_scale.numel() >= grads.size(0),
              "scatter_update: seg_scale shorter than grads");
  const long long* slot_ptr =
      hints ? (const long long*)slot_hint.data_ptr<int64_t>() : nullptr;
  const long long* src_ptr =
      hints ? (const long long*)src_hint.data_ptr<int64_t>() : nullptr;
  const int64_t n_buckets = table_keys.numel() / PA_BUCKET_SIZE;
  const int row_width = (int)arena.size(1);
  TORCH_CHECK(opt < 2 || row_width >= 3 * dim,
              "scatter_update: Adam/FTRL rows hold 3*dim floats");
  // the variants share one signature: launch `kernel` with one wave
  // per `keys_per_wave` unique keys
  auto launch = [&](auto kernel, int keys_per_wave) {
    const int64_t waves = (n + keys_per_wave - 1) / keys_per_wave;
    hipLaunchKernelGGL(kernel, dim3(n_blocks_for(waves, 4)), dim3(256), 0,
                       cur_stream(), (ull*)table_keys.data_ptr<int64_t>(),
                       (unsigned*)ticks.data_ptr<int32_t>(),
                       arena.data_ptr<float>(),
                       (const ull*)uniq.data_ptr<int64_t>(),
                       (const __half*)grads.data_ptr<at::Half>(),
                       perm.data_ptr<int64_t>(), ustarts.data_ptr<int64_t>(),
                       seg_id.data_ptr<int64_t>(), scale_or_null(seg_scale), n,
                       (int)dim, row_width, n_buckets, (int)opt,
                       (float)params[0], (float)params[1], (float)params[2],
                       (float)params[3], (float)b1_power, (float)b2_power,
                       (float)weight_bound, skipped.data_ptr<int32_t>(),
                       count_or_null(u_count), slot_ptr, src_ptr,
                       table_keys.numel(), grads.size(0));
  };
  // small dividing dims keep the sub-wave-packed kernel (more keys per
  // wave); other dims take as many keys per wave as the register-resident
  // gradient allows (memory-level parallelism), down to one above 256
  const bool packed_small = (dim < PA_WAVE && (PA_WAVE % dim) == 0);
  // the hinted code is a separate instantiation: holding loaded rows across
  // the verify costs registers, which callers without hints do not pay.  So
  // is FTRL (opt 3), whose arm cost the other optimizers a wave per SIMD.
  auto pick = [&](auto plain, auto hinted, auto ftrl, auto ftrl_hinted,
                  int keys_per_wave) {
    if (opt == 3) launch(hints ? ftrl_hinted : ftrl, keys_per_wave);
    else launch(hints ? hinted : plain, keys_per_wave);
  };
  if (!packed_small && dim <= 128) {
    pick(scatter_update_multi_kernel<4, false, false>,
         scatter_update_multi_kernel<4, true, false>,
         scatter_update_multi_kernel<4, false, true>,
         scatter_update_multi_kernel<4, true, true>, 4);
  } else if (!packed_small && dim <= 256) {
    pick(scatter_update_multi_kernel<2, false, false>,
         scatter_update_multi_kernel<2, true, false>,
         scatter_update_multi_kernel<2, false, true>,
         scatter_update_multi_kernel<2, true, true>, 2);
  } else {
    pick(scatter_update_kernel<false, false>, scatter_update_kernel<true, false>,
         scatter_update_kernel<false, true>, scatter_update_kernel<true, true>,
         1);
  }
}

// -> (send [world*cap+1] zero-padded, idx [n_pad]); overflow accumulates
// into the caller's persistent device counter
std::vector<torch::Tensor> a2a_route(torch::Tensor uniq, torch::Tensor u_count,
                                     int64_t world, int64_t cap,
                                     torch::Tensor overflow) {
  const int64_t n_pad = uniq.numel();
  auto opts = torch::TensorOptions().dtype(torch::kInt64).device(uniq.device());
  auto send = torch::zeros({world * cap + 1}, opts);
  auto idx = torch::empty({n_pad}, opts);
  auto starts = torch::empty({world + 1}, opts);
  hipStream_t st = cur_stream();
  const long long* n_dev = count_or_null(u_count);
  hipLaunchKernelGGL(a2a_bounds_kernel, dim3(1), dim3(world + 1), 0, st,
                     (const ull*)uniq.data_ptr<int64_t>(), n_dev, n_pad,
                     (int)world, (long long*)starts.data_ptr<int64_t>());
  if (n_pad)
    hipLaunchKernelGGL(a2a_scatter_kernel, dim3(n_blocks_for(n_pad, 256)),
                       dim3(256), 0, st, (const ull*)uniq.data_ptr<int64_t>(),
                       n_dev, n_pad,
                       (const long long*)starts.data_ptr<int64_t>(), (int)world,
                       cap, (ull*)send.data_ptr<int64_t>(),
                       idx.data_ptr<int64_t>(),
                       (long long*)overflow.data_ptr<int64_t>());
  return {send, idx};
}

torch::Tensor sign_prep(torch::Tensor values, torch::Tensor slot_starts,
                        torch::Tensor prefixes, int64_t spacing) {
  const int64_t n = values.numel();
  auto out = torch::empty_like(values);
  if (n == 0) return out;
  hipLaunchKernelGGL(sign_prep_kernel, dim3(n_blocks_for(n, 256)), dim3(256),
                     0, cur_stream(), (const ull*)values.data_ptr<int64_t>(),
                     slot_starts.data_ptr<int64_t>(),
                     (const ull*)prefixes.data_ptr<int64_t>(),
                     (int)(slot_starts.numel() - 1), (ull)spacing,
                     (ull*)out.data_ptr<int64_t>(), n);
  return out;
}

void dedup_finalize(torch::Tensor svals_flipped, torch::Tensor perm,
                    torch::Tensor neq, torch::Tensor rank, int64_t flip,
                    torch::Tensor inverse, torch::Tensor uniq,
                    torch::Tensor ustarts, torch::Tensor u_count) {
  const int64_t n = svals_flipped.numel();
  if (n == 0) return;
  hipLaunchKernelGGL(dedup_finalize_kernel, dim3(n_blocks_for(n, 256)),
                     dim3(256), 0, cur_stream(),
                     (const ull*)svals_flipped.data_ptr<int64_t>(),
                     perm.data_ptr<int64_t>(), neq.data_ptr<bool>(),
                     rank.data_ptr<int64_t>(), n, (ull)flip,
                     inverse.data_ptr<int64_t>(),
                     (ull*)uniq.data_ptr<int64_t>(),
                     ustarts.data_ptr<int64_t>(),
                     (long long*)u_count.data_ptr<int64_t>());
}

torch::Tensor sign_prep_stack(torch::Tensor values, torch::Tensor in_starts,
                              torch::Tensor out_starts, torch::Tensor prefixes,
                              torch::Tensor rounds, torch::Tensor sizes,
                              torch::Tensor off_starts, torch::Tensor all_offs,
                              int64_t spacing, int64_t n_out) {
  const int64_t n_in = values.numel();
  auto out = torch::empty({n_out}, values.options());
  if (n_in == 0) return out;
  hipLaunchKernelGGL(sign_prep_stack_kernel, dim3(n_blocks_for(n_in, 256)),
                     dim3(256), 0, cur_stream(),
                     (const ull*)values.data_ptr<int64_t>(),
                     in_starts.data_ptr<int64_t>(),
                     out_starts.data_ptr<int64_t>(),
                     (const ull*)prefixes.data_ptr<int64_t>(),
                     rounds.data_ptr<int32_t>(), sizes.data_ptr<int64_t>(),
                     off_starts.data_ptr<int64_t>(),
                     all_offs.data_ptr<int64_t>(),
                     (int)(in_starts.numel() - 1), (ull)spacing,
                     (ull*)out.data_ptr<int64_t>(), n_in);
  return out;
}

// Sign prep of a bag group with hashstack slots (sign_prep_bags_kernel).
// `upload` is the group's device buffer
//   values[nnz_in] ‖ slot_starts[S+1] ‖ offsets[S, B+1] ‖ in_starts[S+1]
// with slot_starts and offsets in the expanded position space; rounds i32[S]
// and sizes i64[S] are the slots' hashstack rounds (0: none) and bucket
// counts, on the device.  -> the nnz_out mixed keys.  One thread per output
// position on the capped grid, so nnz_out is held to 16384*256 here.
torch::Tensor sign_prep_bags(torch::Tensor upload, int64_t nnz_in,
                             int64_t nnz_out, int64_t S, int64_t B,
                             torch::Tensor prefixes, torch::Tensor rounds,
                             torch::Tensor sizes, int64_t spacing) {
  TORCH_CHECK(S >= 1 && B >= 0 && nnz_in >= 0 && nnz_out >= 0 &&
                  upload.scalar_type() == torch::kInt64 &&
                  upload.is_contiguous() &&
                  upload.numel() == nnz_in + 2 * (S + 1) + S * (B + 1),
              "sign_prep_bags: upload must be "
              "i64[nnz_in + S+1 + S*(B+1) + S+1]");
  TORCH_CHECK(prefixes.scalar_type() == torch::kInt64 && prefixes.numel() == S,
              "sign_prep_bags: prefixes must be i64[S]");
  TORCH_CHECK(rounds.scalar_type() == torch::kInt32 && rounds.numel() == S &&
                  rounds.is_contiguous(),
              "sign_prep_bags: rounds must be i32[S]");
  TORCH_CHECK(sizes.scalar_type() == torch::kInt64 && sizes.numel() == S &&
                  sizes.is_contiguous(),
              "sign_prep_bags: sizes must be i64[S]");
  TORCH_CHECK(nnz_out <= (int64_t)16384 * 256,
              "sign_prep_bags: ", nnz_out, " positions in one dim-group, the "
              "thread-per-position kernels cover 4194304");
  TORCH_CHECK(nnz_in > 0 || nnz_out == 0,
              "sign_prep_bags: ", nnz_out, " positions from no ids");
  auto out = torch::empty({nnz_out}, upload.options());
  if (nnz_out == 0) return out;
  const int64_t* up = upload.data_ptr<int64_t>();
  const int64_t* plan = up + nnz_in;
  hipLaunchKernelGGL(sign_prep_bags_kernel, dim3(n_blocks_for(nnz_out, 256)),
                     dim3(256), 0, cur_stream(), (const ull*)up, plan,
                     plan + S + 1, plan + S + 1 + S * (B + 1),
                     (const ull*)prefixes.data_ptr<int64_t>(),
                     rounds.data_ptr<int32_t>(), sizes.data_ptr<int64_t>(),
                     (int)S, B, (ull)spacing, (ull*)out.data_ptr<int64_t>(),
                     nnz_in, nnz_out);
  return out;
}

void init_dense(pybind11::module_& m);     // csrc/dense.hip
void init_engine(pybind11::module_& m);    // csrc/engine.cpp
void init_interact(pybind11::module_& m);  // csrc/interact.hip
void init_checkpoint(pybind11::module_& m);  // csrc/checkpoint.hip

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "persia_amd HIP kernels (gfx950)";
  init_dense(m);
  init_engine(m);
  init_interact(m);
  init_checkpoint(m);
  m.def("store_lookup", &store_lookup, "hash-table lookup/insert + gather");
  m.def("store_probe", &store_probe, "probe-only (spill-tier miss detection)");
  m.def("store_lookup_sums", &store_lookup_sums,
        "fast-path lookup: probe + fused init/f16 scatter to sum rows");
  m.def("bag_plan", &bag_plan,
        "bag group segment plan from the uploaded per-slot CSR");
  m.def("store_lookup_bags", &store_lookup_bags,
        "bag lookup: probe + init launch + segment sums read from the arena");
  m.def("raw_plan", &raw_plan,
        "raw group plan: bag_plan plus the cell rows of the raw slots");
  m.def("store_lookup_raw", &store_lookup_raw,
        "raw group lookup: store_lookup_bags + the raw slots' cells gathered "
        "from the arena");
  m.def("store_update", &store_update, "fused sparse optimizer update");
  m.def("store_import", &store_import, "bulk insert rows (checkpoint load)");
  m.def("segment_sum", &segment_sum, "fused gather + per-sample summation");
  m.def("grad_scatter", &grad_scatter, "ordered per-sign gradient scatter");
  m.def("grad_scatter_idx", &grad_scatter_idx,
        "ordered per-sign gradient scatter packed into the a2a send layout");
  m.def("sign_prep", &sign_prep, "prefix-fold + splitmix64 key mixing");
  m.def("sign_prep_stack", &sign_prep_stack,
        "hashstack expansion + prefix-fold + splitmix64 key mixing");
  m.def("sign_prep_bags", &sign_prep_bags,
        "sign prep of a bag group with hashstack slots, from its one upload");
  m.def("dedup_finalize", &dedup_finalize,
        "fixed-shape dedup epilogue (padded uniq/ustarts + device count)");
  m.def("sort_pairs_u64", &sort_pairs_u64, "radix sort-pairs, u64 order");
  m.def("a2a_route", &a2a_route,
        "padded-a2a key routing: range-partition bounds + packed scatter");
  m.def("neq_flags", &neq_flags, "sorted-run boundary flags");
  namespace py = pybind11;
  m.def("scatter_update", &scatter_update,
        "fused ordered grad scatter + optimizer update (no [U,dim] buffer); "
        "slot_hint/src_hint: optional update hints of store_lookup_sums",
        py::arg("table_keys"), py::arg("ticks"), py::arg("arena"),
        py::arg("uniq"), py::arg("grads"), py::arg("perm"),
        py::arg("ustarts"), py::arg("seg_id"), py::arg("seg_scale"),
        py::arg("dim"), py::arg("opt"), py::arg("params"),
        py::arg("b1_power"), py::arg("b2_power"), py::arg("weight_bound"),
        py::arg("skipped"), py::arg("u_count"),
        py::arg("slot_hint") = torch::empty({0}, torch::kInt64),
        py::arg("src_hint") = torch::empty({0}, torch::kInt64));
}
