// Probe-or-claim on the bucketed open-addressing table, shared by the
// training kernels (kernels.hip) and the checkpoint kernels (checkpoint.hip).
#pragma once

#include "common.h"

// Probe-or-claim with bounded-window LRU eviction (store.py _probe_or_claim).
// Returns slot; *is_new = 1 when this thread claimed it (must init the row).
// Rows touched at the CURRENT tick are never eviction victims, so concurrent
// claims within one batch cannot evict each other; when the whole window is
// current-tick the key overflows to a miss (bounded churn).
//
// kOrdered = false publishes the tick AFTER the key CAS: a peer that scans
// in between sees the new key with a stale tick and may evict a row claimed
// at this very tick.  The training path re-initializes such a row (a
// cold-key non-event); a checkpoint load would lose it, so the import
// kernel uses kOrdered = true, which makes the slot current-tick BEFORE the
// key changes hands: an empty slot gets its tick first, a victim is won by a
// CAS on its tick.  Whoever then loses the key CAS or the tick CAS rescans.
// Table words are read with agent-scope atomic loads so a rescan sees what
// the peer published.
//
// Retries: a lost CAS means a peer took that slot during this launch, and a
// slot taken during this launch is (once its tick is published) neither empty
// nor a victim.  So a key loses at most one race per slot of its window
// before a scan finds nothing to claim: one more attempt than the window has
// slots.  Fewer would drop keys while the window still has room -- the lanes
// of a wave that share a window all pick the same first-empty slot, and each
// retry round admits exactly one of them.
template <bool kOrdered>
__device__ __forceinline__ long long probe_claim_impl(
    unsigned long long* __restrict__ keys, unsigned* __restrict__ ticks,
    int64_t n_buckets, unsigned long long k, unsigned cur_tick, int* is_new,
    unsigned long long* victim_out) {
  using ull = unsigned long long;
  const int64_t mask = n_buckets - 1;
  const int64_t b = (int64_t)(k & (ull)mask);
  constexpr int kAttempts = PA_PROBE_BUCKETS * PA_BUCKET_SIZE + 1;
  for (int attempt = 0; attempt < kAttempts; ++attempt) {
    long long empty = -1;
    long long victim = -1;
    unsigned victim_tick = 0xFFFFFFFFu;
    ull victim_key = 0;
    for (int p = 0; p < PA_PROBE_BUCKETS; ++p) {
      const int64_t base = ((b + p) & mask) * PA_BUCKET_SIZE;
#pragma unroll
      for (int s = 0; s < PA_BUCKET_SIZE; ++s) {
        const int64_t i = base + s;
        ull ki;
        if constexpr (kOrdered) {
          ki = __hip_atomic_load(&keys[i], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
        } else {
          ki = keys[i];
        }
        if (ki == k) { *is_new = 0; return i; }
        if (ki == PA_EMPTY_KEY) {
          if (empty < 0) empty = i;
        } else {
          unsigned t;
          if constexpr (kOrdered) {
            t = __hip_atomic_load(&ticks[i], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
          } else {
            t = ticks[i];
          }
          if (t != cur_tick && (victim < 0 || t < victim_tick)) {
            victim = i; victim_tick = t; victim_key = ki;
          }
        }
      }
    }
    if (empty >= 0) {
      if constexpr (kOrdered) {
        // a slot that stops being empty during this launch is claimed at
        // cur_tick whoever wins it, so the early tick is right either way
        atomicExch(&ticks[empty], cur_tick);
        __threadfence();
      }
      if (atomicCAS((ull*)&keys[empty], PA_EMPTY_KEY, k) == PA_EMPTY_KEY) {
        ticks[empty] = cur_tick;  // publish before peers pick victims
        *is_new = 1; return empty;
      }
      continue;  // lost the race; rescan
    }
    if (victim >= 0) {
      if constexpr (kOrdered) {
        if (atomicCAS(&ticks[victim], victim_tick, cur_tick) != victim_tick)
          continue;  // a peer won this victim (or touched it); rescan
        __threadfence();
      }
      if (atomicCAS((ull*)&keys[victim], victim_key, k) == victim_key) {
        ticks[victim] = cur_tick;
        *is_new = 1;
        if (victim_out) *victim_out = victim_key;
        return victim;
      }
      continue;
    }
    break;  // every slot is current-tick: overflow
  }
  *is_new = 0;
  return -1;  // give up: treated as a non-admitted miss
}

static __device__ long long probe_claim(unsigned long long* __restrict__ keys,
                                        unsigned* __restrict__ ticks,
                                        int64_t n_buckets,
                                        unsigned long long k,
                                        unsigned cur_tick, int* is_new,
                                        unsigned long long* victim_out) {
  return probe_claim_impl<false>(keys, ticks, n_buckets, k, cur_tick, is_new,
                                 victim_out);
}
