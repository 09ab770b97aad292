// persia_amd checkpoint kernels (gfx950): bounded-memory table streaming.
//
//   store_export_window : compact the occupied slots of a slot window into
//                         (signs, rows) staging buffers, in ascending slot
//                         order, so a dump moves the table chunk by chunk
//   store_import_signs  : wave-per-row bulk insert of a (signs, rows) chunk
//                         with sign mixing, eviction log and row-width
//                         adaptation on the device
//
// Placement in the export is deterministic: lane offset from a 64-bit ballot,
// wave offset from LDS, block offset from a per-block count written by a
// first kernel.  No atomics decide an output position and no block waits on
// another block.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include "common.h"
#include "probe.h"

using ull = unsigned long long;

namespace {

constexpr int CK_THREADS = 256;
constexpr int CK_WAVES = CK_THREADS / PA_WAVE;           // 4
constexpr int CK_GROUPS = 4;                             // 64-slot groups per wave
constexpr int CK_SLOTS_PER_WAVE = CK_GROUPS * PA_WAVE;   // 256
constexpr int CK_SLOTS_PER_BLOCK = CK_WAVES * CK_SLOTS_PER_WAVE;  // 1024

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = PA_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, PA_WAVE);
  return v;  // valid in lane 0
}

// ------------------------------------------------------------ window export

// pass 1: occupied-slot count of each block's 1024-slot span
__global__ __launch_bounds__(CK_THREADS) void ckpt_count_kernel(
    const ull* __restrict__ table_keys, int64_t slot_begin, int64_t slot_end,
    int* __restrict__ block_counts) {
  __shared__ int wave_cnt[CK_WAVES];
  const int lane = threadIdx.x & (PA_WAVE - 1);
  const int wave = threadIdx.x / PA_WAVE;
  const int64_t base = slot_begin +
                       (int64_t)blockIdx.x * CK_SLOTS_PER_BLOCK +
                       (int64_t)wave * CK_SLOTS_PER_WAVE;
  int cnt = 0;
#pragma unroll
  for (int g = 0; g < CK_GROUPS; ++g) {
    const int64_t s = base + g * PA_WAVE + lane;
    const bool occ = s < slot_end && table_keys[s] != PA_EMPTY_KEY;
    cnt += __popcll(__ballot(occ));
  }
  if (lane == 0) wave_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < CK_WAVES; ++w) t += wave_cnt[w];
    block_counts[blockIdx.x] = t;
  }
}

// pass 2: compact.  VecT = float4 when row_width % 4 == 0 (row bases of the
// arena and of the staging buffer are then 16-byte aligned), float otherwise;
// vpr = VecT elements per row.  Each wave copies the rows of its 64-slot
// group cooperatively: consecutive lanes take consecutive VecT elements of
// the compacted output, so a 256-float row is one wave-wide 16-byte access
// and narrow rows still keep all lanes busy.
template <typename VecT>
__global__ __launch_bounds__(CK_THREADS) void ckpt_compact_kernel(
    const ull* __restrict__ table_keys, const VecT* __restrict__ arena,
    int64_t slot_begin, int64_t slot_end, int vpr,
    const int* __restrict__ block_counts, ull* __restrict__ out_signs,
    VecT* __restrict__ out_rows, int* __restrict__ out_count) {
  __shared__ int wave_cnt[CK_WAVES];
  __shared__ int wave_part[CK_WAVES];
  __shared__ unsigned char src_lane[CK_WAVES][PA_WAVE];
  const int lane = threadIdx.x & (PA_WAVE - 1);
  const int wave = threadIdx.x / PA_WAVE;
  const int64_t base = slot_begin +
                       (int64_t)blockIdx.x * CK_SLOTS_PER_BLOCK +
                       (int64_t)wave * CK_SLOTS_PER_WAVE;

  // this block's offset = sum of the counts of the blocks before it
  int part = 0;
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += CK_THREADS)
    part += block_counts[j];
  part = wave_sum(part);

  ull k[CK_GROUPS];
  int cnt = 0;
#pragma unroll
  for (int g = 0; g < CK_GROUPS; ++g) {
    const int64_t s = base + g * PA_WAVE + lane;
    k[g] = s < slot_end ? table_keys[s] : PA_EMPTY_KEY;
    cnt += __popcll(__ballot(k[g] != PA_EMPTY_KEY));
  }
  if (lane == 0) {
    wave_cnt[wave] = cnt;
    wave_part[wave] = part;
  }
  __syncthreads();
  int64_t off = 0;
  int block_cnt = 0;
#pragma unroll
  for (int w = 0; w < CK_WAVES; ++w) {
    off += wave_part[w];
    if (w < wave) off += wave_cnt[w];
    block_cnt += wave_cnt[w];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
    *out_count = (int)(off + block_cnt);  // thread 0: off is the block offset

#pragma unroll
  for (int g = 0; g < CK_GROUPS; ++g) {
    const bool occ = k[g] != PA_EMPTY_KEY;
    const ull mask = __ballot(occ);
    const int n = __popcll(mask);
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    if (occ) {
      out_signs[off + rank] = pa_splitmix64_inv(k[g]);
      src_lane[wave][rank] = (unsigned char)lane;
    }
    __syncthreads();  // trip count is block-uniform: no lane exits early
    const int64_t gbase = base + g * PA_WAVE;
    const int total = n * vpr;
    for (int e = lane; e < total; e += PA_WAVE) {
      const int r = e / vpr;
      const int c = e - r * vpr;
      const int64_t s = gbase + src_lane[wave][r];
      out_rows[(off + r) * (int64_t)vpr + c] = arena[s * (int64_t)vpr + c];
    }
    off += n;
    __syncthreads();  // src_lane is rewritten by the next group
  }
}

// ------------------------------------------------------------- chunk import

// One wave per row.  Lane 0 mixes the sign and claims a slot; the wave saves
// the victim row to the eviction log and then writes the new row.  src_w may
// differ from arena_w: wider rows are truncated, missing state columns are
// filled with state_init (store.py _adapt_row_width).  Widths are in VecT
// units.  Every lane reads column c of the victim before it writes column c,
// so the save needs no barrier.
template <typename VecT>
__device__ __forceinline__ VecT ck_splat(float v);
template <>
__device__ __forceinline__ float ck_splat<float>(float v) { return v; }
template <>
__device__ __forceinline__ float4 ck_splat<float4>(float v) {
  return make_float4(v, v, v, v);
}

template <typename VecT>
__global__ __launch_bounds__(CK_THREADS) void ckpt_import_kernel(
    ull* __restrict__ table_keys, unsigned* __restrict__ ticks,
    VecT* __restrict__ arena, const ull* __restrict__ signs,
    const VecT* __restrict__ rows, int64_t n, int src_w, int arena_w,
    int64_t n_buckets, unsigned tick, float state_init,
    ull* __restrict__ evict_keys, int* __restrict__ evict_count,
    VecT* __restrict__ evict_rows, int64_t evict_cap,
    ull* __restrict__ imported_count) {
  __shared__ int landed[CK_WAVES];
  const int lane = threadIdx.x & (PA_WAVE - 1);
  const int wave = threadIdx.x / PA_WAVE;
  const int64_t i = (int64_t)blockIdx.x * CK_WAVES + wave;
  long long slot = -1;
  long long eidx = -1;
  if (i < n && lane == 0) {
    ull k = pa_splitmix64(signs[i]);
    if (k == PA_EMPTY_KEY) k = 0xD1B54A32D192ED03ull;  // empty-sentinel remap
    int is_new;
    ull victim = 0;
    // ordered claim: a row of this chunk is never evicted by a peer of the
    // same launch (probe.h), so every row that lands stays
    slot = probe_claim_impl<true>(table_keys, ticks, n_buckets, k, tick,
                                  &is_new, &victim);
    if (slot >= 0) {
      ticks[slot] = tick;
      if (evict_keys && victim != 0) {
        eidx = (long long)atomicAdd(evict_count, 1);
        // the host sizes the log to the chunk and zeroes the counter; a log
        // that is full anyway loses the victim instead of writing past it
        if (eidx < evict_cap) evict_keys[eidx] = victim;
        else eidx = -1;
      }
    }
  }
  slot = __shfl(slot, 0, PA_WAVE);
  eidx = __shfl(eidx, 0, PA_WAVE);
  if (lane == 0) landed[wave] = slot >= 0 ? 1 : 0;
  if (slot >= 0) {
    VecT* dst = arena + slot * (int64_t)arena_w;
    if (eidx >= 0) {
      VecT* spill = evict_rows + eidx * (int64_t)arena_w;
      for (int c = lane; c < arena_w; c += PA_WAVE) spill[c] = dst[c];
    }
    const VecT* src = rows + i * (int64_t)src_w;
    const VecT fill = ck_splat<VecT>(state_init);
    for (int c = lane; c < arena_w; c += PA_WAVE) {
      VecT v = fill;
      if (c < src_w) v = src[c];
      dst[c] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < CK_WAVES; ++w) t += landed[w];
    if (t) atomicAdd(imported_count, (ull)t);
  }
}

hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }

}  // namespace

void store_export_window(torch::Tensor table_keys, torch::Tensor arena,
                         int64_t slot_begin, int64_t slot_end,
                         torch::Tensor out_signs, torch::Tensor out_rows,
                         torch::Tensor out_count) {
  const int64_t n_slots = table_keys.numel();
  const int64_t row_width = arena.size(1);
  PA_CHECK(table_keys.is_cuda() && arena.is_cuda() && out_signs.is_cuda() &&
               out_rows.is_cuda() && out_count.is_cuda(),
           "store_export_window: device tensors expected");
  PA_CHECK(table_keys.scalar_type() == torch::kInt64 &&
               out_signs.scalar_type() == torch::kInt64 &&
               arena.scalar_type() == torch::kFloat32 &&
               out_rows.scalar_type() == torch::kFloat32 &&
               out_count.scalar_type() == torch::kInt32,
           "store_export_window: dtype mismatch");
  PA_CHECK(table_keys.is_contiguous() && arena.is_contiguous() &&
               out_signs.is_contiguous() && out_rows.is_contiguous(),
           "store_export_window: contiguous tensors expected");
  PA_CHECK(arena.dim() == 2 && arena.size(0) == n_slots,
           "store_export_window: arena/keys shape mismatch");
  PA_CHECK(0 <= slot_begin && slot_begin <= slot_end && slot_end <= n_slots,
           "store_export_window: slot window out of range");
  const int64_t window = slot_end - slot_begin;
  PA_CHECK(window < (1ll << 31), "store_export_window: window too large");
  PA_CHECK(out_rows.dim() == 2 && out_rows.size(1) == row_width &&
               out_rows.size(0) >= window && out_signs.numel() >= window &&
               out_count.numel() >= 1,
           "store_export_window: staging buffers smaller than the window");
  hipStream_t st = cur_stream();
  if (window == 0) {
    C10_HIP_CHECK(hipMemsetAsync(out_count.data_ptr<int32_t>(), 0,
                                 sizeof(int32_t), st));
    return;
  }
  const int64_t n_blocks =
      (window + CK_SLOTS_PER_BLOCK - 1) / CK_SLOTS_PER_BLOCK;
  auto block_counts = torch::empty(
      {n_blocks},
      torch::TensorOptions().dtype(torch::kInt32).device(arena.device()));
  const ull* keys_p = (const ull*)table_keys.data_ptr<int64_t>();
  hipLaunchKernelGGL(ckpt_count_kernel, dim3((unsigned)n_blocks),
                     dim3(CK_THREADS), 0, st, keys_p, slot_begin, slot_end,
                     block_counts.data_ptr<int32_t>());
  if (row_width % 4 == 0) {
    hipLaunchKernelGGL(ckpt_compact_kernel<float4>, dim3((unsigned)n_blocks),
                       dim3(CK_THREADS), 0, st, keys_p,
                       (const float4*)arena.data_ptr<float>(), slot_begin,
                       slot_end, (int)(row_width / 4),
                       block_counts.data_ptr<int32_t>(),
                       (ull*)out_signs.data_ptr<int64_t>(),
                       (float4*)out_rows.data_ptr<float>(),
                       out_count.data_ptr<int32_t>());
  } else {
    hipLaunchKernelGGL(ckpt_compact_kernel<float>, dim3((unsigned)n_blocks),
                       dim3(CK_THREADS), 0, st, keys_p,
                       (const float*)arena.data_ptr<float>(), slot_begin,
                       slot_end, (int)row_width,
                       block_counts.data_ptr<int32_t>(),
                       (ull*)out_signs.data_ptr<int64_t>(),
                       out_rows.data_ptr<float>(),
                       out_count.data_ptr<int32_t>());
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void store_import_signs(torch::Tensor table_keys, torch::Tensor ticks,
                        torch::Tensor arena, torch::Tensor signs,
                        torch::Tensor rows, int64_t tick, double state_init,
                        torch::Tensor evict_keys, torch::Tensor evict_count,
                        torch::Tensor evict_rows,
                        torch::Tensor imported_count) {
  const int64_t n = signs.numel();
  if (n == 0) return;
  const int64_t n_slots = table_keys.numel();
  const int64_t arena_w = arena.size(1);
  PA_CHECK(table_keys.is_cuda() && ticks.is_cuda() && arena.is_cuda() &&
               signs.is_cuda() && rows.is_cuda() && imported_count.is_cuda(),
           "store_import_signs: device tensors expected");
  PA_CHECK(table_keys.scalar_type() == torch::kInt64 &&
               ticks.scalar_type() == torch::kInt32 &&
               signs.scalar_type() == torch::kInt64 &&
               arena.scalar_type() == torch::kFloat32 &&
               rows.scalar_type() == torch::kFloat32 &&
               imported_count.scalar_type() == torch::kInt64,
           "store_import_signs: dtype mismatch");
  PA_CHECK(table_keys.is_contiguous() && ticks.is_contiguous() &&
               arena.is_contiguous() && signs.is_contiguous() &&
               rows.is_contiguous(),
           "store_import_signs: contiguous tensors expected");
  PA_CHECK(arena.dim() == 2 && arena.size(0) == n_slots &&
               ticks.numel() == n_slots && n_slots % PA_BUCKET_SIZE == 0,
           "store_import_signs: table shape mismatch");
  const int64_t n_buckets = n_slots / PA_BUCKET_SIZE;
  PA_CHECK(n_buckets > 0 && (n_buckets & (n_buckets - 1)) == 0,
           "store_import_signs: bucket count must be a power of two");
  PA_CHECK(rows.dim() == 2 && rows.size(0) == n && rows.size(1) > 0,
           "store_import_signs: rows/signs shape mismatch");
  PA_CHECK(imported_count.numel() >= 1, "store_import_signs: no counter");
  const int64_t src_w = rows.size(1);
  const bool spill = evict_keys.numel() > 0;
  if (spill) {
    // every imported row evicts at most one victim
    PA_CHECK(evict_keys.scalar_type() == torch::kInt64 &&
                 evict_count.scalar_type() == torch::kInt32 &&
                 evict_rows.scalar_type() == torch::kFloat32 &&
                 evict_keys.numel() >= n && evict_count.numel() >= 1 &&
                 evict_rows.dim() == 2 && evict_rows.size(0) >= n &&
                 evict_rows.size(1) == arena_w && evict_rows.is_contiguous(),
             "store_import_signs: eviction log smaller than the chunk");
  }
  const int64_t n_blocks = (n + CK_WAVES - 1) / CK_WAVES;
  PA_CHECK(n_blocks < (1ll << 31), "store_import_signs: chunk too large");
  hipStream_t st = cur_stream();
  ull* keys_p = (ull*)table_keys.data_ptr<int64_t>();
  unsigned* ticks_p = (unsigned*)ticks.data_ptr<int32_t>();
  const ull* signs_p = (const ull*)signs.data_ptr<int64_t>();
  ull* ev_keys = spill ? (ull*)evict_keys.data_ptr<int64_t>() : nullptr;
  int* ev_count = spill ? evict_count.data_ptr<int32_t>() : nullptr;
  float* ev_rows = spill ? evict_rows.data_ptr<float>() : nullptr;
  const int64_t ev_cap =
      spill ? std::min(evict_keys.numel(), evict_rows.size(0)) : 0;
  ull* imp = (ull*)imported_count.data_ptr<int64_t>();
  if (arena_w % 4 == 0 && src_w % 4 == 0) {
    hipLaunchKernelGGL(ckpt_import_kernel<float4>, dim3((unsigned)n_blocks),
                       dim3(CK_THREADS), 0, st, keys_p, ticks_p,
                       (float4*)arena.data_ptr<float>(), signs_p,
                       (const float4*)rows.data_ptr<float>(), n,
                       (int)(src_w / 4), (int)(arena_w / 4), n_buckets,
                       (unsigned)tick, (float)state_init, ev_keys, ev_count,
                       (float4*)ev_rows, ev_cap, imp);
  } else {
    hipLaunchKernelGGL(ckpt_import_kernel<float>, dim3((unsigned)n_blocks),
                       dim3(CK_THREADS), 0, st, keys_p, ticks_p,
                       arena.data_ptr<float>(), signs_p,
                       (const float*)rows.data_ptr<float>(), n, (int)src_w,
                       (int)arena_w, n_buckets, (unsigned)tick,
                       (float)state_init, ev_keys, ev_count, ev_rows, ev_cap,
                       imp);
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void init_checkpoint(pybind11::module_& m) {
  m.def("store_export_window", &store_export_window,
        "ordered compaction of a slot window (checkpoint dump)");
  m.def("store_import_signs", &store_import_signs,
        "wave-per-row chunk insert by sign (checkpoint load)");
}
