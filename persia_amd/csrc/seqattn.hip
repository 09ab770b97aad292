// Fused target-attention pooling over a raw (sequence) slot (gfx950).
//
//   seq [B, L, D+1] f16: channels 0..D-1 the row k_l, channel D the 0/1 mask
//   q   [B, D]      f16: the query (a sum slot's tensor)
//   s_l = scale * <q, k_l>;  p = softmax of s over the valid l;
//   out = sum_{valid l} p_l * k_l                              -> f16 [B, D]
// backward (s and p are RECOMPUTED from q and seq, nothing is saved):
//   dp_l = <g, k_l>;  ds_l = p_l * (dp_l - sum_j p_j dp_j)
//   dq   = scale * sum_l ds_l * k_l                            -> f16 [B, D]
//   dk_l = p_l * g + scale * ds_l * q  (valid l), 0 otherwise  -> f16 dseq
// The mask selects: an invalid row is never read into arithmetic, so an Inf
// or NaN there reaches nothing.  A sample without a valid cell gives +0.
//
// Work split: one block = a run of consecutive samples, one wave per sample.
//
// Staging.  A row has D+1 halves -- an odd stride, so no row starts on a
// vector boundary.  But a sample's L*(D+1) halves are contiguous and so are
// consecutive samples: the block copies the BYTE range of its samples into
// LDS linearly with 16-byte global loads.  The range is rounded outward to
// 16-byte addresses; a boundary chunk that would leave the tensor's own
// extent [seq, seq + B*L*(D+1)) is assembled half by half from the part
// inside it, so no byte outside the tensor is touched whatever data_ptr's
// alignment is (a contiguous view that starts at an odd half is legal).
// The mask column rides along, and the odd stride is the LDS padding: lanes
// that own consecutive rows read halves D+1 apart, which spreads over the
// banks without a pad column.
//
// Phases of a wave (all sums f32, fixed order, no atomics -> bit-reproducible
// and independent of B and of the sample's place in the batch):
//   score   a lane owns row l (l += 64 past 64 rows), walks d with q read as
//           an LDS broadcast (f32 copy of the query); wave max and wave sum
//           by xor-butterflies, exp is __expf
//   output  a lane owns columns d, d+64, ... and walks l with p_l as the
//           broadcast; consecutive lanes read consecutive halves
//   dseq    (backward) the wave overwrites its staged rows with dk in place
//           (mask column and invalid rows +0), then the block writes its own
//           byte range back with 16-byte stores; boundary chunks shared with
//           a neighbouring block are written half by half.  The launcher
//           gives dseq the same address modulo 16 as seq, so one LDS image
//           serves both directions.
//
// Matrix instructions do not fit: there is ONE query per sample and no
// operand shared between samples, so every product is a matrix-vector one
// with a single use of each k element -- an MFMA tile would be 1/16 full.
// The op is bound by the one pass over seq (and the one over dseq).
//
// Samples per block come from the LDS footprint on the host (sa_plan): up to
// 4 waves inside a 32 KB budget (5 blocks per CU), a single wave up to the
// 64 KB workgroup limit (L = 200, D = 128 is 51.6 KB of rows).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdint>

// no packed-f32 VALU forms in this file's kernels (setup.py builds every
// source with one flag set, so the switch lives here)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

using u16 = unsigned short;

constexpr int SA_LDS_LIMIT = 65536;   // workgroup limit without opt-in
constexpr int SA_LDS_TARGET = 32768;  // 5 blocks per CU in 160 KB
constexpr int SA_MAX_WAVES = 4;
constexpr int SA_SLACK = 32;          // outward rounding: < 16 B at each end

__device__ __forceinline__ float sa_h2f(u16 x) {
  return __half2float(__ushort_as_half(x));
}

__device__ __forceinline__ u16 sa_f2h(float f) {
  return __half_as_ushort(__float2half_rn(f));
}

__device__ __forceinline__ bool sa_valid(u16 mask) {  // != 0, -0 is zero
  return (mask & 0x7fff) != 0;
}

// xor-butterflies: every lane ends with the same bits (a + b == b + a)
__device__ __forceinline__ float sa_wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ float sa_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Copy the halves [h0, h1) of `src` (a tensor of `total` halves) into `img`,
// as whole 16-byte chunks of the address range rounded outward.  -> the
// index in img of half h0.
__device__ __forceinline__ int sa_stage(const u16* __restrict__ src,
                                        int64_t total, int64_t h0, int64_t h1,
                                        u16* img) {
  const uintptr_t t0 = (uintptr_t)src, t1 = t0 + 2 * (uintptr_t)total;
  const uintptr_t a0 = t0 + 2 * (uintptr_t)h0, a1 = t0 + 2 * (uintptr_t)h1;
  const uintptr_t c0 = a0 & ~(uintptr_t)15;
  const int nchunks = (int)((((a1 + 15) & ~(uintptr_t)15) - c0) / 16);
  for (int c = threadIdx.x; c < nchunks; c += blockDim.x) {
    const uintptr_t ca = c0 + 16 * (uintptr_t)c;
    uint4 v;
    if (ca >= t0 && ca + 16 <= t1) {
      v = *(const uint4*)ca;
    } else {  // head or tail of the tensor itself: only what lies inside
      u16* e = (u16*)&v;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uintptr_t a = ca + 2 * k;
        e[k] = (a >= t0 && a < t1) ? *(const u16*)a : (u16)0;
      }
    }
    *(uint4*)(img + 8 * c) = v;
  }
  return (int)((a0 - c0) / 2);
}

// The reverse for the halves [h0, h1) of `dst`, which has src's address
// modulo 16: chunks entirely inside the block's own range as 16-byte stores,
// the two boundary chunks half by half (their other halves belong to the
// neighbouring blocks, or lie outside the tensor).
__device__ __forceinline__ void sa_unstage(u16* __restrict__ dst, int64_t h0,
                                           int64_t h1, const u16* img) {
  const uintptr_t a0 = (uintptr_t)dst + 2 * (uintptr_t)h0;
  const uintptr_t a1 = (uintptr_t)dst + 2 * (uintptr_t)h1;
  const uintptr_t c0 = a0 & ~(uintptr_t)15;
  const int nchunks = (int)((((a1 + 15) & ~(uintptr_t)15) - c0) / 16);
  for (int c = threadIdx.x; c < nchunks; c += blockDim.x) {
    const uintptr_t ca = c0 + 16 * (uintptr_t)c;
    const uint4 v = *(const uint4*)(img + 8 * c);
    if (ca >= a0 && ca + 16 <= a1) {
      *(uint4*)ca = v;
    } else {
      const u16* e = (const u16*)&v;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uintptr_t a = ca + 2 * k;
        if (a >= a0 && a < a1) *(u16*)a = e[k];
      }
    }
  }
}

// Softmax over the valid rows of one sample, by the wave that owns it.
// In: sb[l] = s_l of the valid rows.  Out: sb[l] = p_l, -1 for an invalid
// row (a p is never negative; a NaN p stays a NaN and counts as valid).
// -> the lane's valid-row flag for __any.
__device__ __forceinline__ bool sa_softmax(const u16* k, float* sb, int L,
                                           int W, int lane, float m) {
  m = sa_wave_max(m);
  float sum = 0.0f;
  bool has = false;
  for (int l = lane; l < L; l += 64) {
    if (sa_valid(k[l * W + W - 1])) {
      const float e = __expf(sb[l] - m);
      sb[l] = e;
      sum += e;
      has = true;
    } else {
      sb[l] = -1.0f;
    }
  }
  sum = sa_wave_sum(sum);
  const float inv = 1.0f / sum;  // unused when no row is valid
  for (int l = lane; l < L; l += 64)
    if (!(sb[l] < 0.0f)) sb[l] *= inv;
  return has;
}

// LDS: [image: img_halves u16][per wave: q f32[D], s/p f32[L]]
__global__ __launch_bounds__(256) void seq_attn_fwd_kernel(
    const u16* __restrict__ q, const u16* __restrict__ seq,
    u16* __restrict__ out, int B, int L, int D, float scale, int img_halves) {
  extern __shared__ __align__(16) unsigned char sa_lds[];
  u16* img = (u16*)sa_lds;
  const int spb = blockDim.x / 64;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int W = D + 1;
  const int64_t per = (int64_t)L * W;
  const int64_t b0 = (int64_t)blockIdx.x * spb;
  const int64_t b1 = b0 + spb < B ? b0 + spb : (int64_t)B;
  const int head = sa_stage(seq, (int64_t)B * per, b0 * per, b1 * per, img);
  const int64_t b = b0 + wave;
  const bool active = b < B;
  float* qf = (float*)(sa_lds + 2 * (size_t)img_halves) + wave * (L + D);
  float* sb = qf + D;
  if (active)
    for (int d = lane; d < D; d += 64) qf[d] = sa_h2f(q[b * D + d]);
  __syncthreads();
  const u16* k = img + head + wave * (int)per;
  // score: a lane owns rows l, l + 64, ...
  float m = -INFINITY;
  if (active) {
    for (int l = lane; l < L; l += 64) {
      const u16* row = k + l * W;
      if (sa_valid(row[D])) {
        float acc = 0.0f;
        for (int d = 0; d < D; ++d) acc = fmaf(qf[d], sa_h2f(row[d]), acc);
        const float s = scale * acc;
        sb[l] = s;
        m = fmaxf(m, s);
      }
    }
  }
  sa_softmax(k, sb, active ? L : 0, W, lane, m);
  __syncthreads();
  // output: a lane owns columns d, d + 64, ...
  if (active) {
    for (int d = lane; d < D; d += 64) {
      float acc = 0.0f;
      for (int l = 0; l < L; ++l) {
        const float p = sb[l];
        if (!(p < 0.0f)) acc = fmaf(p, sa_h2f(k[l * W + d]), acc);
      }
      out[b * D + d] = sa_f2h(acc);
    }
  }
}

// LDS: [image][per wave: q f32[D], g f32[D], s/p f32[L], dp/ds f32[L]]
__global__ __launch_bounds__(256) void seq_attn_bwd_kernel(
    const u16* __restrict__ g, const u16* __restrict__ q,
    const u16* __restrict__ seq, u16* __restrict__ dq, u16* __restrict__ dseq,
    int B, int L, int D, float scale, int img_halves) {
  extern __shared__ __align__(16) unsigned char sa_lds[];
  u16* img = (u16*)sa_lds;
  const int spb = blockDim.x / 64;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int W = D + 1;
  const int64_t per = (int64_t)L * W;
  const int64_t b0 = (int64_t)blockIdx.x * spb;
  const int64_t b1 = b0 + spb < B ? b0 + spb : (int64_t)B;
  const int head = sa_stage(seq, (int64_t)B * per, b0 * per, b1 * per, img);
  const int64_t b = b0 + wave;
  const bool active = b < B;
  float* qf = (float*)(sa_lds + 2 * (size_t)img_halves) + wave * 2 * (L + D);
  float* gf = qf + D;
  float* sb = gf + D;
  float* db = sb + L;
  if (active) {
    for (int d = lane; d < D; d += 64) {
      qf[d] = sa_h2f(q[b * D + d]);
      gf[d] = sa_h2f(g[b * D + d]);
    }
  }
  __syncthreads();
  u16* k = img + head + wave * (int)per;
  // score and dp in one walk over the row
  float m = -INFINITY;
  if (active) {
    for (int l = lane; l < L; l += 64) {
      const u16* row = k + l * W;
      if (sa_valid(row[D])) {
        float as = 0.0f, ad = 0.0f;
        for (int d = 0; d < D; ++d) {
          const float kv = sa_h2f(row[d]);
          as = fmaf(qf[d], kv, as);
          ad = fmaf(gf[d], kv, ad);
        }
        const float s = scale * as;
        sb[l] = s;
        db[l] = ad;
        m = fmaxf(m, s);
      }
    }
  }
  const int Lw = active ? L : 0;
  const bool any = __any(sa_softmax(k, sb, Lw, W, lane, m));
  float t = 0.0f;  // sum_j p_j dp_j
  for (int l = lane; l < Lw; l += 64)
    if (!(sb[l] < 0.0f)) t = fmaf(sb[l], db[l], t);
  t = sa_wave_sum(t);
  for (int l = lane; l < Lw; l += 64)
    if (!(sb[l] < 0.0f)) db[l] = sb[l] * (db[l] - t);
  __syncthreads();
  // dq: a lane owns columns d, d + 64, ...
  if (active) {
    for (int d = lane; d < D; d += 64) {
      float acc = 0.0f;
      for (int l = 0; l < L; ++l)
        if (!(sb[l] < 0.0f)) acc = fmaf(db[l], sa_h2f(k[l * W + d]), acc);
      dq[b * D + d] = sa_f2h(any ? scale * acc : 0.0f);
    }
  }
  __syncthreads();  // every read of k is done: the rows become dk in place
  if (active) {
    const int dl = 64 / W, dd = 64 % W;
    int l = lane / W, d = lane % W;
    for (int idx = lane; idx < (int)per; idx += 64) {
      const float p = sb[l];
      u16 v = 0;
      if (d < D && !(p < 0.0f))
        v = sa_f2h(fmaf(scale * db[l], qf[d], p * gf[d]));
      k[idx] = v;
      l += dl;
      d += dd;
      if (d >= W) {
        d -= W;
        ++l;
      }
    }
  }
  __syncthreads();
  sa_unstage(dseq, b0 * per, b1 * per, img);
}

struct SaPlan {
  int waves;       // samples per block; 0 = does not fit
  int img_halves;  // LDS image, a multiple of 8 halves
  int lds_bytes;
};

// nf: f32 arrays of length L and of length D per wave (1 forward, 2 backward)
SaPlan sa_plan(int64_t L, int64_t D, int nf) {
  SaPlan p{0, 0, 0};
  if (L < 1 || L > 1024 || D < 8 || D > 256 || D % 8 != 0) return p;
  const int64_t rows = L * (D + 1) * 2, fl = nf * (L + D) * 4;
  const int64_t per = rows + fl;
  if (per + 16 + SA_SLACK > SA_LDS_LIMIT) return p;
  int64_t waves = (SA_LDS_TARGET - 16 - SA_SLACK) / per;
  waves = waves < 1 ? 1 : (waves > SA_MAX_WAVES ? SA_MAX_WAVES : waves);
  const int64_t img = (waves * rows + 15) / 16 * 16 + SA_SLACK;
  p.waves = (int)waves;
  p.img_halves = (int)(img / 2);
  p.lds_bytes = (int)(img + waves * fl);
  return p;
}

hipStream_t sa_stream() { return at::hip::getCurrentHIPStream().stream(); }

// -> the plan; raises on anything the kernels do not take
SaPlan sa_check(const torch::Tensor& q, const torch::Tensor& seq, int nf,
                const char* who) {
  TORCH_CHECK(q.is_cuda() && seq.is_cuda() && q.device() == seq.device(), who,
              ": q and seq must be on one GPU");
  TORCH_CHECK(q.scalar_type() == torch::kFloat16 &&
                  seq.scalar_type() == torch::kFloat16,
              who, ": q and seq must be float16");
  TORCH_CHECK(q.is_contiguous() && seq.is_contiguous(), who,
              ": q and seq must be contiguous");
  TORCH_CHECK(q.dim() == 2 && seq.dim() == 3 && seq.size(0) == q.size(0) &&
                  seq.size(2) == q.size(1) + 1,
              who, ": expected q [B, D] and seq [B, L, D+1]");
  TORCH_CHECK(q.size(0) <= INT32_MAX, who, ": batch too large");
  const SaPlan p = sa_plan(seq.size(1), q.size(1), nf);
  TORCH_CHECK(p.waves > 0, who, ": no kernel for L=", seq.size(1),
              " D=", q.size(1), " (seq_attn_feasible)");
  return p;
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool seq_attn_feasible(int64_t L, int64_t D) {
  return sa_plan(L, D, 2).waves > 0;  // the backward's footprint is the larger
}

torch::Tensor seq_attn_fwd(torch::Tensor q, torch::Tensor seq, double scale) {
  const SaPlan p = sa_check(q, seq, 1, "seq_attn_fwd");
  const int B = (int)q.size(0), D = (int)q.size(1), L = (int)seq.size(1);
  auto out = torch::empty({B, D}, q.options());
  if (B == 0) return out;
  const int grid = (B + p.waves - 1) / p.waves;
  hipLaunchKernelGGL(seq_attn_fwd_kernel, dim3(grid), dim3(p.waves * 64),
                     p.lds_bytes, sa_stream(), (const u16*)q.data_ptr(),
                     (const u16*)seq.data_ptr(), (u16*)out.data_ptr(), B, L, D,
                     (float)scale, p.img_halves);
  return out;
}

std::vector<torch::Tensor> seq_attn_bwd(torch::Tensor g, torch::Tensor q,
                                        torch::Tensor seq, double scale) {
  const SaPlan p = sa_check(q, seq, 2, "seq_attn_bwd");
  TORCH_CHECK(g.is_cuda() && g.device() == q.device() &&
                  g.scalar_type() == torch::kFloat16 && g.is_contiguous() &&
                  g.sizes() == q.sizes(),
              "seq_attn_bwd: g must be a contiguous float16 [B, D] beside q");
  const int B = (int)q.size(0), D = (int)q.size(1), L = (int)seq.size(1);
  auto dq = torch::empty_like(q);
  // dseq at seq's address modulo 16, so the staged image maps back chunk for
  // chunk: a view `off` halves into a buffer with 8 halves to spare
  const int64_t n = seq.numel();
  const int64_t off = (int64_t)(((uintptr_t)seq.data_ptr() & 15) / 2);
  auto buf = torch::empty({n + 8}, seq.options());
  TORCH_CHECK(((uintptr_t)buf.data_ptr() & 15) == 0);
  auto dseq = buf.narrow(0, off, n).view(seq.sizes());
  if (B == 0) return {dq, dseq};
  const int grid = (B + p.waves - 1) / p.waves;
  hipLaunchKernelGGL(seq_attn_bwd_kernel, dim3(grid), dim3(p.waves * 64),
                     p.lds_bytes, sa_stream(), (const u16*)g.data_ptr(),
                     (const u16*)q.data_ptr(), (const u16*)seq.data_ptr(),
                     (u16*)dq.data_ptr(), (u16*)dseq.data_ptr(), B, L, D,
                     (float)scale, p.img_halves);
  return {dq, dseq};
}

void init_seqattn(pybind11::module_& m) {
  m.def("seq_attn_feasible", &seq_attn_feasible,
        "true if the target-attention pooling kernels take (L, D)");
  m.def("seq_attn_fwd", &seq_attn_fwd,
        "out[b] = softmax_valid(scale * seq[b,:,:D] q[b]) @ seq[b,:,:D]");
  m.def("seq_attn_bwd", &seq_attn_bwd,
        "target-attention pooling backward -> (dq, dseq)");
}
