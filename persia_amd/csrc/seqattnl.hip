// Streamed target-attention pooling over a raw (sequence) slot of any length
// up to 1024 (gfx950).  The function is seqattn.hip's:
//
//   seq [B, L, D+1] f16: channels 0..D-1 the row k_l, channel D the 0/1 mask
//   q   [B, D]      f16: the query
//   s_l = scale * <q, k_l>;  p = softmax of s over the valid l;
//   out = sum_{valid l} p_l * k_l                              -> f16 [B, D]
// backward (nothing is saved but q and seq):
//   dp_l = <g, k_l>;  ds_l = p_l * (dp_l - sum_j p_j dp_j)
//   dq   = scale * sum_l ds_l * k_l                            -> f16 [B, D]
//   dk_l = p_l * g + scale * ds_l * q  (valid l), 0 otherwise  -> f16 dseq
// The mask selects: an invalid row is never read into arithmetic, so an Inf
// or NaN there reaches nothing.  A sample without a valid row gives +0.
//
// seqattn.hip holds a whole sample in LDS, one wave per sample; its footprint
// grows with L and ends at 64 KB.  Here a sample is STREAMED: its L rows are
// cut into chunks of C rows (C from D on the host, a chunk image is about
// 8 KB: 64 rows up to D = 64, 32 up to 128, 16 up to 256), and the sample is
// split over the 4 waves of its block.  The LDS of a block is 4 chunk images
// and a few small f32 arrays -- 35 to 37 KB whatever L is, 4 blocks per CU.
//
// Work split: one block of 4 waves per sample, grid = B.  Wave w owns chunks
// w, w+4, w+8, ... and stages each into a wave-PRIVATE image, so the streaming
// loop has no block barrier, only wave-local synchronisation (sal_wave_sync).
// Block barriers stand where the waves meet: after the f32 copy of q (and g),
// and before each merge of the waves' partial results.
//
// Staging.  A chunk's halves are one contiguous byte range with the odd row
// pitch D+1 (which is the LDS padding).  As in seqattn.hip the range is
// rounded outward to 16-byte addresses and copied with 16-byte loads, by the
// wave instead of the block; a 16-byte unit that would leave the tensor's own
// extent is assembled half by half from the part inside it, so a contiguous
// view at any 2-byte alignment is read without touching a byte outside it.
// Prefetch: the loads of the wave's NEXT chunk are issued into registers (at
// most 9 uint4 per lane: 8320 bytes and the outward rounding are 521 units)
// before the arithmetic of the current chunk and written to the image after.
//
// Score phase of a chunk: G = 64 / C lanes share a row; each walks a D / G
// slice of d with the f32 copy of q in LDS as the broadcast operand, and a
// log2(G)-step xor-butterfly joins the slices (at C = 64 a lane owns a row).
// Invalid rows are skipped, not multiplied.
//
// Forward: an online softmax per wave -- running max m, running sum l and the
// out accumulator, a lane owning columns d, d+64, ... and walking the chunk's
// rows with e_l = __expf(s_l - m) as the broadcast; l and the accumulator are
// rescaled when m moves.  A wave that has met no valid row has m = -inf;
// every difference is taken against (m > -inf ? m : 0), so no (-inf) - (-inf)
// arises, and a chunk without a valid row is skipped.  At the end the waves'
// (m, l, acc[D]) meet in LDS (acc in the wave's own image, dead by then) and
// are merged in wave order by one expression; out = acc / l.
//
// Backward: two streamed passes, same split.  Pass 1 computes s_l and dp_l in
// one walk over the row (g is an f32 copy in LDS) and runs an online
// (m, l, T = sum e_l dp_l) per wave; merged in wave order it gives m, 1/l and
// t = T / l.  Pass 2 walks the wave's chunks in REVERSE -- its first chunk is
// the one pass 1 left in the image, so it is not loaded again, and the next
// ones are the most recently read lines: recompute s_l and dp_l, p_l =
// __expf(s_l - m) / l, ds_l = p_l (dp_l - t), dq in the column layout, then
// the image is overwritten in place with dk_l = fma(scale ds_l, q, p_l g)
// (mask column and invalid rows +0) and the wave's byte range is written back
// with 16-byte stores; the two boundary units, shared with the neighbouring
// chunk of another wave or block, half by half and own halves only.  The
// launcher gives dseq seq's address modulo 16, so the image maps back unit
// for unit.  dq is merged in wave order and multiplied by scale.
//
// Order: all sums f32; chunk-to-wave assignment, in-chunk order and the merge
// in wave order are fixed by L and D alone; no atomics.  A sample's out, dq
// and dseq bits do not depend on B, on its place in the batch or on the run.
//
// Matrix instructions do not fit, for seqattn.hip's reason: there is ONE query
// per sample and no operand shared between samples, so every product is a
// matrix-vector one with a single use of each k element -- an MFMA tile would
// be 1/16 full.  The op is bound by the passes over seq and the one over dseq.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdint>

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

using u16 = unsigned short;
using u4 = __attribute__((ext_vector_type(4))) unsigned int;  // 16 bytes

constexpr int SAL_WAVES = 4;
constexpr int SAL_MAXL = 1024;
constexpr int SAL_SLACK = 32;  // outward rounding: < 16 B at each end
constexpr int SAL_NV = 9;      // u4 per lane that hold a chunk in flight

__device__ __forceinline__ float sal_h2f(u16 x) {
  return __half2float(__ushort_as_half(x));
}

__device__ __forceinline__ u16 sal_f2h(float f) {
  return __half_as_ushort(__float2half_rn(f));
}

__device__ __forceinline__ bool sal_valid(u16 mask) {  // != 0, -0 is zero
  return (mask & 0x7fff) != 0;
}

// Orders a wave's own LDS writes before its own (cross-lane) LDS reads.
__device__ __forceinline__ void sal_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// xor-butterflies: every lane ends with the same bits (a + b == b + a)
__device__ __forceinline__ float sal_wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ float sal_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Host and device: bytes of one wave's chunk image.
__host__ __device__ constexpr int sal_img_bytes(int C, int D) {
  return (C * (D + 1) * 2 + 15) / 16 * 16 + SAL_SLACK;
}

// The halves [h0, h1) of a tensor at `base`, rounded outward to 16-byte units.
struct SalRange {
  uintptr_t a0, a1;  // the halves' own byte range
  uintptr_t c0;      // a0 rounded down to 16
  int n;             // units
  int head;          // index in the image of half h0
};

__device__ __forceinline__ SalRange sal_range(const u16* base, int64_t h0,
                                              int64_t h1) {
  SalRange r;
  r.a0 = (uintptr_t)base + 2 * (uintptr_t)h0;
  r.a1 = (uintptr_t)base + 2 * (uintptr_t)h1;
  r.c0 = r.a0 & ~(uintptr_t)15;
  r.n = (int)((((r.a1 + 15) & ~(uintptr_t)15) - r.c0) / 16);
  r.head = (int)((r.a0 - r.c0) / 2);
  return r;
}

// Issue the wave's loads of a range into registers.  [t0, t1) is the tensor's
// own extent; a unit that leaves it (the first or the last of the whole
// tensor, at most) is not loaded here: sal_put assembles it.
__device__ __forceinline__ void sal_load(uintptr_t t0, uintptr_t t1,
                                         const SalRange& r, int lane,
                                         u4 (&pf)[SAL_NV]) {
#pragma unroll
  for (int i = 0; i < SAL_NV; ++i) {
    const uintptr_t ca = r.c0 + 16 * (uintptr_t)(lane + 64 * i);
    if (lane + 64 * i < r.n && ca >= t0 && ca + 16 <= t1)
      pf[i] = *(const u4*)ca;
  }
}

// Write the loaded units to the image; a unit that leaves the tensor's extent
// is assembled half by half from the part inside it.
__device__ __forceinline__ void sal_put(uintptr_t t0, uintptr_t t1,
                                        const SalRange& r, int lane, u16* img,
                                        const u4 (&pf)[SAL_NV]) {
#pragma unroll
  for (int i = 0; i < SAL_NV; ++i) {
    const int u = lane + 64 * i;
    const uintptr_t ca = r.c0 + 16 * (uintptr_t)u;
    if (u < r.n && ca >= t0 && ca + 16 <= t1) *(u4*)(img + 8 * u) = pf[i];
  }
  for (int u = lane; u < r.n; u += 64) {
    const uintptr_t ca = r.c0 + 16 * (uintptr_t)u;
    if (ca >= t0 && ca + 16 <= t1) continue;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
      const uintptr_t a = ca + 2 * k;
      img[8 * u + k] = (a >= t0 && a < t1) ? *(const u16*)a : (u16)0;
    }
  }
}

// The reverse, for a range of dseq (seq's address modulo 16): units entirely
// inside the wave's own range as 16-byte stores, the two boundary units half
// by half and own halves only.
__device__ __forceinline__ void sal_unstage(const SalRange& r, int lane,
                                            const u16* img) {
  for (int u = lane; u < r.n; u += 64) {
    const uintptr_t ca = r.c0 + 16 * (uintptr_t)u;
    if (ca >= r.a0 && ca + 16 <= r.a1) {
      *(u4*)ca = *(const u4*)(img + 8 * u);
    } else {
#pragma unroll 1
      for (int k = 0; k < 8; ++k) {
        const uintptr_t a = ca + 2 * k;
        if (a >= r.a0 && a < r.a1) *(u16*)a = img[8 * u + k];
      }
    }
  }
}

// Score phase: G lanes share row lane / G, each walks a D / G slice of d.
// -> valid (the lane's row exists and its mask is set); as = <q, k_row> and,
// with BWD, ad = <g, k_row>, the same bits in the G lanes of a row.
template <int G, bool BWD>
__device__ __forceinline__ bool sal_dots(const u16* k, const float* qf,
                                         const float* gf, int D, int rows,
                                         int lane, float& as, float& ad) {
  const int W = D + 1, r = lane / G, ds = D / G, d0 = (lane % G) * ds;
  const u16* row = k + r * W;
  const bool valid = r < rows && sal_valid(row[D]);
  as = 0.0f;
  ad = 0.0f;
  if (valid) {
    for (int d = d0; d < d0 + ds; d += 2) {  // D / G is even
      const float k0 = sal_h2f(row[d]), k1 = sal_h2f(row[d + 1]);
      const float2 qv = *(const float2*)(qf + d);
      as = fmaf(qv.x, k0, as);
      as = fmaf(qv.y, k1, as);
      if constexpr (BWD) {
        const float2 gv = *(const float2*)(gf + d);
        ad = fmaf(gv.x, k0, ad);
        ad = fmaf(gv.y, k1, ad);
      }
    }
  }
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) {
    as += __shfl_xor(as, off, 64);
    if constexpr (BWD) ad += __shfl_xor(ad, off, 64);
  }
  return valid;
}

// The waves' running maxima, merged in wave order.  st[4 * w] = m_w.
__device__ __forceinline__ float sal_merged_max(const float* st) {
  float m = st[0];
#pragma unroll
  for (int w = 1; w < SAL_WAVES; ++w) m = fmaxf(m, st[4 * w]);
  return m;
}

// exp(m_w - ref) of a wave's partial sums; 0 for a wave without a valid row
__device__ __forceinline__ float sal_factor(float mw, float ref) {
  return mw > -INFINITY ? __expf(mw - ref) : 0.0f;
}

// LDS: [4 images][q f32[D]][per wave: e f32[C]][per wave: m, l, -, -]
template <int C>
__global__ __launch_bounds__(256, 4) void seq_attn_long_fwd_kernel(
    const u16* __restrict__ q, const u16* __restrict__ seq,
    u16* __restrict__ out, int L, int D, float scale) {
  constexpr int G = 64 / C;  // lanes per row, and columns per lane
  extern __shared__ __align__(16) unsigned char sal_lds[];
  // wave-uniform, and known to be: the ranges and counters stay scalar
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = threadIdx.x % 64;
  const int W = D + 1, IMG = sal_img_bytes(C, D);
  u16* img = (u16*)(sal_lds + wave * IMG);
  float* qf = (float*)(sal_lds + SAL_WAVES * IMG);
  float* sb = qf + D + wave * C;
  float* st = qf + D + SAL_WAVES * C;
  const int64_t b = blockIdx.x, per = (int64_t)L * W, base = b * per;
  const uintptr_t t0 = (uintptr_t)seq;
  const uintptr_t t1 = t0 + 2 * (uintptr_t)((int64_t)gridDim.x * per);
  const int nch = (L + C - 1) / C;
  for (int d = threadIdx.x; d < D; d += 256) qf[d] = sal_h2f(q[b * D + d]);
  __syncthreads();

  auto range = [&](int c) {
    const int rows = L - c * C < C ? L - c * C : C;
    const int64_t h0 = base + (int64_t)c * C * W;
    return sal_range(seq, h0, h0 + (int64_t)rows * W);
  };
  float m = -INFINITY, l = 0.0f, acc[G];
#pragma unroll
  for (int j = 0; j < G; ++j) acc[j] = 0.0f;
  u4 pf[SAL_NV];
  SalRange cur{}, nxt{};
  if (wave < nch) {
    cur = range(wave);
    sal_load(t0, t1, cur, lane, pf);
    sal_put(t0, t1, cur, lane, img, pf);
  }
  sal_wave_sync();
  for (int c = wave; c < nch; c += SAL_WAVES) {
    const bool more = c + SAL_WAVES < nch;
    if (more) {
      nxt = range(c + SAL_WAVES);
      sal_load(t0, t1, nxt, lane, pf);
    }
    const int rows = L - c * C < C ? L - c * C : C;
    const u16* k = img + cur.head;
    float as, ad;
    const bool valid = sal_dots<G, false>(k, qf, nullptr, D, rows, lane, as, ad);
    const float s = scale * as;
    const float cm = sal_wave_max(valid ? s : -INFINITY);
    if (cm > -INFINITY) {  // a chunk without a valid row is skipped
      const float mn = fmaxf(m, cm);
      const float alpha = sal_factor(m, mn);
      const float e = valid ? __expf(s - mn) : 0.0f;
      if (lane % G == 0) sb[lane / G] = valid ? e : -1.0f;  // -1: not a row
      l = fmaf(l, alpha, sal_wave_sum(lane % G == 0 ? e : 0.0f));
      m = mn;
      sal_wave_sync();
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int d = lane + 64 * j;
        float a = acc[j] * alpha;
        if (d < D) {
          for (int r = 0; r < rows; ++r) {
            const float p = sb[r];
            if (!(p < 0.0f)) a = fmaf(p, sal_h2f(k[r * W + d]), a);
          }
        }
        acc[j] = a;
      }
    }
    sal_wave_sync();  // every read of the image and of sb is done
    if (more) sal_put(t0, t1, nxt, lane, img, pf);
    cur = nxt;
    sal_wave_sync();
  }
  // the waves meet: acc in the wave's own image, (m, l) in st
  float* accw = (float*)img;
#pragma unroll
  for (int j = 0; j < G; ++j)
    if (lane + 64 * j < D) accw[lane + 64 * j] = acc[j];
  if (lane == 0) st[4 * wave] = m, st[4 * wave + 1] = l;
  __syncthreads();
  const int d = threadIdx.x;
  if (d < D) {
    const float mm = sal_merged_max(st);
    const float ref = mm > -INFINITY ? mm : 0.0f;
    float ls = 0.0f, a = 0.0f;
#pragma unroll
    for (int w = 0; w < SAL_WAVES; ++w) {
      const float f = sal_factor(st[4 * w], ref);
      ls = fmaf(f, st[4 * w + 1], ls);
      a = fmaf(f, ((const float*)(sal_lds + w * IMG))[d], a);
    }
    out[b * D + d] = sal_f2h(mm > -INFINITY ? a / ls : 0.0f);
  }
}

// LDS: [4 images][q f32[D]][g f32[D]][per wave: p f32[C], ds f32[C]]
//      [per wave: m, l, T, -]
template <int C>
__global__ __launch_bounds__(256, 4) void seq_attn_long_bwd_kernel(
    const u16* __restrict__ g, const u16* __restrict__ q,
    const u16* __restrict__ seq, u16* __restrict__ dq, u16* __restrict__ dseq,
    int L, int D, float scale) {
  constexpr int G = 64 / C;
  extern __shared__ __align__(16) unsigned char sal_lds[];
  // wave-uniform, and known to be: the ranges and counters stay scalar
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = threadIdx.x % 64;
  const int W = D + 1, IMG = sal_img_bytes(C, D);
  u16* img = (u16*)(sal_lds + wave * IMG);
  float* qf = (float*)(sal_lds + SAL_WAVES * IMG);
  float* gf = qf + D;
  float* sb = gf + D + wave * 2 * C;
  float* db = sb + C;
  float* st = gf + D + SAL_WAVES * 2 * C;
  const int64_t b = blockIdx.x, per = (int64_t)L * W, base = b * per;
  const uintptr_t t0 = (uintptr_t)seq;
  const uintptr_t t1 = t0 + 2 * (uintptr_t)((int64_t)gridDim.x * per);
  const int nch = (L + C - 1) / C;
  for (int d = threadIdx.x; d < D; d += 256) {
    qf[d] = sal_h2f(q[b * D + d]);
    gf[d] = sal_h2f(g[b * D + d]);
  }
  __syncthreads();

  auto rows_of = [&](int c) { return L - c * C < C ? L - c * C : C; };
  auto range = [&](const u16* t, int c) {
    const int64_t h0 = base + (int64_t)c * C * W;
    return sal_range(t, h0, h0 + (int64_t)rows_of(c) * W);
  };
  u4 pf[SAL_NV];
  SalRange cur{}, nxt{};
  // pass 1: online (m, l, T = sum e dp) over the wave's chunks, ascending
  float m = -INFINITY, l = 0.0f, T = 0.0f;
  if (wave < nch) {
    cur = range(seq, wave);
    sal_load(t0, t1, cur, lane, pf);
    sal_put(t0, t1, cur, lane, img, pf);
  }
  sal_wave_sync();
  int last = -1;  // the wave's last chunk: what pass 1 leaves in the image
  for (int c = wave; c < nch; c += SAL_WAVES) {
    const bool more = c + SAL_WAVES < nch;
    if (more) {
      nxt = range(seq, c + SAL_WAVES);
      sal_load(t0, t1, nxt, lane, pf);
    }
    float as, ad;
    const bool valid = sal_dots<G, true>(img + cur.head, qf, gf, D, rows_of(c),
                                         lane, as, ad);
    const float s = scale * as;
    const float cm = sal_wave_max(valid ? s : -INFINITY);
    if (cm > -INFINITY) {
      const float mn = fmaxf(m, cm);
      const float alpha = sal_factor(m, mn);
      const bool own = valid && lane % G == 0;  // one lane of a row adds it
      const float e = own ? __expf(s - mn) : 0.0f;
      l = fmaf(l, alpha, sal_wave_sum(e));
      T = fmaf(T, alpha, sal_wave_sum(own ? e * ad : 0.0f));
      m = mn;
    }
    last = c;
    if (more) {
      sal_wave_sync();  // every read of the image is done
      sal_put(t0, t1, nxt, lane, img, pf);
      cur = nxt;
      sal_wave_sync();
    }
  }
  if (lane == 0) st[4 * wave] = m, st[4 * wave + 1] = l, st[4 * wave + 2] = T;
  __syncthreads();
  const float mm = sal_merged_max(st);
  const bool any = mm > -INFINITY;
  const float ref = any ? mm : 0.0f;
  float ls = 0.0f, Ts = 0.0f;
#pragma unroll
  for (int w = 0; w < SAL_WAVES; ++w) {
    const float f = sal_factor(st[4 * w], ref);
    ls = fmaf(f, st[4 * w + 1], ls);
    Ts = fmaf(f, st[4 * w + 2], Ts);
  }
  const float inv = 1.0f / ls, t = Ts / ls;  // unused when no row is valid

  // pass 2: the wave's chunks again, descending from the one in the image
  const uintptr_t o0 = (uintptr_t)dseq;  // == t0 modulo 16
  float acc[G];
#pragma unroll
  for (int j = 0; j < G; ++j) acc[j] = 0.0f;
  for (int c = last; c >= 0; c -= SAL_WAVES) {
    const bool more = c - SAL_WAVES >= 0;
    if (more) {
      nxt = range(seq, c - SAL_WAVES);
      sal_load(t0, t1, nxt, lane, pf);
    }
    const int rows = rows_of(c);
    u16* k = img + cur.head;
    float as, ad;
    const bool valid = sal_dots<G, true>(k, qf, gf, D, rows, lane, as, ad);
    const float p = valid ? __expf(scale * as - ref) * inv : -1.0f;
    if (lane % G == 0) {
      sb[lane / G] = p;  // -1: not a row (a NaN p stays a NaN and counts)
      db[lane / G] = p * (ad - t);
    }
    sal_wave_sync();
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int d = lane + 64 * j;
      if (d < D) {
        float a = acc[j];
        for (int r = 0; r < rows; ++r)
          if (!(sb[r] < 0.0f)) a = fmaf(db[r], sal_h2f(k[r * W + d]), a);
        acc[j] = a;
      }
    }
    sal_wave_sync();  // every read of k is done: the rows become dk in place
    {
      const int dl = 64 / W, dd = 64 % W;
      int r = lane / W, d = lane % W;
      for (int idx = lane; idx < rows * W; idx += 64) {
        const float pr = sb[r];
        u16 v = 0;
        if (d < D && !(pr < 0.0f))
          v = sal_f2h(fmaf(scale * db[r], qf[d], pr * gf[d]));
        k[idx] = v;
        r += dl;
        d += dd;
        if (d >= W) {
          d -= W;
          ++r;
        }
      }
    }
    sal_wave_sync();
    SalRange wr = cur;  // the same units of dseq: its address is seq's mod 16
    wr.a0 = cur.a0 - t0 + o0;
    wr.a1 = cur.a1 - t0 + o0;
    wr.c0 = cur.c0 - t0 + o0;
    sal_unstage(wr, lane, img);
    sal_wave_sync();  // the image is read out
    if (more) sal_put(t0, t1, nxt, lane, img, pf);
    cur = nxt;
    sal_wave_sync();
  }
  float* accw = (float*)img;
#pragma unroll
  for (int j = 0; j < G; ++j)
    if (lane + 64 * j < D) accw[lane + 64 * j] = acc[j];
  __syncthreads();
  const int d = threadIdx.x;
  if (d < D) {
    float a = ((const float*)sal_lds)[d];
#pragma unroll
    for (int w = 1; w < SAL_WAVES; ++w)
      a += ((const float*)(sal_lds + w * IMG))[d];
    dq[b * D + d] = sal_f2h(any ? scale * a : 0.0f);
  }
}

int sal_chunk_rows(int64_t D) { return D <= 64 ? 64 : D <= 128 ? 32 : 16; }

// nf: f32 arrays of length C per wave and of length D (1 forward, 2 backward)
int sal_lds_bytes(int C, int D, int nf) {
  return SAL_WAVES * sal_img_bytes(C, D) + nf * 4 * (D + SAL_WAVES * C) +
         SAL_WAVES * 16;
}

hipStream_t sal_stream() { return at::hip::getCurrentHIPStream().stream(); }

bool sal_feasible(int64_t L, int64_t D) {
  return L >= 1 && L <= SAL_MAXL && D >= 8 && D <= 256 && D % 8 == 0;
}

// raises on anything the kernels do not take
void sal_check(const torch::Tensor& q, const torch::Tensor& seq,
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
  TORCH_CHECK(sal_feasible(seq.size(1), q.size(1)), who, ": no kernel for L=",
              seq.size(1), " D=", q.size(1), " (seq_attn_long_feasible)");
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool seq_attn_long_feasible(int64_t L, int64_t D) { return sal_feasible(L, D); }

torch::Tensor seq_attn_long_fwd(torch::Tensor q, torch::Tensor seq,
                                double scale) {
  sal_check(q, seq, "seq_attn_long_fwd");
  const int B = (int)q.size(0), D = (int)q.size(1), L = (int)seq.size(1);
  auto out = torch::empty({B, D}, q.options());
  if (B == 0) return out;
  const int C = sal_chunk_rows(D), lds = sal_lds_bytes(C, D, 1);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(B), dim3(SAL_WAVES * 64), lds, sal_stream(),
                       (const u16*)q.data_ptr(), (const u16*)seq.data_ptr(),
                       (u16*)out.data_ptr(), L, D, (float)scale);
  };
  if (C == 64) launch(seq_attn_long_fwd_kernel<64>);
  else if (C == 32) launch(seq_attn_long_fwd_kernel<32>);
  else launch(seq_attn_long_fwd_kernel<16>);
  return out;
}

std::vector<torch::Tensor> seq_attn_long_bwd(torch::Tensor g, torch::Tensor q,
                                             torch::Tensor seq, double scale) {
  sal_check(q, seq, "seq_attn_long_bwd");
  TORCH_CHECK(g.is_cuda() && g.device() == q.device() &&
                  g.scalar_type() == torch::kFloat16 && g.is_contiguous() &&
                  g.sizes() == q.sizes(),
              "seq_attn_long_bwd: g must be a contiguous float16 [B, D] beside q");
  const int B = (int)q.size(0), D = (int)q.size(1), L = (int)seq.size(1);
  auto dq = torch::empty_like(q);
  // dseq at seq's address modulo 16, so the staged image maps back unit for
  // unit: a view `off` halves into a buffer with 8 halves to spare
  const int64_t n = seq.numel();
  const int64_t off = (int64_t)(((uintptr_t)seq.data_ptr() & 15) / 2);
  auto buf = torch::empty({n + 8}, seq.options());
  TORCH_CHECK(((uintptr_t)buf.data_ptr() & 15) == 0);
  auto dseq = buf.narrow(0, off, n).view(seq.sizes());
  if (B == 0) return {dq, dseq};
  const int C = sal_chunk_rows(D), lds = sal_lds_bytes(C, D, 2);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(B), dim3(SAL_WAVES * 64), lds, sal_stream(),
                       (const u16*)g.data_ptr(), (const u16*)q.data_ptr(),
                       (const u16*)seq.data_ptr(), (u16*)dq.data_ptr(),
                       (u16*)dseq.data_ptr(), L, D, (float)scale);
  };
  if (C == 64) launch(seq_attn_long_bwd_kernel<64>);
  else if (C == 32) launch(seq_attn_long_bwd_kernel<32>);
  else launch(seq_attn_long_bwd_kernel<16>);
  return {dq, dseq};
}

void init_seqattnl(pybind11::module_& m) {
  m.def("seq_attn_long_feasible", &seq_attn_long_feasible,
        "true if the streamed target-attention pooling kernels take (L, D)");
  m.def("seq_attn_long_fwd", &seq_attn_long_fwd,
        "seq_attn_fwd's function, the sample streamed through LDS in chunks");
  m.def("seq_attn_long_bwd", &seq_attn_long_bwd,
        "streamed target-attention pooling backward -> (dq, dseq)");
}
