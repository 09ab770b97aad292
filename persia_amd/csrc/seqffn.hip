// The tail of a transformer block over the rows of a raw slot (gfx950):
// out-projection, add & LayerNorm, feed-forward, add & LayerNorm.
//
//   x, a [B, L, D+1] f16: the block input and the attention output, channel D
//                         the 0/1 mask (the mask of x decides)
//   Wo [D, D], W1 [F, D], W2 [D, F] f16 (the f16 roundings of the masters)
//   bo, g1, be1, b2, g2, be2 [D], b1 [F] f32
//   valid i:   u_i = LN(x_i + Wo a_i + bo; g1, be1)
//              h_i = relu(W1 f16(u_i) + b1)
//              y_i = LN(u_i + W2 f16(h_i) + b2; g2, be2);  out_i = f16(y_i)
//   invalid i: out_i = +0;   out[..., D] = x[..., D]
// backward (u, h and both LN statistics are RECOMPUTED, only inputs are saved):
//   dxh2 = g g2;  dw = LN2'(dxh2);  dh = dw W2;  dz = dh [z > 0]
//   du = dw + dz W1;  dv = LN1'(du g1);  dx = dv;  da = dv Wo
//   dW2 = dw^T f16(h);  dW1 = dz^T f16(u);  dWo = dv^T a;  the bias and LN
//   parameter gradients are column sums.
//
// Work split.  Rows are independent, so the R = B L rows of the flattened
// tensor are cut into tiles of 64 rows, four 16-row strips, one wave per
// strip; a persistent grid of 4-wave blocks, block i walks the tiles
// [i T/G, (i+1) T/G).  A strip without a valid row is skipped: it costs its
// zero stores (and, in the backward, its zero rows of the shared images).
//
// Staging is seqsa.hip's: aligned 32-bit words, boundary words half by half,
// never outside the tensor, images of pitch D+8, the mask in its own array,
// invalid rows and the tail zeroed before any product.
//
// A wave owns all D columns of its strip, so a row's D values sit in the 16
// lanes of one accumulator row group (lane = column fi of every 16-column
// tile, rows 4 fg .. 4 fg + 3) and both LayerNorms are xor butterflies over
// those lanes, two-pass (mean, then centred squares), 1 / sqrtf exact.  The
// hidden layer is streamed in chunks of 32 columns: two GEMM1 tiles, bias and
// ReLU, f16 to the wave's rows of a chunk image, one GEMM2 k-step into the D
// column accumulators.  Nothing of width F is stored, on or off chip.  The
// weights are read as B-fragments straight from global memory (they stay in
// L1/L2: at most 72 KB); the backward launcher passes their transposes too, so
// that every fragment is 8 contiguous halves.
//
// The backward runs the chunks twice per strip: once to get w (for LN2's
// statistics), once for dh, dz, du and the weight gradients.  dw, dz and dv
// are f32 values and are staged as TWO f16 images, hi = f16(v) and lo =
// f16((v - hi) 2^11), every product once per image.  dW2, dW1 and dWo reduce
// over the 64 rows of the tile: after a block barrier per chunk the waves
// split the output tiles and read both operands by ds_read_b64_tr_b16 from
// the linear images.  dWo and the D-wide column sums stay in registers across
// the block's tiles; the dW2 and dW1 tiles are added, chunk by chunk and tile
// by tile, into the block's own f32 partial (one owner lane per element, the
// partial stays in L2), db1 into LDS.  Holding dW2 and dW1 in registers too
// needs the chunk loop unrolled, and at D = 64, F > 128 that spilled.  The
// partials are summed in block order by ff_reduce_kernel: no atomics.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

using u16 = unsigned short;
using h8 = __attribute__((ext_vector_type(8))) _Float16;
using h4 = __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16;
using f4 = __attribute__((ext_vector_type(4))) float;
using u4 = __attribute__((ext_vector_type(4))) unsigned int;

constexpr int FF_ROWS = 64;  // rows of a tile: 4 strips of 16
constexpr int FF_HP = 40;    // pitch of the chunk images: 32 columns + 8
constexpr float FF_LO = 2048.0f;
constexpr float FF_LO_INV = 1.0f / 2048.0f;

__device__ __forceinline__ float ff_h2f(u16 x) {
  return (float)__builtin_bit_cast(_Float16, x);
}

__device__ __forceinline__ u16 ff_f2h(float f) {  // round to nearest even
  return __builtin_bit_cast(u16, (_Float16)f);
}

__device__ __forceinline__ void ff_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Orders a wave's own LDS writes before its own (cross-lane) LDS reads.
__device__ __forceinline__ void ff_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float ff_shfl(float v, int src_lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src_lane << 2,
                                          __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ bool ff_valid(u16 mask) {  // != 0, -0 is zero
  return (mask & 0x7fff) != 0;
}

__device__ __forceinline__ f4 ff_mfma(h8 a, h8 b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f4 ff_zero4() { return f4{0.0f, 0.0f, 0.0f, 0.0f}; }

__device__ __forceinline__ h8 ff_ld8(const u16* p) { return *(const h8*)p; }

// The same pointer, as far as the compiler knows a new one: the loads behind
// it are not hoisted out of the tile loop into registers held across it.
template <typename T>
__device__ __forceinline__ const T* ff_opaque(const T* p) {
  asm volatile("" : "+s"(p));
  return p;
}

__device__ __forceinline__ void ff_split(float v, u16& hi, u16& lo) {
  const _Float16 h = (_Float16)v;
  hi = __builtin_bit_cast(u16, h);
  lo = __builtin_bit_cast(u16, (_Float16)((v - (float)h) * FF_LO));
}

// Rows [0, nrows) of the flattened tensor from half s on (pitch D+1) -> img
// (pitch D+8), channel D -> mask.  total = src.numel().
template <int D>
__device__ __forceinline__ void ff_stage(const u16* __restrict__ src,
                                         int64_t total, int64_t s, int nrows,
                                         u16* img, u16* mask) {
  constexpr int W = D + 1, XP = D + 8;
  const uintptr_t t0 = (uintptr_t)src, t1 = t0 + 2 * (uintptr_t)total;
  const uintptr_t a0 = t0 + 2 * (uintptr_t)s;
  const uintptr_t a1 = a0 + 2 * (uintptr_t)(nrows * W);
  const uintptr_t c0 = a0 & ~(uintptr_t)3;
  const int nw = (int)((((a1 + 3) & ~(uintptr_t)3) - c0) / 4);
  for (int base = threadIdx.x; base < nw; base += 4 * 256) {
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // the loads first, then the LDS writes
      const int i = base + j * 256;
      const uintptr_t ca = c0 + 4 * (uintptr_t)i;
      v[j] = 0;
      if (i < nw) {
        if (ca >= t0 && ca + 4 <= t1) {
          v[j] = *(const uint32_t*)ca;
        } else {  // a word across the tensor's own end: the half inside
          if (ca >= t0 && ca < t1) v[j] = *(const u16*)ca;
          if (ca + 2 >= t0 && ca + 2 < t1)
            v[j] |= (uint32_t)(*(const u16*)(ca + 2)) << 16;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = base + j * 256;
      const uintptr_t ca = c0 + 4 * (uintptr_t)i;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const uintptr_t a = ca + 2 * e;
        if (i < nw && a >= a0 && a < a1) {
          const int hx = (int)((a - a0) / 2);
          const int row = hx / W, col = hx - row * W;
          const u16 x = (u16)(v[j] >> (16 * e));
          if (col < D) img[row * XP + col] = x;
          else mask[row] = x;
        }
      }
    }
  }
}

// All 64 rows: rows past nrows and the rows `mask` calls invalid become zeros
// in img.  own: mask belongs to img, its tail is cleared.  A wave touches the
// rows of its own strip only.
template <int D>
__device__ __forceinline__ void ff_fix(u16* img, u16* mask, int nrows,
                                       bool own, int wave, int lane) {
  constexpr int XP = D + 8;
  const int row = wave * 16 + (lane >> 2), part = lane & 3;
  const bool tail = row >= nrows;
  const bool bad = tail || !ff_valid(mask[row]);
  if (bad) {
    for (int c = part; c < D / 8; c += 4)
      *(u4*)&img[row * XP + c * 8] = u4{0, 0, 0, 0};
  }
  if (own && tail && part == 0) mask[row] = 0;
}

// 8 halves img[kb + 8*fg + j][cb + fi], j = 0..7: the fragment of an operand
// whose reduction index runs down the rows of a linear image.
__device__ __forceinline__ h8 ff_tr(const u16* img, int pitch, int kb, int cb,
                                    int lane) {
  const u16* b0 = img + (kb + (lane >> 4) * 8 + ((lane & 15) >> 2)) * pitch +
                  cb + (lane & 3) * 4;
  const h4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16(
      (__attribute__((address_space(3))) h4*)(void*)const_cast<u16*>(b0));
  const h4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16(
      (__attribute__((address_space(3))) h4*)(void*)const_cast<u16*>(
          b0 + 4 * pitch));
  return __builtin_bit_cast(h8,
                            __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// sum over the 16 lanes that hold one row
__device__ __forceinline__ float ff_rowsum(float v, int lane) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v += ff_shfl(v, lane ^ off);
  return v;
}

// sum over the 16 rows of the strip of one column (the same in every fg)
__device__ __forceinline__ float ff_colsum(f4 v, int lane) {
  float s = (v[0] + v[1]) + (v[2] + v[3]);
  s += ff_shfl(s, lane ^ 16);
  s += ff_shfl(s, lane ^ 32);
  return s;
}

// v -> (v - mean) rstd in place, over the 16 NT columns of each row
template <int NT>
__device__ __forceinline__ void ff_ln(f4 (&v)[NT], float eps, int lane,
                                      float (&rstd)[4]) {
  constexpr float inv = 1.0f / (16 * NT);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float s = 0.0f;
#pragma unroll
    for (int n = 0; n < NT; ++n) s += v[n][r];
    const float mean = ff_rowsum(s, lane) * inv;
    float q = 0.0f;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      v[n][r] -= mean;
      q = fmaf(v[n][r], v[n][r], q);
    }
    rstd[r] = 1.0f / sqrtf(ff_rowsum(q, lane) * inv + eps);
#pragma unroll
    for (int n = 0; n < NT; ++n) v[n][r] *= rstd[r];
  }
}

// d (the gradient of the normalised row xh) -> the gradient of LN's input
template <int NT>
__device__ __forceinline__ void ff_ln_bwd(f4 (&d)[NT], const f4 (&xh)[NT],
                                          const float (&rstd)[4], int lane) {
  constexpr float inv = 1.0f / (16 * NT);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float s = 0.0f, q = 0.0f;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      s += d[n][r];
      q = fmaf(d[n][r], xh[n][r], q);
    }
    const float m1 = ff_rowsum(s, lane) * inv, m2 = ff_rowsum(q, lane) * inv;
#pragma unroll
    for (int n = 0; n < NT; ++n)
      d[n][r] = rstd[r] * ((d[n][r] - m1) - xh[n][r] * m2);
  }
}

// xh (normalised, in v) -> u = xh g + b, xh kept
template <int NT>
__device__ __forceinline__ void ff_affine(const f4 (&xh)[NT], f4 (&u)[NT],
                                          const float* __restrict__ g,
                                          const float* __restrict__ b, int fi) {
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const float gg = g[n * 16 + fi], bb = b[n * 16 + fi];
#pragma unroll
    for (int r = 0; r < 4; ++r) u[n][r] = fmaf(xh[n][r], gg, bb);
  }
}

// acc[n] = the strip's rows of img (from row0 on) times W^T, W [16 NT, D]
template <int D>
__device__ __forceinline__ void ff_gemm_dd(const u16* img, int row0,
                                           const u16* __restrict__ W, int lane,
                                           f4 (&acc)[D / 16]) {
  constexpr int XP = D + 8, KD = D / 32;
  const int fi = lane & 15, fg = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < KD; ++ks) {
    const h8 af = ff_ld8(&img[(row0 + fi) * XP + ks * 32 + fg * 8]);
#pragma unroll
    for (int n = 0; n < D / 16; ++n)
      acc[n] = ff_mfma(af, ff_ld8(&W[(n * 16 + fi) * D + ks * 32 + fg * 8]),
                       acc[n]);
  }
}

// One tile t of the hidden layer: uf (the strip's f16 u fragments) times the
// rows 16 t .. of W [F, D]
template <int KD>
__device__ __forceinline__ f4 ff_hidden(const h8 (&uf)[KD],
                                        const u16* __restrict__ W, int t,
                                        int lane) {
  const int fi = lane & 15, fg = lane >> 4;
  f4 acc = ff_zero4();
#pragma unroll
  for (int ks = 0; ks < KD; ++ks)
    acc = ff_mfma(uf[ks],
                  ff_ld8(&W[(t * 16 + fi) * (KD * 32) + ks * 32 + fg * 8]), acc);
  return acc;
}

// The strip's forward: from its zeroed rows of ximg and aimg to xh1, u (f32)
// and w (before LN2).  f16(u) goes over the strip's dead rows of uimg (which
// may be ximg or aimg: both are read before the write), the hidden chunks
// through the strip's rows of himg.
template <int D>
__device__ __forceinline__ void ff_forward_strip(
    const u16* ximg, const u16* aimg, u16* uimg, u16* himg, int row0,
    const bool (&ok)[4], const u16* __restrict__ Wo, const u16* __restrict__ W1,
    const u16* __restrict__ W2, const float* __restrict__ bo,
    const float* __restrict__ g1, const float* __restrict__ be1,
    const float* __restrict__ b1, const float* __restrict__ b2, int F,
    float eps, int lane, f4 (&xh1)[D / 16], float (&r1)[4], f4 (&u)[D / 16],
    h8 (&uf)[D / 32], f4 (&w)[D / 16]) {
  constexpr int XP = D + 8, NT = D / 16, KD = D / 32;
  const int fi = lane & 15, fg = lane >> 4;
#pragma unroll
  for (int n = 0; n < NT; ++n) xh1[n] = ff_zero4();
  ff_gemm_dd<D>(aimg, row0, Wo, lane, xh1);
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const float bb = bo[n * 16 + fi];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      xh1[n][r] = (xh1[n][r] + bb) +
                  ff_h2f(ximg[(row0 + fg * 4 + r) * XP + n * 16 + fi]);
  }
  ff_ln<NT>(xh1, eps, lane, r1);
  ff_affine<NT>(xh1, u, g1, be1, fi);
  ff_wave_sync();  // the strip's reads of ximg and aimg
#pragma unroll
  for (int n = 0; n < NT; ++n) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      uimg[(row0 + fg * 4 + r) * XP + n * 16 + fi] =
          ok[r] ? ff_f2h(u[n][r]) : (u16)0;
  }
  ff_wave_sync();
#pragma unroll
  for (int ks = 0; ks < KD; ++ks)
    uf[ks] = ff_ld8(&uimg[(row0 + fi) * XP + ks * 32 + fg * 8]);
#pragma unroll
  for (int n = 0; n < NT; ++n) w[n] = ff_zero4();
#pragma unroll 1
  for (int c = 0; c < F / 32; ++c) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int t = c * 2 + j;
      const f4 z = ff_hidden<KD>(uf, W1, t, lane);
      const float bb = b1[t * 16 + fi];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float zz = z[r] + bb;
        himg[(row0 + fg * 4 + r) * FF_HP + j * 16 + fi] =
            ff_f2h(zz > 0.0f ? zz : 0.0f);
      }
    }
    ff_wave_sync();
    const h8 hf = ff_ld8(&himg[(row0 + fi) * FF_HP + fg * 8]);
#pragma unroll
    for (int n = 0; n < NT; ++n)
      w[n] = ff_mfma(hf, ff_ld8(&W2[(n * 16 + fi) * F + c * 32 + fg * 8]), w[n]);
    ff_wave_sync();  // before the next chunk overwrites himg
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const float bb = b2[n * 16 + fi];
#pragma unroll
    for (int r = 0; r < 4; ++r) w[n][r] = (w[n][r] + bb) + u[n][r];
  }
}

// ok[r]: row row0 + 4 fg + r of the tile is valid; -> the strip has a valid row
__device__ __forceinline__ bool ff_strip_ok(const u16* mask, int row0, int fg,
                                            bool (&ok)[4]) {
  bool any = false;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    ok[r] = ff_valid(mask[row0 + fg * 4 + r]);
    any = any || ok[r];
  }
  return __builtin_amdgcn_ballot_w64(any) != 0;
}

template <int D>
__global__ __launch_bounds__(256) void seq_ffn_fwd_kernel(
    const u16* __restrict__ x, const u16* __restrict__ a,
    const u16* __restrict__ Wo, const u16* __restrict__ W1,
    const u16* __restrict__ W2, const float* __restrict__ bo,
    const float* __restrict__ g1, const float* __restrict__ be1,
    const float* __restrict__ b1, const float* __restrict__ b2,
    const float* __restrict__ g2, const float* __restrict__ be2,
    u16* __restrict__ out, int64_t R, int F, float eps) {
  constexpr int XP = D + 8, NT = D / 16, KD = D / 32;
  __shared__ __align__(16) u16 ximg[FF_ROWS * XP];
  __shared__ __align__(16) u16 aimg[FF_ROWS * XP];
  __shared__ __align__(16) u16 himg[FF_ROWS * FF_HP];
  __shared__ u16 mask[FF_ROWS];
  __shared__ u16 amask[FF_ROWS];  // channel D of a: staged, never used
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4, row0 = wave * 16;
  const int64_t total = R * (D + 1), ntiles = (R + FF_ROWS - 1) / FF_ROWS;
  const int64_t ts = (int64_t)blockIdx.x * ntiles / gridDim.x;
  const int64_t te = ((int64_t)blockIdx.x + 1) * ntiles / gridDim.x;
  for (int64_t t = ts; t < te; ++t) {
    const int64_t rb = t * FF_ROWS;
    const int nrows = (int)(R - rb < FF_ROWS ? R - rb : FF_ROWS);
    ff_sync();  // the last tile's readers are done
    ff_stage<D>(x, total, rb * (D + 1), nrows, ximg, mask);
    ff_stage<D>(a, total, rb * (D + 1), nrows, aimg, amask);
    ff_sync();
    ff_fix<D>(ximg, mask, nrows, true, wave, lane);
    ff_fix<D>(aimg, mask, nrows, false, wave, lane);
    ff_wave_sync();
    bool ok[4];
    const bool live = ff_strip_ok(mask, row0, fg, ok);
    f4 y[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) y[n] = ff_zero4();
    if (live) {
      f4 xh1[NT], u[NT];
      h8 uf[KD];
      float r1[4], r2[4];
      ff_forward_strip<D>(ximg, aimg, aimg, himg, row0, ok, Wo, W1, W2, bo, g1,
                          be1, b1, b2, F, eps, lane, xh1, r1, u, uf, y);
      ff_ln<NT>(y, eps, lane, r2);
      ff_affine<NT>(y, y, g2, be2, fi);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + fg * 4 + r;
      if (row < nrows) {
        u16* dst = out + (rb + row) * (D + 1);
#pragma unroll
        for (int n = 0; n < NT; ++n)
          dst[n * 16 + fi] = ok[r] ? ff_f2h(y[n][r]) : (u16)0;
        if (fi == 0) dst[D] = mask[row];
      }
    }
  }
}

// Partials of one block, f32, in the order of the op's parameters:
//   [dWo D*D][dbo D][dg1 D][dbe1 D][dW1 F*D][db1 F][dW2 D*F][db2 D][dg2 D][dbe2 D]
template <int D>
__global__ __launch_bounds__(256) void seq_ffn_bwd_kernel(
    const u16* __restrict__ g, const u16* __restrict__ x,
    const u16* __restrict__ a, const u16* __restrict__ Wo_,
    const u16* __restrict__ WoT_, const u16* __restrict__ W1_,
    const u16* __restrict__ W1T_, const u16* __restrict__ W2_,
    const u16* __restrict__ W2T_, const float* __restrict__ bo,
    const float* __restrict__ g1, const float* __restrict__ be1,
    const float* __restrict__ b1_, const float* __restrict__ b2,
    const float* __restrict__ g2, u16* __restrict__ dx, u16* __restrict__ da,
    float* __restrict__ part, int64_t R, int F, float eps) {
  constexpr int XP = D + 8, NT = D / 16, KD = D / 32, FMAX = 256;
  constexpr int TW = NT / 2;         // dW2 / dW1 tiles of a wave and chunk
  constexpr int TO = NT * NT / 4;    // dWo tiles of a wave
  constexpr int IMG = FF_ROWS * XP, CIMG = FF_ROWS * FF_HP;
  static_assert(4 * 6 * D * 4 <= 2 * IMG * 2, "the column sums overlay x and a");
  __shared__ __align__(16) u16 lds[4 * IMG + 3 * CIMG];
  __shared__ float db1s[4 * FMAX];  // db1 of every wave
  __shared__ u16 mask[FF_ROWS];
  __shared__ u16 amask[FF_ROWS];  // channel D of a and of g: staged, never used
  u16* ximg = lds;             // x; then f16(u)
  u16* aimg = lds + IMG;       // a
  u16* dwh = lds + 2 * IMG;    // g; then dw hi; then dv hi
  u16* dwl = lds + 3 * IMG;    // dw lo; then dv lo
  u16* hch = lds + 4 * IMG;    // the chunk's f16(h)
  u16* dzh = hch + CIMG;
  u16* dzl = dzh + CIMG;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4, row0 = wave * 16;
  const int NC = F / 32;
  constexpr int oWo = 0, obo = D * D, oW1 = obo + 3 * D;
  const int ob1 = oW1 + F * D, oW2 = ob1 + F, ob2 = oW2 + D * F, NP = ob2 + 3 * D;
  float* p = part + (int64_t)blockIdx.x * NP;
  // dWo and the D-wide column sums stay in registers across the block's
  // tiles; the dW2 and dW1 tiles of every chunk are added into the block's own
  // partial tile by tile (each element has one owner lane), db1 into LDS
  f4 dWoa[TO];
  float dboa[NT], dg1a[NT], dbe1a[NT], db2a[NT], dg2a[NT], dbe2a[NT];
  for (int i = lane; i < FMAX; i += 64) db1s[wave * FMAX + i] = 0.0f;
#pragma unroll
  for (int i = 0; i < TO; ++i) dWoa[i] = ff_zero4();
#pragma unroll
  for (int n = 0; n < NT; ++n)
    dboa[n] = dg1a[n] = dbe1a[n] = db2a[n] = dg2a[n] = dbe2a[n] = 0.0f;
  const int64_t total = R * (D + 1), ntiles = (R + FF_ROWS - 1) / FF_ROWS;
  const int64_t ts = (int64_t)blockIdx.x * ntiles / gridDim.x;
  const int64_t te = ((int64_t)blockIdx.x + 1) * ntiles / gridDim.x;
  for (int64_t t = ts; t < te; ++t) {
    const int64_t rb = t * FF_ROWS;
    const int nrows = (int)(R - rb < FF_ROWS ? R - rb : FF_ROWS);
    // weight fragments held across the tiles would cost registers the D = 64
    // instance does not have
    const u16 *Wo = ff_opaque(Wo_), *WoT = ff_opaque(WoT_), *W1 = ff_opaque(W1_);
    const u16 *W1T = ff_opaque(W1T_), *W2 = ff_opaque(W2_), *W2T = ff_opaque(W2T_);
    const float* b1 = ff_opaque(b1_);
    ff_sync();  // the last tile's readers are done
    ff_stage<D>(x, total, rb * (D + 1), nrows, ximg, mask);
    ff_stage<D>(a, total, rb * (D + 1), nrows, aimg, amask);
    ff_stage<D>(g, total, rb * (D + 1), nrows, dwh, amask);
    ff_sync();
    ff_fix<D>(ximg, mask, nrows, true, wave, lane);
    ff_fix<D>(aimg, mask, nrows, false, wave, lane);
    ff_fix<D>(dwh, mask, nrows, false, wave, lane);
    ff_wave_sync();
    bool ok[4];
    const bool live = ff_strip_ok(mask, row0, fg, ok);
    f4 xh1[NT], dw[NT];
    h8 uf[KD];
    float r1[4];
#pragma unroll
    for (int n = 0; n < NT; ++n) xh1[n] = dw[n] = ff_zero4();
    if (live) {
      // the forward again, then LN2 backward: dw
      f4 u[NT], xh2[NT];
      float r2[4];
      ff_forward_strip<D>(ximg, aimg, ximg, hch, row0, ok, Wo, W1, W2, bo, g1,
                          be1, b1, b2, F, eps, lane, xh1, r1, u, uf, xh2);
      ff_ln<NT>(xh2, eps, lane, r2);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const float gg = g2[n * 16 + fi];
        f4 gy;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gy[r] = ok[r] ? ff_h2f(dwh[(row0 + fg * 4 + r) * XP + n * 16 + fi])
                        : 0.0f;
          dw[n][r] = gy[r] * gg;
        }
        dg2a[n] += ff_colsum(gy * xh2[n], lane);
        dbe2a[n] += ff_colsum(gy, lane);
      }
      ff_ln_bwd<NT>(dw, xh2, r2, lane);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dw[n][r] = ok[r] ? dw[n][r] : 0.0f;
        db2a[n] += ff_colsum(dw[n], lane);
      }
    } else {  // the strip's rows of x, a and g are zeros; so are these
      for (int i = lane; i < 16 * FF_HP / 8; i += 64) {
        const int o = row0 * FF_HP + i * 8;
        *(u4*)&hch[o] = u4{0, 0, 0, 0};
        *(u4*)&dzh[o] = u4{0, 0, 0, 0};
        *(u4*)&dzl[o] = u4{0, 0, 0, 0};
      }
    }
    ff_wave_sync();  // the strip's reads of g
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = (row0 + fg * 4 + r) * XP + n * 16 + fi;
        ff_split(dw[n][r], dwh[o], dwl[o]);
      }
    }
    ff_wave_sync();
    h8 dwfh[KD], dwfl[KD];
#pragma unroll
    for (int ks = 0; ks < KD; ++ks) {
      dwfh[ks] = ff_ld8(&dwh[(row0 + fi) * XP + ks * 32 + fg * 8]);
      dwfl[ks] = ff_ld8(&dwl[(row0 + fi) * XP + ks * 32 + fg * 8]);
    }
    f4 duh[NT], dul[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) duh[n] = dul[n] = ff_zero4();
#pragma unroll 1
    for (int c = 0; c < NC; ++c) {
      if (live) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int tt = c * 2 + j;
          const f4 z = ff_hidden<KD>(uf, W1, tt, lane);
          const f4 ch = ff_hidden<KD>(dwfh, W2T, tt, lane);
          const f4 cl = ff_hidden<KD>(dwfl, W2T, tt, lane);
          const float bb = b1[tt * 16 + fi];
          f4 dz;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float zz = z[r] + bb;
            const bool on = ok[r] && zz > 0.0f;
            dz[r] = on ? fmaf(cl[r], FF_LO_INV, ch[r]) : 0.0f;
            const int o = (row0 + fg * 4 + r) * FF_HP + j * 16 + fi;
            hch[o] = on ? ff_f2h(zz) : (u16)0;
            ff_split(dz[r], dzh[o], dzl[o]);
          }
          const float s1 = ff_colsum(dz, lane);
          if (fg == 0) db1s[wave * FMAX + tt * 16 + fi] += s1;
        }
      }
      ff_sync();  // every strip's f16(h) and dz of the chunk
      if (live) {
        const h8 zh = ff_ld8(&dzh[(row0 + fi) * FF_HP + fg * 8]);
        const h8 zl = ff_ld8(&dzl[(row0 + fi) * FF_HP + fg * 8]);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const h8 bw = ff_ld8(&W1T[(n * 16 + fi) * F + c * 32 + fg * 8]);
          duh[n] = ff_mfma(zh, bw, duh[n]);
          dul[n] = ff_mfma(zl, bw, dul[n]);
        }
      }
#pragma unroll
      for (int i = 0; i < TW; ++i) {
        const int ti = wave + 4 * i, dn = ti >> 1, j = ti & 1;
        f4 c2h = ff_zero4(), c2l = c2h, c1h = c2h, c1l = c2h;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const h8 bh = ff_tr(hch, FF_HP, ks * 32, j * 16, lane);
          c2h = ff_mfma(ff_tr(dwh, XP, ks * 32, dn * 16, lane), bh, c2h);
          c2l = ff_mfma(ff_tr(dwl, XP, ks * 32, dn * 16, lane), bh, c2l);
          const h8 bu = ff_tr(ximg, XP, ks * 32, dn * 16, lane);
          c1h = ff_mfma(ff_tr(dzh, FF_HP, ks * 32, j * 16, lane), bu, c1h);
          c1l = ff_mfma(ff_tr(dzl, FF_HP, ks * 32, j * 16, lane), bu, c1l);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v2 = fmaf(c2l[r], FF_LO_INV, c2h[r]);
          const float v1 = fmaf(c1l[r], FF_LO_INV, c1h[r]);
          float* q2 = p + oW2 + (dn * 16 + fg * 4 + r) * F + c * 32 + j * 16 + fi;
          float* q1 = p + oW1 + (c * 32 + j * 16 + fg * 4 + r) * D + dn * 16 + fi;
          *q2 = t == ts ? v2 : *q2 + v2;
          *q1 = t == ts ? v1 : *q1 + v1;
        }
      }
      ff_sync();  // before the next chunk (or dv) overwrites the images
    }
    // LN1 backward: dv over the dead dw images
    f4 dv[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) dv[n] = ff_zero4();
    if (live) {
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const float gg = g1[n * 16 + fi];
        f4 du;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          du[r] = dw[n][r] + fmaf(dul[n][r], FF_LO_INV, duh[n][r]);
          dv[n][r] = du[r] * gg;
        }
        dg1a[n] += ff_colsum(du * xh1[n], lane);
        dbe1a[n] += ff_colsum(du, lane);
      }
      ff_ln_bwd<NT>(dv, xh1, r1, lane);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dv[n][r] = ok[r] ? dv[n][r] : 0.0f;
        dboa[n] += ff_colsum(dv[n], lane);
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = (row0 + fg * 4 + r) * XP + n * 16 + fi;
          ff_split(dv[n][r], dwh[o], dwl[o]);
        }
      }
    }
    ff_wave_sync();
    f4 dah[NT], dal[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) dah[n] = dal[n] = ff_zero4();
    if (live) {
      ff_gemm_dd<D>(dwh, row0, WoT, lane, dah);
      ff_gemm_dd<D>(dwl, row0, WoT, lane, dal);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + fg * 4 + r;
      if (row < nrows) {
        u16* px = dx + (rb + row) * (D + 1);
        u16* pa = da + (rb + row) * (D + 1);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          px[n * 16 + fi] = ok[r] ? ff_f2h(dv[n][r]) : (u16)0;
          pa[n * 16 + fi] =
              ok[r] ? ff_f2h(fmaf(dal[n][r], FF_LO_INV, dah[n][r])) : (u16)0;
        }
        if (fi == 0) px[D] = pa[D] = 0;
      }
    }
    ff_sync();  // every strip's dv
#pragma unroll
    for (int i = 0; i < TO; ++i) {
      const int ti = wave + 4 * i, dm = ti / NT, dn = ti % NT;
      f4 ch = ff_zero4(), cl = ch;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const h8 ba = ff_tr(aimg, XP, ks * 32, dn * 16, lane);
        ch = ff_mfma(ff_tr(dwh, XP, ks * 32, dm * 16, lane), ba, ch);
        cl = ff_mfma(ff_tr(dwl, XP, ks * 32, dm * 16, lane), ba, cl);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) dWoa[i][r] += fmaf(cl[r], FF_LO_INV, ch[r]);
    }
  }
  // the block's partial
#pragma unroll
  for (int i = 0; i < TO; ++i) {
    const int ti = wave + 4 * i, dm = ti / NT, dn = ti % NT;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      p[oWo + (dm * 16 + fg * 4 + r) * D + dn * 16 + fi] = dWoa[i][r];
  }
  // column sums: [dbo | dg1 | dbe1 | db2 | dg2 | dbe2] of every wave, summed
  // in wave order, and db1 alike
  constexpr int VN = 6 * D;
  ff_sync();  // the images are dead
  float* red = (float*)lds + wave * VN;
  if (fg == 0) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int d = n * 16 + fi;
      red[d] = dboa[n];
      red[D + d] = dg1a[n];
      red[2 * D + d] = dbe1a[n];
      red[3 * D + d] = db2a[n];
      red[4 * D + d] = dg2a[n];
      red[5 * D + d] = dbe2a[n];
    }
  }
  ff_sync();
  const float* rd = (const float*)lds;
  for (int i = threadIdx.x; i < VN; i += 256) {
    const float v = ((rd[i] + rd[VN + i]) + rd[2 * VN + i]) + rd[3 * VN + i];
    p[i < 3 * D ? obo + i : ob2 + (i - 3 * D)] = v;
  }
  for (int i = threadIdx.x; i < F; i += 256)
    p[ob1 + i] = ((db1s[i] + db1s[FMAX + i]) + db1s[2 * FMAX + i]) +
                 db1s[3 * FMAX + i];
}

// out[i] = sum over the blocks' partials, in block order
__global__ __launch_bounds__(256) void ff_reduce_kernel(
    const float* __restrict__ part, float* __restrict__ out, int nblk, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float acc = 0.0f;
  for (int k = 0; k < nblk; ++k) acc += part[(int64_t)k * n + i];
  out[i] = acc;
}

bool ff_feasible(int64_t D, int64_t F) {
  return (D == 32 || D == 64) && F % 32 == 0 && F >= 32 && F <= 256;
}

hipStream_t ff_stream() { return at::hip::getCurrentHIPStream().stream(); }

bool ff_is(const torch::Tensor& t, const torch::Tensor& like,
           c10::ScalarType st) {
  return t.is_cuda() && t.device() == like.device() && t.scalar_type() == st &&
         t.is_contiguous();
}

struct FfArgs {
  torch::Tensor x, a, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2;
};

// -> the grid for `per_cu` blocks per CU; raises on anything the kernels do
// not take
int ff_check(const FfArgs& p, int64_t max_blocks, int per_cu, const char* who) {
  const auto& x = p.x;
  TORCH_CHECK(x.is_cuda(), who, ": x must be on a GPU");
  TORCH_CHECK(ff_is(x, x, torch::kFloat16) && ff_is(p.a, x, torch::kFloat16),
              who, ": x and a must be contiguous float16 on one GPU");
  TORCH_CHECK(x.dim() == 3 && x.size(2) >= 2 && p.a.sizes() == x.sizes(), who,
              ": expected x and a [B, L, D+1]");
  const int64_t D = x.size(2) - 1;
  for (const auto* w : {&p.Wo, &p.W1, &p.W2}) {
    TORCH_CHECK(ff_is(*w, x, torch::kFloat16) && w->dim() == 2, who,
                ": Wo, W1, W2 must be contiguous float16 matrices beside x");
    TORCH_CHECK(((uintptr_t)w->data_ptr() & 15) == 0, who,
                ": the matrices must start on 16 bytes");
  }
  const int64_t F = p.W1.size(0);
  TORCH_CHECK(p.Wo.size(0) == D && p.Wo.size(1) == D && p.W1.size(1) == D &&
                  p.W2.size(0) == D && p.W2.size(1) == F,
              who, ": expected Wo [D, D], W1 [F, D], W2 [D, F]");
  for (const auto* v : {&p.bo, &p.g1, &p.be1, &p.b2, &p.g2, &p.be2, &p.b1}) {
    TORCH_CHECK(ff_is(*v, x, torch::kFloat32) && v->dim() == 1 &&
                    v->size(0) == (v == &p.b1 ? F : D),
                who, ": biases and LayerNorm parameters must be contiguous "
                "float32 [D] (b1 [F]) beside x");
  }
  TORCH_CHECK(ff_feasible(D, F), who, ": no kernel for D=", D, " F=", F,
              " (seq_ffn_feasible)");
  TORCH_CHECK(max_blocks >= 0, who, ": max_blocks must be >= 0");
  const int64_t R = x.size(0) * x.size(1);
  const int64_t ntiles = (R + FF_ROWS - 1) / FF_ROWS;
  int64_t grid =
      max_blocks > 0
          ? max_blocks
          : per_cu * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  grid = grid < ntiles ? grid : ntiles;
  return (int)grid;
}

#define FF_P16(t) (const u16*)(t).data_ptr()
#define FF_P32(t) (const float*)(t).data_ptr()

template <int D>
void ff_launch_fwd(int grid, const FfArgs& p, torch::Tensor& out, float eps) {
  hipLaunchKernelGGL((seq_ffn_fwd_kernel<D>), dim3(grid), dim3(256), 0,
                     ff_stream(), FF_P16(p.x), FF_P16(p.a), FF_P16(p.Wo),
                     FF_P16(p.W1), FF_P16(p.W2), FF_P32(p.bo), FF_P32(p.g1),
                     FF_P32(p.be1), FF_P32(p.b1), FF_P32(p.b2), FF_P32(p.g2),
                     FF_P32(p.be2), (u16*)out.data_ptr(),
                     p.x.size(0) * p.x.size(1), (int)p.W1.size(0), eps);
}

template <int D>
void ff_launch_bwd(int grid, const torch::Tensor& g, const FfArgs& p,
                   const torch::Tensor& WoT, const torch::Tensor& W1T,
                   const torch::Tensor& W2T, torch::Tensor& dx,
                   torch::Tensor& da, torch::Tensor& part, float eps) {
  hipLaunchKernelGGL((seq_ffn_bwd_kernel<D>), dim3(grid), dim3(256), 0,
                     ff_stream(), FF_P16(g), FF_P16(p.x), FF_P16(p.a),
                     FF_P16(p.Wo), FF_P16(WoT), FF_P16(p.W1), FF_P16(W1T),
                     FF_P16(p.W2), FF_P16(W2T), FF_P32(p.bo), FF_P32(p.g1),
                     FF_P32(p.be1), FF_P32(p.b1), FF_P32(p.b2), FF_P32(p.g2),
                     (u16*)dx.data_ptr(), (u16*)da.data_ptr(),
                     (float*)part.data_ptr(), p.x.size(0) * p.x.size(1),
                     (int)p.W1.size(0), eps);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool seq_ffn_feasible(int64_t D, int64_t F) { return ff_feasible(D, F); }

torch::Tensor seq_ffn_fwd(torch::Tensor x, torch::Tensor a, torch::Tensor Wo,
                          torch::Tensor bo, torch::Tensor g1, torch::Tensor be1,
                          torch::Tensor W1, torch::Tensor b1, torch::Tensor W2,
                          torch::Tensor b2, torch::Tensor g2, torch::Tensor be2,
                          double eps, int64_t max_blocks) {
  const FfArgs p{x, a, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2};
  const int grid = ff_check(p, max_blocks, 2, "seq_ffn_fwd");
  auto out = torch::empty_like(x);
  if (grid == 0) return out;
  if (x.size(2) - 1 == 32) ff_launch_fwd<32>(grid, p, out, (float)eps);
  else ff_launch_fwd<64>(grid, p, out, (float)eps);
  return out;
}

// -> (dx, da, dWo, dbo, dg1, dbe1, dW1, db1, dW2, db2, dg2, dbe2)
std::vector<torch::Tensor> seq_ffn_bwd(
    torch::Tensor g, torch::Tensor x, torch::Tensor a, torch::Tensor Wo,
    torch::Tensor bo, torch::Tensor g1, torch::Tensor be1, torch::Tensor W1,
    torch::Tensor b1, torch::Tensor W2, torch::Tensor b2, torch::Tensor g2,
    torch::Tensor be2, double eps, int64_t max_blocks) {
  const FfArgs p{x, a, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2};
  const int grid = ff_check(p, max_blocks, 1, "seq_ffn_bwd");
  TORCH_CHECK(ff_is(g, x, torch::kFloat16) && g.sizes() == x.sizes(),
              "seq_ffn_bwd: g must be a contiguous float16 [B, L, D+1] beside x");
  const int64_t D = x.size(2) - 1, F = W1.size(0);
  const int64_t n = D * D + 2 * F * D + F + 6 * D;
  auto dx = torch::empty_like(x), da = torch::empty_like(x);
  auto sums = torch::zeros({n}, bo.options());
  if (grid > 0) {
    auto part = torch::empty({(int64_t)grid, n}, bo.options());
    const auto WoT = Wo.t().contiguous(), W1T = W1.t().contiguous(),
               W2T = W2.t().contiguous();
    if (D == 32)
      ff_launch_bwd<32>(grid, g, p, WoT, W1T, W2T, dx, da, part, (float)eps);
    else
      ff_launch_bwd<64>(grid, g, p, WoT, W1T, W2T, dx, da, part, (float)eps);
    hipLaunchKernelGGL(ff_reduce_kernel, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, ff_stream(), (const float*)part.data_ptr(),
                       (float*)sums.data_ptr(), grid, (int)n);
  }
  std::vector<torch::Tensor> out{dx, da};
  int64_t o = 0;
  auto take = [&](int64_t rows, int64_t cols) {
    auto t = sums.narrow(0, o, rows * cols);
    o += rows * cols;
    out.push_back(cols > 1 ? t.view({rows, cols}) : t);
  };
  take(D, D); take(D, 1); take(D, 1); take(D, 1);  // dWo dbo dg1 dbe1
  take(F, D); take(F, 1);                          // dW1 db1
  take(D, F); take(D, 1); take(D, 1); take(D, 1);  // dW2 db2 dg2 dbe2
  return out;
}

void init_seqffn(pybind11::module_& m) {
  namespace py = pybind11;
  m.def("seq_ffn_feasible", &seq_ffn_feasible,
        "true if the transformer-tail kernels take (D, F)");
  m.def("seq_ffn_fwd", &seq_ffn_fwd,
        "out-projection, add & LayerNorm, feed-forward, add & LayerNorm over "
        "the rows of a raw slot -> out [B, L, D+1]",
        py::arg("x"), py::arg("a"), py::arg("Wo"), py::arg("bo"), py::arg("g1"),
        py::arg("be1"), py::arg("W1"), py::arg("b1"), py::arg("W2"),
        py::arg("b2"), py::arg("g2"), py::arg("be2"), py::arg("eps") = 1e-5,
        py::arg("max_blocks") = 0);
  m.def("seq_ffn_bwd", &seq_ffn_bwd,
        "seq_ffn backward -> (dx, da, dWo, dbo, dg1, dbe1, dW1, db1, dW2, db2, "
        "dg2, dbe2)",
        py::arg("g"), py::arg("x"), py::arg("a"), py::arg("Wo"), py::arg("bo"),
        py::arg("g1"), py::arg("be1"), py::arg("W1"), py::arg("b1"),
        py::arg("W2"), py::arg("b2"), py::arg("g2"), py::arg("be2"),
        py::arg("eps") = 1e-5, py::arg("max_blocks") = 0);
}
