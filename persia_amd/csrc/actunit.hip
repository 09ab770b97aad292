// DIN activation-unit (MLP attention) pooling over a raw slot (gfx950).
//
//   seq [B, L, D+1] f16: channels 0..D-1 the row k_l, channel D the 0/1 mask
//   q   [B, D]      f16: the query
//   u   [B, H]      f32: (Wq+Wd) q_b + b1            (torch, outside)
//   Wb, Wp [H, D]   f16: f16(Wk-Wd), f16(Wp);  w2 [H] f32;  b2 [] f32
//   M_b = f16(Wb + Wp * q_b)   (f32 arithmetic, one rounding)
//   h_l = u_b + M_b k_l;  a_l = sigmoid(h_l);  w_l = <w2, a_l> + b2
//   out = sum_{valid l} w_l * k_l                              -> f16 [B, D]
// backward (h, a, w are RECOMPUTED, nothing but the inputs is saved):
//   dw_l = <g, k_l>;  dh_l = dw_l * w2 * a_l (1 - a_l)   (valid l, else 0)
//   du_b = sum_l dh_l;  dw2 += sum_l dw_l a_l;  db2 += sum_l dw_l
//   dk_l = w_l g + M_b^T dh_l;  dM_b = dh^T K
//   dWb += dM_b;  dWp += dM_b * q_b;  dq_k[d] = sum_h dM_b[h,d] Wp[h,d]
//
// Why matrix instructions fit here and not in seqattn.hip: the first layer's
// weights are shared by every (b, l), so h = K M_b^T is a GEMM over the rows
// of the sequence with a full 16-column tile per 16 hidden units, and so are
// both gradients (dk = dh M_b, dM = dh^T K).
//
// Work split: a persistent grid of 4-wave blocks; block i walks the samples
// [i*B/G, (i+1)*B/G).  A sample's rows stream through LDS in tiles of 64, one
// 16-row strip per wave, so LDS holds one tile, the M_b image and one dh
// tile whatever L is.  There is no softmax, hence no pass over the sample
// before the first product: one read of seq per direction.
//
// Staging.  A row has D+1 halves, so nothing in seq is vector-aligned.  The
// tile's halves are contiguous in memory; the block reads them as aligned
// 32-bit words (boundary words, and words across the tensor's own ends, half
// by half from the part inside) and scatters the halves into an image of
// pitch D+8 halves, mask column into its own array.  Then each wave zeroes
// the invalid rows and the tail of its strip: the mask SELECTS, an Inf or NaN
// in an invalid row never enters a product -- with MFMA that is what keeps
// 0 * NaN out of dM = dh^T K.
//
// Fragments (mfma_f32_16x16x32_f16, maps in dense.hip): row operands (K rows
// for h, M_b rows for h, dh rows for dk) are 8 contiguous halves of an image
// row; operands whose reduction index runs down the rows of a LINEAR image
// (M_b for dk; dh and K for dM) come from ds_read_b64_tr_b16, addressed as in
// interact.hip.  The epilogues stay in the accumulator layout (lane = column
// fi, rows 4*fg .. 4*fg+3).
//
// Precision.  Products of f16 operands are exact in the MFMA's f32
// accumulator, so h is an f32 sum of exact products.  dh is an f32 value and
// is staged as TWO f16 images, hi = f16(dh) and lo = f16((dh - hi) * 2^11):
// dh = hi + lo * 2^-11 to about 2^-23 relative, and every gradient product
// runs once per image into accumulators of its own.  du, dw2 and db2 use the
// f32 dh and dw in registers.
//
// Order.  Every sum has a fixed order that depends on the sample alone (rows
// in strip order, waves 0..3), so the per-sample results do not depend on B,
// on the sample's place in the batch or on the grid.  The weight gradients
// are accumulated in registers over a block's samples, written as one
// partial per block and summed in block order by au_reduce_kernel: no
// atomics, same bits run to run for one grid.
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

constexpr int AU_ROWS = 64;        // rows of seq per tile: 4 waves x 16
constexpr float AU_LO = 2048.0f;   // scale of the low dh image
constexpr float AU_LO_INV = 1.0f / 2048.0f;

// Builtins only inside the kernels: the functions of the HIP headers carry
// the default target features and would not be inlined into functions that
// switch the packed-f32 forms off.
__device__ __forceinline__ float au_h2f(u16 x) {
  return (float)__builtin_bit_cast(_Float16, x);
}

__device__ __forceinline__ u16 au_f2h(float f) {  // round to nearest even
  return __builtin_bit_cast(u16, (_Float16)f);
}

__device__ __forceinline__ void au_sync() {  // what __syncthreads() does
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float au_shfl(float v, int src_lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src_lane << 2,
                                          __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ bool au_valid(u16 mask) {  // != 0, -0 is zero
  return (mask & 0x7fff) != 0;
}

// Rows [row0, row0 + nrows) of seq (pitch D+1) -> img (pitch D+8), their mask
// halves -> mask.  s = index in seq of the first half, total = seq.numel().
template <int D>
__device__ __forceinline__ void au_stage(const u16* __restrict__ seq,
                                         int64_t total, int64_t s, int nrows,
                                         u16* img, u16* mask) {
  constexpr int W = D + 1, KP = D + 8;
  const uintptr_t t0 = (uintptr_t)seq, t1 = t0 + 2 * (uintptr_t)total;
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
          if (col < D) img[row * KP + col] = x;
          else mask[row] = x;
        }
      }
    }
  }
}

// The wave's strip: rows past nrows get mask 0; they and the invalid rows
// become zeros in the image.
template <int D>
__device__ __forceinline__ void au_fix(u16* img, u16* mask, int nrows,
                                       int wave, int lane) {
  constexpr int KP = D + 8;
  const int row = wave * 16 + (lane >> 2), part = lane & 3;
  const bool tail = row >= nrows;
  const bool bad = tail || !au_valid(mask[row]);
  if (bad) {
    for (int c = part; c < D / 8; c += 4)
      *(u4*)&img[row * KP + c * 8] = u4{0, 0, 0, 0};
  }
  if (tail && part == 0) mask[row] = 0;
}

// M_b image: rows hh < H of pitch D+8, f16(Wb + Wp * q) with one rounding
// (the product of two f16 values is exact in f32).
template <int H, int D>
__device__ __forceinline__ void au_build_m(const u16* __restrict__ Wb,
                                           const u16* __restrict__ Wp,
                                           const float* qf, u16* mimg) {
  constexpr int KP = D + 8, C = D / 8;
  for (int idx = threadIdx.x; idx < H * C; idx += 256) {
    const int hh = idx / C, c8 = (idx % C) * 8;
    const h8 vb = *(const h8*)&Wb[hh * D + c8];
    const h8 vp = *(const h8*)&Wp[hh * D + c8];
    h8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      o[k] = (_Float16)fmaf((float)vp[k], qf[c8 + k], (float)vb[k]);
    *(h8*)&mimg[hh * KP + c8] = o;
  }
}

// 8 halves img[kb + 8*fg + j][cb + fi], j = 0..7: the fragment of an operand
// whose reduction index runs down the rows of a linear image.  Lane m of a
// 16-lane group addresses the slot (row + m/4, 4*(m%4)); the group's slots
// form a 4 x 16 block and lane m receives its column m.
__device__ __forceinline__ h8 au_tr(const u16* img, int pitch, int kb, int cb,
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

// h of the wave's strip -> a[ht][r] (row 4*fg + r, hidden unit 16*ht + fi),
// w[r] the same in every lane of the group; afr keeps the K fragments.
template <int HT, int DT>
__device__ __forceinline__ void au_strip(const u16* kimg, const u16* mimg,
                                         int wave, int lane,
                                         const float (&ur)[HT],
                                         const float (&w2r)[HT], float b2v,
                                         h8 (&afr)[DT / 2], float (&a)[HT][4],
                                         float (&w)[4]) {
  constexpr int KP = DT * 16 + 8;
  const int fi = lane & 15, fg = lane >> 4;
  f4 acc[HT];
#pragma unroll
  for (int ht = 0; ht < HT; ++ht) acc[ht] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int ks = 0; ks < DT / 2; ++ks) {
    afr[ks] = *(const h8*)&kimg[(wave * 16 + fi) * KP + ks * 32 + fg * 8];
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) {
      const h8 bfr = *(const h8*)&mimg[(ht * 16 + fi) * KP + ks * 32 + fg * 8];
      acc[ht] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afr[ks], bfr, acc[ht],
                                                       0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) w[r] = 0.0f;
#pragma unroll
  for (int ht = 0; ht < HT; ++ht) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float hv = acc[ht][r] + ur[ht];
      a[ht][r] = 1.0f / (1.0f + __expf(-hv));
      w[r] = fmaf(w2r[ht], a[ht][r], w[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) w[r] += au_shfl(w[r], lane ^ off);
    w[r] += b2v;
  }
}

template <int HT, int DT>
__global__ __launch_bounds__(256) void act_unit_fwd_kernel(
    const u16* __restrict__ q, const u16* __restrict__ seq,
    const float* __restrict__ u, const u16* __restrict__ Wb,
    const u16* __restrict__ Wp, const float* __restrict__ w2,
    const float* __restrict__ b2, u16* __restrict__ out, int B, int L) {
  constexpr int H = HT * 16, D = DT * 16, KP = D + 8, NO = (D + 63) / 64;
  __shared__ __align__(16) u16 kimg[AU_ROWS * KP];
  __shared__ __align__(16) u16 mimg[H * KP];
  __shared__ u16 mask[AU_ROWS];
  __shared__ float qf[D];
  __shared__ float wrow[AU_ROWS];
  __shared__ float red[4 * D];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4;
  float w2r[HT], ur[HT];
#pragma unroll
  for (int ht = 0; ht < HT; ++ht) w2r[ht] = w2[ht * 16 + fi];
  const float b2v = *b2;
  const int64_t total = (int64_t)B * L * (D + 1);
  const int64_t bs = (int64_t)blockIdx.x * B / gridDim.x;
  const int64_t be = ((int64_t)blockIdx.x + 1) * B / gridDim.x;
  for (int64_t b = bs; b < be; ++b) {
    au_sync();  // the last sample's readers of qf, mimg, red are done
    for (int d = threadIdx.x; d < D; d += 256) qf[d] = au_h2f(q[b * D + d]);
    au_sync();
    au_build_m<H, D>(Wb, Wp, qf, mimg);
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) ur[ht] = u[b * H + ht * 16 + fi];
    float oacc[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) oacc[j] = 0.0f;
    for (int l0 = 0; l0 < L; l0 += AU_ROWS) {
      const int nrows = L - l0 < AU_ROWS ? L - l0 : AU_ROWS;
      au_sync();  // the last tile's readers are done; mimg is written
      au_stage<D>(seq, total, (b * L + l0) * (D + 1), nrows, kimg, mask);
      au_sync();
      au_fix<D>(kimg, mask, nrows, wave, lane);
      au_sync();
      if (wave * 16 < nrows) {
        h8 afr[DT / 2];
        float a[HT][4], w[4];
        au_strip<HT, DT>(kimg, mimg, wave, lane, ur, w2r, b2v, afr, a, w);
        if (fi == 0) {
#pragma unroll
          for (int r = 0; r < 4; ++r) wrow[wave * 16 + fg * 4 + r] = w[r];
        }
      }
      au_sync();
      // out: a lane owns columns lane, lane + 64 and walks its strip's rows
      if (wave * 16 < nrows) {
#pragma unroll
        for (int j = 0; j < NO; ++j) {
          const int d = lane + 64 * j;
          if (d < D) {
            for (int r = 0; r < 16; ++r) {
              const int row = wave * 16 + r;
              if (au_valid(mask[row]))
                oacc[j] = fmaf(wrow[row], au_h2f(kimg[row * KP + d]), oacc[j]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NO; ++j)
      if (lane + 64 * j < D) red[wave * D + lane + 64 * j] = oacc[j];
    au_sync();
    for (int d = threadIdx.x; d < D; d += 256)
      out[b * D + d] =
          au_f2h(((red[d] + red[D + d]) + red[2 * D + d]) + red[3 * D + d]);
  }
}

// Partials of one block, f32: [dWb H*D][dWp H*D][dw2 H][db2 1].
template <int HT, int DT>
__global__ __launch_bounds__(256) void act_unit_bwd_kernel(
    const u16* __restrict__ g, const u16* __restrict__ q,
    const u16* __restrict__ seq, const float* __restrict__ u,
    const u16* __restrict__ Wb, const u16* __restrict__ Wp,
    const float* __restrict__ w2, const float* __restrict__ b2,
    u16* __restrict__ dq, u16* __restrict__ dseq, float* __restrict__ du,
    float* __restrict__ part, int B, int L) {
  constexpr int H = HT * 16, D = DT * 16, KP = D + 8;
  constexpr int HK = (HT + 1) / 2;   // 32-wide steps over the hidden units
  constexpr int HP = HK * 32 + 8;    // pitch of the dh images
  constexpr int NDT = (DT + 3) / 4;  // dM column tiles of a wave
  constexpr int RW = D > H ? D : H;
  __shared__ __align__(16) u16 kimg[AU_ROWS * KP];
  __shared__ __align__(16) u16 mimg[HK * 32 * KP];
  __shared__ __align__(16) u16 dhh[AU_ROWS * HP];
  __shared__ __align__(16) u16 dhl[AU_ROWS * HP];
  __shared__ u16 mask[AU_ROWS];
  __shared__ float qf[D];
  __shared__ float gf[D];
  __shared__ float red[4 * RW];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4;
  // rows H.. of mimg and columns H.. of the dh images are the zero padding
  // of the 32-wide step; nothing below writes them
  for (int i = threadIdx.x; i < HK * 32 * KP / 8; i += 256)
    *(u4*)&mimg[i * 8] = u4{0, 0, 0, 0};
  for (int i = threadIdx.x; i < AU_ROWS * HP / 8; i += 256) {
    *(u4*)&dhh[i * 8] = u4{0, 0, 0, 0};
    *(u4*)&dhl[i * 8] = u4{0, 0, 0, 0};
  }
  float w2r[HT], ur[HT], dw2a[HT];
#pragma unroll
  for (int ht = 0; ht < HT; ++ht) {
    w2r[ht] = w2[ht * 16 + fi];
    dw2a[ht] = 0.0f;
  }
  const float b2v = *b2;
  float db2a = 0.0f;
  f4 dWb[NDT][HT], dWp[NDT][HT];
#pragma unroll
  for (int n = 0; n < NDT; ++n) {
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) {
      dWb[n][ht] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      dWp[n][ht] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
  }
  const int64_t total = (int64_t)B * L * (D + 1);
  const int64_t bs = (int64_t)blockIdx.x * B / gridDim.x;
  const int64_t be = ((int64_t)blockIdx.x + 1) * B / gridDim.x;
  for (int64_t b = bs; b < be; ++b) {
    au_sync();  // the last sample's readers of qf, gf, mimg, red
    for (int d = threadIdx.x; d < D; d += 256) {
      qf[d] = au_h2f(q[b * D + d]);
      gf[d] = au_h2f(g[b * D + d]);
    }
    au_sync();
    au_build_m<H, D>(Wb, Wp, qf, mimg);
    float dua[HT];
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) {
      ur[ht] = u[b * H + ht * 16 + fi];
      dua[ht] = 0.0f;
    }
    f4 dMh[NDT][HT], dMl[NDT][HT];
#pragma unroll
    for (int n = 0; n < NDT; ++n) {
#pragma unroll
      for (int ht = 0; ht < HT; ++ht) {
        dMh[n][ht] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        dMl[n][ht] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
    for (int l0 = 0; l0 < L; l0 += AU_ROWS) {
      const int nrows = L - l0 < AU_ROWS ? L - l0 : AU_ROWS;
      const bool active = wave * 16 < nrows;
      au_sync();  // the last tile's readers are done; mimg is written
      au_stage<D>(seq, total, (b * L + l0) * (D + 1), nrows, kimg, mask);
      au_sync();
      au_fix<D>(kimg, mask, nrows, wave, lane);
      au_sync();
      float w[4];
      bool ok[4];
      if (active) {
        h8 afr[DT / 2];
        float a[HT][4];
        au_strip<HT, DT>(kimg, mimg, wave, lane, ur, w2r, b2v, afr, a, w);
        // dw of row fi: this lane's slice of d, then over the four fg
        float dwp = 0.0f;
#pragma unroll
        for (int ks = 0; ks < DT / 2; ++ks) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            dwp = fmaf(gf[ks * 32 + fg * 8 + j], (float)afr[ks][j], dwp);
        }
        dwp += au_shfl(dwp, lane ^ 16);
        dwp += au_shfl(dwp, lane ^ 32);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wave * 16 + fg * 4 + r;
          const float dw = au_shfl(dwp, fg * 4 + r);  // lane = row in strip
          ok[r] = au_valid(mask[row]);
          if (ok[r]) db2a += dw;
#pragma unroll
          for (int ht = 0; ht < HT; ++ht) {
            const float av = a[ht][r];
            const float dh = ok[r] ? dw * w2r[ht] * (av * (1.0f - av)) : 0.0f;
            dua[ht] += dh;
            if (ok[r]) dw2a[ht] = fmaf(dw, av, dw2a[ht]);
            const _Float16 hi = (_Float16)dh;
            const _Float16 lo = (_Float16)((dh - (float)hi) * AU_LO);
            dhh[row * HP + ht * 16 + fi] = __builtin_bit_cast(u16, hi);
            dhl[row * HP + ht * 16 + fi] = __builtin_bit_cast(u16, lo);
          }
        }
      } else {  // no row of this tile: the strip's dh is zero for dM
        for (int i = lane; i < 16 * HP / 8; i += 64) {
          *(u4*)&dhh[wave * 16 * HP + i * 8] = u4{0, 0, 0, 0};
          *(u4*)&dhl[wave * 16 * HP + i * 8] = u4{0, 0, 0, 0};
        }
      }
      au_sync();
      // dk of the wave's strip: w_l g + dh_l M_b, straight to dseq
      if (active) {
        h8 ah[HK], al[HK];
#pragma unroll
        for (int kk = 0; kk < HK; ++kk) {
          const int o = (wave * 16 + fi) * HP + kk * 32 + fg * 8;
          ah[kk] = *(const h8*)&dhh[o];
          al[kk] = *(const h8*)&dhl[o];
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          f4 ch = f4{0.0f, 0.0f, 0.0f, 0.0f}, cl = ch;
#pragma unroll
          for (int kk = 0; kk < HK; ++kk) {
            const h8 bfr = au_tr(mimg, KP, kk * 32, dt * 16, lane);
            ch = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[kk], bfr, ch, 0, 0, 0);
            cl = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[kk], bfr, cl, 0, 0, 0);
          }
          const int d = dt * 16 + fi;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int l = l0 + wave * 16 + fg * 4 + r;
            if (l < L) {
              const float dk = fmaf(w[r], gf[d], fmaf(cl[r], AU_LO_INV, ch[r]));
              u16* row = dseq + (b * L + l) * (D + 1);
              row[d] = ok[r] ? au_f2h(dk) : (u16)0;
              if (dt == 0 && fi == 0) row[D] = 0;
            }
          }
        }
      }
      // dM += dh^T K over the tile's rows: the wave owns column tiles
      // wave, wave + 4 and all the hidden units
#pragma unroll
      for (int n = 0; n < NDT; ++n) {
        const int dt = wave + 4 * n;
        if (dt < DT) {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            if (ks * 32 < nrows) {
              const h8 bfr = au_tr(kimg, KP, ks * 32, dt * 16, lane);
#pragma unroll
              for (int ht = 0; ht < HT; ++ht) {
                const h8 fh = au_tr(dhh, HP, ks * 32, ht * 16, lane);
                const h8 fl = au_tr(dhl, HP, ks * 32, ht * 16, lane);
                dMh[n][ht] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                    fh, bfr, dMh[n][ht], 0, 0, 0);
                dMl[n][ht] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                    fl, bfr, dMl[n][ht], 0, 0, 0);
              }
            }
          }
        }
      }
    }
    // the sample's dM (row 16*ht + 4*fg + r, column 16*dt + fi) is complete
#pragma unroll
    for (int n = 0; n < NDT; ++n) {
      const int dt = wave + 4 * n;
      if (dt < DT) {
        const int d = dt * 16 + fi;
        const float qd = qf[d];
        float dqp = 0.0f;
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float dm = fmaf(dMl[n][ht][r], AU_LO_INV, dMh[n][ht][r]);
            dWb[n][ht][r] += dm;
            dWp[n][ht][r] = fmaf(dm, qd, dWp[n][ht][r]);
            const int hh = ht * 16 + fg * 4 + r;
            dqp = fmaf(dm, au_h2f(Wp[hh * D + d]), dqp);
          }
        }
        dqp += au_shfl(dqp, lane ^ 16);
        dqp += au_shfl(dqp, lane ^ 32);
        if (fg == 0) dq[b * D + d] = au_f2h(dqp);
      }
    }
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) {
      float v = dua[ht];
      v += au_shfl(v, lane ^ 16);
      v += au_shfl(v, lane ^ 32);
      if (fg == 0) red[wave * H + ht * 16 + fi] = v;
    }
    au_sync();
    if (threadIdx.x < H) {
      const int t = threadIdx.x;
      du[b * H + t] = ((red[t] + red[H + t]) + red[2 * H + t]) + red[3 * H + t];
    }
  }
  // the block's partial
  float* p = part + (int64_t)blockIdx.x * (2 * H * D + H + 1);
#pragma unroll
  for (int n = 0; n < NDT; ++n) {
    const int dt = wave + 4 * n;
    if (dt < DT) {
#pragma unroll
      for (int ht = 0; ht < HT; ++ht) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = (ht * 16 + fg * 4 + r) * D + dt * 16 + fi;
          p[o] = dWb[n][ht][r];
          p[H * D + o] = dWp[n][ht][r];
        }
      }
    }
  }
  au_sync();
#pragma unroll
  for (int ht = 0; ht < HT; ++ht) {
    float v = dw2a[ht];
    v += au_shfl(v, lane ^ 16);
    v += au_shfl(v, lane ^ 32);
    if (fg == 0) red[wave * H + ht * 16 + fi] = v;
  }
  au_sync();
  if (threadIdx.x < H) {
    const int t = threadIdx.x;
    p[2 * H * D + t] =
        ((red[t] + red[H + t]) + red[2 * H + t]) + red[3 * H + t];
  }
  au_sync();
  // db2a is the same in the 16 lanes of a group; lane 0 sums the four groups
  db2a += au_shfl(db2a, lane ^ 16);
  db2a += au_shfl(db2a, lane ^ 32);
  if (lane == 0) red[wave] = db2a;
  au_sync();
  if (threadIdx.x == 0)
    p[2 * H * D + H] = ((red[0] + red[1]) + red[2]) + red[3];
}

// out[i] = sum over the blocks' partials, in block order
__global__ __launch_bounds__(256) void au_reduce_kernel(
    const float* __restrict__ part, float* __restrict__ out, int nblk, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float acc = 0.0f;
  for (int k = 0; k < nblk; ++k) acc += part[(int64_t)k * n + i];
  out[i] = acc;
}

bool au_feasible(int64_t L, int64_t D, int64_t H) {
  return D % 32 == 0 && D >= 32 && D <= 128 && H % 16 == 0 && H >= 16 &&
         H <= 64 && L >= 1 && L <= 1024;
}

hipStream_t au_stream() { return at::hip::getCurrentHIPStream().stream(); }

bool au_is(const torch::Tensor& t, const torch::Tensor& like,
           c10::ScalarType st) {
  return t.is_cuda() && t.device() == like.device() && t.scalar_type() == st &&
         t.is_contiguous();
}

// -> the grid; raises on anything the kernels do not take
int au_check(const torch::Tensor& q, const torch::Tensor& seq,
             const torch::Tensor& u, const torch::Tensor& Wb,
             const torch::Tensor& Wp, const torch::Tensor& w2,
             const torch::Tensor& b2, int64_t max_blocks, const char* who) {
  TORCH_CHECK(q.is_cuda(), who, ": q must be on a GPU");
  TORCH_CHECK(au_is(q, q, torch::kFloat16) && au_is(seq, q, torch::kFloat16) &&
                  au_is(Wb, q, torch::kFloat16) && au_is(Wp, q, torch::kFloat16),
              who, ": q, seq, Wb, Wp must be contiguous float16 on one GPU");
  TORCH_CHECK(au_is(u, q, torch::kFloat32) && au_is(w2, q, torch::kFloat32) &&
                  au_is(b2, q, torch::kFloat32),
              who, ": u, w2, b2 must be contiguous float32 beside q");
  TORCH_CHECK(q.dim() == 2 && seq.dim() == 3 && seq.size(0) == q.size(0) &&
                  seq.size(2) == q.size(1) + 1,
              who, ": expected q [B, D] and seq [B, L, D+1]");
  const int64_t B = q.size(0), D = q.size(1), L = seq.size(1);
  TORCH_CHECK(Wb.dim() == 2 && Wb.size(1) == D && Wp.sizes() == Wb.sizes(), who,
              ": expected Wb and Wp [H, D]");
  const int64_t H = Wb.size(0);
  TORCH_CHECK(u.dim() == 2 && u.size(0) == B && u.size(1) == H &&
                  w2.dim() == 1 && w2.size(0) == H && b2.numel() == 1,
              who, ": expected u [B, H], w2 [H] and a one-element b2");
  TORCH_CHECK(((uintptr_t)Wb.data_ptr() & 15) == 0 &&
                  ((uintptr_t)Wp.data_ptr() & 15) == 0,
              who, ": Wb and Wp must start on 16 bytes");
  TORCH_CHECK(B <= INT32_MAX, who, ": batch too large");
  TORCH_CHECK(au_feasible(L, D, H), who, ": no kernel for L=", L, " D=", D,
              " H=", H, " (act_unit_feasible)");
  TORCH_CHECK(max_blocks >= 0, who, ": max_blocks must be >= 0");
  // plan: two blocks per CU (the backward's LDS allows two to three)
  int64_t grid = max_blocks > 0
                     ? max_blocks
                     : 2 * at::cuda::getCurrentDeviceProperties()
                               ->multiProcessorCount;
  grid = grid < B ? grid : B;
  return (int)grid;
}

#define AU_CASE(HT, DT, ...)        \
  if (H == 16 * HT && D == 16 * DT) \
    return [&] { constexpr int kHT = HT, kDT = DT; __VA_ARGS__; }();
#define AU_DISPATCH(...)                                                     \
  AU_CASE(1, 2, __VA_ARGS__) AU_CASE(1, 4, __VA_ARGS__)                      \
  AU_CASE(1, 6, __VA_ARGS__) AU_CASE(1, 8, __VA_ARGS__)                      \
  AU_CASE(2, 2, __VA_ARGS__) AU_CASE(2, 4, __VA_ARGS__)                      \
  AU_CASE(2, 6, __VA_ARGS__) AU_CASE(2, 8, __VA_ARGS__)                      \
  AU_CASE(3, 2, __VA_ARGS__) AU_CASE(3, 4, __VA_ARGS__)                      \
  AU_CASE(3, 6, __VA_ARGS__) AU_CASE(3, 8, __VA_ARGS__)                      \
  AU_CASE(4, 2, __VA_ARGS__) AU_CASE(4, 4, __VA_ARGS__)                      \
  AU_CASE(4, 6, __VA_ARGS__) AU_CASE(4, 8, __VA_ARGS__)

void au_launch_fwd(int H, int D, int grid, const torch::Tensor& q,
                   const torch::Tensor& seq, const torch::Tensor& u,
                   const torch::Tensor& Wb, const torch::Tensor& Wp,
                   const torch::Tensor& w2, const torch::Tensor& b2,
                   torch::Tensor& out) {
  const int B = (int)q.size(0), L = (int)seq.size(1);
  AU_DISPATCH(hipLaunchKernelGGL(
      (act_unit_fwd_kernel<kHT, kDT>), dim3(grid), dim3(256), 0, au_stream(),
      (const u16*)q.data_ptr(), (const u16*)seq.data_ptr(),
      (const float*)u.data_ptr(), (const u16*)Wb.data_ptr(),
      (const u16*)Wp.data_ptr(), (const float*)w2.data_ptr(),
      (const float*)b2.data_ptr(), (u16*)out.data_ptr(), B, L))
  TORCH_CHECK(false, "act_unit_fwd: no instance for H=", H, " D=", D);
}

void au_launch_bwd(int H, int D, int grid, const torch::Tensor& g,
                   const torch::Tensor& q, const torch::Tensor& seq,
                   const torch::Tensor& u, const torch::Tensor& Wb,
                   const torch::Tensor& Wp, const torch::Tensor& w2,
                   const torch::Tensor& b2, torch::Tensor& dq,
                   torch::Tensor& dseq, torch::Tensor& du,
                   torch::Tensor& part) {
  const int B = (int)q.size(0), L = (int)seq.size(1);
  AU_DISPATCH(hipLaunchKernelGGL(
      (act_unit_bwd_kernel<kHT, kDT>), dim3(grid), dim3(256), 0, au_stream(),
      (const u16*)g.data_ptr(), (const u16*)q.data_ptr(),
      (const u16*)seq.data_ptr(), (const float*)u.data_ptr(),
      (const u16*)Wb.data_ptr(), (const u16*)Wp.data_ptr(),
      (const float*)w2.data_ptr(), (const float*)b2.data_ptr(),
      (u16*)dq.data_ptr(), (u16*)dseq.data_ptr(), (float*)du.data_ptr(),
      (float*)part.data_ptr(), B, L))
  TORCH_CHECK(false, "act_unit_bwd: no instance for H=", H, " D=", D);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool act_unit_feasible(int64_t L, int64_t D, int64_t H) {
  return au_feasible(L, D, H);
}

torch::Tensor act_unit_fwd(torch::Tensor q, torch::Tensor seq, torch::Tensor u,
                           torch::Tensor Wb, torch::Tensor Wp, torch::Tensor w2,
                           torch::Tensor b2, int64_t max_blocks) {
  const int grid =
      au_check(q, seq, u, Wb, Wp, w2, b2, max_blocks, "act_unit_fwd");
  auto out = torch::empty_like(q);
  if (q.size(0) == 0) return out;
  au_launch_fwd((int)Wb.size(0), (int)q.size(1), grid, q, seq, u, Wb, Wp, w2,
                b2, out);
  return out;
}

std::vector<torch::Tensor> act_unit_bwd(torch::Tensor g, torch::Tensor q,
                                        torch::Tensor seq, torch::Tensor u,
                                        torch::Tensor Wb, torch::Tensor Wp,
                                        torch::Tensor w2, torch::Tensor b2,
                                        int64_t max_blocks) {
  const int grid =
      au_check(q, seq, u, Wb, Wp, w2, b2, max_blocks, "act_unit_bwd");
  TORCH_CHECK(au_is(g, q, torch::kFloat16) && g.sizes() == q.sizes(),
              "act_unit_bwd: g must be a contiguous float16 [B, D] beside q");
  const int64_t H = Wb.size(0), D = q.size(1), n = 2 * H * D + H + 1;
  auto dq = torch::empty_like(q);
  auto dseq = torch::empty_like(seq);
  auto du = torch::empty_like(u);
  auto sums = torch::zeros({n}, u.options());
  if (q.size(0) > 0) {
    auto part = torch::empty({(int64_t)grid, n}, u.options());
    au_launch_bwd((int)H, (int)D, grid, g, q, seq, u, Wb, Wp, w2, b2, dq, dseq,
                  du, part);
    hipLaunchKernelGGL(au_reduce_kernel, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, au_stream(),
                       (const float*)part.data_ptr(), (float*)sums.data_ptr(),
                       grid, (int)n);
  }
  return {dq,
          dseq,
          du,
          sums.narrow(0, 0, H * D).view({H, D}),
          sums.narrow(0, H * D, H * D).view({H, D}),
          sums.narrow(0, 2 * H * D, H),
          sums.narrow(0, 2 * H * D + H, 1).squeeze(0)};
}

void init_actunit(pybind11::module_& m) {
  m.def("act_unit_feasible", &act_unit_feasible,
        "true if the activation-unit pooling kernels take (L, D, H)");
  m.def("act_unit_fwd", &act_unit_fwd,
        "out[b] = sum_valid (w2 . sigmoid(u[b] + M_b k_l) + b2) k_l",
        pybind11::arg("q"), pybind11::arg("seq"), pybind11::arg("u"),
        pybind11::arg("Wb"), pybind11::arg("Wp"), pybind11::arg("w2"),
        pybind11::arg("b2"), pybind11::arg("max_blocks") = 0);
  m.def("act_unit_bwd", &act_unit_bwd,
        "activation-unit pooling backward -> (dq_k, dseq, du, dWb, dWp, dw2, "
        "db2)",
        pybind11::arg("g"), pybind11::arg("q"), pybind11::arg("seq"),
        pybind11::arg("u"), pybind11::arg("Wb"), pybind11::arg("Wp"),
        pybind11::arg("w2"), pybind11::arg("b2"),
        pybind11::arg("max_blocks") = 0);
}
