// Multi-head self-attention among the rows of a raw slot (gfx950).
//
//   seq  [B, L, D+1] f16: channels 0..D-1 the row x_l, channel D the 0/1 mask
//   W    [3D, D]     f16: f16(in_proj_weight), rows q | k | v
//   bias [3D]        f32
//   valid i:  [q_i | k_i | v_i] = W x_i + bias, per head h of dh = D / heads
//             s_ij = dh^-1/2 <q_i^h, k_j^h>;  j allowed iff valid and (not
//             causal or j <= i);  p_i. = softmax over the allowed j
//             o_i^h = sum_j p_ij v_j^h;  out_i = f16(o_i (+ x_i if residual))
//   invalid i: out_i = +0;   out[..., D] = seq[..., D]
// backward (q, k, v, p are RECOMPUTED from seq and W, nothing else is saved):
//   per head  dP = g V^T;  delta_i = sum_j p_ij dP_ij  (= <g_i, o_i^h>)
//             dS = dh^-1/2 P (dP - delta);  dV = P^T g;  dQ = dS K;
//             dK = dS^T Q
//   dX = sum_h [dQ|dK|dV]^h W^h (+ g if residual);  dW^h = [dQ|dK|dV]^h^T X;
//   db^h = column sums of [dQ|dK|dV]^h
//
// Work split: a persistent grid of 4-wave blocks; block i walks the samples
// [i*B/G, (i+1)*B/G) one at a time.  L <= 64, so a sample is ONE tile of
// NS = ceil(L/16) 16-row strips and everything between reading seq and
// writing out (or dseq) lives in LDS and registers: no [B, L, 3D] buffer and
// nothing of size L x L reaches global memory.
//
// Staging is actunit.hip's: the sample's contiguous halves are read as
// aligned 32-bit words (boundary words half by half, never outside the
// tensor) and scattered into an image of pitch D+8, the mask into its own
// array; then the invalid rows and the tail of the tile are zeroed, because
// under MFMA a zero weight times a NaN row still poisons a sum.  The
// epilogues select by the mask as well.
//
// Forward.  Projection is split by output columns: a wave owns the 16-column
// tiles wave, wave+4, ... of the 3D columns as B-fragments of W, loaded once
// per block and held in registers across its samples, and writes its columns
// of Q, K, V as f16 images.  Attention is split by (head, query strip) over
// the waves: S = Q^h K^h^T on mfma_f32_16x16x32_f16 (dh = 16: the upper half
// of the reduction is zero operands), softmax in the accumulator layout
// (lane = key column fi, rows 4*fg .. 4*fg+3; row max and sum by xor
// butterfly over the 16 lanes of a row), P to a per-wave f16 image for the
// A-fragment role, O = P V^h with V read by ds_read_b64_tr_b16 from the
// linear image.
//
// Backward runs the heads one at a time so that the per-head images are
// [64, dh+8]: (1) project the head's q, k, v, split by column tiles; (2) wave
// = query strip: S, P, dP, delta, dS in registers, P and dS to images, dQ of
// the strip; (3) wave = key strip: dK = dS^T Q, dV = P^T g, the strip's part
// of db; (4) [dQ|dK|dV] to images over the dead q, k, v, P and dS images; (5)
// wave = column tile of D: dX += dZ W^h and dW^h += dZ^T X with the B
// fragments of W^h (transposed role) held in registers for all samples.
//
// Precision.  q, k, v and p are f16 MFMA operands -- the approximation that
// ops.reference emulates with operand_dtype=float16.  The gradient operands
// dS and [dQ|dK|dV] are f32 values and are staged as TWO f16 images, hi =
// f16(v) and lo = f16((v - hi) * 2^11), every product running once per image
// (as in actunit.hip and seqgru.hip): a single f16 image would put a second
// and third 2^-12 rounding into the f32 weight gradients, which the bound of
// the tests has no room for.
//
// Order.  Every per-sample sum has an order fixed by the sample alone, so out
// and dseq do not depend on B, the sample's place or the grid.  dW and db are
// accumulated in registers over a block's samples, written as one partial
// per block and summed in block order by sa_reduce_kernel: no atomics.
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

constexpr int SA_ROWS = 64;       // rows of the tile: 4 strips of 16
constexpr int SA_PP = SA_ROWS + 8;  // pitch of the P and dS images
constexpr float SA_LO = 2048.0f;  // scale of the low gradient images
constexpr float SA_LO_INV = 1.0f / 2048.0f;

// Builtins only inside the kernels (see actunit.hip).
__device__ __forceinline__ float sa_h2f(u16 x) {
  return (float)__builtin_bit_cast(_Float16, x);
}

__device__ __forceinline__ u16 sa_f2h(float f) {  // round to nearest even
  return __builtin_bit_cast(u16, (_Float16)f);
}

__device__ __forceinline__ void sa_sync() {  // what __syncthreads() does
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Orders a wave's own LDS writes before its own (cross-lane) LDS reads.
__device__ __forceinline__ void sa_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float sa_shfl(float v, int src_lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src_lane << 2,
                                          __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ bool sa_valid(u16 mask) {  // != 0, -0 is zero
  return (mask & 0x7fff) != 0;
}

__device__ __forceinline__ f4 sa_mfma(h8 a, h8 b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ h8 sa_zero8() {
  return h8{0, 0, 0, 0, 0, 0, 0, 0};
}

// 8 contiguous halves of an image row, or zeros past the reduction's end.
__device__ __forceinline__ h8 sa_row(const u16* p, bool on) {
  return on ? *(const h8*)p : sa_zero8();
}

__device__ __forceinline__ void sa_split(float v, u16& hi, u16& lo) {
  const _Float16 h = (_Float16)v;
  hi = __builtin_bit_cast(u16, h);
  lo = __builtin_bit_cast(u16, (_Float16)((v - (float)h) * SA_LO));
}

// Rows [0, nrows) of a sample (pitch D+1, first half at index s of src) ->
// img (pitch D+8), channel D -> mask.  total = src.numel().
template <int D>
__device__ __forceinline__ void sa_stage(const u16* __restrict__ src,
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
// in img.  own: mask belongs to img, its tail is cleared.
template <int D>
__device__ __forceinline__ void sa_fix(u16* img, u16* mask, int nrows,
                                       bool own, int wave, int lane) {
  constexpr int XP = D + 8;
  const int row = wave * 16 + (lane >> 2), part = lane & 3;
  const bool tail = row >= nrows;
  const bool bad = tail || !sa_valid(mask[row]);
  if (bad) {
    for (int c = part; c < D / 8; c += 4)
      *(u4*)&img[row * XP + c * 8] = u4{0, 0, 0, 0};
  }
  if (own && tail && part == 0) mask[row] = 0;
}

// 8 halves img[kb + 8*fg + j][cb + fi], j = 0..7: the fragment of an operand
// whose reduction index runs down the rows of a linear image (actunit.hip's
// au_tr, addressed as in interact.hip).
__device__ __forceinline__ h8 sa_tr(const u16* img, int pitch, int kb, int cb,
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

// The softmax of query strip s against every key strip: p[js][r] = p_ij for
// i = 16 s + 4 fg + r, j = 16 js + fi (0 where j is not allowed, where i is
// invalid and for js >= NS), ok[r] = row i is valid.  q and k are the head's
// columns coff .. coff+DH of images of the given pitch.
template <int DH>
__device__ __forceinline__ void sa_probs(const u16* qimg, const u16* kimg,
                                         int pitch, int coff, int s, int NS,
                                         const u16* mask, bool causal,
                                         int lane, float (&p)[4][4],
                                         bool (&ok)[4]) {
  constexpr float scale = DH == 16 ? 0.25f : 0.17677669529663687f;
  const int fi = lane & 15, fg = lane >> 4;
  const float ninf = -__builtin_inff();
  const h8 aq = sa_row(&qimg[(s * 16 + fi) * pitch + coff + fg * 8], fg * 8 < DH);
  float m[4] = {ninf, ninf, ninf, ninf};
#pragma unroll
  for (int js = 0; js < 4; ++js) {
    const bool on = js < NS && (!causal || js <= s);
    f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
    if (on) {
      const h8 bk =
          sa_row(&kimg[(js * 16 + fi) * pitch + coff + fg * 8], fg * 8 < DH);
      acc = sa_mfma(aq, bk, acc);
    }
    const int j = js * 16 + fi;
    const bool vj = on && sa_valid(mask[j]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = s * 16 + fg * 4 + r;
      p[js][r] = vj && (!causal || j <= i) ? scale * acc[r] : ninf;
      m[r] = __builtin_fmaxf(m[r], p[js][r]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
      m[r] = __builtin_fmaxf(m[r], sa_shfl(m[r], lane ^ off));
    if (!(m[r] > ninf)) m[r] = 0.0f;  // no allowed key (an invalid row)
    ok[r] = sa_valid(mask[s * 16 + fg * 4 + r]);
  }
  float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int js = 0; js < 4; ++js) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[js][r] = p[js][r] > ninf ? __expf(p[js][r] - m[r]) : 0.0f;
      sum[r] += p[js][r];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) sum[r] += sa_shfl(sum[r], lane ^ off);
    const float inv = ok[r] && sum[r] > 0.0f ? 1.0f / sum[r] : 0.0f;
#pragma unroll
    for (int js = 0; js < 4; ++js) p[js][r] *= inv;
  }
}

template <int D, int DH>
__global__ __launch_bounds__(256) void seq_self_attn_fwd_kernel(
    const u16* __restrict__ seq, const u16* __restrict__ W,
    const float* __restrict__ bias, u16* __restrict__ out, int B, int L,
    int causal, int residual) {
  constexpr int XP = D + 8, NH = D / DH, KD = D / 32;
  constexpr int NT = 3 * D / 16;     // column tiles of [q | k | v]
  constexpr int NTW = (NT + 3) / 4;  // of one wave
  __shared__ __align__(16) u16 ximg[SA_ROWS * XP];
  __shared__ __align__(16) u16 qkv[3 * SA_ROWS * XP];
  __shared__ __align__(16) u16 pimg[4 * 16 * SA_PP];
  __shared__ u16 mask[SA_ROWS];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4;
  const int NS = (L + 15) / 16, KS = (NS + 1) / 2;
  // the strips NS.. of q, k, v are never computed: zeros, so that the second
  // half of a 32-row reduction step over an odd NS adds nothing
  for (int i = threadIdx.x; i < 3 * SA_ROWS * XP / 8; i += 256)
    *(u4*)&qkv[i * 8] = u4{0, 0, 0, 0};
  h8 wfr[NTW][KD];
  float br[NTW];
#pragma unroll
  for (int n = 0; n < NTW; ++n) {
    const int t = wave + 4 * n;
    br[n] = t < NT ? bias[t * 16 + fi] : 0.0f;
#pragma unroll
    for (int ks = 0; ks < KD; ++ks)
      wfr[n][ks] = t < NT ? *(const h8*)&W[(t * 16 + fi) * D + ks * 32 + fg * 8]
                          : sa_zero8();
  }
  const u16 *qimg = qkv, *kimg = qkv + SA_ROWS * XP, *vimg = qkv + 2 * SA_ROWS * XP;
  u16* pw = pimg + wave * 16 * SA_PP;
  const int64_t total = (int64_t)B * L * (D + 1);
  const int64_t bs = (int64_t)blockIdx.x * B / gridDim.x;
  const int64_t be = ((int64_t)blockIdx.x + 1) * B / gridDim.x;
  for (int64_t b = bs; b < be; ++b) {
    sa_sync();  // the last sample's readers are done (and qkv is zeroed)
    sa_stage<D>(seq, total, b * L * (D + 1), L, ximg, mask);
    sa_sync();
    sa_fix<D>(ximg, mask, L, true, wave, lane);
    sa_sync();
    // projection: the wave's column tiles of every strip
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s < NS) {
        h8 a[KD];
#pragma unroll
        for (int ks = 0; ks < KD; ++ks)
          a[ks] = *(const h8*)&ximg[(s * 16 + fi) * XP + ks * 32 + fg * 8];
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
          const int t = wave + 4 * n;
          if (t < NT) {
            f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int ks = 0; ks < KD; ++ks) acc = sa_mfma(a[ks], wfr[n][ks], acc);
            const int which = t * 16 / D, col = t * 16 - which * D + fi;
            u16* dst = qkv + which * SA_ROWS * XP + (s * 16 + fg * 4) * XP + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[r * XP] = sa_f2h(acc[r] + br[n]);
          }
        }
      }
    }
    sa_sync();
    // attention: (head, query strip) items over the waves
    for (int it = wave; it < NH * NS; it += 4) {
      const int h = it / NS, s = it - h * NS;
      float p[4][4];
      bool ok[4];
      sa_probs<DH>(qimg, kimg, XP, h * DH, s, NS, mask, causal != 0, lane, p, ok);
      sa_wave_sync();  // the last item's reads of pw
#pragma unroll
      for (int js = 0; js < 4; ++js) {
        if (js < 2 * KS) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            pw[(fg * 4 + r) * SA_PP + js * 16 + fi] = sa_f2h(p[js][r]);
        }
      }
      sa_wave_sync();
#pragma unroll
      for (int nt = 0; nt < DH / 16; ++nt) {
        f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          if (ks < KS) {
            const h8 a = *(const h8*)&pw[fi * SA_PP + ks * 32 + fg * 8];
            acc = sa_mfma(a, sa_tr(vimg, XP, ks * 32, h * DH + nt * 16, lane), acc);
          }
        }
        const int d = h * DH + nt * 16 + fi;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int l = s * 16 + fg * 4 + r;
          if (l < L) {
            float o = acc[r];
            if (residual) o += sa_h2f(ximg[l * XP + d]);
            u16* row = out + (b * L + l) * (D + 1);
            row[d] = ok[r] ? sa_f2h(o) : (u16)0;
            if (h == 0 && nt == 0 && fi == 0) row[D] = mask[l];
          }
        }
      }
    }
  }
}

// Partials of one block, f32: [dW 3D*D][db 3D].
template <int D, int DH>
__global__ __launch_bounds__(256) void seq_self_attn_bwd_kernel(
    const u16* __restrict__ g, const u16* __restrict__ seq,
    const u16* __restrict__ W, const float* __restrict__ bias,
    u16* __restrict__ dseq, float* __restrict__ part, int B, int L, int causal,
    int residual) {
  constexpr int XP = D + 8, HP = DH + 8, NH = D / DH, KD = D / 32;
  constexpr int CT = DH / 16;          // 16-column tiles of a head
  constexpr int T3 = 3 * CT;           // tiles of the head's [q | k | v]
  constexpr int TPW = (T3 + 3) / 4;    // projection tiles of a wave
  constexpr int NDT = D / 16;          // column tiles of D
  constexpr int SPLIT = 4 / NDT;       // waves that share one of them
  constexpr int TW = (T3 + SPLIT - 1) / SPLIT;  // dW tiles of a wave and head
  constexpr int HIMG = SA_ROWS * HP, PIMG = SA_ROWS * SA_PP;
  __shared__ __align__(16) u16 ximg[SA_ROWS * XP];
  __shared__ __align__(16) u16 gimg[SA_ROWS * XP];
  // q, k, v of the head; later the hi images of dQ, dK, dV
  __shared__ __align__(16) u16 rega[3 * HIMG];
  // P, dS hi, dS lo; later the lo images of dQ, dK, dV (3 HIMG <= 3 PIMG)
  __shared__ __align__(16) u16 regb[3 * PIMG];
  __shared__ u16 mask[SA_ROWS];
  __shared__ u16 gmask[SA_ROWS];  // channel D of g: staged, never used
  __shared__ float red[4 * 3 * DH];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4;
  const int NS = (L + 15) / 16, KS = (NS + 1) / 2;
  const int dt = wave % NDT, grp = wave / NDT;  // the wave's part of dX, dW
  u16 *pimg = regb, *dsh = regb + PIMG, *dsl = regb + 2 * PIMG;
  for (int i = threadIdx.x; i < 3 * HIMG / 8; i += 256)
    *(u4*)&rega[i * 8] = u4{0, 0, 0, 0};
  for (int i = threadIdx.x; i < 3 * PIMG / 8; i += 256)
    *(u4*)&regb[i * 8] = u4{0, 0, 0, 0};
  // projection fragments: tile ti = wave + 4 n of head h
  h8 wpr[NH][TPW][KD];
  float bpr[NH][TPW];
  // fragments of W^h for dX: reduction down the rows of W, column dt*16 + fi
  h8 wxr[NH][3];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
#pragma unroll
    for (int n = 0; n < TPW; ++n) {
      const int ti = wave + 4 * n;
      const int rowq = (ti / CT) * D + h * DH + (ti % CT) * 16 + fi;
      bpr[h][n] = ti < T3 ? bias[rowq] : 0.0f;
#pragma unroll
      for (int ks = 0; ks < KD; ++ks)
        wpr[h][n][ks] = ti < T3 ? *(const h8*)&W[rowq * D + ks * 32 + fg * 8]
                                : sa_zero8();
    }
#pragma unroll
    for (int which = 0; which < 3; ++which) {
      h8 f = sa_zero8();
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = fg * 8 + j;
        if (c < DH)
          f[j] = __builtin_bit_cast(
              _Float16, W[(which * D + h * DH + c) * D + dt * 16 + fi]);
      }
      wxr[h][which] = f;
    }
  }
  f4 dWa[NH][TW];
  float dba[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    dba[h] = 0.0f;
#pragma unroll
    for (int n = 0; n < TW; ++n) dWa[h][n] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  const int64_t total = (int64_t)B * L * (D + 1);
  const int64_t bs = (int64_t)blockIdx.x * B / gridDim.x;
  const int64_t be = ((int64_t)blockIdx.x + 1) * B / gridDim.x;
  for (int64_t b = bs; b < be; ++b) {
    sa_sync();  // the last sample's readers are done (and the images zeroed)
    sa_stage<D>(seq, total, b * L * (D + 1), L, ximg, mask);
    sa_stage<D>(g, total, b * L * (D + 1), L, gimg, gmask);
    sa_sync();
    sa_fix<D>(ximg, mask, L, true, wave, lane);
    sa_fix<D>(gimg, mask, L, false, wave, lane);
    f4 dXa[4 / SPLIT];
#pragma unroll
    for (int n = 0; n < 4 / SPLIT; ++n) dXa[n] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      u16 *qh = rega, *kh = rega + HIMG, *vh = rega + 2 * HIMG;
      sa_sync();  // the last head's readers of rega; the fixes above
      // (1) the head's q, k, v: the wave's column tiles of every strip
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (s < NS) {
          h8 a[KD];
#pragma unroll
          for (int ks = 0; ks < KD; ++ks)
            a[ks] = *(const h8*)&ximg[(s * 16 + fi) * XP + ks * 32 + fg * 8];
#pragma unroll
          for (int n = 0; n < TPW; ++n) {
            const int ti = wave + 4 * n;
            if (ti < T3) {
              f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
              for (int ks = 0; ks < KD; ++ks)
                acc = sa_mfma(a[ks], wpr[h][n][ks], acc);
              u16* dst = rega + (ti / CT) * HIMG + (s * 16 + fg * 4) * HP +
                         (ti % CT) * 16 + fi;
#pragma unroll
              for (int r = 0; r < 4; ++r)
                dst[r * HP] = sa_f2h(acc[r] + bpr[h][n]);
            }
          }
        }
      }
      sa_sync();
      // (2) wave = query strip: P, dS and the strip's dQ
      f4 dZ[3][CT];
#pragma unroll
      for (int w3 = 0; w3 < 3; ++w3) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) dZ[w3][ct] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      }
      if (wave < NS) {
        const int s = wave;
        float p[4][4];
        bool ok[4];
        sa_probs<DH>(qh, kh, HP, 0, s, NS, mask, causal != 0, lane, p, ok);
        constexpr float scale = DH == 16 ? 0.25f : 0.17677669529663687f;
        const h8 ag = sa_row(&gimg[(s * 16 + fi) * XP + h * DH + fg * 8], fg * 8 < DH);
        f4 dP[4];
        float delta[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int js = 0; js < 4; ++js) {
          dP[js] = f4{0.0f, 0.0f, 0.0f, 0.0f};
          if (js < NS && (!causal || js <= s)) {
            const h8 bv = sa_row(&vh[(js * 16 + fi) * HP + fg * 8], fg * 8 < DH);
            dP[js] = sa_mfma(ag, bv, dP[js]);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) delta[r] = fmaf(p[js][r], dP[js][r], delta[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int off = 1; off < 16; off <<= 1)
            delta[r] += sa_shfl(delta[r], lane ^ off);
        }
#pragma unroll
        for (int js = 0; js < 4; ++js) {
          if (js < 2 * KS) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int o = (s * 16 + fg * 4 + r) * SA_PP + js * 16 + fi;
              const float ds = scale * p[js][r] * (dP[js][r] - delta[r]);
              pimg[o] = sa_f2h(p[js][r]);
              sa_split(ds, dsh[o], dsl[o]);
            }
          }
        }
        sa_wave_sync();
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          f4 ch = f4{0.0f, 0.0f, 0.0f, 0.0f}, cl = ch;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            if (ks < KS) {
              const int o = (s * 16 + fi) * SA_PP + ks * 32 + fg * 8;
              const h8 bk = sa_tr(kh, HP, ks * 32, ct * 16, lane);
              ch = sa_mfma(*(const h8*)&dsh[o], bk, ch);
              cl = sa_mfma(*(const h8*)&dsl[o], bk, cl);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) dZ[0][ct][r] = fmaf(cl[r], SA_LO_INV, ch[r]);
        }
      } else if (wave < 2 * KS) {  // the strip that pads an odd NS: zeros
        for (int i = lane; i < 16 * SA_PP / 8; i += 64) {
          const int o = wave * 16 * SA_PP + i * 8;
          *(u4*)&pimg[o] = u4{0, 0, 0, 0};
          *(u4*)&dsh[o] = u4{0, 0, 0, 0};
          *(u4*)&dsl[o] = u4{0, 0, 0, 0};
        }
      }
      sa_sync();
      // (3) wave = key strip: dK = dS^T Q, dV = P^T g, column sums for db
      if (wave < NS) {
        const int js = wave;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          f4 ch = f4{0.0f, 0.0f, 0.0f, 0.0f}, cl = ch, cv = ch;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            if (ks < KS) {
              const h8 bq = sa_tr(qh, HP, ks * 32, ct * 16, lane);
              ch = sa_mfma(sa_tr(dsh, SA_PP, ks * 32, js * 16, lane), bq, ch);
              cl = sa_mfma(sa_tr(dsl, SA_PP, ks * 32, js * 16, lane), bq, cl);
              cv = sa_mfma(sa_tr(pimg, SA_PP, ks * 32, js * 16, lane),
                           sa_tr(gimg, XP, ks * 32, h * DH + ct * 16, lane), cv);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            dZ[1][ct][r] = fmaf(cl[r], SA_LO_INV, ch[r]);
            dZ[2][ct][r] = cv[r];
          }
        }
      }
#pragma unroll
      for (int w3 = 0; w3 < 3; ++w3) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const f4 z = dZ[w3][ct];
          float v = (z[0] + z[1]) + (z[2] + z[3]);
          v += sa_shfl(v, lane ^ 16);
          v += sa_shfl(v, lane ^ 32);
          if (fg == 0) red[wave * 3 * DH + w3 * DH + ct * 16 + fi] = v;
        }
      }
      sa_sync();
      // (4) [dQ | dK | dV] of the wave's strip as hi and lo images over the
      // dead ones; a wave without a strip writes the zeros of its rows
      if (threadIdx.x < 3 * DH) {
        const int t = threadIdx.x;
        dba[h] += ((red[t] + red[3 * DH + t]) + red[6 * DH + t]) + red[9 * DH + t];
      }
#pragma unroll
      for (int w3 = 0; w3 < 3; ++w3) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = w3 * HIMG + (wave * 16 + fg * 4 + r) * HP + ct * 16 + fi;
            sa_split(dZ[w3][ct][r], rega[o], regb[o]);
          }
        }
      }
      sa_sync();
      // (5) wave = column tile dt of D (and strips / tiles grp mod SPLIT)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (s < NS && s % SPLIT == grp) {
          f4 ch = f4{0.0f, 0.0f, 0.0f, 0.0f}, cl = ch;
#pragma unroll
          for (int w3 = 0; w3 < 3; ++w3) {
            const int o = w3 * HIMG + (s * 16 + fi) * HP + fg * 8;
            ch = sa_mfma(sa_row(&rega[o], fg * 8 < DH), wxr[h][w3], ch);
            cl = sa_mfma(sa_row(&regb[o], fg * 8 < DH), wxr[h][w3], cl);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r)
            dXa[s / SPLIT][r] += fmaf(cl[r], SA_LO_INV, ch[r]);
        }
      }
#pragma unroll
      for (int ti = 0; ti < T3; ++ti) {
        if (ti % SPLIT == grp) {
          f4 ch = f4{0.0f, 0.0f, 0.0f, 0.0f}, cl = ch;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            if (ks < KS) {
              const h8 bx = sa_tr(ximg, XP, ks * 32, dt * 16, lane);
              const u16* zi = rega + (ti / CT) * HIMG;
              const u16* zl = regb + (ti / CT) * HIMG;
              ch = sa_mfma(sa_tr(zi, HP, ks * 32, (ti % CT) * 16, lane), bx, ch);
              cl = sa_mfma(sa_tr(zl, HP, ks * 32, (ti % CT) * 16, lane), bx, cl);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r)
            dWa[h][ti / SPLIT][r] += fmaf(cl[r], SA_LO_INV, ch[r]);
        }
      }
    }
    // dseq: rows of the wave's strips, column dt*16 + fi
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s < NS && s % SPLIT == grp) {
        const int d = dt * 16 + fi;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int l = s * 16 + fg * 4 + r;
          if (l < L) {
            float v = dXa[s / SPLIT][r];
            if (residual) v += sa_h2f(gimg[l * XP + d]);
            u16* row = dseq + (b * L + l) * (D + 1);
            row[d] = sa_valid(mask[l]) ? sa_f2h(v) : (u16)0;
            if (dt == 0 && fi == 0) row[D] = 0;
          }
        }
      }
    }
  }
  // the block's partial
  float* p = part + (int64_t)blockIdx.x * (3 * D * D + 3 * D);
#pragma unroll
  for (int h = 0; h < NH; ++h) {
#pragma unroll
    for (int ti = 0; ti < T3; ++ti) {
      if (ti % SPLIT == grp) {
        const int row0 = (ti / CT) * D + h * DH + (ti % CT) * 16 + fg * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          p[(row0 + r) * D + dt * 16 + fi] = dWa[h][ti / SPLIT][r];
      }
    }
    if (threadIdx.x < 3 * DH) {
      const int t = threadIdx.x;
      p[3 * D * D + (t / DH) * D + h * DH + t % DH] = dba[h];
    }
  }
}

// out[i] = sum over the blocks' partials, in block order
__global__ __launch_bounds__(256) void sa_reduce_kernel(
    const float* __restrict__ part, float* __restrict__ out, int nblk, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float acc = 0.0f;
  for (int k = 0; k < nblk; ++k) acc += part[(int64_t)k * n + i];
  out[i] = acc;
}

bool sa_feasible(int64_t L, int64_t D, int64_t heads) {
  if (!(D == 32 || D == 64) || heads < 1 || D % heads != 0) return false;
  const int64_t dh = D / heads;
  return (dh == 16 || dh == 32) && L >= 1 && L <= SA_ROWS;
}

hipStream_t sa_stream() { return at::hip::getCurrentHIPStream().stream(); }

bool sa_is(const torch::Tensor& t, const torch::Tensor& like,
           c10::ScalarType st) {
  return t.is_cuda() && t.device() == like.device() && t.scalar_type() == st &&
         t.is_contiguous();
}

// -> the grid; raises on anything the kernels do not take
int sa_check(const torch::Tensor& seq, const torch::Tensor& W,
             const torch::Tensor& bias, int64_t heads, int64_t max_blocks,
             const char* who) {
  TORCH_CHECK(seq.is_cuda(), who, ": seq must be on a GPU");
  TORCH_CHECK(sa_is(seq, seq, torch::kFloat16) && sa_is(W, seq, torch::kFloat16),
              who, ": seq and Wqkv must be contiguous float16 on one GPU");
  TORCH_CHECK(sa_is(bias, seq, torch::kFloat32), who,
              ": bqkv must be contiguous float32 beside seq");
  TORCH_CHECK(seq.dim() == 3 && seq.size(2) >= 2, who,
              ": expected seq [B, L, D+1]");
  const int64_t B = seq.size(0), L = seq.size(1), D = seq.size(2) - 1;
  TORCH_CHECK(W.dim() == 2 && W.size(0) == 3 * D && W.size(1) == D &&
                  bias.dim() == 1 && bias.size(0) == 3 * D,
              who, ": expected Wqkv [3D, D] and bqkv [3D]");
  TORCH_CHECK(((uintptr_t)W.data_ptr() & 15) == 0, who,
              ": Wqkv must start on 16 bytes");
  TORCH_CHECK(B <= INT32_MAX, who, ": batch too large");
  TORCH_CHECK(sa_feasible(L, D, heads), who, ": no kernel for L=", L, " D=", D,
              " heads=", heads, " (seq_self_attn_feasible)");
  TORCH_CHECK(max_blocks >= 0, who, ": max_blocks must be >= 0");
  // plan: two blocks per CU, as act_unit (the backward's LDS allows two)
  int64_t grid = max_blocks > 0
                     ? max_blocks
                     : 2 * at::cuda::getCurrentDeviceProperties()
                               ->multiProcessorCount;
  grid = grid < B ? grid : B;
  return (int)grid;
}

#define SA_CASE(DD, DHH, ...)    \
  if (D == DD && DH == DHH)      \
    return [&] { constexpr int kD = DD, kDH = DHH; __VA_ARGS__; }();
#define SA_DISPATCH(...)                                  \
  SA_CASE(32, 16, __VA_ARGS__) SA_CASE(32, 32, __VA_ARGS__) \
  SA_CASE(64, 16, __VA_ARGS__) SA_CASE(64, 32, __VA_ARGS__)

void sa_launch_fwd(int D, int DH, int grid, const torch::Tensor& seq,
                   const torch::Tensor& W, const torch::Tensor& bias,
                   torch::Tensor& out, bool causal, bool residual) {
  const int B = (int)seq.size(0), L = (int)seq.size(1);
  SA_DISPATCH(hipLaunchKernelGGL(
      (seq_self_attn_fwd_kernel<kD, kDH>), dim3(grid), dim3(256), 0,
      sa_stream(), (const u16*)seq.data_ptr(), (const u16*)W.data_ptr(),
      (const float*)bias.data_ptr(), (u16*)out.data_ptr(), B, L, (int)causal,
      (int)residual))
  TORCH_CHECK(false, "seq_self_attn_fwd: no instance for D=", D, " dh=", DH);
}

void sa_launch_bwd(int D, int DH, int grid, const torch::Tensor& g,
                   const torch::Tensor& seq, const torch::Tensor& W,
                   const torch::Tensor& bias, torch::Tensor& dseq,
                   torch::Tensor& part, bool causal, bool residual) {
  const int B = (int)seq.size(0), L = (int)seq.size(1);
  SA_DISPATCH(hipLaunchKernelGGL(
      (seq_self_attn_bwd_kernel<kD, kDH>), dim3(grid), dim3(256), 0,
      sa_stream(), (const u16*)g.data_ptr(), (const u16*)seq.data_ptr(),
      (const u16*)W.data_ptr(), (const float*)bias.data_ptr(),
      (u16*)dseq.data_ptr(), (float*)part.data_ptr(), B, L, (int)causal,
      (int)residual))
  TORCH_CHECK(false, "seq_self_attn_bwd: no instance for D=", D, " dh=", DH);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool seq_self_attn_feasible(int64_t L, int64_t D, int64_t heads) {
  return sa_feasible(L, D, heads);
}

torch::Tensor seq_self_attn_fwd(torch::Tensor seq, torch::Tensor W,
                                torch::Tensor bias, int64_t heads, bool causal,
                                bool residual, int64_t max_blocks) {
  const int grid = sa_check(seq, W, bias, heads, max_blocks, "seq_self_attn_fwd");
  auto out = torch::empty_like(seq);
  if (seq.size(0) == 0) return out;
  const int D = (int)seq.size(2) - 1;
  sa_launch_fwd(D, D / (int)heads, grid, seq, W, bias, out, causal, residual);
  return out;
}

std::vector<torch::Tensor> seq_self_attn_bwd(torch::Tensor g, torch::Tensor seq,
                                             torch::Tensor W, torch::Tensor bias,
                                             int64_t heads, bool causal,
                                             bool residual, int64_t max_blocks) {
  const int grid = sa_check(seq, W, bias, heads, max_blocks, "seq_self_attn_bwd");
  TORCH_CHECK(sa_is(g, seq, torch::kFloat16) && g.sizes() == seq.sizes(),
              "seq_self_attn_bwd: g must be a contiguous float16 [B, L, D+1] "
              "beside seq");
  const int64_t D = seq.size(2) - 1, n = 3 * D * D + 3 * D;
  auto dseq = torch::empty_like(seq);
  auto sums = torch::zeros({n}, bias.options());
  if (seq.size(0) > 0) {
    auto part = torch::empty({(int64_t)grid, n}, bias.options());
    sa_launch_bwd((int)D, (int)(D / heads), grid, g, seq, W, bias, dseq, part,
                  causal, residual);
    hipLaunchKernelGGL(sa_reduce_kernel, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, sa_stream(), (const float*)part.data_ptr(),
                       (float*)sums.data_ptr(), grid, (int)n);
  }
  return {dseq, sums.narrow(0, 0, 3 * D * D).view({3 * D, D}),
          sums.narrow(0, 3 * D * D, 3 * D)};
}

void init_seqsa(pybind11::module_& m) {
  m.def("seq_self_attn_feasible", &seq_self_attn_feasible,
        "true if the self-attention kernels take (L, D, heads)");
  m.def("seq_self_attn_fwd", &seq_self_attn_fwd,
        "multi-head self-attention among the rows of a raw slot -> out "
        "[B, L, D+1]",
        pybind11::arg("seq"), pybind11::arg("Wqkv"), pybind11::arg("bqkv"),
        pybind11::arg("heads"), pybind11::arg("causal") = false,
        pybind11::arg("residual") = false, pybind11::arg("max_blocks") = 0);
  m.def("seq_self_attn_bwd", &seq_self_attn_bwd,
        "self-attention backward -> (dseq, dWqkv, dbqkv)", pybind11::arg("g"),
        pybind11::arg("seq"), pybind11::arg("Wqkv"), pybind11::arg("bqkv"),
        pybind11::arg("heads"), pybind11::arg("causal") = false,
        pybind11::arg("residual") = false, pybind11::arg("max_blocks") = 0);
}
