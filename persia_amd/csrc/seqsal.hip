// Multi-head self-attention among the rows of a raw slot, any L <= 1024
// (gfx950): seqsa.hip's function with the keys streamed.
//
//   seq  [B, L, D+1] f16: channels 0..D-1 the row x_l, channel D the 0/1 mask
//   W    [3D, D]     f16: f16(in_proj_weight), rows q | k | v
//   bias [3D]        f32
//   valid i:  [q_i | k_i | v_i] = W x_i + bias, per head h of dh = D / heads
//             s_ij = dh^-1/2 <q_i^h, k_j^h>;  j allowed iff valid and (not
//             causal or j <= i);  p_i. = softmax over the allowed j
//             o_i^h = sum_j p_ij v_j^h;  out_i = f16(o_i (+ x_i if residual))
//             lse[b, h, i] = log sum_j exp(s_ij)
//   invalid i: out_i = +0, lse = +0;   out[..., D] = seq[..., D]
// backward (q, k, v are RECOMPUTED; saved are seq, W, bias and lse):
//   per head  p_ij = exp(s_ij - lse_i);  dP = g V^T;  delta_i = sum_j p_ij dP_ij
//             dS = dh^-1/2 P (dP - delta);  dV = P^T g;  dQ = dS K;  dK = dS^T Q
//   dX = [dQ|dK|dV] W (+ g if residual);  dW = [dQ|dK|dV]^T X;  db = column sums
//
// Past 64 rows a sample's K and V no longer fit a workgroup's LDS beside
// anything else, so -- the one place where this project gives up "nothing of
// width 3D reaches global memory" -- the projection gets workspaces:
//   qkv  [B, L, 3D] f16   6 D bytes a row   (forward and backward)
//   msk  [B, L]     u16   the mask channel, contiguous
//   g16  [B, L, D]  f16   g_out with its invalid rows zeroed (backward)
//   dz   [B, L, 3D] f32   [dQ | dK | dV], 12 D bytes a row (backward)
//   delta [B, heads, L] f32 (backward)
// At B 4096, L 200, D 64: qkv 315 MB, dz 629 MB, g16 105 MB.  A row of qkv and
// dz is head-major, [q^0 | k^0 | v^0 | q^1 | ...], so a head's q, k and v are
// contiguous 16-byte multiples.  The workspaces live for one call.
//
// Kernels.  (1) sl_project_kernel: the B L rows in tiles of 64 whatever L is
// (seqffn.hip's split and staging: aligned 32-bit words, boundary words half
// by half, pitch D+8, the mask in its own array, invalid rows zeroed), wave =
// column tiles w, w+4, .. of [q|k|v] with their B-fragments of W held across
// the block's tiles; writes qkv (invalid rows +0), msk and, in the backward,
// g16.  (2) seq_self_attn_long_fwd_kernel: item = (sample, 64-row query
// tile), a persistent grid over the items, wave = 16-row query strip, the
// heads in a loop; Q^h fragments in registers, 64-row tiles of [K^h | V^h]
// copied into two LDS images in turn (the next tile's global loads are issued
// before the current tile's MFMAs, its LDS writes after them: one barrier a
// tile), S = Q K^T one MFMA per key strip, online softmax in the accumulator
// layout, f16(exp(s - running max)) to a per-wave image, O += P V with V by
// ds_read_b64_tr_b16.  Key tiles without a valid row, key tiles above the
// diagonal under `causal` and query strips without a valid row are skipped.
// A row that has met no allowed key yet has running max -inf; every
// difference is taken against (max > -inf ? max : 0), so no (-inf) - (-inf).
// (3) sl_dq_kernel: the forward's items, two passes over the key tiles: delta,
// then dS and dQ += dS K.  (4) sl_dkv_kernel: item = (sample, key tile), wave
// = key strip, tiles of [Q^h | g^h], lse and delta streamed: S^T = K Q^T and
// dP^T = V g^T come out transposed, so P^T and dS^T are A operands as they
// are; dV += P^T g, dK += dS^T Q.  (5) sl_project_bwd_kernel: row tiles again;
// dz in three chunks of D columns as hi/lo images; dX and dW as in seqsa.hip's
// phase (5), db the f32 column sums of dz; dW and db in registers across the
// block's tiles, one partial per block, summed in block order by
// sl_reduce_kernel.
//
// Precision: q, k, v and the probabilities are f16 MFMA operands; the forward
// rounds the un-normalised exp(s - running max), the backward exp(s - lse).
// dS and [dQ|dK|dV] are f32 values used as hi + lo 2^-11, two f16 images,
// every product once per image.
//
// Order: no atomics; every per-sample sum has an order fixed by the sample
// alone (its own list of live tiles), so out, lse and dseq do not depend on B,
// the sample's place or the grid; dW and db are bit-identical run to run for
// one batch and grid.
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
using s4 = __attribute__((ext_vector_type(4))) unsigned short;

constexpr int SL_ROWS = 64;          // rows of a tile: 4 strips of 16
constexpr int SL_PP = SL_ROWS + 8;   // pitch of the P and dS images
constexpr int SL_MAXL = 1024;
constexpr int SL_MAXT = SL_MAXL / SL_ROWS;
constexpr float SL_LO = 2048.0f;
constexpr float SL_LO_INV = 1.0f / 2048.0f;

__device__ __forceinline__ float sl_h2f(u16 x) {
  return (float)__builtin_bit_cast(_Float16, x);
}

__device__ __forceinline__ u16 sl_f2h(float f) {  // round to nearest even
  return __builtin_bit_cast(u16, (_Float16)f);
}

__device__ __forceinline__ void sl_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Orders a wave's own LDS writes before its own (cross-lane) LDS reads.
__device__ __forceinline__ void sl_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float sl_shfl(float v, int src_lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src_lane << 2,
                                          __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ bool sl_valid(u16 mask) {  // != 0, -0 is zero
  return (mask & 0x7fff) != 0;
}

__device__ __forceinline__ f4 sl_mfma(h8 a, h8 b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f4 sl_zero4() { return f4{0.0f, 0.0f, 0.0f, 0.0f}; }

__device__ __forceinline__ h8 sl_zero8() { return h8{0, 0, 0, 0, 0, 0, 0, 0}; }

// 8 contiguous halves, or zeros past the reduction's end (or the tensor's).
__device__ __forceinline__ h8 sl_row(const u16* p, bool on) {
  return on ? *(const h8*)p : sl_zero8();
}

__device__ __forceinline__ void sl_split(float v, u16& hi, u16& lo) {
  const _Float16 h = (_Float16)v;
  hi = __builtin_bit_cast(u16, h);
  lo = __builtin_bit_cast(u16, (_Float16)((v - (float)h) * SL_LO));
}

// sum / max over the 16 lanes that hold one accumulator row
__device__ __forceinline__ float sl_rowsum(float v, int lane) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v += sl_shfl(v, lane ^ off);
  return v;
}

__device__ __forceinline__ float sl_rowmax(float v, int lane) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1)
    v = __builtin_fmaxf(v, sl_shfl(v, lane ^ off));
  return v;
}

// seqffn.hip's ff_stage: rows [0, nrows) of the flattened tensor from half s
// on (pitch D+1) -> img (pitch D+8), channel D -> mask.  total = src.numel().
template <int D>
__device__ __forceinline__ void sl_stage(const u16* __restrict__ src,
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
__device__ __forceinline__ void sl_fix(u16* img, u16* mask, int nrows,
                                       bool own, int wave, int lane) {
  constexpr int XP = D + 8;
  const int row = wave * 16 + (lane >> 2), part = lane & 3;
  const bool tail = row >= nrows;
  const bool bad = tail || !sl_valid(mask[row]);
  if (bad) {
    for (int c = part; c < D / 8; c += 4)
      *(u4*)&img[row * XP + c * 8] = u4{0, 0, 0, 0};
  }
  if (own && tail && part == 0) mask[row] = 0;
}

// 8 halves img[kb + 8*fg + j][cb + fi], j = 0..7: the fragment of an operand
// whose reduction index runs down the rows of a linear image.
__device__ __forceinline__ h8 sl_tr(const u16* img, int pitch, int kb, int cb,
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

// Column c of a head-major workspace row -> the row of W (q | k | v order).
__device__ __forceinline__ int sl_wrow(int c, int D, int DH) {
  const int h = c / (3 * DH), rem = c - h * 3 * DH, which = rem / DH;
  return which * D + h * DH + (rem - which * DH);
}

// ------------------------------------------------------------ projection
template <int D>
__global__ __launch_bounds__(256) void sl_project_kernel(
    const u16* __restrict__ seq, const u16* __restrict__ W,
    const float* __restrict__ bias, const u16* __restrict__ g,
    u16* __restrict__ qkv, u16* __restrict__ msk, u16* __restrict__ g16,
    int64_t R, int DH) {
  constexpr int XP = D + 8, KD = D / 32;
  constexpr int NT = 3 * D / 16;     // column tiles of [q | k | v]
  constexpr int NTW = (NT + 3) / 4;  // of one wave
  __shared__ __align__(16) u16 ximg[SL_ROWS * XP];
  __shared__ __align__(16) u16 gimg[SL_ROWS * XP];
  __shared__ u16 mask[SL_ROWS];
  __shared__ u16 gmask[SL_ROWS];  // channel D of g: staged, never used
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4;
  h8 wfr[NTW][KD];
  float br[NTW];
  int dcol[NTW];  // the tile's column in the head-major row
#pragma unroll
  for (int n = 0; n < NTW; ++n) {
    const int t = wave + 4 * n;
    br[n] = t < NT ? bias[t * 16 + fi] : 0.0f;
#pragma unroll
    for (int ks = 0; ks < KD; ++ks)
      wfr[n][ks] = t < NT ? *(const h8*)&W[(t * 16 + fi) * D + ks * 32 + fg * 8]
                          : sl_zero8();
    const int which = t * 16 / D, d = t * 16 - which * D, h = d / DH;
    dcol[n] = h * 3 * DH + which * DH + (d - h * DH) + fi;
  }
  const int64_t total = R * (D + 1), ntiles = (R + SL_ROWS - 1) / SL_ROWS;
  const int64_t ts = (int64_t)blockIdx.x * ntiles / gridDim.x;
  const int64_t te = ((int64_t)blockIdx.x + 1) * ntiles / gridDim.x;
  for (int64_t t = ts; t < te; ++t) {
    const int64_t rb = t * SL_ROWS;
    const int nrows = (int)(R - rb < SL_ROWS ? R - rb : SL_ROWS);
    sl_sync();  // the last tile's readers are done
    sl_stage<D>(seq, total, rb * (D + 1), nrows, ximg, mask);
    if (g) sl_stage<D>(g, total, rb * (D + 1), nrows, gimg, gmask);
    sl_sync();
    sl_fix<D>(ximg, mask, nrows, true, wave, lane);
    if (g) sl_fix<D>(gimg, mask, nrows, false, wave, lane);
    sl_sync();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s * 16 < nrows) {
        h8 a[KD];
#pragma unroll
        for (int ks = 0; ks < KD; ++ks)
          a[ks] = *(const h8*)&ximg[(s * 16 + fi) * XP + ks * 32 + fg * 8];
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
          f4 acc = sl_zero4();
#pragma unroll
          for (int ks = 0; ks < KD; ++ks) acc = sl_mfma(a[ks], wfr[n][ks], acc);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = s * 16 + fg * 4 + r;
            if (row < nrows && wave + 4 * n < NT)
              qkv[(rb + row) * (3 * D) + dcol[n]] =
                  sl_valid(mask[row]) ? sl_f2h(acc[r] + br[n]) : (u16)0;
          }
        }
      }
    }
    if ((int)threadIdx.x < nrows) msk[rb + threadIdx.x] = mask[threadIdx.x];
    if (g) {
      for (int i = threadIdx.x; i < SL_ROWS * (D / 8); i += 256) {
        const int row = i / (D / 8), cc = i - row * (D / 8);
        if (row < nrows)
          *(u4*)&g16[(rb + row) * D + cc * 8] = *(const u4*)&gimg[row * XP + cc * 8];
      }
    }
  }
}

// ------------------------------------------------- the attention kernels
// The sample's mask (zeros from L on) and which of its 64-row tiles hold a
// valid row.  Ends in a barrier.
__device__ __forceinline__ void sl_load_mask(const u16* __restrict__ msk,
                                             int64_t row0, int L, int NT,
                                             u16* mask, int* tv, int wave,
                                             int lane) {
  for (int i = threadIdx.x; i < NT * SL_ROWS; i += 256)
    mask[i] = i < L ? msk[row0 + i] : (u16)0;
  sl_sync();
  for (int t = wave; t < SL_MAXT; t += 4) {
    const bool v = t < NT && sl_valid(mask[(t < NT ? t : 0) * SL_ROWS + lane]);
    const bool any = __builtin_amdgcn_ballot_w64(v) != 0;
    if (lane == 0) tv[t] = any ? 1 : 0;
  }
  sl_sync();
}

// the next live tile after k, or hi
__device__ __forceinline__ int sl_next(const int* tv, int k, int hi) {
  do ++k; while (k < hi && !tv[k]);
  return k;
}

// Tile t (64 rows) of head h of sample rows row0.. -> v: the 16-byte chunks
// of this thread.  QG = false: [K^h | V^h] from qkv; true: [Q^h | g^h] from
// qkv and g16.  Rows from L on are zeros.
template <int D, int DH, bool QG>
__device__ __forceinline__ void sl_gload(const u16* __restrict__ qkv,
                                         const u16* __restrict__ g16,
                                         int64_t row0, int L, int h, int t,
                                         u4 (&v)[DH / 16]) {
  constexpr int CPR = DH / 4;  // chunks of an image row of 2 DH halves
#pragma unroll
  for (int k = 0; k < DH / 16; ++k) {
    const int idx = threadIdx.x + 256 * k;
    const int row = idx / CPR, cc = idx - row * CPR, l = t * SL_ROWS + row;
    v[k] = u4{0, 0, 0, 0};
    if (l < L) {
      const u16* p;
      if (!QG) p = qkv + (row0 + l) * (3 * D) + h * 3 * DH + DH + cc * 8;
      else if (cc < DH / 8) p = qkv + (row0 + l) * (3 * D) + h * 3 * DH + cc * 8;
      else p = g16 + (row0 + l) * D + h * DH + (cc - DH / 8) * 8;
      v[k] = *(const u4*)p;
    }
  }
}

template <int DH>
__device__ __forceinline__ void sl_lstore(u16* img, const u4 (&v)[DH / 16]) {
  constexpr int CPR = DH / 4, KP = 2 * DH + 8;
#pragma unroll
  for (int k = 0; k < DH / 16; ++k) {
    const int idx = threadIdx.x + 256 * k;
    const int row = idx / CPR, cc = idx - row * CPR;
    *(u4*)&img[row * KP + cc * 8] = v[k];
  }
}

// The wave's 16 rows of a workspace as an A fragment: row l0 + fi, DH halves
// from p (the row's first) on.
template <int DH>
__device__ __forceinline__ h8 sl_afrag(const u16* __restrict__ base,
                                       int64_t pitch, int64_t row0, int l0,
                                       int L, int col, int lane) {
  const int fi = lane & 15, fg = lane >> 4;
  const bool on = l0 + fi < L && fg * 8 < DH;
  return sl_row(base + (row0 + (on ? l0 + fi : 0)) * pitch + col + fg * 8, on);
}

// c[js] = a times the rows 16 js .. of the image's columns coff .. coff + DH
template <int DH>
__device__ __forceinline__ void sl_strips(h8 a, const u16* img, int coff,
                                          int lane, f4 (&c)[4]) {
  constexpr int KP = 2 * DH + 8;
  const int fi = lane & 15, fg = lane >> 4;
#pragma unroll
  for (int js = 0; js < 4; ++js)
    c[js] = sl_mfma(a, sl_row(&img[(js * 16 + fi) * KP + coff + fg * 8],
                              fg * 8 < DH), sl_zero4());
}

// ok[r]: row l0 + 4 fg + r is valid; -> the strip has a valid row
__device__ __forceinline__ bool sl_strip_ok(const u16* mask, int l0, int fg,
                                            bool (&ok)[4]) {
  bool any = false;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    ok[r] = sl_valid(mask[l0 + fg * 4 + r]);
    any = any || ok[r];
  }
  return __builtin_amdgcn_ballot_w64(any) != 0;
}

template <int DH>
constexpr float sl_scale() {
  return DH == 16 ? 0.25f : 0.17677669529663687f;
}

template <int D, int DH>
__global__ __launch_bounds__(256) void seq_self_attn_long_fwd_kernel(
    const u16* __restrict__ seq, const u16* __restrict__ qkv,
    const u16* __restrict__ msk, u16* __restrict__ out,
    float* __restrict__ lse, int B, int L, int causal, int residual) {
  constexpr int NH = D / DH, KP = 2 * DH + 8, CT = DH / 16;
  constexpr int IMG = SL_ROWS * KP;
  constexpr float scale = sl_scale<DH>();
  __shared__ __align__(16) u16 kv[2 * IMG];
  __shared__ __align__(16) u16 pimg[4 * 16 * SL_PP];
  __shared__ u16 mask[SL_MAXL];
  __shared__ int tv[SL_MAXT];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4;
  const float ninf = -__builtin_inff();
  u16* pw = pimg + wave * 16 * SL_PP;
  const int NT = (L + SL_ROWS - 1) / SL_ROWS;
  const int64_t nitems = (int64_t)B * NT;
  const int64_t is = (int64_t)blockIdx.x * nitems / gridDim.x;
  const int64_t ie = ((int64_t)blockIdx.x + 1) * nitems / gridDim.x;
  for (int64_t it = is; it < ie; ++it) {
    const int64_t b = it / NT, row0 = b * L;
    const int qt = (int)(it - b * NT), i0 = qt * SL_ROWS + wave * 16;
    sl_sync();  // the last item's readers are done
    sl_load_mask(msk, row0, L, NT, mask, tv, wave, lane);
    bool ok[4];
    const bool live = sl_strip_ok(mask, i0, fg, ok);
    const int hi = causal ? qt + 1 : NT, first = sl_next(tv, -1, hi);
    h8 aq = sl_zero8();
    f4 O[CT];
    float m[4], l[4];
    auto init = [&](int h) {
      aq = live ? sl_afrag<DH>(qkv, 3 * D, row0, i0, L, h * 3 * DH, lane)
                : sl_zero8();
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) O[ct] = sl_zero4();
#pragma unroll
      for (int r = 0; r < 4; ++r) m[r] = ninf, l[r] = 0.0f;
    };
    // O / l (+ x) and lse of the head: every row of the strip, valid or not
    auto fini = [&](int h) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + fg * 4 + r;
        if (i < L) {
          const bool on = ok[r] && l[r] > 0.0f;
          const float inv = on ? 1.0f / l[r] : 0.0f;
          u16* row = out + (row0 + i) * (D + 1);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const int d = h * DH + ct * 16 + fi;
            float o = O[ct][r] * inv;
            if (residual && ok[r]) o += sl_h2f(seq[(row0 + i) * (D + 1) + d]);
            row[d] = ok[r] ? sl_f2h(o) : (u16)0;
          }
          if (fi == 0) {
            lse[(b * NH + h) * L + i] = on ? m[r] + logf(l[r]) : 0.0f;
            if (h == 0) row[D] = mask[i];
          }
        }
      }
    };
    if (first >= hi) {  // no key at all: no valid query row either
      for (int h = 0; h < NH; ++h) {
        init(h);
        fini(h);
      }
      continue;
    }
    int h = 0, k = first, cur = 0;
    u4 v[DH / 16];
    sl_gload<D, DH, false>(qkv, nullptr, row0, L, h, k, v);
    sl_lstore<DH>(kv, v);
    sl_sync();
    while (h < NH) {
      int k2 = sl_next(tv, k, hi), h2 = h;
      if (k2 >= hi) k2 = first, ++h2;
      const bool more = h2 < NH;
      if (more) sl_gload<D, DH, false>(qkv, nullptr, row0, L, h2, k2, v);
      if (k == first) init(h);
      if (live) {
        const u16* kb = kv + cur * IMG;
        f4 s[4];
        sl_strips<DH>(aq, kb, 0, lane, s);
        float p[4][4], mx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[r] = m[r];
#pragma unroll
        for (int js = 0; js < 4; ++js) {
          const int j = k * SL_ROWS + js * 16 + fi;
          const bool vj = sl_valid(mask[j]);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = i0 + fg * 4 + r;
            p[js][r] = vj && (!causal || j <= i) ? scale * s[js][r] : ninf;
            mx[r] = __builtin_fmaxf(mx[r], p[js][r]);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          mx[r] = sl_rowmax(mx[r], lane);
          // a row without an allowed key so far: max -inf, reference 0
          const float ref = mx[r] > ninf ? mx[r] : 0.0f;
          const float alpha = m[r] > ninf ? __expf(m[r] - ref) : 0.0f;
          m[r] = mx[r];
          float sum = 0.0f;
#pragma unroll
          for (int js = 0; js < 4; ++js) {
            p[js][r] = p[js][r] > ninf ? __expf(p[js][r] - ref) : 0.0f;
            sum += p[js][r];
          }
          l[r] = fmaf(l[r], alpha, sl_rowsum(sum, lane));
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) O[ct][r] *= alpha;
        }
        sl_wave_sync();  // the last tile's reads of pw
#pragma unroll
        for (int js = 0; js < 4; ++js) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            pw[(fg * 4 + r) * SL_PP + js * 16 + fi] = sl_f2h(p[js][r]);
        }
        sl_wave_sync();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const h8 a = *(const h8*)&pw[fi * SL_PP + ks * 32 + fg * 8];
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            O[ct] = sl_mfma(a, sl_tr(kb, KP, ks * 32, DH + ct * 16, lane), O[ct]);
        }
      }
      if (h2 != h) fini(h);
      if (more) sl_lstore<DH>(kv + (cur ^ 1) * IMG, v);
      sl_sync();
      cur ^= 1, h = h2, k = k2;
    }
  }
}

// Query-stationary backward: delta (pass 0), then dS and dQ (pass 1).
template <int D, int DH>
__global__ __launch_bounds__(256) void sl_dq_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ g16,
    const u16* __restrict__ msk, const float* __restrict__ lse,
    float* __restrict__ dz, float* __restrict__ delta, int B, int L,
    int causal) {
  constexpr int NH = D / DH, KP = 2 * DH + 8, CT = DH / 16;
  constexpr int IMG = SL_ROWS * KP, WIMG = 16 * SL_PP;
  constexpr float scale = sl_scale<DH>();
  __shared__ __align__(16) u16 kv[2 * IMG];
  __shared__ __align__(16) u16 dsimg[4 * 2 * WIMG];  // per wave: dS hi, lo
  __shared__ u16 mask[SL_MAXL];
  __shared__ int tv[SL_MAXT];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4;
  u16 *dsh = dsimg + wave * 2 * WIMG, *dsl = dsh + WIMG;
  const int NT = (L + SL_ROWS - 1) / SL_ROWS;
  const int64_t nitems = (int64_t)B * NT;
  const int64_t is = (int64_t)blockIdx.x * nitems / gridDim.x;
  const int64_t ie = ((int64_t)blockIdx.x + 1) * nitems / gridDim.x;
  for (int64_t it = is; it < ie; ++it) {
    const int64_t b = it / NT, row0 = b * L;
    const int qt = (int)(it - b * NT), i0 = qt * SL_ROWS + wave * 16;
    sl_sync();  // the last item's readers are done
    sl_load_mask(msk, row0, L, NT, mask, tv, wave, lane);
    bool ok[4];
    const bool live = sl_strip_ok(mask, i0, fg, ok);
    const int hi = causal ? qt + 1 : NT, first = sl_next(tv, -1, hi);
    h8 aq = sl_zero8(), ag = sl_zero8();
    f4 dQh[CT], dQl[CT];
    float ls[4], de[4];
    auto init = [&](int h) {
      aq = ag = sl_zero8();
      if (live) {
        aq = sl_afrag<DH>(qkv, 3 * D, row0, i0, L, h * 3 * DH, lane);
        ag = sl_afrag<DH>(g16, D, row0, i0, L, h * DH, lane);
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) dQh[ct] = dQl[ct] = sl_zero4();
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + fg * 4 + r;
        ls[r] = ok[r] ? lse[(b * NH + h) * L + i] : 0.0f;  // ok: i < L
        de[r] = 0.0f;
      }
    };
    auto fini = [&](int h) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + fg * 4 + r;
        if (i < L) {
          float* row = dz + (row0 + i) * (3 * D) + h * 3 * DH;
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            row[ct * 16 + fi] =
                ok[r] ? fmaf(dQl[ct][r], SL_LO_INV, dQh[ct][r]) : 0.0f;
          if (fi == 0) delta[(b * NH + h) * L + i] = ok[r] ? de[r] : 0.0f;
        }
      }
    };
    if (first >= hi) {
      for (int h = 0; h < NH; ++h) {
        init(h);
        fini(h);
      }
      continue;
    }
    // hv = 2 h + pass
    int hv = 0, k = first, cur = 0;
    u4 v[DH / 16];
    sl_gload<D, DH, false>(qkv, nullptr, row0, L, 0, k, v);
    sl_lstore<DH>(kv, v);
    sl_sync();
    while (hv < 2 * NH) {
      int k2 = sl_next(tv, k, hi), hv2 = hv;
      if (k2 >= hi) k2 = first, ++hv2;
      const bool more = hv2 < 2 * NH;
      if (more) sl_gload<D, DH, false>(qkv, nullptr, row0, L, hv2 >> 1, k2, v);
      if (k == first && (hv & 1) == 0) init(hv >> 1);
      if (live) {
        const u16* kb = kv + cur * IMG;
        f4 s[4], dP[4];
        sl_strips<DH>(aq, kb, 0, lane, s);
        sl_strips<DH>(ag, kb, DH, lane, dP);
        float p[4][4];
#pragma unroll
        for (int js = 0; js < 4; ++js) {
          const int j = k * SL_ROWS + js * 16 + fi;
          const bool vj = sl_valid(mask[j]);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = i0 + fg * 4 + r;
            p[js][r] = ok[r] && vj && (!causal || j <= i)
                           ? __expf(scale * s[js][r] - ls[r]) : 0.0f;
          }
        }
        if ((hv & 1) == 0) {
#pragma unroll
          for (int js = 0; js < 4; ++js) {
#pragma unroll
            for (int r = 0; r < 4; ++r) de[r] = fmaf(p[js][r], dP[js][r], de[r]);
          }
        } else {
          sl_wave_sync();  // the last tile's reads of the images
#pragma unroll
          for (int js = 0; js < 4; ++js) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int o = (fg * 4 + r) * SL_PP + js * 16 + fi;
              sl_split(scale * p[js][r] * (dP[js][r] - de[r]), dsh[o], dsl[o]);
            }
          }
          sl_wave_sync();
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const h8 ah = *(const h8*)&dsh[fi * SL_PP + ks * 32 + fg * 8];
            const h8 al = *(const h8*)&dsl[fi * SL_PP + ks * 32 + fg * 8];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
              const h8 bk = sl_tr(kb, KP, ks * 32, ct * 16, lane);
              dQh[ct] = sl_mfma(ah, bk, dQh[ct]);
              dQl[ct] = sl_mfma(al, bk, dQl[ct]);
            }
          }
        }
      }
      if (hv2 != hv) {
        if ((hv & 1) == 0) {
#pragma unroll
          for (int r = 0; r < 4; ++r) de[r] = sl_rowsum(de[r], lane);
        } else {
          fini(hv >> 1);
        }
      }
      if (more) sl_lstore<DH>(kv + (cur ^ 1) * IMG, v);
      sl_sync();
      cur ^= 1, hv = hv2, k = k2;
    }
  }
}

// Key-stationary backward: dK and dV of the wave's key strip.
template <int D, int DH>
__global__ __launch_bounds__(256) void sl_dkv_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ g16,
    const u16* __restrict__ msk, const float* __restrict__ lse,
    const float* __restrict__ delta, float* __restrict__ dz, int B, int L,
    int causal) {
  constexpr int NH = D / DH, KP = 2 * DH + 8, CT = DH / 16;
  constexpr int IMG = SL_ROWS * KP, WIMG = 16 * SL_PP;
  constexpr float scale = sl_scale<DH>();
  __shared__ __align__(16) u16 qg[2 * IMG];
  __shared__ __align__(16) u16 wimg[4 * 3 * WIMG];  // per wave: P^T, dS^T hi, lo
  __shared__ float aux[2 * 2 * SL_ROWS];  // per image: lse, delta of its rows
  __shared__ u16 mask[SL_MAXL];
  __shared__ int tv[SL_MAXT];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4;
  u16 *pT = wimg + wave * 3 * WIMG, *dsh = pT + WIMG, *dsl = dsh + WIMG;
  const int NT = (L + SL_ROWS - 1) / SL_ROWS;
  const int64_t nitems = (int64_t)B * NT;
  const int64_t is = (int64_t)blockIdx.x * nitems / gridDim.x;
  const int64_t ie = ((int64_t)blockIdx.x + 1) * nitems / gridDim.x;
  for (int64_t it = is; it < ie; ++it) {
    const int64_t b = it / NT, row0 = b * L;
    const int kt = (int)(it - b * NT), j0 = kt * SL_ROWS + wave * 16;
    sl_sync();  // the last item's readers are done
    sl_load_mask(msk, row0, L, NT, mask, tv, wave, lane);
    bool ok[4];
    const bool live = sl_strip_ok(mask, j0, fg, ok);
    const int lo = causal ? kt : 0, first = sl_next(tv, lo - 1, NT);
    h8 ak = sl_zero8(), av = sl_zero8();
    f4 dKh[CT], dKl[CT], dV[CT];
    auto init = [&](int h) {
      ak = av = sl_zero8();
      if (live) {
        ak = sl_afrag<DH>(qkv, 3 * D, row0, j0, L, h * 3 * DH + DH, lane);
        av = sl_afrag<DH>(qkv, 3 * D, row0, j0, L, h * 3 * DH + 2 * DH, lane);
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) dKh[ct] = dKl[ct] = dV[ct] = sl_zero4();
    };
    auto fini = [&](int h) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + fg * 4 + r;
        if (j < L) {
          float* row = dz + (row0 + j) * (3 * D) + h * 3 * DH + DH;
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            row[ct * 16 + fi] =
                ok[r] ? fmaf(dKl[ct][r], SL_LO_INV, dKh[ct][r]) : 0.0f;
            row[DH + ct * 16 + fi] = ok[r] ? dV[ct][r] : 0.0f;
          }
        }
      }
    };
    if (first >= NT) {
      for (int h = 0; h < NH; ++h) {
        init(h);
        fini(h);
      }
      continue;
    }
    // lse (threads 0..63) and delta (64..127) of the tile's rows
    auto aload = [&](int h, int t) -> float {
      const int x = threadIdx.x, l = t * SL_ROWS + (x & 63);
      if (x >= 2 * SL_ROWS || l >= L) return 0.0f;
      return (x < SL_ROWS ? lse : delta)[(b * NH + h) * L + l];
    };
    int h = 0, k = first, cur = 0;
    u4 v[DH / 16];
    sl_gload<D, DH, true>(qkv, g16, row0, L, h, k, v);
    float ax = aload(h, k);
    sl_lstore<DH>(qg, v);
    if (threadIdx.x < 2 * SL_ROWS) aux[threadIdx.x] = ax;
    sl_sync();
    while (h < NH) {
      int k2 = sl_next(tv, k, NT), h2 = h;
      if (k2 >= NT) k2 = first, ++h2;
      const bool more = h2 < NH;
      if (more) {
        sl_gload<D, DH, true>(qkv, g16, row0, L, h2, k2, v);
        ax = aload(h2, k2);
      }
      if (k == first) init(h);
      if (live) {
        const u16* qb = qg + cur * IMG;
        const float* xb = aux + cur * 2 * SL_ROWS;
        f4 st[4], dpt[4];  // [key 4 fg + r][query 16 is + fi]
        sl_strips<DH>(ak, qb, 0, lane, st);
        sl_strips<DH>(av, qb, DH, lane, dpt);
        sl_wave_sync();  // the last tile's reads of the images
#pragma unroll
        for (int qs = 0; qs < 4; ++qs) {
          const int i = k * SL_ROWS + qs * 16 + fi;
          const bool vi = sl_valid(mask[i]);
          const float li = xb[qs * 16 + fi], di = xb[SL_ROWS + qs * 16 + fi];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = j0 + fg * 4 + r;
            const float p = vi && ok[r] && (!causal || j <= i)
                                ? __expf(scale * st[qs][r] - li) : 0.0f;
            const int o = (fg * 4 + r) * SL_PP + qs * 16 + fi;
            pT[o] = sl_f2h(p);
            sl_split(scale * p * (dpt[qs][r] - di), dsh[o], dsl[o]);
          }
        }
        sl_wave_sync();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int o = fi * SL_PP + ks * 32 + fg * 8;
          const h8 ap = *(const h8*)&pT[o];
          const h8 ah = *(const h8*)&dsh[o];
          const h8 al = *(const h8*)&dsl[o];
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const h8 bq = sl_tr(qb, KP, ks * 32, ct * 16, lane);
            dKh[ct] = sl_mfma(ah, bq, dKh[ct]);
            dKl[ct] = sl_mfma(al, bq, dKl[ct]);
            dV[ct] = sl_mfma(ap, sl_tr(qb, KP, ks * 32, DH + ct * 16, lane),
                             dV[ct]);
          }
        }
      }
      if (h2 != h) fini(h);
      if (more) {
        sl_lstore<DH>(qg + (cur ^ 1) * IMG, v);
        if (threadIdx.x < 2 * SL_ROWS) aux[(cur ^ 1) * 2 * SL_ROWS + threadIdx.x] = ax;
      }
      sl_sync();
      cur ^= 1, h = h2, k = k2;
    }
  }
}

// ---------------------------------------------------- projection backward
// Partials of one block, f32: [dW 3D*D][db 3D].
template <int D>
__global__ __launch_bounds__(256) void sl_project_bwd_kernel(
    const u16* __restrict__ seq, const u16* __restrict__ W,
    const float* __restrict__ dz, const u16* __restrict__ g,
    u16* __restrict__ dseq, float* __restrict__ part, int64_t R, int DH,
    int residual) {
  constexpr int XP = D + 8, KD = D / 32;
  constexpr int NDT = D / 16;        // column tiles of D
  constexpr int SPLIT = 4 / NDT;     // waves that share one of them
  constexpr int NS = 4 / SPLIT;      // strips of a wave
  constexpr int NA = NDT / SPLIT;    // dW tiles of a wave and chunk
  constexpr int C4 = D / 4;          // float4 of a chunk row
  __shared__ __align__(16) u16 ximg[SL_ROWS * XP];
  __shared__ __align__(16) u16 zimg[2 * SL_ROWS * XP];  // the chunk's hi, lo
  __shared__ u16 mask[SL_ROWS];
  static_assert(256 * 16 <= 2 * SL_ROWS * XP * 2, "db's sums overlay zimg");
  u16 *zh = zimg, *zl = zimg + SL_ROWS * XP;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4;
  const int dt = wave % NDT, grp = wave / NDT;
  // fragments of W for dX: chunk q covers the columns q D .. of a dz row;
  // reduction down the rows of W, column dt*16 + fi
  h8 wx[3][KD];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int ks = 0; ks < KD; ++ks) {
      const int wr = sl_wrow(q * D + ks * 32 + fg * 8, D, DH);
      h8 f;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        f[j] = __builtin_bit_cast(_Float16, W[(wr + j) * D + dt * 16 + fi]);
      wx[q][ks] = f;
    }
  }
  f4 dWa[3][NA], dba[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    dba[q] = sl_zero4();
#pragma unroll
    for (int a = 0; a < NA; ++a) dWa[q][a] = sl_zero4();
  }
  const int64_t total = R * (D + 1), ntiles = (R + SL_ROWS - 1) / SL_ROWS;
  const int64_t ts = (int64_t)blockIdx.x * ntiles / gridDim.x;
  const int64_t te = ((int64_t)blockIdx.x + 1) * ntiles / gridDim.x;
  for (int64_t t = ts; t < te; ++t) {
    const int64_t rb = t * SL_ROWS;
    const int nrows = (int)(R - rb < SL_ROWS ? R - rb : SL_ROWS);
    sl_sync();  // the last tile's readers are done
    sl_stage<D>(seq, total, rb * (D + 1), nrows, ximg, mask);
    sl_sync();
    sl_fix<D>(ximg, mask, nrows, true, wave, lane);
    sl_sync();
    f4 xh[NS], xl[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) xh[n] = xl[n] = sl_zero4();
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (q > 0) sl_sync();  // the last chunk's readers
#pragma unroll
      for (int k = 0; k < SL_ROWS * C4 / 256; ++k) {
        const int idx = threadIdx.x + 256 * k;
        const int row = idx / C4, c4 = idx - row * C4;
        f4 z = sl_zero4();
        if (row < nrows && sl_valid(mask[row]))
          z = *(const f4*)&dz[(rb + row) * (3 * D) + q * D + c4 * 4];
        dba[q] += z;
        s4 hi4, lo4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          u16 a, c;
          sl_split(z[e], a, c);
          hi4[e] = a, lo4[e] = c;
        }
        *(s4*)&zh[row * XP + c4 * 4] = hi4;
        *(s4*)&zl[row * XP + c4 * 4] = lo4;
      }
      sl_sync();
#pragma unroll
      for (int n = 0; n < NS; ++n) {
        const int s = n * SPLIT + grp;
        if (s * 16 < nrows) {
#pragma unroll
          for (int ks = 0; ks < KD; ++ks) {
            const int o = (s * 16 + fi) * XP + ks * 32 + fg * 8;
            xh[n] = sl_mfma(*(const h8*)&zh[o], wx[q][ks], xh[n]);
            xl[n] = sl_mfma(*(const h8*)&zl[o], wx[q][ks], xl[n]);
          }
        }
      }
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int ci = a * SPLIT + grp;
        f4 ch = sl_zero4(), cl = ch;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          if (ks * 32 < nrows) {
            const h8 bx = sl_tr(ximg, XP, ks * 32, dt * 16, lane);
            ch = sl_mfma(sl_tr(zh, XP, ks * 32, ci * 16, lane), bx, ch);
            cl = sl_mfma(sl_tr(zl, XP, ks * 32, ci * 16, lane), bx, cl);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dWa[q][a][r] += fmaf(cl[r], SL_LO_INV, ch[r]);
      }
    }
    // dseq: the rows of the wave's strips, column dt*16 + fi
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      const int s = n * SPLIT + grp, d = dt * 16 + fi;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = s * 16 + fg * 4 + r;
        if (row < nrows) {
          const bool ok = sl_valid(mask[row]);
          float v = fmaf(xl[n][r], SL_LO_INV, xh[n][r]);
          if (residual && ok) v += sl_h2f(g[(rb + row) * (D + 1) + d]);
          u16* o = dseq + (rb + row) * (D + 1);
          o[d] = ok ? sl_f2h(v) : (u16)0;
          if (dt == 0 && fi == 0) o[D] = 0;
        }
      }
    }
  }
  // the block's partial
  float* p = part + (int64_t)blockIdx.x * (3 * D * D + 3 * D);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int wr = sl_wrow(q * D + (a * SPLIT + grp) * 16 + fg * 4, D, DH);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        p[(wr + r) * D + dt * 16 + fi] = dWa[q][a][r];
    }
  }
  // db: a thread's sums belong to the columns 4 (x % C4) .. of its chunk; the
  // 256 / C4 threads of a column are summed in thread order
  f4* red = (f4*)zimg;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    sl_sync();
    red[threadIdx.x] = dba[q];
    sl_sync();
    if (threadIdx.x < D) {
      const int c4 = threadIdx.x / 4, e = threadIdx.x % 4;
      float acc = 0.0f;
      for (int i = 0; i < 256 / C4; ++i) acc += red[i * C4 + c4][e];
      p[3 * D * D + sl_wrow(q * D + threadIdx.x, D, DH)] = acc;
    }
  }
}

// out[i] = sum over the blocks' partials, in block order
__global__ __launch_bounds__(256) void sl_reduce_kernel(
    const float* __restrict__ part, float* __restrict__ out, int nblk, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float acc = 0.0f;
  for (int k = 0; k < nblk; ++k) acc += part[(int64_t)k * n + i];
  out[i] = acc;
}

// ----------------------------------------------------------------- host
bool sl_feasible(int64_t L, int64_t D, int64_t heads) {
  if (!(D == 32 || D == 64) || heads < 1 || D % heads != 0) return false;
  const int64_t dh = D / heads;
  return (dh == 16 || dh == 32) && L >= 1 && L <= SL_MAXL;
}

hipStream_t sl_stream() { return at::hip::getCurrentHIPStream().stream(); }

bool sl_is(const torch::Tensor& t, const torch::Tensor& like,
           c10::ScalarType st) {
  return t.is_cuda() && t.device() == like.device() && t.scalar_type() == st &&
         t.is_contiguous();
}

// raises on anything the kernels do not take
void sl_check(const torch::Tensor& seq, const torch::Tensor& W,
              const torch::Tensor& bias, int64_t heads, int64_t max_blocks,
              const char* who) {
  TORCH_CHECK(seq.is_cuda(), who, ": seq must be on a GPU");
  TORCH_CHECK(sl_is(seq, seq, torch::kFloat16) && sl_is(W, seq, torch::kFloat16),
              who, ": seq and Wqkv must be contiguous float16 on one GPU");
  TORCH_CHECK(sl_is(bias, seq, torch::kFloat32), who,
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
  TORCH_CHECK(sl_feasible(L, D, heads), who, ": no kernel for L=", L, " D=", D,
              " heads=", heads, " (seq_self_attn_long_feasible)");
  TORCH_CHECK(max_blocks >= 0, who, ": max_blocks must be >= 0");
}

// the grid of a persistent kernel over `items`, `per_cu` blocks per CU
int sl_grid(int64_t items, int64_t max_blocks, int per_cu) {
  int64_t grid =
      max_blocks > 0
          ? max_blocks
          : per_cu * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  return (int)(grid < items ? grid : items);
}

#define SL_P16(t) (const u16*)(t).data_ptr()
#define SL_P32(t) (const float*)(t).data_ptr()
#define SL_CASE(DD, DHH, ...)    \
  if (D == DD && DH == DHH)      \
    return [&] { constexpr int kD = DD, kDH = DHH; __VA_ARGS__; }();
#define SL_DISPATCH(...)                                  \
  SL_CASE(32, 16, __VA_ARGS__) SL_CASE(32, 32, __VA_ARGS__) \
  SL_CASE(64, 16, __VA_ARGS__) SL_CASE(64, 32, __VA_ARGS__)

struct SlWork {
  torch::Tensor qkv, msk, g16;
};

// [q | k | v] of every row (and g with its invalid rows zeroed) -> workspaces
SlWork sl_project(const torch::Tensor& seq, const torch::Tensor& W,
                  const torch::Tensor& bias, const torch::Tensor* g, int DH,
                  int64_t max_blocks) {
  const int64_t B = seq.size(0), L = seq.size(1), D = seq.size(2) - 1;
  SlWork w;
  w.qkv = torch::empty({B, L, 3 * D}, seq.options());
  w.msk = torch::empty({B, L}, seq.options());
  if (g) w.g16 = torch::empty({B, L, D}, seq.options());
  const int64_t R = B * L;
  const int grid = sl_grid((R + SL_ROWS - 1) / SL_ROWS, max_blocks, 2);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, sl_stream(),
                       SL_P16(seq), SL_P16(W), SL_P32(bias),
                       g ? SL_P16(*g) : (const u16*)nullptr,
                       (u16*)w.qkv.data_ptr(), (u16*)w.msk.data_ptr(),
                       g ? (u16*)w.g16.data_ptr() : (u16*)nullptr, R, DH);
  };
  if (D == 32) go(sl_project_kernel<32>);
  else go(sl_project_kernel<64>);
  return w;
}

void sl_launch_fwd(int D, int DH, int grid, const torch::Tensor& seq,
                   const SlWork& w, torch::Tensor& out, torch::Tensor& lse,
                   bool causal, bool residual) {
  const int B = (int)seq.size(0), L = (int)seq.size(1);
  SL_DISPATCH(hipLaunchKernelGGL(
      (seq_self_attn_long_fwd_kernel<kD, kDH>), dim3(grid), dim3(256), 0,
      sl_stream(), SL_P16(seq), SL_P16(w.qkv), SL_P16(w.msk),
      (u16*)out.data_ptr(), (float*)lse.data_ptr(), B, L, (int)causal,
      (int)residual))
  TORCH_CHECK(false, "seq_self_attn_long_fwd: no instance for D=", D, " dh=", DH);
}

void sl_launch_dq(int D, int DH, int grid, const SlWork& w,
                  const torch::Tensor& lse, torch::Tensor& dz,
                  torch::Tensor& delta, int B, int L, bool causal) {
  SL_DISPATCH(hipLaunchKernelGGL(
      (sl_dq_kernel<kD, kDH>), dim3(grid), dim3(256), 0, sl_stream(),
      SL_P16(w.qkv), SL_P16(w.g16), SL_P16(w.msk), SL_P32(lse),
      (float*)dz.data_ptr(), (float*)delta.data_ptr(), B, L, (int)causal))
  TORCH_CHECK(false, "seq_self_attn_long_bwd: no instance for D=", D, " dh=", DH);
}

void sl_launch_dkv(int D, int DH, int grid, const SlWork& w,
                   const torch::Tensor& lse, const torch::Tensor& delta,
                   torch::Tensor& dz, int B, int L, bool causal) {
  SL_DISPATCH(hipLaunchKernelGGL(
      (sl_dkv_kernel<kD, kDH>), dim3(grid), dim3(256), 0, sl_stream(),
      SL_P16(w.qkv), SL_P16(w.g16), SL_P16(w.msk), SL_P32(lse), SL_P32(delta),
      (float*)dz.data_ptr(), B, L, (int)causal))
  TORCH_CHECK(false, "seq_self_attn_long_bwd: no instance for D=", D, " dh=", DH);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool seq_self_attn_long_feasible(int64_t L, int64_t D, int64_t heads) {
  return sl_feasible(L, D, heads);
}

std::vector<torch::Tensor> seq_self_attn_long_fwd(
    torch::Tensor seq, torch::Tensor W, torch::Tensor bias, int64_t heads,
    bool causal, bool residual, int64_t max_blocks) {
  sl_check(seq, W, bias, heads, max_blocks, "seq_self_attn_long_fwd");
  const int64_t B = seq.size(0), L = seq.size(1), D = seq.size(2) - 1;
  auto out = torch::empty_like(seq);
  auto lse = torch::empty({B, heads, L}, bias.options());
  if (B == 0) return {out, lse};
  const int DH = (int)(D / heads);
  const SlWork w = sl_project(seq, W, bias, nullptr, DH, max_blocks);
  const int grid = sl_grid(B * ((L + SL_ROWS - 1) / SL_ROWS), max_blocks, 4);
  sl_launch_fwd((int)D, DH, grid, seq, w, out, lse, causal, residual);
  return {out, lse};
}

std::vector<torch::Tensor> seq_self_attn_long_bwd(
    torch::Tensor g, torch::Tensor seq, torch::Tensor W, torch::Tensor bias,
    torch::Tensor lse, int64_t heads, bool causal, bool residual,
    int64_t max_blocks) {
  sl_check(seq, W, bias, heads, max_blocks, "seq_self_attn_long_bwd");
  TORCH_CHECK(sl_is(g, seq, torch::kFloat16) && g.sizes() == seq.sizes(),
              "seq_self_attn_long_bwd: g must be a contiguous float16 "
              "[B, L, D+1] beside seq");
  const int64_t B = seq.size(0), L = seq.size(1), D = seq.size(2) - 1;
  TORCH_CHECK(sl_is(lse, seq, torch::kFloat32) && lse.dim() == 3 &&
                  lse.size(0) == B && lse.size(1) == heads && lse.size(2) == L,
              "seq_self_attn_long_bwd: lse must be a contiguous float32 "
              "[B, heads, L] beside seq");
  const int64_t n = 3 * D * D + 3 * D;
  auto dseq = torch::empty_like(seq);
  auto sums = torch::zeros({n}, bias.options());
  if (B > 0) {
    const int DH = (int)(D / heads);
    const SlWork w = sl_project(seq, W, bias, &g, DH, max_blocks);
    auto dz = torch::empty({B, L, 3 * D}, bias.options());
    auto delta = torch::empty({B, heads, L}, bias.options());
    const int grid = sl_grid(B * ((L + SL_ROWS - 1) / SL_ROWS), max_blocks, 2);
    sl_launch_dq((int)D, DH, grid, w, lse, dz, delta, (int)B, (int)L, causal);
    sl_launch_dkv((int)D, DH, grid, w, lse, delta, dz, (int)B, (int)L, causal);
    const int64_t R = B * L;
    const int pgrid = sl_grid((R + SL_ROWS - 1) / SL_ROWS, max_blocks, 2);
    auto part = torch::empty({(int64_t)pgrid, n}, bias.options());
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(pgrid), dim3(256), 0, sl_stream(),
                         SL_P16(seq), SL_P16(W), SL_P32(dz), SL_P16(g),
                         (u16*)dseq.data_ptr(), (float*)part.data_ptr(), R, DH,
                         (int)residual);
    };
    if (D == 32) go(sl_project_bwd_kernel<32>);
    else go(sl_project_bwd_kernel<64>);
    hipLaunchKernelGGL(sl_reduce_kernel, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, sl_stream(), (const float*)part.data_ptr(),
                       (float*)sums.data_ptr(), pgrid, (int)n);
  }
  return {dseq, sums.narrow(0, 0, 3 * D * D).view({3 * D, D}),
          sums.narrow(0, 3 * D * D, 3 * D)};
}

void init_seqsal(pybind11::module_& m) {
  namespace py = pybind11;
  m.def("seq_self_attn_long_feasible", &seq_self_attn_long_feasible,
        "true if the streamed-key self-attention kernels take (L, D, heads)");
  m.def("seq_self_attn_long_fwd", &seq_self_attn_long_fwd,
        "multi-head self-attention among the rows of a raw slot, keys "
        "streamed -> (out [B, L, D+1], lse [B, heads, L])",
        py::arg("seq"), py::arg("Wqkv"), py::arg("bqkv"), py::arg("heads"),
        py::arg("causal") = false, py::arg("residual") = false,
        py::arg("max_blocks") = 0);
  m.def("seq_self_attn_long_bwd", &seq_self_attn_long_bwd,
        "streamed-key self-attention backward -> (dseq, dWqkv, dbqkv)",
        py::arg("g"), py::arg("seq"), py::arg("Wqkv"), py::arg("bqkv"),
        py::arg("lse"), py::arg("heads"), py::arg("causal") = false,
        py::arg("residual") = false, py::arg("max_blocks") = 0);
}
