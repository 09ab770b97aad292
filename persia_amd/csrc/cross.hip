// DCN-v2 low-rank cross layer on MFMA (gfx950 / CDNA4, wave64), forward and
// backward.  One layer is
//
//   h   = bf16(x_l V^T)                       [B, r]   V [r, D]
//   out = bf16(x0 * (h U^T + b) + x_l)        [B, D]   U [D, r], b [D] f32
//
// a GEMM -> GEMM -> elementwise chain over a narrow [rows, r <= 256]
// intermediate.  Every kernel here gives a block 64 rows and the FULL rank, so
// the intermediate lives in LDS between the two GEMMs and the projection
// h U^T + b never exists in memory:
//
//   cross_fwd     phase 1 streams x_l and V in K-chunks of 64 through a
//                 double-buffered global_load_lds pipeline into the h
//                 accumulators; h is rounded once into an LDS tile (and written
//                 out for the backward); phase 2 walks 64-column tiles of U with
//                 K = r read entirely from that tile and applies
//                 x0 * (acc + b) + x_l in the epilogue.
//   cross_bwd_dh  dp = bf16(g * x0) is formed on the way into LDS, written out
//                 once (the dU wgrad operand), column-summed per wave into one
//                 partial row each (db), and multiplied into dh = bf16(dp U).
//   cross_bwd_dx  the h and dh row tiles sit whole in LDS; per 32-column tile
//                 two GEMMs (dh V and h U^T) run into two accumulator sets and
//                 the epilogue writes g_l = bf16(g + dh V) and
//                 dx0 = bf16(dx0_in + g * (h U^T + b)); on layer 0 the f32
//                 g + dh V is added into dx0 before its one rounding.
//   cross_db_reduce sums the partial rows in a fixed order (no atomics).
//
// All GEMMs are the NT form C = A B^T with both operands K-contiguous, so the
// two backward operands that reduce over a weight's leading dim take a
// contiguous transpose (U^T [r, D] for dh, V^T [D, r] for dh V) that the
// caller makes once per call from the bf16 weight image.
//
// mfma_f32_16x16x32_bf16 fragment maps as in dense.hip.  256 threads = 2 x 2
// waves; a wave owns 32 rows x half the columns of the tile at hand.  A row's
// results depend on that row's operands only (rows past the batch are clamped
// duplicates of the last row and never stored).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) short;

constexpr int CR_BM = 64;  // rows per block

__device__ __forceinline__ float cr_bf2f(short x) {
  union { float f; unsigned u; } v;
  v.u = ((unsigned)(unsigned short)x) << 16;
  return v.f;
}

__device__ __forceinline__ short cr_f2bf(float f) {
  union { float f; unsigned u; } v;
  v.f = f;
  const unsigned lsb = (v.u >> 16) & 1;
  v.u += 0x7fff + lsb;  // round-to-nearest-even
  return (short)(v.u >> 16);
}

__device__ __forceinline__ void cr_wait_barrier() {
  // staged tiles landed (vmcnt), LDS traffic of this step retired (lgkmcnt)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---- K-chunk images: [rows][64] shorts, 128 B per row, as gemm_nt_glds_kernel.
// LDS granule (16 B) gl of row holds logical granule gl ^ (row & 7); the XOR is
// applied to the SOURCE address here and to the fragment read below.  One glds
// chunk is 8 rows (64 lanes x 16 B); wave w takes chunks w, w + 4, ...
// A tail step (K - k0 == 32) points the upper four logical granules 32 columns
// back: in bounds, and never read (the MFMA loop runs one half-step there).
__device__ __forceinline__ void cr_stage_k(const short* __restrict__ src,
                                           int row0, int row_max, int ld,
                                           int k0, int K, short* dst,
                                           int n_chunks, int wave, int lane) {
  const int s_rl = lane >> 3;
  int kc = k0 + (((lane & 7) ^ s_rl) << 3);
  if (kc >= K) kc -= 32;
  for (int c = wave; c < n_chunks; c += 4) {
    const int srow = min(row0 + c * 8 + s_rl, row_max);
    __builtin_amdgcn_global_load_lds(
        (const uint32_t*)(src + (int64_t)srow * ld + kc),
        (uint32_t*)(dst + c * 512), 16, 0, 0);
  }
}

__device__ __forceinline__ bf16x8 cr_frag_k(const short* img, int row, int gr) {
  return *(const bf16x8*)&img[row * 64 + ((gr ^ (row & 7)) << 3)];
}

// ---- full-rank images: [rows][r] shorts, a row is r/8 granules.  LDS granule
// gl of row holds logical granule gl ^ (row & sw), sw = 7 when r % 64 == 0
// (the XOR stays inside an aligned group of 8 granules) and 3 otherwise
// (groups of 4: r % 32 == 0).  A tile of consecutive rows of a [*, r] matrix is
// contiguous in memory, so staging is a flat copy in 1 KB chunks with the XOR
// on the source granule.  CrMap holds a thread's (row, source column) for the
// chunks wave + 4 i; it depends on r only, so it is built once per kernel.
template <int NCH>
struct CrMap {
  int row[NCH], off[NCH];
};

template <int NCH>
__device__ __forceinline__ CrMap<NCH> cr_map(int r8, int sw, int wave,
                                             int lane) {
  CrMap<NCH> m;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int p = (wave + i * 4) * 64 + lane;
    const int row = p / r8, gl = p - row * r8;
    m.row[i] = row;
    m.off[i] = (gl ^ (row & sw)) << 3;
  }
  return m;
}

// rows [row0, row0 + n_chunks * 512 / r) of src ([*, r], rows clamped to
// row_max) -> dst
template <int NCH>
__device__ __forceinline__ void cr_stage_r(const short* __restrict__ src,
                                           int row0, int row_max, int r,
                                           short* dst, int n_chunks,
                                           const CrMap<NCH>& m, int wave) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = wave + i * 4;
    if (c < n_chunks) {
      const int srow = min(row0 + m.row[i], row_max);
      __builtin_amdgcn_global_load_lds(
          (const uint32_t*)(src + (int64_t)srow * r + m.off[i]),
          (uint32_t*)(dst + c * 512), 16, 0, 0);
    }
  }
}

__device__ __forceinline__ bf16x8 cr_frag_r(const short* img, int row, int gr,
                                            int r, int sw) {
  return *(const bf16x8*)&img[row * r + ((gr ^ (row & sw)) << 3)];
}

__device__ __forceinline__ int cr_elem_r(int row, int col, int r, int sw) {
  return row * r + ((((col >> 3) ^ (row & sw)) << 3) | (col & 7));
}

// acc[am][bn] += A[32 rows of wave row wr] @ B[rows wc * half + bn * 16 ..]^T
// over one K-chunk image pair (nk half-steps of 32).
template <int NB>
__device__ __forceinline__ void cr_mma_k(f32x4 (&acc)[2][NB], const short* ia,
                                         const short* ib, int nk, int nb,
                                         int wr, int bcol0, int fi, int g16) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    if (kk < nk) {
      const bf16x8 a0 = cr_frag_k(ia, wr * 32 + fi, kk * 4 + g16);
      const bf16x8 a1 = cr_frag_k(ia, wr * 32 + 16 + fi, kk * 4 + g16);
#pragma unroll
      for (int bn = 0; bn < NB; ++bn) {
        if (bn < nb) {
          const bf16x8 bf = cr_frag_k(ib, bcol0 + bn * 16 + fi, kk * 4 + g16);
          acc[0][bn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, bf,
                                                               acc[0][bn], 0, 0, 0);
          acc[1][bn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, bf,
                                                               acc[1][bn], 0, 0, 0);
        }
      }
    }
  }
}

// ------------------------------------------------------------------ forward
// RMAX: the rank the instantiation is sized for (r <= RMAX; LDS and the h
// accumulators scale with it).  LDS: stg = 2 x (64 + RMAX) x 64 shorts (phase
// 1: x_l and V K-chunks; phase 2: two U tiles of 64 x r), hts = 64 x RMAX.
template <int RMAX>
__global__ __launch_bounds__(256) void cross_fwd_kernel(
    const short* __restrict__ x0, const short* __restrict__ xl,
    const short* __restrict__ V, const short* __restrict__ U,
    const float* __restrict__ b, short* __restrict__ out,
    short* __restrict__ h_out, int M, int D, int r) {
  constexpr int NB = RMAX / 32;
  constexpr int STG = (CR_BM + RMAX) * 64;
  __shared__ __align__(16) short stg[2 * STG];
  __shared__ __align__(16) short hts[CR_BM * RMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, fi = lane & 15, g16 = lane >> 4;
  const int r8 = r >> 3, sw = (r & 63) ? 3 : 7, nb = r >> 5, half = r >> 1;
  const int m0 = blockIdx.x * CR_BM;

  // phase 1: h = x_l V^T
  f32x4 acc[2][NB] = {};
  auto stage1 = [&](int bufi, int k0) {
    short* s = stg + bufi * STG;
    cr_stage_k(xl, m0, M - 1, D, k0, D, s, CR_BM / 8, wave, lane);
    cr_stage_k(V, 0, r - 1, D, k0, D, s + CR_BM * 64, r8, wave, lane);
  };
  stage1(0, 0);
  cr_wait_barrier();
  int buf = 0;
  for (int k0 = 0; k0 < D; k0 += 64) {
    if (k0 + 64 < D) stage1(buf ^ 1, k0 + 64);
    const short* s = stg + buf * STG;
    cr_mma_k<NB>(acc, s, s + CR_BM * 64, (D - k0 >= 64) ? 2 : 1, nb, wr,
                 wc * half, fi, g16);
    cr_wait_barrier();
    buf ^= 1;
  }

  // h: one rounding, into the LDS tile and out for the backward
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int bn = 0; bn < NB; ++bn) {
      if (bn < nb) {
        const int col = wc * half + bn * 16 + fi;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = wr * 32 + am * 16 + g16 * 4 + q;
          const short hv = cr_f2bf(acc[am][bn][q]);
          hts[cr_elem_r(row, col, r, sw)] = hv;
          if (m0 + row < M) h_out[(int64_t)(m0 + row) * r + col] = hv;
        }
      }
    }

  // phase 2: out = x0 * (h U^T + b) + x_l over 64-column tiles of U
  const CrMap<NB> map = cr_map<NB>(r8, sw, wave, lane);
  const int n_tiles = (D + 63) / 64;
  cr_stage_r<NB>(U, 0, D - 1, r, stg, r8, map, wave);
  cr_wait_barrier();  // also publishes hts
  buf = 0;
  for (int t = 0; t < n_tiles; ++t) {
    const int n0 = t * 64;
    if (t + 1 < n_tiles)
      cr_stage_r<NB>(U, n0 + 64, D - 1, r, stg + (buf ^ 1) * CR_BM * RMAX, r8,
                     map, wave);
    const short* ub = stg + buf * CR_BM * RMAX;
    f32x4 c2[2][2] = {};
    for (int ks = 0; ks < nb; ++ks) {
      const int gr = ks * 4 + g16;
      const bf16x8 a0 = cr_frag_r(hts, wr * 32 + fi, gr, r, sw);
      const bf16x8 a1 = cr_frag_r(hts, wr * 32 + 16 + fi, gr, r, sw);
#pragma unroll
      for (int bn = 0; bn < 2; ++bn) {
        const bf16x8 bf = cr_frag_r(ub, wc * 32 + bn * 16 + fi, gr, r, sw);
        c2[0][bn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, bf, c2[0][bn],
                                                            0, 0, 0);
        c2[1][bn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, bf, c2[1][bn],
                                                            0, 0, 0);
      }
    }
#pragma unroll
    for (int am = 0; am < 2; ++am)
#pragma unroll
      for (int bn = 0; bn < 2; ++bn) {
        const int col = n0 + wc * 32 + bn * 16 + fi;
        if (col < D) {
          const float bval = b[col];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int row = m0 + wr * 32 + am * 16 + g16 * 4 + q;
            if (row < M) {
              const int64_t idx = (int64_t)row * D + col;
              const float v = cr_bf2f(x0[idx]) * (c2[am][bn][q] + bval) +
                              cr_bf2f(xl[idx]);
              out[idx] = cr_f2bf(v);
            }
          }
        }
      }
    cr_wait_barrier();
    buf ^= 1;
  }
}

// --------------------------------------------------------------- backward: dh
// dp = bf16(g * x0) -> LDS K-chunk image (register staged: it is computed),
// global dp, per-wave column sums; dh = bf16(dp Ut^T), Ut [r, D].
// part: [gridDim.x * 4, D] f32, row blockIdx.x * 4 + wave holds the column sums
// of the wave's 16 rows (rows past M are zero in the image).
template <int RMAX>
__global__ __launch_bounds__(256) void cross_bwd_dh_kernel(
    const short* __restrict__ g, const short* __restrict__ x0,
    const short* __restrict__ Ut, short* __restrict__ dp,
    short* __restrict__ dh, float* __restrict__ part, int M, int D, int r) {
  constexpr int NB = RMAX / 32;
  __shared__ __align__(16) short sa[2][CR_BM * 64];
  __shared__ __align__(16) short sb[2][RMAX * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, fi = lane & 15, g16 = lane >> 4;
  const int r8 = r >> 3, nb = r >> 5, half = r >> 1;
  const int m0 = blockIdx.x * CR_BM;

  // a thread forms granule gl of rows a_row and a_row + 32; both rows share
  // row & 7, hence the logical granule
  const int a_row = tid >> 3, a_gl = tid & 7;
  const int a_col = (a_gl ^ (a_row & 7)) << 3;
  auto load_a = [&](int k0, bf16x8 (&gv)[2], bf16x8 (&xv)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      gv[i] = bf16x8{};
      xv[i] = bf16x8{};
      const int row = m0 + a_row + i * 32;
      if (row < M && k0 + a_col < D) {
        const int64_t idx = (int64_t)row * D + k0 + a_col;
        gv[i] = *(const bf16x8*)(g + idx);
        xv[i] = *(const bf16x8*)(x0 + idx);
      }
    }
  };
  auto write_a = [&](int bufi, int k0, const bf16x8 (&gv)[2],
                     const bf16x8 (&xv)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      bf16x8 pv;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        pv[j] = cr_f2bf(cr_bf2f(gv[i][j]) * cr_bf2f(xv[i][j]));
      *(bf16x8*)&sa[bufi][(a_row + i * 32) * 64 + a_gl * 8] = pv;
      const int row = m0 + a_row + i * 32;
      if (row < M && k0 + a_col < D)
        *(bf16x8*)(dp + (int64_t)row * D + k0 + a_col) = pv;
    }
  };

  f32x4 acc[2][NB] = {};
  {
    bf16x8 gv[2], xv[2];
    load_a(0, gv, xv);
    cr_stage_k(Ut, 0, r - 1, D, 0, D, sb[0], r8, wave, lane);
    write_a(0, 0, gv, xv);
  }
  cr_wait_barrier();
  int buf = 0;
  float* prow = part + (int64_t)(blockIdx.x * 4 + wave) * D;
  for (int k0 = 0; k0 < D; k0 += 64) {
    const bool nxt = k0 + 64 < D;
    bf16x8 gv[2], xv[2];
    if (nxt) {
      cr_stage_k(Ut, 0, r - 1, D, k0 + 64, D, sb[buf ^ 1], r8, wave, lane);
      load_a(k0 + 64, gv, xv);
    }
    {  // db partial: column k0 + lane over the wave's 16 rows, in row order
      float s = 0.0f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int row = wave * 16 + j;
        s += cr_bf2f(
            sa[buf][row * 64 + ((((lane >> 3) ^ (row & 7)) << 3) | (lane & 7))]);
      }
      if (k0 + lane < D) prow[k0 + lane] = s;
    }
    cr_mma_k<NB>(acc, sa[buf], sb[buf], (D - k0 >= 64) ? 2 : 1, nb, wr,
                 wc * half, fi, g16);
    if (nxt) write_a(buf ^ 1, k0 + 64, gv, xv);
    cr_wait_barrier();
    buf ^= 1;
  }
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int bn = 0; bn < NB; ++bn) {
      if (bn < nb) {
        const int col = wc * half + bn * 16 + fi;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = m0 + wr * 32 + am * 16 + g16 * 4 + q;
          if (row < M) dh[(int64_t)row * r + col] = cr_f2bf(acc[am][bn][q]);
        }
      }
    }
}

// db[c] (+)= sum over the partial rows in a fixed order: a block takes 32
// columns x 8 slices of consecutive rows, a slice adds its rows in row order,
// and the eight slice sums are added in slice order (no atomics; one thread
// per column walking all P rows left the grid at D / 256 blocks).
__global__ __launch_bounds__(256) void cross_db_reduce_kernel(
    const float* __restrict__ part, int P, int D, float* __restrict__ db,
    int accum) {
  __shared__ float red[8][32];
  const int cl = threadIdx.x & 31, s = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const int per = (P + 7) / 8;
  const int p1 = min(P, (s + 1) * per);
  float v = 0.0f;
  if (c < D)
    for (int p = s * per; p < p1; ++p) v += part[(int64_t)p * D + c];
  red[s][cl] = v;
  __syncthreads();
  if (s == 0 && c < D) {
    float t = red[0][cl];
#pragma unroll
    for (int i = 1; i < 8; ++i) t += red[i][cl];
    db[c] = accum ? db[c] + t : t;
  }
}

// --------------------------------------------------------------- backward: dx
// Per 32-column tile n0: acc1 = dh Vt[n0..]^T (Vt [D, r]), acc2 = h U[n0..]^T.
//   g_out = bf16(g + acc1)                               (not on layer 0)
//   dx0   = bf16(dx0_in + g * (acc2 + b) [+ (g + acc1)])  ([..] on layer 0)
// LDS: th, tdh = 64 x RMAX each; wt = 2 buffers x (Vt tile | U tile) x 32 x RMAX.
template <int RMAX>
__global__ __launch_bounds__(256) void cross_bwd_dx_kernel(
    const short* __restrict__ g, const short* __restrict__ dh,
    const short* __restrict__ h, const short* __restrict__ Vt,
    const short* __restrict__ U, const float* __restrict__ b,
    const short* __restrict__ dx0_in, short* __restrict__ g_out,
    short* __restrict__ dx0, int M, int D, int r, int last) {
  constexpr int NB = RMAX / 32;
  constexpr int WT = 32 * RMAX;
  __shared__ __align__(16) short th[CR_BM * RMAX];
  __shared__ __align__(16) short tdh[CR_BM * RMAX];
  __shared__ __align__(16) short wt[4 * WT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, fi = lane & 15, g16 = lane >> 4;
  const int r8 = r >> 3, sw = (r & 63) ? 3 : 7, nb = r >> 5;
  const int m0 = blockIdx.x * CR_BM;
  const CrMap<NB> map = cr_map<NB>(r8, sw, wave, lane);

  auto stage_w = [&](int bufi, int n0) {
    cr_stage_r<NB>(Vt, n0, D - 1, r, wt + bufi * 2 * WT, r8 / 2, map, wave);
    cr_stage_r<NB>(U, n0, D - 1, r, wt + bufi * 2 * WT + WT, r8 / 2, map, wave);
  };
  cr_stage_r<NB>(h, m0, M - 1, r, th, r8, map, wave);
  cr_stage_r<NB>(dh, m0, M - 1, r, tdh, r8, map, wave);
  stage_w(0, 0);
  cr_wait_barrier();
  int buf = 0;
  for (int n0 = 0; n0 < D; n0 += 32) {
    if (n0 + 32 < D) stage_w(buf ^ 1, n0 + 32);
    const short* wv = wt + buf * 2 * WT;
    const short* wu = wv + WT;
    f32x4 acc1[2] = {}, acc2[2] = {};
    for (int ks = 0; ks < nb; ++ks) {
      const int gr = ks * 4 + g16;
      const bf16x8 bv = cr_frag_r(wv, wc * 16 + fi, gr, r, sw);
      const bf16x8 bu = cr_frag_r(wu, wc * 16 + fi, gr, r, sw);
#pragma unroll
      for (int am = 0; am < 2; ++am) {
        const int row = wr * 32 + am * 16 + fi;
        acc1[am] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            cr_frag_r(tdh, row, gr, r, sw), bv, acc1[am], 0, 0, 0);
        acc2[am] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            cr_frag_r(th, row, gr, r, sw), bu, acc2[am], 0, 0, 0);
      }
    }
    const int col = n0 + wc * 16 + fi;  // < D: D % 32 == 0
    const float bval = b[col];
#pragma unroll
    for (int am = 0; am < 2; ++am)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = m0 + wr * 32 + am * 16 + g16 * 4 + q;
        if (row < M) {
          const int64_t idx = (int64_t)row * D + col;
          const float gf = cr_bf2f(g[idx]);
          const float gl = gf + acc1[am][q];
          float t = gf * (acc2[am][q] + bval);
          if (dx0_in) t += cr_bf2f(dx0_in[idx]);
          if (last) t += gl;
          else g_out[idx] = cr_f2bf(gl);
          dx0[idx] = cr_f2bf(t);
        }
      }
    cr_wait_barrier();
    buf ^= 1;
  }
}

// ------------------------------------------------------------------ host side

hipStream_t cr_stream() { return at::hip::getCurrentHIPStream().stream(); }

bool cr_feasible(int64_t D, int64_t r) {
  return D >= 32 && D % 32 == 0 && r % 32 == 0 && r >= 32 && r <= 256;
}

void cr_check_rows(const torch::Tensor& t, const torch::Tensor& like,
                   int64_t rows, int64_t cols, const char* who,
                   const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), who, ": ", name,
              " must be on x0's device");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, who, ": ", name,
              " must be bfloat16");
  TORCH_CHECK(t.is_contiguous(), who, ": ", name, " must be contiguous");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == cols, who,
              ": ", name, " must be [", rows, ", ", cols, "]");
}

void cr_check_bias(const torch::Tensor& b, const torch::Tensor& like, int64_t D,
                   const char* who) {
  TORCH_CHECK(b.is_cuda() && b.device() == like.device() &&
                  b.scalar_type() == torch::kFloat32 && b.is_contiguous() &&
                  b.dim() == 1 && b.size(0) == D,
              who, ": b must be a contiguous float32 [", D, "] on x0's device");
}

// x0 [B, D] and the rank -> (B, D), after the checks every launcher shares
void cr_check_x0(const torch::Tensor& x0, int64_t r, const char* who) {
  TORCH_CHECK(x0.is_cuda(), who, ": x0 must be a CUDA tensor");
  TORCH_CHECK(x0.scalar_type() == torch::kBFloat16, who,
              ": x0 must be bfloat16");
  TORCH_CHECK(x0.dim() == 2 && x0.is_contiguous(), who,
              ": x0 must be a contiguous [B, D]");
  TORCH_CHECK(cr_feasible(x0.size(1), r), who, ": no kernel for D=", x0.size(1),
              " r=", r, " (cross_feasible)");
  TORCH_CHECK(x0.size(0) <= (int64_t)INT32_MAX - CR_BM, who,
              ": batch too large");
}

#define CR_DISPATCH(r, KERNEL, ...)                                      \
  do {                                                                   \
    if ((r) <= 64) hipLaunchKernelGGL(KERNEL<64>, __VA_ARGS__);          \
    else if ((r) <= 128) hipLaunchKernelGGL(KERNEL<128>, __VA_ARGS__);   \
    else hipLaunchKernelGGL(KERNEL<256>, __VA_ARGS__);                   \
  } while (0)

}  // namespace

bool cross_feasible(int64_t D, int64_t r) { return cr_feasible(D, r); }

// One cross layer: (x0, x_l, V [r, D], U [D, r], b [D]) -> (x_{l+1}, h).
std::vector<torch::Tensor> cross_fwd(torch::Tensor x0, torch::Tensor xl,
                                     torch::Tensor V, torch::Tensor U,
                                     torch::Tensor b) {
  const char* who = "cross_fwd";
  TORCH_CHECK(V.dim() == 2, who, ": V must be [r, D]");
  const int64_t r = V.size(0);
  cr_check_x0(x0, r, who);
  const int64_t B = x0.size(0), D = x0.size(1);
  cr_check_rows(xl, x0, B, D, who, "xl");
  cr_check_rows(V, x0, r, D, who, "V");
  cr_check_rows(U, x0, D, r, who, "U");
  cr_check_bias(b, x0, D, who);
  auto out = torch::empty_like(x0);
  auto h = torch::empty({B, r}, x0.options());
  if (B == 0) return {out, h};
  const int grid = (int)((B + CR_BM - 1) / CR_BM);
  CR_DISPATCH(r, cross_fwd_kernel, dim3(grid), dim3(256), 0, cr_stream(),
              (const short*)x0.data_ptr(), (const short*)xl.data_ptr(),
              (const short*)V.data_ptr(), (const short*)U.data_ptr(),
              b.data_ptr<float>(), (short*)out.data_ptr(),
              (short*)h.data_ptr(), (int)B, (int)D, (int)r);
  return {out, h};
}

// (g, x0, Ut [r, D]) -> (dp = bf16(g * x0), dh = bf16(dp U), partial column
// sums of dp [4 * ceil(B / 64), D] for cross_db_reduce).
std::vector<torch::Tensor> cross_bwd_dh(torch::Tensor g, torch::Tensor x0,
                                        torch::Tensor Ut) {
  const char* who = "cross_bwd_dh";
  TORCH_CHECK(Ut.dim() == 2, who, ": Ut must be [r, D]");
  const int64_t r = Ut.size(0);
  cr_check_x0(x0, r, who);
  const int64_t B = x0.size(0), D = x0.size(1);
  cr_check_rows(g, x0, B, D, who, "g");
  cr_check_rows(Ut, x0, r, D, who, "Ut");
  const int grid = (int)((B + CR_BM - 1) / CR_BM);
  auto dp = torch::empty_like(x0);
  auto dh = torch::empty({B, r}, x0.options());
  auto part = torch::empty({(int64_t)grid * 4, D},
                           x0.options().dtype(torch::kFloat32));
  if (B == 0) return {dp, dh, part};
  CR_DISPATCH(r, cross_bwd_dh_kernel, dim3(grid), dim3(256), 0, cr_stream(),
              (const short*)g.data_ptr(), (const short*)x0.data_ptr(),
              (const short*)Ut.data_ptr(), (short*)dp.data_ptr(),
              (short*)dh.data_ptr(), part.data_ptr<float>(), (int)B, (int)D,
              (int)r);
  return {dp, dh, part};
}

static void cr_db_reduce(const torch::Tensor& part, torch::Tensor& db,
                         int accum, const char* who) {
  TORCH_CHECK(part.is_cuda() && part.scalar_type() == torch::kFloat32 &&
                  part.is_contiguous() && part.dim() == 2,
              who, ": part must be a contiguous CUDA float32 [P, D]");
  const int64_t P = part.size(0), D = part.size(1);
  TORCH_CHECK(db.is_cuda() && db.device() == part.device() &&
                  db.scalar_type() == torch::kFloat32 && db.is_contiguous() &&
                  db.numel() == D,
              who, ": db must be a contiguous float32 of ", D,
              " elements on part's device");
  TORCH_CHECK(P <= INT32_MAX && D <= INT32_MAX, who, ": part too large");
  if (D == 0) return;
  hipLaunchKernelGGL(cross_db_reduce_kernel, dim3((unsigned)((D + 31) / 32)),
                     dim3(256), 0, cr_stream(), part.data_ptr<float>(), (int)P,
                     (int)D, db.data_ptr<float>(), accum);
}

// db [D] = column sums of the partial rows, added in row order.
torch::Tensor cross_db_reduce(torch::Tensor part) {
  TORCH_CHECK(part.dim() == 2, "cross_db_reduce: part must be [P, D]");
  auto db = torch::empty({part.size(1)}, part.options());
  cr_db_reduce(part, db, 0, "cross_db_reduce");
  return db;
}

// Side-band form: the same sum ADDED to `out` (a flat f32 gradient slot).
void cross_db_reduce_into(torch::Tensor part, torch::Tensor out) {
  cr_db_reduce(part, out, 1, "cross_db_reduce_into");
}

// (g, dh, h, Vt [D, r], U [D, r], b, dx0_in or an empty tensor, last)
// -> (g_l, dx0); g_l is an empty tensor when last (layer 0), where g + dh V is
// folded into dx0 instead.
std::vector<torch::Tensor> cross_bwd_dx(torch::Tensor g, torch::Tensor dh,
                                        torch::Tensor h, torch::Tensor Vt,
                                        torch::Tensor U, torch::Tensor b,
                                        torch::Tensor dx0_in, bool last) {
  const char* who = "cross_bwd_dx";
  TORCH_CHECK(U.dim() == 2, who, ": U must be [D, r]");
  const int64_t r = U.size(1);
  cr_check_x0(g, r, who);
  const int64_t B = g.size(0), D = g.size(1);
  cr_check_rows(dh, g, B, r, who, "dh");
  cr_check_rows(h, g, B, r, who, "h");
  cr_check_rows(Vt, g, D, r, who, "Vt");
  cr_check_rows(U, g, D, r, who, "U");
  cr_check_bias(b, g, D, who);
  const bool has_in = dx0_in.dim() == 2;  // absent: any 1-D (empty) tensor
  if (has_in) cr_check_rows(dx0_in, g, B, D, who, "dx0_in");
  auto dx0 = torch::empty_like(g);
  auto g_out = last ? torch::empty({0}, g.options()) : torch::empty_like(g);
  if (B == 0) return {g_out, dx0};
  const int grid = (int)((B + CR_BM - 1) / CR_BM);
  CR_DISPATCH(r, cross_bwd_dx_kernel, dim3(grid), dim3(256), 0, cr_stream(),
              (const short*)g.data_ptr(), (const short*)dh.data_ptr(),
              (const short*)h.data_ptr(), (const short*)Vt.data_ptr(),
              (const short*)U.data_ptr(), b.data_ptr<float>(),
              has_in ? (const short*)dx0_in.data_ptr() : nullptr,
              last ? nullptr : (short*)g_out.data_ptr(),
              (short*)dx0.data_ptr(), (int)B, (int)D, (int)r, last ? 1 : 0);
  return {g_out, dx0};
}

void init_cross(pybind11::module_& m) {
  m.def("cross_feasible", &cross_feasible,
        "true if the fused cross-layer kernels take (D, r)");
  m.def("cross_fwd", &cross_fwd,
        "DCN-v2 low-rank cross layer forward -> (x_next, h)");
  m.def("cross_bwd_dh", &cross_bwd_dh,
        "cross layer backward, first half -> (dp, dh, db partial rows)");
  m.def("cross_db_reduce", &cross_db_reduce,
        "ordered sum of cross_bwd_dh's partial rows -> db");
  m.def("cross_db_reduce_into", &cross_db_reduce_into,
        "ordered sum of cross_bwd_dh's partial rows, added to a f32 slot");
  m.def("cross_bwd_dx", &cross_bwd_dx,
        "cross layer backward, second half -> (g_l, dx0)");
}
