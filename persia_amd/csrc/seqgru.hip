// GRU / AUGRU over a raw slot's sequence (gfx950): DIEN's interest layers and
// GRU4Rec-style encoders on the (B, sample_fixed_size, dim+1) layout.
//
//   seq [B, L, D+1] f16: channels 0..D-1 the row x_t, channel D the 0/1 mask
//   Wx [3H, D], Wh [3H, H] f16 (the f16 roundings of the f32 masters), gate
//   order (r, z, n) as in torch.nn.GRU;  bx, bh [3H] f32;  att [B, L] f32 or
//   none (a_t = 1)
//   valid t:   r = sig(Wx_r x + bx_r + Wh_r h + bh_r),  z alike,
//              n = tanh(Wx_n x + bx_n + r (Wh_n h + bh_n)),
//              h_t = h + a_t (1 - z)(n - h)
//   invalid t: h_t = h_{t-1}
//   states [B, L, H] f16 = every h_t;  last [B, H] f16 = h_{L-1}
//
// Work split.  One block owns 16 consecutive samples -- the M of the MFMA --
// and walks t for them; it has H/16 waves, wave w owns the hidden units
// [16w, 16w+16) of all three gates, so a unit's gate arithmetic and its f32
// master state never leave the wave (accumulator layout: lane = unit fi,
// samples 4*fg .. 4*fg+3).  The wave's column tiles of Wx and Wh are MFMA
// B-fragments held in registers for the whole kernel; LDS holds activations
// only.  The grid is ceil(B/16): small batches underfill the device.
//
// Staging.  Per sample a chunk of T consecutive steps is contiguous in seq
// (T (D+1) halves); the block reads it as aligned 32-bit words (words across
// the chunk's or the tensor's end half by half from the part inside, as
// au_stage does) into an image [sample][step][D+8], mask column into an array
// of its own, then zeroes the invalid rows: the mask SELECTS.  T = 8, and 4
// at D = 128 so that two images stay below 64 KB of LDS.  In forward the loads
// of chunk c+1 are spread over the steps of chunk c -- issued at the top of a
// step, written to the second image at its end -- rather than held in
// registers all at once (at D = 128, H = 32 that would be 65 registers).
//
// Forward.  gx_t = Wx x_t + bx does not depend on h: all T steps of a chunk
// are computed up front as independent MFMAs into registers.  The serial step
// is 3 H/32 MFMAs on the f16 image of h, the gate epilogue, the update of the
// f32 master h, the f16 copy into the other h image and into states, and one
// barrier.
//
// Backward (BPTT) walks t down with dh in registers and recomputes the gates
// from x_t and h_{t-1} = states[t-1].  The four gate gradients (da_r, da_z,
// da_n, dgh_n) are f32 in the accumulator layout, which IS the A-fragment
// layout of mfma_f32_16x16x16_f16 with the 16 samples as reduction index: the
// weight gradients dWx += dgx^T x_t, dWh += dgh^T h_{t-1} take them from
// registers, and x_t / h_{t-1} by ds_read_b64_tr_b16 from the linear images.
// dh_{t-1} = dh (1 - a(1-z)) + dgh Wh and dx_t = dgx Wx read the gate
// gradients back from an LDS image and the weights, in the transposed role,
// from a second register copy.  Every gate gradient is used as hi + lo*2^-11
// (two f16 values, as actunit.hip stages dh): a single f16 image cannot hold
// the f32 bounds of the weight gradients (at L = 1 nothing but f32 rounding
// separates the references).  Images are double (h: triple) buffered so a
// step has one barrier.
//
// Order.  Sums run in a fixed order that depends on the sample alone; the
// weight and bias gradients stay in registers over the block's steps, go out
// as one partial per block and are summed in block order.  No atomics.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <optional>
#include <tuple>

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

using u16 = unsigned short;
using h8 = __attribute__((ext_vector_type(8))) _Float16;
using hf4 = __attribute__((ext_vector_type(4))) _Float16;
using h4 = __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16;
using f4 = __attribute__((ext_vector_type(4))) float;
using u4 = __attribute__((ext_vector_type(4))) unsigned int;
using OptT = std::optional<torch::Tensor>;

constexpr float SG_LO = 2048.0f;  // scale of the low half of a gate gradient
constexpr float SG_LO_INV = 1.0f / 2048.0f;

template <int D, int NT>
struct SgGeom {
  static constexpr int T = D > 64 ? 4 : 8;    // steps per chunk (even)
  static constexpr int W = D + 1;             // pitch of seq
  static constexpr int KP = D + 8;            // pitch of an image row
  static constexpr int XS = T * KP + 8;       // pitch of a sample's rows
  static constexpr int NWS = T * W / 2 + 1;   // 32-bit words of a chunk, at most
  // words per thread and step when a chunk is staged in T portions
  static constexpr int PER = (16 * NWS + T * NT - 1) / (T * NT);
};

__device__ __forceinline__ float sg_h2f(u16 x) {
  return (float)__builtin_bit_cast(_Float16, x);
}

__device__ __forceinline__ u16 sg_f2h(float f) {  // round to nearest even
  return __builtin_bit_cast(u16, (_Float16)f);
}

__device__ __forceinline__ void sg_sync() {  // what __syncthreads() does
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float sg_shfl(float v, int src_lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src_lane << 2,
                                          __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ bool sg_valid(u16 mask) {  // != 0, -0 is zero
  return (mask & 0x7fff) != 0;
}

__device__ __forceinline__ float sg_sigmoid(float v) {
  return 1.0f / (1.0f + __expf(-v));
}

__device__ __forceinline__ float sg_tanh(float v) {
  return 2.0f / (1.0f + __expf(-2.0f * v)) - 1.0f;
}

__device__ __forceinline__ f4 sg_splat(float v) { return f4{v, v, v, v}; }

// Portion p (of T) of the chunk [t0, t0 + T) of the block's 16 samples: the
// loads.  Item i = (sample, word of the sample's chunk); a word is read only
// where it overlaps the sample's rows, and never outside the tensor.
template <int D, int NT>
__device__ __forceinline__ void sg_stage_load(
    const u16* __restrict__ seq, int64_t total, int64_t b0, int B, int L,
    int t0, int p, uint32_t (&v)[SgGeom<D, NT>::PER]) {
  using G = SgGeom<D, NT>;
  const int nst = L - t0 < G::T ? L - t0 : G::T;
  const uintptr_t tb = (uintptr_t)seq, te = tb + 2 * (uintptr_t)total;
#pragma unroll
  for (int j = 0; j < G::PER; ++j) {
    const int i = (p * G::PER + j) * NT + (int)threadIdx.x;
    const int s = i / G::NWS, wd = i - s * G::NWS;
    v[j] = 0;
    if (s < 16 && b0 + s < B) {
      const uintptr_t a0 =
          tb + 2 * (uintptr_t)(((b0 + s) * L + t0) * (int64_t)G::W);
      const uintptr_t a1 = a0 + 2 * (uintptr_t)(nst * G::W);
      const uintptr_t ca = (a0 & ~(uintptr_t)3) + 4 * (uintptr_t)wd;
      if (ca < a1) {
        if (ca >= tb && ca + 4 <= te) {
          v[j] = *(const uint32_t*)ca;
        } else {  // a word across the tensor's own end: the half inside
          if (ca >= tb && ca < te) v[j] = *(const u16*)ca;
          if (ca + 2 >= tb && ca + 2 < te)
            v[j] |= (uint32_t)(*(const u16*)(ca + 2)) << 16;
        }
      }
    }
  }
}

// ... and the scatter of the same words into the image and the mask array.
// Portion 0 also fills what no word of seq reaches: mask 0 for the cells past
// B or L, and the chunk's attention weights (1 without att).
template <int D, int NT>
__device__ __forceinline__ void sg_stage_store(
    const u16* __restrict__ seq, const float* __restrict__ att, int64_t b0,
    int B, int L, int t0, int p, const uint32_t (&v)[SgGeom<D, NT>::PER],
    u16* ximg, u16* mk, float* ac) {
  using G = SgGeom<D, NT>;
  const int nst = L - t0 < G::T ? L - t0 : G::T;
  const uintptr_t tb = (uintptr_t)seq;
#pragma unroll
  for (int j = 0; j < G::PER; ++j) {
    const int i = (p * G::PER + j) * NT + (int)threadIdx.x;
    const int s = i / G::NWS, wd = i - s * G::NWS;
    if (s < 16 && b0 + s < B) {
      const uintptr_t a0 =
          tb + 2 * (uintptr_t)(((b0 + s) * L + t0) * (int64_t)G::W);
      const uintptr_t a1 = a0 + 2 * (uintptr_t)(nst * G::W);
      const uintptr_t ca = (a0 & ~(uintptr_t)3) + 4 * (uintptr_t)wd;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const uintptr_t a = ca + 2 * e;
        if (a >= a0 && a < a1) {
          const int hx = (int)((a - a0) / 2);
          const int row = hx / G::W, col = hx - row * G::W;
          const u16 x = (u16)(v[j] >> (16 * e));
          if (col < D) ximg[s * G::XS + row * G::KP + col] = x;
          else mk[s * G::T + row] = x;
        }
      }
    }
  }
  if (p == 0) {
    for (int idx = threadIdx.x; idx < 16 * G::T; idx += NT) {
      const int s = idx / G::T, tt = idx - s * G::T;
      const bool in = b0 + s < B && t0 + tt < L;
      if (!in) mk[idx] = 0;
      ac[idx] = in && att != nullptr ? att[(b0 + s) * L + t0 + tt] : 1.0f;
    }
  }
}

// Invalid rows of the image (and the rows past B or L) become zeros.
template <int D, int NT>
__device__ __forceinline__ void sg_fix(u16* ximg, const u16* mk) {
  using G = SgGeom<D, NT>;
  constexpr int C = D / 8;
  for (int idx = threadIdx.x; idx < 16 * G::T * C; idx += NT) {
    const int row = idx / C, c = idx - row * C;
    if (!sg_valid(mk[row])) {
      const int s = row / G::T, tt = row - s * G::T;
      *(u4*)&ximg[s * G::XS + tt * G::KP + c * 8] = u4{0, 0, 0, 0};
    }
  }
}

// 4 halves img[4*fg + j][cb + fi], j = 0..3: the mfma_16x16x16 fragment of an
// operand whose reduction index (the sample) runs down the rows of a linear
// image.  Lane m of a 16-lane group addresses the slot (row m/4, 4*(m%4));
// the group's slots form a 4 x 16 block and lane m receives its column m.
__device__ __forceinline__ hf4 sg_tr(const u16* img, int pitch, int cb,
                                     int lane) {
  const u16* b0 = img + ((lane >> 4) * 4 + ((lane & 15) >> 2)) * pitch + cb +
                  (lane & 3) * 4;
  const h4 v = __builtin_amdgcn_ds_read_tr16_b64_v4f16(
      (__attribute__((address_space(3))) h4*)(void*)const_cast<u16*>(b0));
  return __builtin_bit_cast(hf4, v);
}

template <int HT, int DK>
__global__ __launch_bounds__(64 * HT) void seq_gru_fwd_kernel(
    const u16* __restrict__ seq, const u16* __restrict__ Wx,
    const u16* __restrict__ Wh, const float* __restrict__ bx,
    const float* __restrict__ bh, const float* __restrict__ att,
    u16* __restrict__ states, u16* __restrict__ last, int B, int L) {
  constexpr int H = HT * 16, D = DK * 32, NT = 64 * HT, HK = H / 32;
  constexpr int HP = H + 8;
  using G = SgGeom<D, NT>;
  constexpr int T = G::T, KP = G::KP, XS = G::XS;
  __shared__ __align__(16) u16 ximg[2][16 * XS];
  __shared__ __align__(16) u16 himg[2][16 * HP];
  __shared__ u16 mk[2][16 * T];
  __shared__ float ac[2][16 * T];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4;
  const int u = 16 * wave + fi;  // the lane's hidden unit
  // the wave's column tiles of the weights, for the whole kernel
  h8 wxf[3][DK], whf[3][HK];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int ks = 0; ks < DK; ++ks)
      wxf[g][ks] = *(const h8*)&Wx[(g * H + u) * D + ks * 32 + fg * 8];
#pragma unroll
    for (int ks = 0; ks < HK; ++ks)
      whf[g][ks] = *(const h8*)&Wh[(g * H + u) * H + ks * 32 + fg * 8];
  }
  const float b_r = bx[u] + bh[u], b_z = bx[H + u] + bh[H + u];
  const float b_nx = bx[2 * H + u], b_nh = bh[2 * H + u];
  const int64_t b0 = (int64_t)blockIdx.x * 16;
  const int64_t total = (int64_t)B * L * (D + 1);
  for (int i = threadIdx.x; i < 16 * HP / 8; i += NT)  // h_{-1} = 0
    *(u4*)&himg[0][i * 8] = u4{0, 0, 0, 0};
  float hm[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // the f32 master state
  uint32_t v[G::PER];
  for (int p = 0; p < T; ++p) {
    sg_stage_load<D, NT>(seq, total, b0, B, L, 0, p, v);
    sg_stage_store<D, NT>(seq, att, b0, B, L, 0, p, v, ximg[0], mk[0], ac[0]);
  }
  sg_sync();
  const int nchunks = (L + T - 1) / T;
  for (int c = 0; c < nchunks; ++c) {
    const int cur = c & 1, t0 = c * T;
    const int nst = L - t0 < T ? L - t0 : T;
    const bool more = c + 1 < nchunks;  // then nst == T
    sg_fix<D, NT>(ximg[cur], mk[cur]);
    sg_sync();
    // gx of the chunk's steps: nothing here waits for h
    f4 gx[T][3];
#pragma unroll
    for (int tt = 0; tt < T; ++tt) {
      gx[tt][0] = sg_splat(b_r);
      gx[tt][1] = sg_splat(b_z);
      gx[tt][2] = sg_splat(b_nx);
#pragma unroll
      for (int ks = 0; ks < DK; ++ks) {
        const h8 xa =
            *(const h8*)&ximg[cur][fi * XS + tt * KP + ks * 32 + fg * 8];
#pragma unroll
        for (int g = 0; g < 3; ++g)
          gx[tt][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
              xa, wxf[g][ks], gx[tt][g], 0, 0, 0);
      }
    }
#pragma unroll
    for (int tt = 0; tt < T; ++tt) {
      if (tt < nst) {
        const int hb = tt & 1;  // t0 is even
        if (more) sg_stage_load<D, NT>(seq, total, b0, B, L, t0 + T, tt, v);
        f4 ar = gx[tt][0], az = gx[tt][1], an = sg_splat(b_nh);
#pragma unroll
        for (int ks = 0; ks < HK; ++ks) {
          const h8 ha = *(const h8*)&himg[hb][fi * HP + ks * 32 + fg * 8];
          ar = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, whf[0][ks], ar, 0, 0, 0);
          az = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, whf[1][ks], az, 0, 0, 0);
          an = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, whf[2][ks], an, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s = 4 * fg + r;
          const bool ok = sg_valid(mk[cur][s * T + tt]);
          const float a = ac[cur][s * T + tt];
          const float rr = sg_sigmoid(ar[r]), zz = sg_sigmoid(az[r]);
          const float nn = sg_tanh(fmaf(rr, an[r], gx[tt][2][r]));
          const float hn = fmaf(a, (1.0f - zz) * (nn - hm[r]), hm[r]);
          hm[r] = ok ? hn : hm[r];
          const u16 hv = sg_f2h(hm[r]);
          himg[hb ^ 1][s * HP + u] = hv;
          if (b0 + s < B) states[((b0 + s) * L + t0 + tt) * H + u] = hv;
        }
        if (more)
          sg_stage_store<D, NT>(seq, att, b0, B, L, t0 + T, tt, v, ximg[cur ^ 1],
                                mk[cur ^ 1], ac[cur ^ 1]);
        sg_sync();
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int s = 4 * fg + r;
    if (b0 + s < B) last[(b0 + s) * H + u] = sg_f2h(hm[r]);
  }
}

// Partials of one block, f32: [dWx 3H*D][dWh 3H*H][dbx 3H][dbh 3H].
template <int HT, int DK>
__global__ __launch_bounds__(64 * HT) void seq_gru_bwd_kernel(
    const u16* __restrict__ g_states, const u16* __restrict__ g_last,
    const u16* __restrict__ seq, const u16* __restrict__ states,
    const u16* __restrict__ Wx, const u16* __restrict__ Wh,
    const u16* __restrict__ WxT, const float* __restrict__ bx,
    const float* __restrict__ bh, const float* __restrict__ att,
    u16* __restrict__ dseq, float* __restrict__ datt,
    float* __restrict__ part, int B, int L) {
  constexpr int H = HT * 16, D = DK * 32, NT = 64 * HT, HK = H / 32;
  constexpr int HP = H + 8, DT = D / 16;
  constexpr int NDX = (DT + HT - 1) / HT;  // dx column tiles of a wave
  constexpr int GP = 4 * H + 8;  // gate-gradient image: da_r|da_z|da_n|dgh_n
  constexpr int GK = 3 * HK;     // 32-wide steps over the 3H gate units
  constexpr int HC = H / 8;      // 16-byte pieces of a state row
  // Wx in the transposed role lives in registers, except at H = 64, D = 128
  // where the register file cannot hold it beside the accumulators: there the
  // fragments are 16-byte loads of WxT [D, 3H] in every step (48 KB, cached)
  constexpr bool XREG = !(HT == 4 && DK == 4);
  constexpr int NXR = XREG ? NDX : 1;
  using G = SgGeom<D, NT>;
  constexpr int T = G::T, KP = G::KP, XS = G::XS;
  __shared__ __align__(16) u16 ximg[16 * XS];
  __shared__ __align__(16) u16 himg[3][16 * HP];
  __shared__ __align__(16) u16 dgh[2][16 * GP];
  __shared__ __align__(16) u16 dgl[2][16 * GP];
  __shared__ u16 mk[16 * T];
  __shared__ float ac[16 * T];
  __shared__ float dap[2][HT * 16];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int fi = lane & 15, fg = lane >> 4;
  const int u = 16 * wave + fi;
  const int64_t b0 = (int64_t)blockIdx.x * 16;
  const int64_t total = (int64_t)B * L * (D + 1);
  // forward role: the wave's column tiles; transposed role: rows = gate
  // units down the reduction, columns = the wave's hidden units / dx tiles
  h8 wxf[3][DK], whf[3][HK], whT[GK], wxT[NXR][GK];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int ks = 0; ks < DK; ++ks)
      wxf[g][ks] = *(const h8*)&Wx[(g * H + u) * D + ks * 32 + fg * 8];
#pragma unroll
    for (int ks = 0; ks < HK; ++ks)
      whf[g][ks] = *(const h8*)&Wh[(g * H + u) * H + ks * 32 + fg * 8];
  }
#pragma unroll
  for (int kk = 0; kk < GK; ++kk) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = kk * 32 + fg * 8 + j;
      whT[kk][j] = __builtin_bit_cast(_Float16, Wh[row * H + u]);
      if constexpr (XREG) {
#pragma unroll
        for (int n = 0; n < NDX; ++n) {
          const int dt = wave + HT * n;
          wxT[n][kk][j] = dt < DT
              ? __builtin_bit_cast(_Float16, Wx[row * D + dt * 16 + fi])
              : (_Float16)0.0f;
        }
      }
    }
  }
  const float b_r = bx[u] + bh[u], b_z = bx[H + u] + bh[H + u];
  const float b_nx = bx[2 * H + u], b_nh = bh[2 * H + u];
  f4 dWx[3][DT], dWh[3][HT];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dWx[g][dt] = sg_splat(0.0f);
#pragma unroll
    for (int nt = 0; nt < HT; ++nt) dWh[g][nt] = sg_splat(0.0f);
  }
  float db[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sums of da_r, da_z, da_n, dgh_n
  float dh[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int s = 4 * fg + r;
    dh[r] = g_last != nullptr && b0 + s < B
                ? sg_h2f(g_last[(b0 + s) * H + u]) : 0.0f;
  }
  // this thread's piece of a state row, for the h_{t-1} images
  const bool hload = (int)threadIdx.x < 16 * HC;
  const int hs = threadIdx.x / HC, hc = threadIdx.x % HC;
  if (hload) {
    u4 h0 = u4{0, 0, 0, 0};
    if (L >= 2 && b0 + hs < B)
      h0 = *(const u4*)&states[((b0 + hs) * L + (L - 2)) * H + hc * 8];
    *(u4*)&himg[0][hs * HP + hc * 8] = h0;
  }
  int hb = 0, pb = 0;  // buffers of this step: h image (of 3), the others
  for (int t = L - 1; t >= 0; --t) {
    const int t0 = t - t % T, tt = t - t0;
    if (tt == T - 1 || t == L - 1) {  // a new chunk of x
      uint32_t v[G::PER];
      sg_sync();  // the last step's readers of ximg, mk and ac are done
      for (int p = 0; p < T; ++p) {
        sg_stage_load<D, NT>(seq, total, b0, B, L, t0, p, v);
        sg_stage_store<D, NT>(seq, att, b0, B, L, t0, p, v, ximg, mk, ac);
      }
      sg_sync();
      sg_fix<D, NT>(ximg, mk);
      sg_sync();
    }
    const int hn = hb == 2 ? 0 : hb + 1;
    u4 hpre = u4{0, 0, 0, 0};  // h_{t-2}, the next step's h_prev
    if (hload && t >= 2 && b0 + hs < B)
      hpre = *(const u4*)&states[((b0 + hs) * L + (t - 2)) * H + hc * 8];
    // the gates again, from x_t and h_{t-1}
    f4 ar = sg_splat(b_r), az = sg_splat(b_z);
    f4 anx = sg_splat(b_nx), anh = sg_splat(b_nh);
#pragma unroll
    for (int ks = 0; ks < DK; ++ks) {
      const h8 xa = *(const h8*)&ximg[fi * XS + tt * KP + ks * 32 + fg * 8];
      ar = __builtin_amdgcn_mfma_f32_16x16x32_f16(xa, wxf[0][ks], ar, 0, 0, 0);
      az = __builtin_amdgcn_mfma_f32_16x16x32_f16(xa, wxf[1][ks], az, 0, 0, 0);
      anx = __builtin_amdgcn_mfma_f32_16x16x32_f16(xa, wxf[2][ks], anx, 0, 0, 0);
    }
#pragma unroll
    for (int ks = 0; ks < HK; ++ks) {
      const h8 ha = *(const h8*)&himg[hb][fi * HP + ks * 32 + fg * 8];
      ar = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, whf[0][ks], ar, 0, 0, 0);
      az = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, whf[1][ks], az, 0, 0, 0);
      anh = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, whf[2][ks], anh, 0, 0, 0);
    }
    float keep[4], qs[4];
    bool ok[4];
    hf4 ahi[4], alo[4];  // A-fragments: da_r, da_z, da_n, dgh_n
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int s = 4 * fg + r;
      ok[r] = sg_valid(mk[s * T + tt]);
      const float a = ac[s * T + tt];
      const float hp = sg_h2f(himg[hb][s * HP + u]);
      float dhv = dh[r];
      if (g_states != nullptr && b0 + s < B)
        dhv += sg_h2f(g_states[((b0 + s) * L + t) * H + u]);
      const float rr = sg_sigmoid(ar[r]), zz = sg_sigmoid(az[r]);
      const float ghn = anh[r];
      const float nn = sg_tanh(fmaf(rr, ghn, anx[r]));
      const float omz = 1.0f - zz, nmh = nn - hp;
      qs[r] = ok[r] ? dhv * (omz * nmh) : 0.0f;
      const float da_n = (dhv * a * omz) * (1.0f - nn * nn);
      const float da_z = (-dhv * a * nmh) * (zz * (1.0f - zz));
      const float da_r = (da_n * ghn) * (rr * (1.0f - rr));
      const float dgn = da_n * rr;
      keep[r] = ok[r] ? dhv * (1.0f - a * omz) : dhv;
      const float dv[4] = {ok[r] ? da_r : 0.0f, ok[r] ? da_z : 0.0f,
                           ok[r] ? da_n : 0.0f, ok[r] ? dgn : 0.0f};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const _Float16 hi = (_Float16)dv[k];
        const _Float16 lo = (_Float16)((dv[k] - (float)hi) * SG_LO);
        ahi[k][r] = hi;
        alo[k][r] = lo;
        dgh[pb][s * GP + k * H + u] = __builtin_bit_cast(u16, hi);
        dgl[pb][s * GP + k * H + u] = __builtin_bit_cast(u16, lo);
        db[k] += dv[k];
      }
    }
    if (datt != nullptr) {  // over the wave's units; the waves after the barrier
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
          qs[r] += sg_shfl(qs[r], lane ^ off);
        if (fi == 0) dap[pb][wave * 16 + 4 * fg + r] = qs[r];
      }
    }
    if (hload) *(u4*)&himg[hn][hs * HP + hc * 8] = hpre;
    sg_sync();  // the step's one barrier
    if (datt != nullptr && threadIdx.x < 16 && b0 + threadIdx.x < B) {
      float sum = dap[pb][threadIdx.x];
#pragma unroll
      for (int w = 1; w < HT; ++w) sum += dap[pb][w * 16 + threadIdx.x];
      datt[(b0 + threadIdx.x) * L + t] = sum;
    }
    // dh_{t-1} = dh (1 - a(1-z)) + dgh Wh   (columns r, z and dgh_n)
    {
      f4 ch = sg_splat(0.0f), cl = sg_splat(0.0f);
#pragma unroll
      for (int kk = 0; kk < GK; ++kk) {
        const int col = kk * 32 + (kk >= 2 * HK ? H : 0) + fg * 8;
        const h8 fh = *(const h8*)&dgh[pb][fi * GP + col];
        const h8 fl = *(const h8*)&dgl[pb][fi * GP + col];
        ch = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh, whT[kk], ch, 0, 0, 0);
        cl = __builtin_amdgcn_mfma_f32_16x16x32_f16(fl, whT[kk], cl, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        dh[r] = keep[r] + fmaf(cl[r], SG_LO_INV, ch[r]);
    }
    // dx_t = dgx Wx   (columns r, z and da_n), straight to dseq
#pragma unroll
    for (int n = 0; n < NDX; ++n) {
      const int dt = wave + HT * n;
      if (dt < DT) {
        f4 ch = sg_splat(0.0f), cl = sg_splat(0.0f);
#pragma unroll
        for (int kk = 0; kk < GK; ++kk) {
          const int col = kk * 32 + fg * 8;
          const h8 fh = *(const h8*)&dgh[pb][fi * GP + col];
          const h8 fl = *(const h8*)&dgl[pb][fi * GP + col];
          h8 wf;
          if constexpr (XREG) wf = wxT[n][kk];
          else wf = *(const h8*)&WxT[(dt * 16 + fi) * (3 * H) + col];
          ch = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh, wf, ch, 0, 0, 0);
          cl = __builtin_amdgcn_mfma_f32_16x16x32_f16(fl, wf, cl, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s = 4 * fg + r;
          if (b0 + s < B) {
            u16* row = dseq + ((b0 + s) * L + t) * (D + 1);
            row[dt * 16 + fi] =
                ok[r] ? sg_f2h(fmaf(cl[r], SG_LO_INV, ch[r])) : (u16)0;
            if (dt == 0 && fi == 0) row[D] = 0;
          }
        }
      }
    }
    // dWx += dgx^T x_t, dWh += dgh^T h_{t-1}: the samples are the reduction
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const hf4 bf = sg_tr(ximg + tt * KP, XS, dt * 16, lane);
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        const f4 lo = __builtin_amdgcn_mfma_f32_16x16x16f16(
            alo[g], bf, sg_splat(0.0f), 0, 0, 0);
        dWx[g][dt] = __builtin_amdgcn_mfma_f32_16x16x16f16(ahi[g], bf,
                                                           dWx[g][dt], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          dWx[g][dt][r] = fmaf(lo[r], SG_LO_INV, dWx[g][dt][r]);
      }
    }
#pragma unroll
    for (int nt = 0; nt < HT; ++nt) {
      const hf4 bf = sg_tr(himg[hb], HP, nt * 16, lane);
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        const int k = g == 2 ? 3 : g;
        const f4 lo = __builtin_amdgcn_mfma_f32_16x16x16f16(
            alo[k], bf, sg_splat(0.0f), 0, 0, 0);
        dWh[g][nt] = __builtin_amdgcn_mfma_f32_16x16x16f16(ahi[k], bf,
                                                           dWh[g][nt], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          dWh[g][nt][r] = fmaf(lo[r], SG_LO_INV, dWh[g][nt][r]);
      }
    }
    hb = hn;
    pb ^= 1;
  }
  // the block's partial: row = gate unit 16*wave + 4*fg + r, column = fi
  float* p = part + (int64_t)blockIdx.x * (3 * H * (D + H + 2));
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = g * H + 16 * wave + 4 * fg + r;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        p[row * D + dt * 16 + fi] = dWx[g][dt][r];
#pragma unroll
      for (int nt = 0; nt < HT; ++nt)
        p[3 * H * D + row * H + nt * 16 + fi] = dWh[g][nt][r];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // samples 4*fg + r are summed; now the fg
    db[k] += sg_shfl(db[k], lane ^ 16);
    db[k] += sg_shfl(db[k], lane ^ 32);
  }
  if (fg == 0) {
    float* pb_ = p + 3 * H * (D + H);
    pb_[u] = db[0];
    pb_[H + u] = db[1];
    pb_[2 * H + u] = db[2];
    pb_[3 * H + u] = db[0];
    pb_[4 * H + u] = db[1];
    pb_[5 * H + u] = db[3];
  }
}

// out[i] = sum over the blocks' partials, in block order
__global__ __launch_bounds__(256) void sg_reduce_kernel(
    const float* __restrict__ part, float* __restrict__ out, int nblk, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float acc = 0.0f;
  for (int k = 0; k < nblk; ++k) acc += part[(int64_t)k * n + i];
  out[i] = acc;
}

bool sg_feasible(int64_t L, int64_t D, int64_t H) {
  return (D == 32 || D == 64 || D == 128) && (H == 32 || H == 64) && L >= 1 &&
         L <= 1024;
}

hipStream_t sg_stream() { return at::hip::getCurrentHIPStream().stream(); }

bool sg_is(const torch::Tensor& t, const torch::Tensor& like,
           c10::ScalarType st) {
  return t.is_cuda() && t.device() == like.device() && t.scalar_type() == st &&
         t.is_contiguous();
}

// raises on anything the kernels do not take
void sg_check(const torch::Tensor& seq, const torch::Tensor& Wx,
              const torch::Tensor& Wh, const torch::Tensor& bx,
              const torch::Tensor& bh, const OptT& att, const char* who) {
  TORCH_CHECK(seq.is_cuda(), who, ": seq must be on a GPU");
  TORCH_CHECK(sg_is(seq, seq, torch::kFloat16) &&
                  sg_is(Wx, seq, torch::kFloat16) &&
                  sg_is(Wh, seq, torch::kFloat16),
              who, ": seq, Wx, Wh must be contiguous float16 on one GPU");
  TORCH_CHECK(sg_is(bx, seq, torch::kFloat32) && sg_is(bh, seq, torch::kFloat32),
              who, ": bx, bh must be contiguous float32 beside seq");
  TORCH_CHECK(seq.dim() == 3 && seq.size(2) >= 2, who,
              ": expected seq [B, L, D+1]");
  const int64_t B = seq.size(0), L = seq.size(1), D = seq.size(2) - 1;
  TORCH_CHECK(Wh.dim() == 2 && Wh.size(0) == 3 * Wh.size(1), who,
              ": expected Wh [3H, H]");
  const int64_t H = Wh.size(1);
  TORCH_CHECK(Wx.dim() == 2 && Wx.size(0) == 3 * H && Wx.size(1) == D, who,
              ": expected Wx [3H, D] beside seq [B, L, D+1]");
  TORCH_CHECK(bx.dim() == 1 && bx.size(0) == 3 * H && bh.sizes() == bx.sizes(),
              who, ": expected bx and bh [3H]");
  TORCH_CHECK(((uintptr_t)Wx.data_ptr() & 15) == 0 &&
                  ((uintptr_t)Wh.data_ptr() & 15) == 0,
              who, ": Wx and Wh must start on 16 bytes");
  if (att.has_value())
    TORCH_CHECK(sg_is(*att, seq, torch::kFloat32) && att->dim() == 2 &&
                    att->size(0) == B && att->size(1) == L,
                who, ": att must be a contiguous float32 [B, L] beside seq");
  TORCH_CHECK(B <= INT32_MAX, who, ": batch too large");
  TORCH_CHECK(sg_feasible(L, D, H), who, ": no kernel for L=", L, " D=", D,
              " H=", H, " (seq_gru_feasible)");
}

#define SG_CASE(HT, DK, ...)        \
  if (H == 16 * HT && D == 32 * DK) \
    return [&] { constexpr int kHT = HT, kDK = DK; __VA_ARGS__; }();
#define SG_DISPATCH(...)                                                     \
  SG_CASE(2, 1, __VA_ARGS__) SG_CASE(2, 2, __VA_ARGS__)                      \
  SG_CASE(2, 4, __VA_ARGS__) SG_CASE(4, 1, __VA_ARGS__)                      \
  SG_CASE(4, 2, __VA_ARGS__) SG_CASE(4, 4, __VA_ARGS__)

const float* sg_attp(const OptT& att) {
  return att.has_value() ? (const float*)att->data_ptr() : nullptr;
}

const u16* sg_halfp(const OptT& t) {
  return t.has_value() ? (const u16*)t->data_ptr() : nullptr;
}

void sg_launch_fwd(int H, int D, const torch::Tensor& seq,
                   const torch::Tensor& Wx, const torch::Tensor& Wh,
                   const torch::Tensor& bx, const torch::Tensor& bh,
                   const OptT& att, torch::Tensor& states,
                   torch::Tensor& last) {
  const int B = (int)seq.size(0), L = (int)seq.size(1);
  const unsigned grid = (unsigned)((B + 15) / 16);
  SG_DISPATCH(hipLaunchKernelGGL(
      (seq_gru_fwd_kernel<kHT, kDK>), dim3(grid), dim3(64 * kHT), 0,
      sg_stream(), (const u16*)seq.data_ptr(), (const u16*)Wx.data_ptr(),
      (const u16*)Wh.data_ptr(), (const float*)bx.data_ptr(),
      (const float*)bh.data_ptr(), sg_attp(att), (u16*)states.data_ptr(),
      (u16*)last.data_ptr(), B, L))
  TORCH_CHECK(false, "seq_gru_fwd: no instance for H=", H, " D=", D);
}

void sg_launch_bwd(int H, int D, const OptT& g_states, const OptT& g_last,
                   const torch::Tensor& seq, const torch::Tensor& states,
                   const torch::Tensor& Wx, const torch::Tensor& Wh,
                   const torch::Tensor& bx, const torch::Tensor& bh,
                   const OptT& att, torch::Tensor& dseq, float* datt,
                   torch::Tensor& part) {
  const int B = (int)seq.size(0), L = (int)seq.size(1);
  torch::Tensor WxT;  // [D, 3H], read by the one instance that needs it
  if (H == 64 && D == 128) WxT = Wx.t().contiguous();
  const u16* wxt = WxT.defined() ? (const u16*)WxT.data_ptr() : nullptr;
  const unsigned grid = (unsigned)((B + 15) / 16);
  SG_DISPATCH(hipLaunchKernelGGL(
      (seq_gru_bwd_kernel<kHT, kDK>), dim3(grid), dim3(64 * kHT), 0,
      sg_stream(), sg_halfp(g_states), sg_halfp(g_last),
      (const u16*)seq.data_ptr(), (const u16*)states.data_ptr(),
      (const u16*)Wx.data_ptr(), (const u16*)Wh.data_ptr(), wxt,
      (const float*)bx.data_ptr(), (const float*)bh.data_ptr(), sg_attp(att),
      (u16*)dseq.data_ptr(), datt, (float*)part.data_ptr(), B, L))
  TORCH_CHECK(false, "seq_gru_bwd: no instance for H=", H, " D=", D);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool seq_gru_feasible(int64_t L, int64_t D, int64_t H) {
  return sg_feasible(L, D, H);
}

std::tuple<torch::Tensor, torch::Tensor> seq_gru_fwd(
    torch::Tensor seq, torch::Tensor Wx, torch::Tensor Wh, torch::Tensor bx,
    torch::Tensor bh, OptT att) {
  sg_check(seq, Wx, Wh, bx, bh, att, "seq_gru_fwd");
  const int64_t B = seq.size(0), L = seq.size(1), H = Wh.size(1);
  auto states = torch::empty({B, L, H}, seq.options());
  auto last = torch::empty({B, H}, seq.options());
  if (B > 0)
    sg_launch_fwd((int)H, (int)seq.size(2) - 1, seq, Wx, Wh, bx, bh, att,
                  states, last);
  return {states, last};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, OptT>
seq_gru_bwd(OptT g_states, OptT g_last, torch::Tensor seq,
            torch::Tensor states, torch::Tensor Wx, torch::Tensor Wh,
            torch::Tensor bx, torch::Tensor bh, OptT att) {
  sg_check(seq, Wx, Wh, bx, bh, att, "seq_gru_bwd");
  const int64_t B = seq.size(0), L = seq.size(1), D = seq.size(2) - 1;
  const int64_t H = Wh.size(1), n = 3 * H * (D + H + 2);
  TORCH_CHECK(sg_is(states, seq, torch::kFloat16) && states.dim() == 3 &&
                  states.size(0) == B && states.size(1) == L &&
                  states.size(2) == H &&
                  ((uintptr_t)states.data_ptr() & 15) == 0,
              "seq_gru_bwd: states must be a contiguous float16 [B, L, H] "
              "beside seq, starting on 16 bytes");
  if (g_states.has_value())
    TORCH_CHECK(sg_is(*g_states, seq, torch::kFloat16) &&
                    g_states->sizes() == states.sizes(),
                "seq_gru_bwd: g_states must be a contiguous float16 [B, L, H] "
                "beside seq");
  if (g_last.has_value())
    TORCH_CHECK(sg_is(*g_last, seq, torch::kFloat16) && g_last->dim() == 2 &&
                    g_last->size(0) == B && g_last->size(1) == H,
                "seq_gru_bwd: g_last must be a contiguous float16 [B, H] "
                "beside seq");
  auto dseq = torch::empty_like(seq);
  auto sums = torch::zeros({n}, bx.options());
  OptT datt;
  if (att.has_value()) datt = torch::empty_like(*att);
  if (B > 0) {
    const int64_t grid = (B + 15) / 16;
    auto part = torch::empty({grid, n}, bx.options());
    sg_launch_bwd((int)H, (int)D, g_states, g_last, seq, states, Wx, Wh, bx,
                  bh, att, dseq,
                  datt.has_value() ? (float*)datt->data_ptr() : nullptr, part);
    hipLaunchKernelGGL(sg_reduce_kernel, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, sg_stream(),
                       (const float*)part.data_ptr(), (float*)sums.data_ptr(),
                       (int)grid, (int)n);
  }
  return {dseq,
          sums.narrow(0, 0, 3 * H * D).view({3 * H, D}),
          sums.narrow(0, 3 * H * D, 3 * H * H).view({3 * H, H}),
          sums.narrow(0, 3 * H * (D + H), 3 * H),
          sums.narrow(0, 3 * H * (D + H + 1), 3 * H),
          datt};
}

void init_seqgru(pybind11::module_& m) {
  m.def("seq_gru_feasible", &seq_gru_feasible,
        "true if the GRU/AUGRU sequence kernels take (L, D, H)");
  m.def("seq_gru_fwd", &seq_gru_fwd,
        "GRU (att none) or AUGRU over a raw slot's rows -> (states, last)",
        pybind11::arg("seq"), pybind11::arg("Wx"), pybind11::arg("Wh"),
        pybind11::arg("bx"), pybind11::arg("bh"),
        pybind11::arg("att") = pybind11::none());
  m.def("seq_gru_bwd", &seq_gru_bwd,
        "GRU/AUGRU backward -> (dseq, dWx, dWh, dbx, dbh, datt or None)",
        pybind11::arg("g_states"), pybind11::arg("g_last"),
        pybind11::arg("seq"), pybind11::arg("states"), pybind11::arg("Wx"),
        pybind11::arg("Wh"), pybind11::arg("bx"), pybind11::arg("bh"),
        pybind11::arg("att") = pybind11::none());
}
