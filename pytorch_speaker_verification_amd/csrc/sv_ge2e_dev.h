// GE2E loss: what sv_ge2e.hip (the training path), sv_ge2e_contrast.h (the contrast row step) and
// sv_ge2e_utils.hip (the stand-alone utils.py helpers) share -- the constants, the workspace carve,
// the kernels that more than one of them launches, and the one definition of every formula that
// several kernels evaluate: the fused row frame (tile stage, cosine step), the dE epilogue terms
// and the loss / dw / db tail.
#pragma once
#include <algorithm>
#include "sv_common.h"
#include "../../include/sv_ge2e.h"

#define EPS_COS 1e-8f
#define EPS_SIM 1e-6f
#define EPS_LOG 1e-6f

// the fused path's domain (sv_ge2e_train_ok) and tiles
#define GF_NMAX 256
#define GF_DMAX 256
#define GF_MMAX 16
#define GF_MMAX_FIN 16  // utterances per speaker of the one-pass finalize (one wave each)
#define GF_ROWW 4       // rows (waves) per workgroup of the fused row step; the contrast step: 4, or 8 / 16 above GF_TILE speakers
#define GF_TILE 128     // speakers per LDS tile of C^ (133 KB of fp32 at D = 256)
#define GF_COLW 16      // waves of ge2e_cols_kernel
#define GF_COLU 10      // its row loads in flight per lane
constexpr int GF_CH = 128;  // speakers per chunk of ge2e_rows4r_kernel
// ge2e_rows4r_kernel's centroid tile stride: 288 = 32 mod 64 banks, so the two speakers of a 16-lane
// LDS pass (8-lane groups reading 32 consecutive floats each) fall on disjoint banks
constexpr int GF_R4LDC = 288;

namespace {

// workspace carve (all fp32), see sv_ge2e_workspace_size
struct Ge2eWs {
  float *Ehat, *Uhat, *En, *Un, *rawd, *cos, *logz, *Chat, *Cn, *dcos, *alpha, *G1, *dwdb_rows, *betap, *dcd, *gemm;
  size_t total;
};

size_t al(size_t n) { return (n + 63) & ~size_t(63); }  // 256-byte granules

Ge2eWs carve(float* base, int Nl, int M, int D, int N) {
  Ge2eWs w;
  N = (N + 3) & ~3;  // speaker dimension padded to a multiple of 4 (zero rows/cols)
  const size_t Bl = (size_t)Nl * M;
  size_t off = 0;
  auto take = [&](size_t n) {
    float* p = base ? base + off : nullptr;
    off += al(n);
    return p;
  };
  w.Ehat = take(Bl * D);
  w.Uhat = take(Bl * D);
  w.En = take(Bl);
  w.Un = take(Bl);
  w.rawd = take(Bl);
  w.cos = take(Bl * N);
  w.logz = take(Bl);
  w.Chat = take((size_t)N * D);
  w.Cn = take(N);
  w.dcos = take(Bl * N);
  w.alpha = take(Bl);
  w.G1 = take(Bl * D);
  w.dwdb_rows = take(2 * Bl);
  w.betap = take(((Bl + 63) / 64) * (size_t)N);
  w.dcd = take(Bl);  // dcos on the diagonal, w dS[r, s(r)], on every path
  const size_t g1 = sv_gemm_f32_workspace((int)Bl, D, N);
  const size_t g2 = sv_gemm_f32_workspace(N, D, (int)Bl);
  w.gemm = take((std::max(g1, g2) + 3) / 4);
  w.total = off * sizeof(float);
  return w;
}

}  // namespace

// kernels of sv_ge2e.hip that sv_ge2e_utils.hip launches too
__global__ void ge2e_sums_kernel(const float* __restrict__ E, int M, int D, float* __restrict__ ssum);
__global__ void ge2e_centroid_kernel(const float* __restrict__ ssum, int N, int M, int D, float* __restrict__ Chat,
                                     float* __restrict__ Cn);
__global__ void ge2e_rowprep_kernel(const float* __restrict__ E, const float* __restrict__ ssum, int Bl, int M, int D,
                                    int s0, float* __restrict__ Ehat, float* __restrict__ Uhat, float* __restrict__ En,
                                    float* __restrict__ Un, float* __restrict__ rawd);
__global__ void sum_kernel(const float* __restrict__ x, int n, float* __restrict__ out);
__global__ void ge2e_beta_partial_kernel(const float* __restrict__ dcos, const float* __restrict__ cos, int Bl, int N,
                                         int ldc, float* __restrict__ partial);
__global__ void ge2e_beta_final_kernel(const float* __restrict__ partial, int nchunk, int N, float* __restrict__ beta);

// ---------------------------------------------------------------------------
// The fused row frame of ge2e_rows_kernel and ge2e_rows_contrast_kernel: NW rows per workgroup, one
// wave per row; C^ in LDS as Cs [NT][D + 4] (16-B padded rows: the 16 lanes of a ds_read_b128 group
// hit disjoint banks), the rows' E^ in Es [NW][D] (each kernel copies its row there itself, after
// staging tile 0 and before its vmcnt(0) + barrier).  The helpers take no __restrict__ pointers and
// keep the kernels' int thread indices: the kernels then compile as they did with the text inline.
//
// global -> LDS copy of C^ rows k0 .. (at most NT, up to N).  D = 256 (every c1-c5 shape): by
// LDS-DMA, one 1 KB row per wave instruction (no VGPR round trip, every row in flight at once; the
// register copy below kept ~8 loads per lane in flight and took ~12 us per 128-speaker tile at c5's
// rank shape), waited for by the caller's vmcnt(0) + barrier; else through registers (distinct
// address spaces: the unrolled loads issue back to back)
template <int NW>
__device__ __forceinline__ void ge2e_stage_tile(const float* Chat, float* Cs, int k0, int NT, int N, int D) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int LDC = D + 4, D4 = D / 4;
  const int nk = min(NT, N - k0);
  if (D == 256) {
    for (int row = w; row < nk; row += NW)
      __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(Chat + (long)(k0 + row) * D + lane * 4),
                                       (__attribute__((address_space(3))) void*)(Cs + row * LDC), 16, 0, 0);
    return;
  }
  const int NQ = nk * D4;
#pragma unroll 8
  for (int q = tid; q < NQ; q += 64 * NW) {
    const int row = q / D4, col = (q - row * D4) * 4;
    *reinterpret_cast<float4*>(Cs + row * LDC + col) =
        *reinterpret_cast<const float4*>(Chat + (long)(k0 + row) * D + col);
  }
}

// cosines of this wave's row (e0, in Es) with every speaker: KS speaker lanes x DS d-slices (DS = 1
// for N > 32: lane k and k + 64 over all of D; small N splits D so the wave's lanes all work, the
// caller's butterfly `for (o = KS; o < 64; o <<= 1)` over cv[0] then joins the slices), E^
// broadcast; four independent partial sums (d mod 4), added pairwise at the end.  Speaker
// lane + 64 h is cv[h].  NH = 64-speaker groups per lane: 2 for N <= GF_TILE (tile 0 holds them
// all), 4 above, where tile 1 is staged here by every wave of the workgroup, live or not, and is
// the resident one on return.  Returns KS.
template <int NH, int NW>
__device__ __forceinline__ int ge2e_cos_step(const float* Chat, float* Cs, const float* e0, bool live, int NT,
                                             int N, int D, float (&cv)[NH]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int LDC = D + 4;
  int DS = N <= 8 ? 8 : N <= 16 ? 4 : N <= 32 ? 2 : 1;
  while (DS > 1 && D % (4 * DS)) DS >>= 1;
  const int KS = 64 / DS, dlen = D / DS;
  const int kl = lane & (KS - 1), d0 = (lane / KS) * dlen;
#pragma unroll
  for (int h = 0; h < NH; ++h) cv[h] = 0.f;
#pragma unroll
  for (int t = 0; t < NH / 2; ++t) {
    if (t > 0) {  // NH == 4: the second tile
      __syncthreads();
      ge2e_stage_tile<NW>(Chat, Cs, t * GF_TILE, NT, N, D);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
#pragma unroll
    for (int hk = 0; hk < 2; ++hk) {
      const int kt = kl + 64 * hk;  // speaker within the tile
      if (live && t * GF_TILE + kt < N) {
        float4 a = float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int c = d0; c < d0 + dlen; c += 4) {
          const float4 cc = *reinterpret_cast<const float4*>(Cs + kt * LDC + c);
          const float4 x0 = *reinterpret_cast<const float4*>(e0 + c);
          a.x += x0.x * cc.x;
          a.y += x0.y * cc.y;
          a.z += x0.z * cc.z;
          a.w += x0.w * cc.w;
        }
        cv[2 * t + hk] = (a.x + a.y) + (a.z + a.w);
      }
    }
  }
  return KS;
}

// ---------------------------------------------------------------------------
// The dE epilogue (ge2e_finalize_serial_kernel, ge2e_finalize_kernel, ge2e_cols_kernel), per (row r
// of speaker j, column d), with dcd = dcos on the diagonal, w dS[r, s(r)]:
//   dU_r  = dcd (E^_r - raw_d U^_r [|U|>eps]) / max(|U_r|, eps)
//   gE_r  = (G1_r + dcd U^_r - alpha_r E^_r [|E|>eps]) / max(|E_r|, eps)
//   dC_j  = (dChat_j - beta_j C^_j [|C|>eps]) / max(|C_j|, eps)
//   dE_r  = gE_r + dC_j / M + (sum_i' dU_ji' - dU_r) / (M - 1)
// Ge2eNorm: a norm's two factors in them, 1 / max(|x|, eps) and the projection [|x| > eps], formed
// where the kernel reads the norm (ge2e_cols_kernel: before its reduction loops, for every thread)
struct Ge2eNorm {
  float inv, proj;
};
__device__ __forceinline__ Ge2eNorm ge2e_norm(float n) { return {1.0f / fmaxf(n, EPS_COS), n > EPS_COS ? 1.f : 0.f}; }
__device__ __forceinline__ float ge2e_dU(Ge2eNorm u, float dcd, float eh, float rawd, float uh) {
  return dcd * (eh - rawd * uh * u.proj) * u.inv;
}
__device__ __forceinline__ float ge2e_gE(Ge2eNorm e, float g1, float dcd, float uh, float alpha, float eh) {
  return (g1 + dcd * uh - alpha * eh * e.proj) * e.inv;
}
__device__ __forceinline__ float ge2e_dC(Ge2eNorm c, float dchat, float beta, float chat) {
  return (dchat - beta * chat * c.proj) * c.inv;
}
__device__ __forceinline__ float ge2e_dE(float gE, float dC, float sumdU, float dU, int M) {
  const float invM = 1.0f / (float)M, invm1 = 1.0f / (float)(M - 1);
  return gE + dC * invM + (sumdU - dU) * invm1;
}

// ---------------------------------------------------------------------------
// loss = sum per (fp64, rounded once: sum_kernel's note), dw, db = sums of the per-row partials, by
// one whole workgroup of NW waves (a block-uniform call): thread strides, then the waves' sums in
// wave order
template <int NW>
__device__ __forceinline__ void ge2e_loss_tail(const float* per, const float* dwdb_rows, int Bl,
                                               float* loss, float* dwdb) {
  __shared__ float red2[2][NW];
  __shared__ double redl[NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double l = 0.0;
  float a = 0.f, b = 0.f;
  for (int i = tid; i < Bl; i += 64 * NW) {
    l += (double)per[i];
    a += dwdb_rows[i];
    b += dwdb_rows[Bl + i];
  }
  l = wave_sum_d(l);
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane == 0) {
    redl[w] = l;
    red2[0][w] = a;
    red2[1][w] = b;
  }
  __syncthreads();
  if (tid == 0) {
    double s0 = 0.0;
    float s1 = 0.f, s2 = 0.f;
    for (int i = 0; i < NW; ++i) {
      s0 += redl[i];
      s1 += red2[0][i];
      s2 += red2[1][i];
    }
    loss[0] = (float)s0;
    dwdb[0] = s1;
    dwdb[1] = s2;
  }
}
