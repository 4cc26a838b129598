// GE2E contrast loss (arXiv 1710.10467 eq. 7):
//   per_r = 1 - sigma(S[r, s(r)]) + max_{k != s(r)} sigma(S[r, k]),   loss = sum per
// on the same cos and S = w (cos + 1e-6) + b as the softmax loss.  This header holds the loss's row
// arithmetic (inline device functions) and its fused row kernel (a template), so any translation
// unit may include it: sv_ge2e.hip launches the fused kernel and defines the split path's row
// kernels on this arithmetic, sv_ge2e_utils.hip the stand-alone calc_contrast helpers.  Every
// kernel around the row step -- prep, centroids, the cosine and Jacobian GEMMs, beta, cols,
// finalize -- is the softmax path's, unchanged.
//
// sigma is monotone, so the maximum sits where S is largest over k != s(r) (a negative w selects the
// smallest cosine); ties go to the lowest k, torch.max(dim)'s index.  With p = sigma(S_d) on the
// diagonal and q = sigma(S_k*):
//   dS_d = -p (1 - p),  dS_k* = q (1 - q),  every other dS exactly 0,
// so the dense dcos row handed to the column step has one live entry and G1 = dcos_k* C^_k* is one
// scaled centroid row.
#pragma once
#include <limits.h>
#include "sv_ge2e_dev.h"

// sigma(x) from e = e^{-|x|} in (0, 1]: e / (1 + e) below 0 (no overflow, the small tail kept: at
// S = -14 it is 8.3e-7 to fp32 relative precision, where 1 - 1 / (1 + e^14) would keep 3 digits)
__device__ __forceinline__ float ct_sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return (x < 0.f ? e : 1.0f) / (1.0f + e);
}
// sigma(x) (1 - sigma(x)) = e / (1 + e)^2, symmetric in x
__device__ __forceinline__ float ct_dsigmoid(float x) {
  const float e = expf(-fabsf(x));
  const float d = 1.0f + e;
  return e / (d * d);
}

// wave-wide arg max of (value, index) pairs: the largest value, among equals the lowest index; every
// lane gets the result.  A lane without a candidate passes (-inf, INT_MAX).
__device__ __forceinline__ void ct_wave_argmax(float& v, int& k) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int ok = __shfl_xor(k, o, 64);
    if (ov > v || (ov == v && ok < k)) {
      v = ov;
      k = ok;
    }
  }
}
// no candidate compared greater than -inf (NaN or -inf rows): any legal off-diagonal column, so that
// nothing downstream indexes out of range
__device__ __forceinline__ int ct_legal(int k, int n, int diag) { return (unsigned)k < (unsigned)n ? k : (diag == 0 ? 1 : 0); }

// the row's scalars from S on the diagonal (sd) and at k* (sk), their cosines cd / ck, upstream g
struct CtRow {
  float per, dcd, dck, alpha, dw, db;
};
__device__ __forceinline__ CtRow ct_row(float wv, float bv, float g, float cd, float ck) {
  const float sd = wv * (cd + EPS_SIM) + bv, sk = wv * (ck + EPS_SIM) + bv;
  const float dsd = -g * ct_dsigmoid(sd), dsk = g * ct_dsigmoid(sk);
  CtRow o;
  o.per = ct_sigmoid(-sd) + ct_sigmoid(sk);  // 1 - sigma(S_d) = sigma(-S_d)
  o.dcd = wv * dsd;
  o.dck = wv * dsk;
  o.alpha = wv * (dsd * cd + dsk * ck);  // sum_k dcos_k cos_k, the diagonal included
  o.dw = dsd * (cd + EPS_SIM) + dsk * (ck + EPS_SIM);
  o.db = dsd + dsk;
  return o;
}

// k* of a row of a given S [K] whose positive is column j: the maximum runs over every k != j, k < K
// (the stand-alone helpers; bs: the maximum itself)
__device__ __forceinline__ int ct_row_argmax(const float* __restrict__ s, int K, int j, int lane, float& bs) {
  bs = -INFINITY;
  int bk = INT_MAX;
  for (int k = lane; k < K; k += 64) {
    const float v = s[k];
    if (k != j && v > bs) {
      bs = v;
      bk = k;
    }
  }
  ct_wave_argmax(bs, bk);
  return ct_legal(bk, K, j);
}

// F2 of the fused path for the contrast loss, local and sharded (s0 > 0, C^ from
// ge2e_centroid_kernel) alike, over the whole sv_ge2e_train_ok domain.  The frame is
// ge2e_rows_kernel's, from sv_ge2e_dev.h: RW rows per workgroup, one wave per row, C^ staged in LDS
// (one tile up to GF_TILE speakers, NH = 2; two tiles above, NH = 4), the cosines with lanes over
// speakers and E^ broadcast.  What follows differs: no exponent sum and no
// pass over the tiles for G1.  Each lane keeps the best (S, k) of its off-diagonal speakers across
// the tiles, one wave arg max picks k*, and G1_r = dcos_k* C^_k* reads that one centroid row from
// global memory (1 KB, L2 resident), so tile 0 is never staged a second time.  Writes exactly what
// ge2e_rows_kernel hands to F1 / F3: per, the cos row, a dense dcos row [ldc] (zero outside k*, the
// padding columns N .. ldc - 1 included), alpha, dcd, dwdb_rows and G1.
// RW (the launcher's choice, ct_rows_per_wg): above GF_TILE speakers the kernel is bound by the
// staging, 266 KB from L2 per WORKGROUP whatever its row count, so a workgroup should carry as many
// rows as still leaves one workgroup per CU.  Measured at (256, 10, 256), 2560 rows on 256 CUs, the
// whole three-launch step: RW = 4 (640 workgroups, three rounds) 113.4 us, RW = 8 (320) 102.8,
// RW = 16 (160, one round) 93.8, results bit-identical; the softmax step 111.7.
template <int NH, int RW>
__global__ __launch_bounds__(64 * RW) void ge2e_rows_contrast_kernel(
    const float* __restrict__ Chat, const float* __restrict__ Ehat, const float* __restrict__ rawd, int Bl, int M, int N,
    int D, int ldc, int s0, const float* __restrict__ wp, const float* __restrict__ bp, float* __restrict__ per,
    float* __restrict__ cos, float* __restrict__ dcos, float* __restrict__ alpha, float* __restrict__ dcd,
    float* __restrict__ dwdb_rows, float* __restrict__ G1) {
  static_assert(NH == 2 || NH == 4, "NH: 64-speaker groups per lane");
  extern __shared__ __attribute__((aligned(16))) float gsm[];
  const int LDC = D + 4;
  const int NT = NH == 2 ? N : GF_TILE;  // speakers per LDS tile
  float* Cs = gsm;                       // [NT][LDC]
  float* Es = Cs + (size_t)NT * LDC;     // [RW][D]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  ge2e_stage_tile<RW>(Chat, Cs, 0, NT, N, D);
  const int r = blockIdx.x * RW + w;  // this wave's row
  const bool live = r < Bl;
  if (live)
    for (int c = lane * 4; c < D; c += 256)
      *reinterpret_cast<float4*>(Es + w * D + c) = *reinterpret_cast<const float4*>(Ehat + (long)r * D + c);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS-DMA of C^ landed
  __syncthreads();
  float cv[NH];
  const int KS = ge2e_cos_step<NH, RW>(Chat, Cs, Es + w * D, live, NT, N, D, cv);
  if (!live) return;  // (no workgroup barrier below; the second tile's are above, for every wave)
  for (int o = KS; o < 64; o <<= 1) cv[0] += __shfl_xor(cv[0], o, 64);  // lane k < KS: speaker k
  const float wv = *wp, bv = *bp;
  const int sg = s0 + r / M;  // global speaker of this row
  const float rd = rawd[r];
  // the running (S, k) of this lane's off-diagonal speakers, ascending k: a later equal S does not
  // replace an earlier one
  float bs = -INFINITY;
  int bk = INT_MAX;
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const int k = lane + 64 * h;
    if (k == sg) cv[h] = rd;  // get_cossim's diagonal overwrite (utils.py:112-113)
    const float s = wv * (cv[h] + EPS_SIM) + bv;
    if (k < N && k != sg && s > bs) {
      bs = s;
      bk = k;
    }
  }
  ct_wave_argmax(bs, bk);
  bk = ct_legal(bk, N, sg);
  float ck = 0.f;
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const float t = __shfl(cv[h], bk & 63, 64);
    if ((bk >> 6) == h) ck = t;
  }
  const CtRow o = ct_row(wv, bv, 1.0f, rd, ck);
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const int k = lane + 64 * h;
    if (k < N) cos[(long)r * ldc + k] = cv[h];
    if (k < ldc) dcos[(long)r * ldc + k] = (k == bk) ? o.dck : 0.f;
  }
  if (lane == 0) {
    per[r] = o.per;
    dcd[r] = o.dcd;
    alpha[r] = o.alpha;
    dwdb_rows[r] = o.dw;
    dwdb_rows[Bl + r] = o.db;
  }
  const int c = lane * 4;
  if (c < D) {
    const float4 cc = *reinterpret_cast<const float4*>(Chat + (long)bk * D + c);
    *reinterpret_cast<float4*>(G1 + (long)r * D + c) = float4{o.dck * cc.x, o.dck * cc.y, o.dck * cc.z, o.dck * cc.w};
  }
}
