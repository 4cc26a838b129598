// The 128 x 128 score tile of the verification kernels (sv_trials.hip, sv_snorm.hip): the fp32 dot
// products of 128 rows of A with 128 rows of B on the exact fp32 MFMA, left in the accumulators of
// the workgroup's 4 waves (each a 64 x 64 quarter as 2 x 2 v_mfma_f32_32x32x2_f32 blocks).  The tile
// plan, the operand staging and the LDS layout are described at the top of sv_trials.hip; both
// kernels run this one k-loop, so a pair of rows scores the same bits in either of them.
#pragma once
#include "sv_common.h"

namespace {

constexpr int TR_T = 128;       // tile edge (pairs)
constexpr int TR_KC = 32;       // operand columns per chunk
constexpr int TR_LD = TR_T + 4; // LDS row stride of one k (floats)
constexpr int TR_NLD = TR_T * TR_KC / 4 / 256;  // 16-byte loads per thread and operand per chunk
constexpr int TR_MAX_D = 1024;
constexpr int TR_OPERAND_FLOATS = 2 * TR_KC * TR_LD;  // As then Bs

__device__ __forceinline__ void trial_load(const float* __restrict__ P, long ld, int N, int D, long row0, int k0,
                                           int tid, f32x4 (&v)[TR_NLD]) {
#pragma unroll
  for (int p = 0; p < TR_NLD; ++p) {
    const int f = tid + p * 256;
    const long row = row0 + (f >> 3);
    const int k = k0 + (f & 7) * 4;
    v[p] = (row < N && k < D) ? *reinterpret_cast<const f32x4*>(P + row * ld + k) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

__device__ __forceinline__ void trial_store(float* __restrict__ S, int tid, const f32x4 (&v)[TR_NLD]) {
#pragma unroll
  for (int p = 0; p < TR_NLD; ++p) {
    const int f = tid + p * 256;
    float* dst = S + (f & 7) * 4 * TR_LD + (f >> 3);
    dst[0] = v[p].x;
    dst[TR_LD] = v[p].y;
    dst[2 * TR_LD] = v[p].z;
    dst[3 * TR_LD] = v[p].w;
  }
}

// acc := the scores of A rows i0 .. i0 + 127 against B rows j0 .. j0 + 127 (rows >= Na / Nb and
// columns >= D count as zeros).  As, Bs: TR_KC * TR_LD floats of LDS each.  first_chunk() runs once,
// between the two barriers of the first chunk: the place to stage per-row side tables of this tile
// into LDS -- the first barrier has the last tile's reads of them behind it, the second publishes them.
template <class F>
__device__ __forceinline__ void trial_tile_scores(f32x16 (&acc)[4], const float* __restrict__ A, long lda, int Na,
                                                  long i0, const float* __restrict__ B, long ldb, int Nb, long j0,
                                                  int D, float* __restrict__ As, float* __restrict__ Bs, int tid,
                                                  int lane, int wr, int wc, F first_chunk) {
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
  f32x4 va[TR_NLD], vb[TR_NLD];
  trial_load(A, lda, Na, D, i0, 0, tid, va);
  trial_load(B, ldb, Nb, D, j0, 0, tid, vb);
  for (int k0 = 0; k0 < D; k0 += TR_KC) {
    __syncthreads();  // the last chunk's reads, and the last tile's side-table reads, are done
    trial_store(As, tid, va);
    trial_store(Bs, tid, vb);
    if (k0 == 0) first_chunk();
    __syncthreads();
    if (k0 + TR_KC < D) {
      trial_load(A, lda, Na, D, i0, k0 + TR_KC, tid, va);
      trial_load(B, ldb, Nb, D, j0, k0 + TR_KC, tid, vb);
    }
    const float* ap = As + (lane >> 5) * TR_LD + wr + (lane & 31);
    const float* bp = Bs + (lane >> 5) * TR_LD + wc + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < TR_KC / 2; ++kk) {
      const float a0 = ap[2 * kk * TR_LD], a1 = ap[2 * kk * TR_LD + 32];
      const float b0 = bp[2 * kk * TR_LD], b1 = bp[2 * kk * TR_LD + 32];
      acc[0] = mfma32x32x2(a0, b0, acc[0]);
      acc[1] = mfma32x32x2(a0, b1, acc[1]);
      acc[2] = mfma32x32x2(a1, b0, acc[2]);
      acc[3] = mfma32x32x2(a1, b1, acc[3]);
    }
  }
}

}  // namespace
