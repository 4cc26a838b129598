// Verification trials scored and binned in one pass (sv_trial_hist of the C ABI): every pair (i, j)
// of rows of A [Na][D] and B [Nb][D] gets the fp32 dot product s = sum_d A[i][d] B[j][d] on the exact
// fp32 MFMA, and the score goes straight from the accumulator into a histogram -- target or
// non-target by the rows' labels -- so the Na x Nb score matrix never exists.
//   tile     one workgroup of 256 threads = 4 waves owns a 128 x 128 tile of pairs, each wave a 64 x 64
//            quarter as 2 x 2 v_mfma_f32_32x32x2_f32 blocks (64 accumulator registers).  A persistent
//            grid strides over the tiles; in symmetric mode only the tiles with tile-row <= tile-column
//            exist (a triangular index), and the pairs i >= j of a diagonal tile are masked.
//   operands k-chunks of TR_KC = 32 columns of the 128 A rows and 128 B rows go global -> registers
//            (16-byte loads, 8 lanes along a row; rows >= N and columns >= D load nothing and count
//            as zeros) -> LDS k-major [k][row] with a row stride of 132 floats, so an MFMA operand
//            read is 32 consecutive floats per half wave.  One LDS buffer, two barriers per chunk;
//            the next chunk's global loads are in flight under the current chunk's 64 MFMAs per wave.
//   epilogue every lane bins its 64 scores by the slot rule of include/sv_ge2e.h and adds 1 to the
//            slot with a no-return LDS atomic; the pair of 32-bit histograms [2][n_bins + 2] is the
//            workgroup's own and lives across all of its tiles.
//   flush    non-zero slots go to the 64-bit global histogram with one atomicAdd each, at the end
//            and after every TR_FLUSH tiles.  A tile adds at most 128 * 128 = 2^14 to one slot, so a
//            32-bit slot cannot wrap before 2^32 / 2^14 = 2^18 tiles; TR_FLUSH = 256 stays far below
//            that bound (2^22 counts) so that a test can reach a mid-run flush with one workgroup,
//            and costs one pass over the slots per 256 tiles.
//   LDS      2 * 32 * 132 * 4 = 33 792 B of operands + 1 KB of labels + 8 (n_bins + 2) B of
//            histograms: 100 368 B at the limit n_bins = 8192 (one workgroup per CU), 67 600 B at the
//            default 4096 (two per CU: one's epilogue runs under the other's MFMAs).
// Counts are integers: the result does not depend on the grid or on arrival order.
// -DSV_TRIAL_STAMP (an A/B build, never the shipped library): two more 64-bit words behind the
// histogram take wave 0's cycles inside the k-loops and inside the epilogues, summed over workgroups.
#include "sv_common.h"
#include "../../include/sv_ge2e.h"

#include <algorithm>

namespace {

constexpr int TR_T = 128;       // tile edge (pairs)
constexpr int TR_KC = 32;       // operand columns per chunk
constexpr int TR_LD = TR_T + 4; // LDS row stride of one k (floats)
constexpr int TR_NLD = TR_T * TR_KC / 4 / 256;  // 16-byte loads per thread and operand per chunk
constexpr int TR_FLUSH = 256;   // tiles between two flushes (bound: 2^18, see above)
constexpr int TR_MAX_BINS = 8192, TR_MAX_D = 1024;
constexpr size_t TR_LDS_FIXED = (size_t)(2 * TR_KC * TR_LD + 2 * TR_T) * 4;

struct TrialArgs {
  const float *A, *B;
  const int *lab_a, *lab_b;
  long lda, ldb;
  int Na, Nb, D, symmetric, n_bins;
  float lo, inv_width;
  long long n_tiles;
  int ntb;  // tile columns (rectangular mode)
  unsigned long long* hist;
};

// the slot rule of include/sv_ge2e.h: two separately rounded fp32 operations, then floorf; the three
// cases as one clamp of q + 1 into [0, n_bins + 1] (top): q is a whole number, so q + 1 is exact below
// 2^24 and beyond the clamp above it, and fmaxf drops a NaN for the 0 of slot 0
__device__ __forceinline__ int trial_slot(float s, float lo, float inv_width, float top) {
  const float q = floorf(__fmul_rn(__fsub_rn(s, lo), inv_width));
  return (int)fminf(fmaxf(q + 1.f, 0.f), top);
}

// one wave's 64 x 64 scores into the workgroup's histograms.  The row labels are read before the
// first atomic (the compiler cannot move an LDS read across one); DIAG: a diagonal tile of the
// symmetric mode, where only row < col counts
template <bool DIAG>
__device__ __forceinline__ void trial_bin(const f32x16 (&acc)[4], const int* __restrict__ labs, unsigned* __restrict__ hs,
                                          int wr, int wc, int lane, float lo, float inv_width, int n_bins) {
  int la[2][16];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int r = 0; r < 16; ++r) la[bi][r] = labs[wr + bi * 32 + acc_row(r, lane)];
  const float top = (float)(n_bins + 1);
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int col = wc + (b & 1) * 32 + (lane & 31);
    const int lb = labs[TR_T + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int l = la[b >> 1][r];
      bool live = (l | lb) >= 0;  // neither label negative
      if constexpr (DIAG) live = live && wr + (b >> 1) * 32 + acc_row(r, lane) < col;
      if (live) atomicAdd(hs + (l == lb ? n_bins + 2 : 0) + trial_slot(acc[b][r], lo, inv_width, top), 1u);
    }
  }
}

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

// the workgroup's non-zero slots into the global histogram; leaves the LDS slots zero
__device__ __forceinline__ void trial_flush(unsigned* __restrict__ hs, unsigned long long* __restrict__ hist,
                                            int n_slots, int tid) {
  __syncthreads();
  for (int i = tid; i < n_slots; i += 256) {
    const unsigned v = hs[i];
    if (v) {
      atomicAdd(hist + i, (unsigned long long)v);
      hs[i] = 0;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void trial_hist_kernel(const TrialArgs a) {
  extern __shared__ float lds[];
  float* As = lds;
  float* Bs = As + TR_KC * TR_LD;
  int* labs = reinterpret_cast<int*>(Bs + TR_KC * TR_LD);  // [0, 128) rows of A, [128, 256) rows of B
  unsigned* hs = reinterpret_cast<unsigned*>(labs + 2 * TR_T);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
  const int n_slots = 2 * (a.n_bins + 2);
  for (int i = tid; i < n_slots; i += 256) hs[i] = 0;  // (the first tile's barriers order this)
#ifdef SV_TRIAL_STAMP
  long long cyc_k = 0, cyc_e = 0;
#endif
  int since_flush = 0;
  for (long long t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    long long ti, tj;
    if (a.symmetric) {  // t counts the tiles ti <= tj column by column
      tj = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
      while (tj * (tj + 1) / 2 > t) --tj;
      while ((tj + 1) * (tj + 2) / 2 <= t) ++tj;
      ti = t - tj * (tj + 1) / 2;
    } else {
      ti = t / a.ntb;
      tj = t - ti * a.ntb;
    }
    const long i0 = ti * TR_T, j0 = tj * TR_T;
#ifdef SV_TRIAL_STAMP
    const long long c0 = clock64();
#endif
    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    f32x4 va[TR_NLD], vb[TR_NLD];
    trial_load(a.A, a.lda, a.Na, a.D, i0, 0, tid, va);
    trial_load(a.B, a.ldb, a.Nb, a.D, j0, 0, tid, vb);
    for (int k0 = 0; k0 < a.D; k0 += TR_KC) {
      __syncthreads();  // the last chunk's reads, and the last tile's label reads, are done
      trial_store(As, tid, va);
      trial_store(Bs, tid, vb);
      if (k0 == 0) {
        const long g = (tid < TR_T ? i0 : j0 - TR_T) + tid;
        const int n = tid < TR_T ? a.Na : a.Nb;
        labs[tid] = g < n ? (tid < TR_T ? a.lab_a : a.lab_b)[g] : -1;
      }
      __syncthreads();
      if (k0 + TR_KC < a.D) {
        trial_load(a.A, a.lda, a.Na, a.D, i0, k0 + TR_KC, tid, va);
        trial_load(a.B, a.ldb, a.Nb, a.D, j0, k0 + TR_KC, tid, vb);
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
#ifdef SV_TRIAL_STAMP
    const long long c1 = clock64();
#endif
    if (a.symmetric && ti == tj)
      trial_bin<true>(acc, labs, hs, wr, wc, lane, a.lo, a.inv_width, a.n_bins);
    else
      trial_bin<false>(acc, labs, hs, wr, wc, lane, a.lo, a.inv_width, a.n_bins);
#ifdef SV_TRIAL_STAMP
    const long long c2 = clock64();
    cyc_k += c1 - c0;
    cyc_e += c2 - c1;
#endif
    if (++since_flush == TR_FLUSH) {
      trial_flush(hs, a.hist, n_slots, tid);
      since_flush = 0;
    }
  }
  if (since_flush) trial_flush(hs, a.hist, n_slots, tid);
#ifdef SV_TRIAL_STAMP
  if (tid == 0) {
    atomicAdd(a.hist + n_slots, (unsigned long long)cyc_k);
    atomicAdd(a.hist + n_slots + 1, (unsigned long long)cyc_e);
  }
#endif
}

}  // namespace

extern "C" size_t sv_trial_hist_size(int n_bins) {
  if (n_bins < 1) return 0;
  size_t words = 2 * ((size_t)n_bins + 2);
#ifdef SV_TRIAL_STAMP
  words += 2;
#endif
  return words * 8;
}

extern "C" int sv_trial_hist(const float* A, long lda, const int* lab_a, int Na, const float* B, long ldb,
                             const int* lab_b, int Nb, int D, int symmetric, float lo, float inv_width, int n_bins,
                             unsigned long long* hist, int grid, hipStream_t stream) {
  if (!A || !B || !lab_a || !lab_b || !hist || Na < 1 || Nb < 1 || D < 1 || n_bins < 1 || grid < 0) return SV_EARG;
  if (symmetric && (A != B || lab_a != lab_b || Na != Nb || lda != ldb)) return SV_EARG;
  if ((((uintptr_t)A | (uintptr_t)B) & 15) || (((uintptr_t)lab_a | (uintptr_t)lab_b) & 3) || ((uintptr_t)hist & 7) ||
      lda % 4 || ldb % 4 || D % 4 || lda < D || ldb < D)
    return SV_EALIGN;
  if (n_bins > TR_MAX_BINS || D > TR_MAX_D) return SV_ESHAPE;
  const long long nta = ((long long)Na + TR_T - 1) / TR_T, ntb = ((long long)Nb + TR_T - 1) / TR_T;
  TrialArgs a{A, B, lab_a, lab_b, lda, ldb, Na, Nb, D, symmetric != 0, n_bins, lo, inv_width,
              symmetric ? nta * (nta + 1) / 2 : nta * ntb, (int)ntb, hist};
  const size_t lds = TR_LDS_FIXED + 2 * ((size_t)n_bins + 2) * 4;
  if (grid == 0) {  // every CU busy; two workgroups on each where the histograms leave room for them
    const int cus = sv_stream_cus(stream);
    const int per_cu = 2 * lds <= 160 * 1024 ? 2 : 1;
    grid = (int)std::min<long long>(a.n_tiles, (long long)(cus > 0 ? cus : 256) * per_cu);
  }
  grid = (int)std::min<long long>(grid, a.n_tiles);
  hipLaunchKernelGGL(trial_hist_kernel, dim3(grid), dim3(256), lds, stream, a);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
