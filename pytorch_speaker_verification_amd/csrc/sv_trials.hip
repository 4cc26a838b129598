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
//   norm     sv_trial_hist_norm is the same kernel with NORM = true: the score passes through the
//            normalisation step of include/sv_ge2e.h on its way to the slot rule, and mu and inv of
//            the tile's 128 + 128 rows are staged beside the labels (2 KB more LDS: 69 648 B at 4096
//            bins, still two workgroups per CU).
// Counts are integers: the result does not depend on the grid or on arrival order.  The tile's k-loop
// and operand staging are in sv_trial_tile.h, shared with sv_snorm.hip.
// -DSV_TRIAL_STAMP (an A/B build, never the shipped library): two more 64-bit words behind the
// histogram take wave 0's cycles inside the k-loops and inside the epilogues, summed over workgroups.
#include "sv_trial_tile.h"
#include "../../include/sv_ge2e.h"

#include <algorithm>

namespace {

constexpr int TR_FLUSH = 256;   // tiles between two flushes (bound: 2^18, see above)
constexpr int TR_MAX_BINS = 8192;
constexpr size_t TR_LDS_FIXED = (size_t)(TR_OPERAND_FLOATS + 2 * TR_T) * 4;
constexpr size_t TR_LDS_NORM = (size_t)4 * TR_T * 4;  // NORM: mu and inv of the tile's A rows and B rows

struct TrialArgs {
  const float *A, *B;
  const int *lab_a, *lab_b;
  long lda, ldb;
  int Na, Nb, D, symmetric, n_bins;
  float lo, inv_width;
  long long n_tiles;
  int ntb;  // tile columns (rectangular mode)
  unsigned long long* hist;
  const float *mu_a, *inv_a, *mu_b, *inv_b;  // sv_trial_hist_norm only
};

// the slot rule of include/sv_ge2e.h: two separately rounded fp32 operations, then floorf; the three
// cases as one clamp of q + 1 into [0, n_bins + 1] (top): q is a whole number, so q + 1 is exact below
// 2^24 and beyond the clamp above it, and fmaxf drops a NaN for the 0 of slot 0
__device__ __forceinline__ int trial_slot(float s, float lo, float inv_width, float top) {
  const float q = floorf(__fmul_rn(__fsub_rn(s, lo), inv_width));
  return (int)fminf(fmaxf(q + 1.f, 0.f), top);
}

// the score-normalisation step of sv_trial_hist_norm (include/sv_ge2e.h): four separately rounded
// fp32 operations, then the factor 0.5 (exact short of underflow)
__device__ __forceinline__ float trial_norm(float s, float mu_a, float inv_a, float mu_b, float inv_b) {
  const float za = __fmul_rn(__fsub_rn(s, mu_a), inv_a), zb = __fmul_rn(__fsub_rn(s, mu_b), inv_b);
  return __fmul_rn(0.5f, __fadd_rn(za, zb));
}

// one wave's scores into the workgroup's histograms, the NB 32-row accumulator blocks from B0 on.
// The rows' labels -- and with NORM their mu and inv, nrm = [mu_a | inv_a | mu_b | inv_b] of the
// tile's rows -- are read before the first atomic (the compiler cannot move an LDS read across one);
// DIAG: a diagonal tile of the symmetric mode, where only row < col counts
template <bool DIAG, bool NORM, int B0, int NB>
__device__ __forceinline__ void trial_bin_rows(const f32x16 (&acc)[4], const int* __restrict__ labs,
                                               const float* __restrict__ nrm, unsigned* __restrict__ hs, int wr,
                                               int wc, int lane, float lo, float inv_width, int n_bins) {
  int la[NB][16];
  float mu[NORM ? NB : 1][16], iv[NORM ? NB : 1][16], mub[2], ivb[2];
#pragma unroll
  for (int bi = 0; bi < NB; ++bi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wr + (B0 + bi) * 32 + acc_row(r, lane);
      la[bi][r] = labs[row];
      if constexpr (NORM) {
        mu[bi][r] = nrm[row];
        iv[bi][r] = nrm[TR_T + row];
      }
    }
  if constexpr (NORM)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      mub[bj] = nrm[2 * TR_T + wc + bj * 32 + (lane & 31)];
      ivb[bj] = nrm[3 * TR_T + wc + bj * 32 + (lane & 31)];
    }
  const float top = (float)(n_bins + 1);
#pragma unroll
  for (int b = 2 * B0; b < 2 * (B0 + NB); ++b) {
    const int col = wc + (b & 1) * 32 + (lane & 31);
    const int lb = labs[TR_T + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int l = la[(b >> 1) - B0][r];
      bool live = (l | lb) >= 0;  // neither label negative
      if constexpr (DIAG) live = live && wr + (b >> 1) * 32 + acc_row(r, lane) < col;
      float s = acc[b][r];
      if constexpr (NORM) s = trial_norm(s, mu[(b >> 1) - B0][r], iv[(b >> 1) - B0][r], mub[b & 1], ivb[b & 1]);
      if (live) atomicAdd(hs + (l == lb ? n_bins + 2 : 0) + trial_slot(s, lo, inv_width, top), 1u);
    }
  }
}

// one wave's 64 x 64 scores.  Plain: all 32 row labels ahead of the first atomic.  NORM: the two
// 32-row halves one after the other, each with its 16 labels, mu and inv per lane ahead of its
// atomics -- 48 table registers instead of 96 keep the kernel at two waves per SIMD, for one more
// exposed LDS read latency per tile
template <bool DIAG, bool NORM>
__device__ __forceinline__ void trial_bin(const f32x16 (&acc)[4], const int* __restrict__ labs,
                                          const float* __restrict__ nrm, unsigned* __restrict__ hs, int wr, int wc,
                                          int lane, float lo, float inv_width, int n_bins) {
  if constexpr (NORM) {
    trial_bin_rows<DIAG, true, 0, 1>(acc, labs, nrm, hs, wr, wc, lane, lo, inv_width, n_bins);
    trial_bin_rows<DIAG, true, 1, 1>(acc, labs, nrm, hs, wr, wc, lane, lo, inv_width, n_bins);
  } else {
    trial_bin_rows<DIAG, false, 0, 2>(acc, labs, nrm, hs, wr, wc, lane, lo, inv_width, n_bins);
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

// NORM: sv_trial_hist_norm -- the score takes the normalisation step on its way to the slot rule,
// and the tile's per-row constants are staged beside the labels
template <bool NORM>
__global__ __launch_bounds__(256) void trial_hist_kernel(const TrialArgs a) {
  extern __shared__ float lds[];
  float* As = lds;
  float* Bs = As + TR_KC * TR_LD;
  int* labs = reinterpret_cast<int*>(lds + TR_OPERAND_FLOATS);  // [0, 128) rows of A, [128, 256) rows of B
  float* nrm = reinterpret_cast<float*>(labs + 2 * TR_T);       // NORM: [mu_a | inv_a | mu_b | inv_b]
  unsigned* hs = reinterpret_cast<unsigned*>(nrm + (NORM ? 4 * TR_T : 0));
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
    trial_tile_scores(acc, a.A, a.lda, a.Na, i0, a.B, a.ldb, a.Nb, j0, a.D, As, Bs, tid, lane, wr, wc, [&] {
      const bool rows_a = tid < TR_T;
      const long g = (rows_a ? i0 : j0 - TR_T) + tid;
      const bool in = g < (rows_a ? a.Na : a.Nb);
      labs[tid] = in ? (rows_a ? a.lab_a : a.lab_b)[g] : -1;
      if constexpr (NORM) {  // (a row outside is in no pair: its constants are never used)
        nrm[(rows_a ? 0 : TR_T) + tid] = in ? (rows_a ? a.mu_a : a.mu_b)[g] : 0.f;
        nrm[(rows_a ? TR_T : 2 * TR_T) + tid] = in ? (rows_a ? a.inv_a : a.inv_b)[g] : 0.f;
      }
    });
#ifdef SV_TRIAL_STAMP
    const long long c1 = clock64();
#endif
    if (a.symmetric && ti == tj)
      trial_bin<true, NORM>(acc, labs, nrm, hs, wr, wc, lane, a.lo, a.inv_width, a.n_bins);
    else
      trial_bin<false, NORM>(acc, labs, nrm, hs, wr, wc, lane, a.lo, a.inv_width, a.n_bins);
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

// the checks and the launch of both entry points; nrm: {mu_a, inv_a, mu_b, inv_b} or NULL
int trial_hist_launch(const float* A, long lda, const int* lab_a, int Na, const float* B, long ldb, const int* lab_b,
                      int Nb, int D, int symmetric, float lo, float inv_width, int n_bins,
                      const float* const* nrm, unsigned long long* hist, int grid, hipStream_t stream) {
  if (!A || !B || !lab_a || !lab_b || !hist || Na < 1 || Nb < 1 || D < 1 || n_bins < 1 || grid < 0) return SV_EARG;
  if (nrm && (!nrm[0] || !nrm[1] || !nrm[2] || !nrm[3])) return SV_EARG;
  if (symmetric && (A != B || lab_a != lab_b || Na != Nb || lda != ldb)) return SV_EARG;
  if (symmetric && nrm && (nrm[0] != nrm[2] || nrm[1] != nrm[3])) return SV_EARG;
  if ((((uintptr_t)A | (uintptr_t)B) & 15) || (((uintptr_t)lab_a | (uintptr_t)lab_b) & 3) || ((uintptr_t)hist & 7) ||
      lda % 4 || ldb % 4 || D % 4 || lda < D || ldb < D)
    return SV_EALIGN;
  if (nrm && (((uintptr_t)nrm[0] | (uintptr_t)nrm[1] | (uintptr_t)nrm[2] | (uintptr_t)nrm[3]) & 3)) return SV_EALIGN;
  if (n_bins > TR_MAX_BINS || D > TR_MAX_D) return SV_ESHAPE;
  const long long nta = ((long long)Na + TR_T - 1) / TR_T, ntb = ((long long)Nb + TR_T - 1) / TR_T;
  TrialArgs a{A, B, lab_a, lab_b, lda, ldb, Na, Nb, D, symmetric != 0, n_bins, lo, inv_width,
              symmetric ? nta * (nta + 1) / 2 : nta * ntb, (int)ntb, hist,
              nrm ? nrm[0] : nullptr, nrm ? nrm[1] : nullptr, nrm ? nrm[2] : nullptr, nrm ? nrm[3] : nullptr};
  const size_t lds = TR_LDS_FIXED + (nrm ? TR_LDS_NORM : 0) + 2 * ((size_t)n_bins + 2) * 4;
  if (grid == 0) {  // every CU busy; two workgroups on each where the histograms leave room for them
    const int cus = sv_stream_cus(stream);
    const int per_cu = 2 * lds <= 160 * 1024 ? 2 : 1;
    grid = (int)std::min<long long>(a.n_tiles, (long long)(cus > 0 ? cus : 256) * per_cu);
  }
  grid = (int)std::min<long long>(grid, a.n_tiles);
  if (nrm)
    hipLaunchKernelGGL(trial_hist_kernel<true>, dim3(grid), dim3(256), lds, stream, a);
  else
    hipLaunchKernelGGL(trial_hist_kernel<false>, dim3(grid), dim3(256), lds, stream, a);
  SV_LAUNCH_CHECK();
  return SV_OK;
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
  return trial_hist_launch(A, lda, lab_a, Na, B, ldb, lab_b, Nb, D, symmetric, lo, inv_width, n_bins, nullptr, hist,
                           grid, stream);
}

extern "C" int sv_trial_hist_norm(const float* A, long lda, const int* lab_a, int Na, const float* B, long ldb,
                                  const int* lab_b, int Nb, int D, int symmetric, float lo, float inv_width,
                                  int n_bins, const float* mu_a, const float* inv_a, const float* mu_b,
                                  const float* inv_b, unsigned long long* hist, int grid, hipStream_t stream) {
  const float* nrm[4] = {mu_a, inv_a, mu_b, inv_b};
  return trial_hist_launch(A, lda, lab_a, Na, B, ldb, lab_b, Nb, D, symmetric, lo, inv_width, n_bins, nrm, hist, grid,
                           stream);
}
