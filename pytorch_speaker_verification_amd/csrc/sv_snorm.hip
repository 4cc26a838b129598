// Per-row top-K cohort statistics for adaptive score normalisation (sv_cohort_topk_stats of the C
// ABI): for every row i of X [N][D] the mean and the population standard deviation of the top_k
// largest of the Nc scores s_c = X[i] . C[c], without writing a score and without a workspace.
//   scores   the 128 x 128 tile of sv_trial_tile.h (the k-loop of sv_trial_hist): a workgroup of 256
//            threads owns a block of 128 rows of X and streams every 128-row cohort tile once per
//            pass.  Every pass recomputes the tile with the same code in the same k order, so a
//            pair's score has the same bits in all of them.
//   key      the order-preserving 32-bit key of a fp32 score: all bits flipped for a negative (sign
//            bit set), the sign bit flipped otherwise; a NaN takes 0xffffffff, above +inf.  -0 sorts
//            just below +0, which no value statistic can see.
//   select   an MSD radix select with 8-bit digits: in pass p = 0 .. 3 every score whose key agrees
//            with the row's prefix in the 8 p digits fixed so far adds 1 to the row's 256-bin
//            histogram of the next digit (a no-return LDS atomic on a packed 16-bit counter).  After
//            the pass two threads per row walk the bins from the top -- the totals of the upper and
//            lower 128 bins decide which of the two holds the crossing -- fix the digit and lower
//            the count still wanted by the scores above it.  After four passes the prefix is tau, the
//            key of the top_k-th largest score, and `want` = top_k - n_gt copies of tau belong to
//            the top_k, n_gt the number of scores strictly above tau.
//   sums     pass 4: every score above tau adds d = s - tau and d^2, in fp64, to the lane's sums of
//            its row (the copies of tau add nothing); the 32 lanes and 2 waves that share a row are
//            combined in a fixed order, so the result depends on neither the grid nor arrival order.
//            mean = tau + S1 / K, var = S2 / K - (S1 / K)^2 -- shifted by tau the subtraction loses at
//            most a factor K of fp64's 2^-53, because d = 0 is always among the K values.
//   LDS      33 792 B of operands + 128 rows x 129 words of packed histograms (66 048 B: two 16-bit
//            counters per word hold a row's 256 bins, a bin counts at most Nc <= 65 535 scores, and
//            the odd row stride spreads the rows over the banks) + 1 KB of row state + 4 KB for the
//            combination of the sums = 104 960 B: one workgroup per CU.  (32-bit counters would be
//            131 072 B + operands, past the 160 KB of a CU.)
// -DSV_SNORM_STAMP (an A/B build, never the shipped library): wave 0's cycles inside each of the five
// passes, summed over the workgroups, in a device array read and cleared by sv_snorm_stamp_read.
#include "sv_trial_tile.h"
#include "../../include/sv_ge2e.h"

#include <algorithm>

namespace {

constexpr int SN_BINS = 256, SN_HLD = SN_BINS / 2 + 1;  // words per row: 128 packed pairs + 1 of padding
constexpr int SN_PASSES = 4;                            // 8-bit digits of the 32-bit key
constexpr int SN_MAX_NC = 65535;
constexpr size_t SN_LDS = (size_t)(TR_OPERAND_FLOATS + TR_T * SN_HLD + 2 * TR_T) * 4 + (size_t)2 * TR_T * 2 * 8;

struct SnormArgs {
  const float *X, *C;
  long ldx, ldc;
  int N, Nc, D, top_k;
  float *mean, *std;
  int n_blocks;
};

#ifdef SV_SNORM_STAMP
__device__ unsigned long long snorm_cycles[SN_PASSES + 1];
#endif

__device__ __forceinline__ unsigned snorm_key(float s) {
  const unsigned u = __float_as_uint(s);
  return s != s ? 0xffffffffu : (u & 0x80000000u) ? ~u : u | 0x80000000u;
}

__device__ __forceinline__ float snorm_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? k & 0x7fffffffu : ~k);
}

__device__ __forceinline__ unsigned snorm_count(const unsigned* __restrict__ h, int bin) {
  return (h[bin >> 1] >> ((bin & 1) * 16)) & 0xffffu;
}

// one pass over the cohort for the row block at i0.  PASS < SN_PASSES: the digit histograms of the
// scores that match the rows' prefixes; PASS == SN_PASSES: the lanes' fp64 sums above tau
template <int PASS>
__device__ __forceinline__ void snorm_pass(const SnormArgs& a, long i0, float* As, float* Bs, unsigned* hist,
                                           const unsigned* prefix, double* fin, int tid, int lane, int wr, int wc) {
  constexpr bool FINAL = PASS == SN_PASSES;
  constexpr int shift = FINAL ? 0 : 24 - 8 * PASS;
  constexpr unsigned fixed = PASS == 0 ? 0u : FINAL ? 0xffffffffu : 0xffffffffu << (shift + 8);
  unsigned pre[2][16];  // prefix, after the last select pass tau, of the lane's 32 rows
  if constexpr (PASS > 0)
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int r = 0; r < 16; ++r) pre[bi][r] = prefix[wr + bi * 32 + acc_row(r, lane)];
  double s1[FINAL ? 2 : 1][16], s2[FINAL ? 2 : 1][16];
  if constexpr (FINAL)
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int r = 0; r < 16; ++r) s1[bi][r] = s2[bi][r] = 0.0;
  for (long j0 = 0; j0 < a.Nc; j0 += TR_T) {
    f32x16 acc[4];
    trial_tile_scores(acc, a.X, a.ldx, a.N, i0, a.C, a.ldc, a.Nc, j0, a.D, As, Bs, tid, lane, wr, wc, [] {});
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const bool live = j0 + wc + (b & 1) * 32 + (lane & 31) < a.Nc;  // a cohort row, not padding
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float s = acc[b][r];
        const unsigned key = snorm_key(s);
        if constexpr (FINAL) {
          const unsigned tau = pre[b >> 1][r];
          if (live && key > tau) {
            const double d = (double)s - (double)snorm_unkey(tau);
            s1[b >> 1][r] += d;
            s2[b >> 1][r] = fma(d, d, s2[b >> 1][r]);
          }
        } else {
          bool match = live;
          if constexpr (PASS > 0) match = match && ((key ^ pre[b >> 1][r]) & fixed) == 0;
          const unsigned dg = (key >> shift) & 255u;
          if (match) atomicAdd(hist + (wr + (b >> 1) * 32 + acc_row(r, lane)) * SN_HLD + (dg >> 1), 1u << ((dg & 1) * 16));
        }
      }
    }
  }
  if constexpr (FINAL) {  // the 32 lanes of a row in a fixed tree, then one slot per wave column
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        double u = s1[bi][r], v = s2[bi][r];
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {
          u += __shfl_xor(u, m);
          v += __shfl_xor(v, m);
        }
        if ((lane & 31) == 0) {
          double* f = fin + ((wc >> 6) * TR_T + wr + bi * 32 + acc_row(r, lane)) * 2;
          f[0] = u;
          f[1] = v;
        }
      }
  }
}

// after select pass PASS: two threads per row fix the next digit of the row's prefix from its
// histogram and lower `want` by the scores above that digit.  h = 0 owns the bins 255 .. 128, h = 1
// the bins 127 .. 0; the thread whose half holds the crossing walks it from the top.  The matching
// scores of a row are never fewer than `want` (all Nc >= top_k at the start; afterwards the count
// of the chosen bin), so the walk ends inside the half.
template <int PASS>
__device__ __forceinline__ void snorm_walk(const unsigned* __restrict__ hist, unsigned* prefix, unsigned* want,
                                           int tid) {
  constexpr int shift = 24 - 8 * PASS;
  const int row = tid >> 1, h = tid & 1;
  const unsigned* hr = hist + row * SN_HLD + (h ? 0 : SN_BINS / 4);
  unsigned total = 0;
  for (int w = 0; w < SN_BINS / 4; ++w) total += (hr[w] & 0xffffu) + (hr[w] >> 16);
  const unsigned upper = __shfl(total, (tid & 63) & ~1);  // the pair's h = 0 thread
  // both threads of the pair read want[row] and one of them writes it below, with no barrier between:
  // they are adjacent lanes of one wave, and the read comes first in program order
  const unsigned w0 = want[row];
  const bool mine = h == 0 ? upper >= w0 : upper < w0;
  if (mine) {
    const unsigned w = h == 0 ? w0 : w0 - upper;
    unsigned above = 0;
    int bin = SN_BINS / 2 - 1;
    for (; bin > 0; --bin) {
      const unsigned c = snorm_count(hr, bin);
      if (above + c >= w) break;
      above += c;
    }
    prefix[row] |= (unsigned)(bin + (h ? 0 : SN_BINS / 2)) << shift;
    want[row] = w - above;
  }
}

template <int PASS>
__device__ __forceinline__ void snorm_select(const SnormArgs& a, long i0, float* As, float* Bs, unsigned* hist,
                                             unsigned* prefix, unsigned* want, int tid, int lane, int wr, int wc) {
  snorm_pass<PASS>(a, i0, As, Bs, hist, prefix, nullptr, tid, lane, wr, wc);
  __syncthreads();  // every wave's adds
  snorm_walk<PASS>(hist, prefix, want, tid);
  __syncthreads();  // the walks' reads; the row state for the next pass
  for (int i = tid; i < TR_T * SN_HLD; i += 256) hist[i] = 0;  // (the next tile's barriers order this)
}

#ifdef SV_SNORM_STAMP
#define SN_STAMP(p)                                                                   \
  do {                                                                                \
    const long long c__ = clock64();                                                  \
    if (tid == 0) atomicAdd(snorm_cycles + (p), (unsigned long long)(c__ - stamp__)); \
    stamp__ = c__;                                                                    \
  } while (0)
#else
#define SN_STAMP(p)
#endif

__global__ __launch_bounds__(256) void cohort_topk_stats_kernel(const SnormArgs a) {
  extern __shared__ float lds[];
  float* As = lds;
  float* Bs = As + TR_KC * TR_LD;
  unsigned* hist = reinterpret_cast<unsigned*>(lds + TR_OPERAND_FLOATS);  // [128][SN_HLD]
  unsigned* prefix = hist + TR_T * SN_HLD;                                // [128]
  unsigned* want = prefix + TR_T;                                         // [128]
  double* fin = reinterpret_cast<double*>(want + TR_T);                   // [2][128][2] (8-byte aligned)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
  for (int i = tid; i < TR_T * SN_HLD; i += 256) hist[i] = 0;
  for (int rb = blockIdx.x; rb < a.n_blocks; rb += gridDim.x) {
    const long i0 = (long)rb * TR_T;
#ifdef SV_SNORM_STAMP
    long long stamp__ = clock64();
#endif
    __syncthreads();  // the last block's reads of the row state and of fin
    if (tid < TR_T) {
      prefix[tid] = 0;
      want[tid] = (unsigned)a.top_k;
    }
    snorm_select<0>(a, i0, As, Bs, hist, prefix, want, tid, lane, wr, wc);
    SN_STAMP(0);
    snorm_select<1>(a, i0, As, Bs, hist, prefix, want, tid, lane, wr, wc);
    SN_STAMP(1);
    snorm_select<2>(a, i0, As, Bs, hist, prefix, want, tid, lane, wr, wc);
    SN_STAMP(2);
    snorm_select<3>(a, i0, As, Bs, hist, prefix, want, tid, lane, wr, wc);
    SN_STAMP(3);
    snorm_pass<SN_PASSES>(a, i0, As, Bs, hist, prefix, fin, tid, lane, wr, wc);
    __syncthreads();
    if (tid < TR_T && i0 + tid < a.N) {
      const double k = (double)a.top_k, tau = (double)snorm_unkey(prefix[tid]);
      const double m = (fin[tid * 2] + fin[(TR_T + tid) * 2]) / k;
      const double var = (fin[tid * 2 + 1] + fin[(TR_T + tid) * 2 + 1]) / k - m * m;
      a.mean[i0 + tid] = (float)(tau + m);
      // the NaN rule of the header: a NaN above tau is in the sums (this comparison keeps it), a NaN tau is not
      a.std[i0 + tid] = tau != tau ? (float)tau : (float)sqrt(var < 0.0 ? 0.0 : var);
    }
    SN_STAMP(4);
  }
}

}  // namespace

extern "C" int sv_cohort_topk_stats(const float* X, long ldx, int N, const float* C, long ldc, int Nc, int D,
                                    int top_k, float* mean, float* std, int grid, hipStream_t stream) {
  if (!X || !C || !mean || !std || N < 1 || Nc < 1 || D < 1 || top_k < 1 || top_k > Nc || grid < 0) return SV_EARG;
  if ((((uintptr_t)X | (uintptr_t)C) & 15) || (((uintptr_t)mean | (uintptr_t)std) & 3) || ldx % 4 || ldc % 4 || D % 4 ||
      ldx < D || ldc < D)
    return SV_EALIGN;
  if (Nc > SN_MAX_NC || D > TR_MAX_D) return SV_ESHAPE;
  const int n_blocks = (int)(((long long)N + TR_T - 1) / TR_T);
  SnormArgs a{X, C, ldx, ldc, N, Nc, D, top_k, mean, std, n_blocks};
  if (grid == 0) {  // one workgroup per CU: the histograms take two thirds of its LDS
    const int cus = sv_stream_cus(stream);
    grid = cus > 0 ? cus : 256;
  }
  grid = std::min(grid, n_blocks);
  hipLaunchKernelGGL(cohort_topk_stats_kernel, dim3(grid), dim3(256), SN_LDS, stream, a);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

#ifdef SV_SNORM_STAMP
// out[5] := wave 0's cycles in the passes 0 .. 4 since the last call, summed over the workgroups
extern "C" int sv_snorm_stamp_read(unsigned long long* out) {
  unsigned long long zero[SN_PASSES + 1] = {};
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(snorm_cycles), sizeof(zero));
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(snorm_cycles), zero, sizeof(zero));
  return (int)e;
}
#endif
