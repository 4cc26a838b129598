// The library's general fp32 GEMM on gfx950 (sv_gemm_f32 of the C ABI; gemm_f32 inside the library):
// the LSTM stack's input projections, dx and weight-gradient GEMMs, the projection head and the
// GE2E similarity GEMMs all run through it.
//   kernels    gemm_km_kernel (k-major "NT" operands, 64 x 64 / 128 x 128 tiles), gemm_f32_kernel
//              (the other layouts), gemm_f32_narrow_kernel (N <= 48), the 256 x BN LDS-DMA tile
//              (sv_gemm_f32_256.h) and the split-K reduces slab_reduce_kernel / slab_rownorm_kernel
//   host       plan_gemm / plan_gf256 (tile and split-K choice), gemm_f32 (dispatch),
//              sv_gemm_f32_workspace, proj_norm_fused (the projection forward's fused reduce + norm),
//              the dx GEMM on the persistent backward's fragment-order hand-off (gemm_f32_dx_afrag)
//   state      the calling thread's fp32 product mode (F32ProductScope, gemm_x / k2_x / k3_x)
#include <stdlib.h>
#include <algorithm>
#include "sv_common.h"
#include "sv_gemm.h"
#include "sv_gemm_f32_256.h"
#include "../../include/sv_ge2e.h"

// ============================================================================
// generic fp32 GEMM  C[M,N] = op(A) op(B) (+ bias) (+ beta C), or split-K slabs
// ============================================================================
enum { EPI_STORE = 0, EPI_SLAB = 1 };

template <int BM, int BN, bool AK, bool BKC, int EPI>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ A, long lda,
                                                       const float* __restrict__ B, long ldb, float* __restrict__ C,
                                                       long ldc, long slab, int M, int N, int K, int kchunk,
                                                       const float* __restrict__ bias0,
                                                       const float* __restrict__ bias1, float beta) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int TM = BM / 64, TN = BN / 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // column tile fastest: the blocks an XCD runs together share one A row-panel (the large
  // operand, read from HBM once) and sweep the small B operand, which stays cache-resident
  const int tiles_n = (N + BN - 1) / BN;
  const int nwg = tiles_n * ((M + BM - 1) / BM);
  const int id = xcd_remap(blockIdx.x, nwg);
  const int tn = id % tiles_n, tm = id / tiles_n;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);
  const int wm0 = (w >> 1) * (BM / 2), wn0 = (w & 1) * (BN / 2);
  f32x16 acc[TM][TN];
  zero_acc(acc);
  gemm_mainloop<BM, BN, 256, AK, BKC, TM, TN>(A, lda, RowMapLinear{tm * BM, M}, B, ldb, RowMapLinear{tn * BN, N},
                                              kbeg, kend, lds, tid, wm0, wn0, acc);
  float* Cz = C + (EPI == EPI_SLAB ? (long)blockIdx.y * slab : 0);
  // bias sums of the lane's columns, loaded before any store (a load between stores waits for
  // every store issued before it)
  float bsum[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = tn * BN + wn0 + 32 * j + (lane & 31);
    float badd = 0.f;
    if (EPI == EPI_STORE && col < N) {
      if (bias0) badd += bias0[col];
      if (bias1) badd += bias1[col];
    }
    bsum[j] = badd;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = tn * BN + wn0 + 32 * j + (lane & 31);
      if (col >= N) continue;
      const float badd = bsum[j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = tm * BM + wm0 + 32 * i + acc_row(r, lane);
        if (row >= M) continue;
        float v = acc[i][j][r];
        float* dst = Cz + (long)row * ldc + col;
        if (EPI == EPI_STORE) {
          v += badd;
          if (beta != 0.f) v += beta * *dst;
        }
        *dst = v;
      }
    }
}

// out[M,N] (ld ldc) = sum_z slab[z][M,N] (+ beta*out), fixed summation order
__global__ void slab_reduce_kernel(const float* __restrict__ slab, int nz, long zstride, float* __restrict__ out,
                                   long ldc, int M, int N, float beta, const float* __restrict__ bias0,
                                   const float* __restrict__ bias1) {
  const long total = (long)M * N;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int row = (int)(e / N), col = (int)(e % N);
    float s = 0.f;
    for (int z = 0; z < nz; ++z) s += slab[z * zstride + e];
    if (bias0) s += bias0[col];
    if (bias1) s += bias1[col];
    float* dst = out + (long)row * ldc + col;
    *dst = (beta != 0.f ? beta * *dst : 0.f) + s;
  }
}

// k-major ("NT") GEMM: both operands k-contiguous; the fast path for every large GEMM.
// X6 / X3: the bf16x6 / bf16x3 product forms of the `products` argument (sv_lstm_stack_fwd).
template <int BM, int BN, int EPI, int D = 1, bool X6 = false, bool X3 = false>
__global__ __launch_bounds__(256) void gemm_km_kernel(const float* __restrict__ A, long lda, const float* __restrict__ B,
                                                      long ldb, float* __restrict__ C, long ldc, long slab, int M,
                                                      int N, int K, int kchunk, const float* __restrict__ bias0,
                                                      const float* __restrict__ bias1, float beta) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int BLK = 32;                                // MFMA output block edge
  constexpr int TM = BM / 2 / BLK, TN = BN / 2 / BLK;    // blocks per wave (2x2 waves)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // column tile fastest: the blocks an XCD runs together share one A row-panel (the large
  // operand, read from HBM once) and sweep the small B operand, which stays cache-resident
  const int tiles_n = (N + BN - 1) / BN, tiles_m = (M + BM - 1) / BM;
  const int nwg = tiles_n * tiles_m;
  const int id = xcd_remap(blockIdx.x, nwg);
  const int tn = id % tiles_n, tm = id / tiles_n;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);
  const int wm0 = (w >> 1) * (BM / 2), wn0 = (w & 1) * (BN / 2);
  f32x16 acc[TM][TN];
  zero_acc(acc);
  if constexpr (X3)
    gemm_mainloop_x3<BM, BN, 256, 16, 2, TM, TN>(A, lda, RowMapLinear{tm * BM, M}, B, ldb, RowMapLinear{tn * BN, N},
                                                 kbeg, kend, lds, tid, wm0, wn0, acc);
  else
    gemm_mainloop_km_d<BM, BN, 256, SV_BKM, D, TM, TN, false, X6>(A, lda, RowMapLinear{tm * BM, M}, B, ldb,
                                                                RowMapLinear{tn * BN, N}, kbeg, kend, lds, tid, wm0,
                                                                wn0, acc);
  float* Cz = C + (EPI == EPI_SLAB ? (long)blockIdx.y * slab : 0);
  // bias sums of the lane's columns, loaded before any store (a load between stores waits for
  // every store issued before it)
  float bsum[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = tn * BN + wn0 + BLK * j + (lane & (BLK - 1));
    float badd = 0.f;
    if (EPI == EPI_STORE && col < N) {
      if (bias0) badd += bias0[col];
      if (bias1) badd += bias1[col];
    }
    bsum[j] = badd;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = tn * BN + wn0 + BLK * j + (lane & (BLK - 1));
      if (col >= N) continue;
      const float badd = bsum[j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = tm * BM + wm0 + BLK * i + acc_row(r, lane);
        if (row >= M) continue;
        float v = acc[i][j][r];
        float* dst = Cz + (long)row * ldc + col;
        if (EPI == EPI_STORE) {
          v += badd;
          if (beta != 0.f) v += beta * *dst;
        }
        *dst = v;
      }
    }
}

// ============================================================================
// host side
// ============================================================================
// fp32 product mode of the calling thread's current entry point (the `products` argument of
// sv_gemm_f32 / sv_lstm_stack_fwd / sv_lstm_stack_bwd, set for the duration of that call by
// F32ProductScope; every other entry point runs exact):
//   0  exact fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere -- the default
//   1  bf16x6 split where it measured faster: NT GEMMs split in registers (x6), K2 split at the
//      LDS store (x3), K3 exact
//   2  x3 everywhere, 3  x6 everywhere (diagnostics)
namespace {
thread_local int t_f32_mode = 0;
int gemm_x() {  // 0 exact, 1 x6, 2 x3
  const int m = t_f32_mode;
  return m == 1 || m == 3 ? 1 : m == 2 ? 2 : 0;
}
}  // namespace
int k2_x() {
  const int m = t_f32_mode;
  return m == 1 || m == 2 ? 2 : m == 3 ? 1 : 0;
}
int k3_x() {
  const int m = t_f32_mode;
  return m == 2 ? 2 : m == 3 ? 1 : 0;
}
F32ProductScope::F32ProductScope(int mode) : prev(t_f32_mode) { t_f32_mode = mode; }
F32ProductScope::~F32ProductScope() { t_f32_mode = prev; }

namespace {

template <int BM, int BN, bool AK, bool BKC, int EPI>
int launch_gemm_t(const float* A, long lda, const float* B, long ldb, float* C, long ldc, long slab, int M, int N,
                  int K, int splitk, int kchunk, const float* b0, const float* b1, float beta, hipStream_t s) {
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  if (AK && BKC) {
    // KTileStage's buffer loads address a tile's rows with 32-bit byte offsets
    if ((long)BM * lda * 4 >= (1L << 31) || (long)BN * ldb * 4 >= (1L << 31)) return SV_ESHAPE;
    constexpr int LDS_KM = 2 * (BM + BN) * (SV_BKM + 4);
    if (gemm_x() == 2)
      hipLaunchKernelGGL((gemm_km_kernel<BM, BN, EPI, 1, false, true>), dim3(tiles, splitk), dim3(256),
                         12 * (BM + BN) * (16 + 8), s, A, lda, B, ldb, C, ldc, slab, M, N, K, kchunk, b0, b1, beta);
    else if (gemm_x() == 1)
      hipLaunchKernelGGL((gemm_km_kernel<BM, BN, EPI, 1, true>), dim3(tiles, splitk), dim3(256), LDS_KM * sizeof(float),
                         s, A, lda, B, ldb, C, ldc, slab, M, N, K, kchunk, b0, b1, beta);
    else
      hipLaunchKernelGGL((gemm_km_kernel<BM, BN, EPI>), dim3(tiles, splitk), dim3(256), LDS_KM * sizeof(float), s, A,
                         lda, B, ldb, C, ldc, slab, M, N, K, kchunk, b0, b1, beta);
  } else {
    constexpr int LDS_FLOATS = 2 * SV_BK * (TileLd<AK, BM>::value + TileLd<BKC, BN>::value);
    hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, AK, BKC, EPI>), dim3(tiles, splitk), dim3(256),
                       LDS_FLOATS * sizeof(float), s, A, lda, B, ldb, C, ldc, slab, M, N, K, kchunk, b0, b1, beta);
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

template <int BM, int BN, int EPI>
int dispatch_layout(bool ak, bool bk, const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                    long slab, int M, int N, int K, int splitk, int kchunk, const float* b0, const float* b1,
                    float beta, hipStream_t s) {
  if (ak && bk) return launch_gemm_t<BM, BN, true, true, EPI>(A, lda, B, ldb, C, ldc, slab, M, N, K, splitk, kchunk, b0, b1, beta, s);
  if (ak && !bk) return launch_gemm_t<BM, BN, true, false, EPI>(A, lda, B, ldb, C, ldc, slab, M, N, K, splitk, kchunk, b0, b1, beta, s);
  if (!ak && bk) return launch_gemm_t<BM, BN, false, true, EPI>(A, lda, B, ldb, C, ldc, slab, M, N, K, splitk, kchunk, b0, b1, beta, s);
  return launch_gemm_t<BM, BN, false, false, EPI>(A, lda, B, ldb, C, ldc, slab, M, N, K, splitk, kchunk, b0, b1, beta, s);
}

struct GemmPlan {
  int bm, bn, splitk, kchunk;
};

// Tile 128x128 when there are enough tiles to fill the chip, else 64x64.  When the tiles leave
// resident slots (2 blocks/CU x 256 CUs, 4 for 64x64) idle, split K: the split count minimises
// a wave-quantised time model, rounds(tiles*sk / slots) x (time of one K/sk chunk) + the slab
// traffic of the split (sk x M x N x 4 B written and read back), over sk <= 32 with K chunks of
// at least 512.  At the dW shape (144 tiles, K = 102400) this picks 32 splits = 9 full rounds of
// 512 blocks (the old 512/144 = 3 left 80 CUs with one block and the rest with two).
GemmPlan plan_gemm(int M, int N, int K, bool fine = false) {
  GemmPlan p;
  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
  const bool small = t128 < 128;
  p.bm = small ? 64 : 128;
  p.bn = small ? 64 : 128;
  const long tiles = (long)((M + p.bm - 1) / p.bm) * ((N + p.bn - 1) / p.bn);
  const long slots = small ? 1024 : 512;
  int sk = 1;
  if (tiles < slots) {
    // per-block rate at ~120 TF/s shared by all resident blocks; HBM ~5 TB/s for the slabs
    const double rate = 120e12 / (double)slots, hbm = 5e12;
    // K chunks of at least 512, or with `fine` 128 when the tiles alone would leave most of the
    // chip idle (the projection GEMMs: 8-48 tiles of 64 x 64 over K = 256-768 ran 12-24 us on 8-48
    // CUs)
    const int kmax = std::max(1, std::min(32, K / (fine && tiles * 8 < slots ? 128 : 512)));
    double best = 1e30;
    for (int c = 1; c <= kmax; ++c) {
      const long rounds = (tiles * c + slots - 1) / slots;
      const double kc = (double)K / c;
      const double t = rounds * (2.0 * p.bm * p.bn * kc / rate) + (c > 1 ? 2.0 * c * M * N * 4.0 / hbm + 5e-6 : 0.0);
      if (t < best * 0.999) {
        best = t;
        sk = c;
      }
    }
  }
  const int q = SV_BKM;
  p.kchunk = ((K + sk - 1) / sk + q - 1) / q * q;
  p.splitk = (K + p.kchunk - 1) / p.kchunk;
  return p;
}

// ---- narrow NT GEMM (N <= 48): layer 0's dW_ih = dG^T x (M = 4H, N = F = 40, K = T B) ----
// The 64 x 64 tiles (4 waves of v_mfma_f32_32x32x2_f32) padded N = 40 to 64 and ran this shape at
// 75 TF/s (334 us at c2); it streams dG^T (1.26 GB at c2) once.  Here a workgroup is 128 rows x 48
// columns (3 blocks of 16) over a K chunk: v_mfma_f32_16x16x4_f32, exact fp32 products, each wave
// 32 rows (2 x 3 accumulators).  A lane reads 4 consecutive k of its row (one 16-B LDS read) and
// spends them over 4 MFMAs (MFMA j takes k = 4 q + j of lane group q, for A and B alike, so the 4
// MFMAs cover 16 k); LDS images are [rows][32 k] with 16-B chunk c of row r at c ^ (r & 7), filled
// by LDS-DMA (two stages of 32 k).  Split-K slabs, reduced by slab_reduce_kernel.
constexpr int GN_BM = 128, GN_BN = 48, GN_BK = 32;
__global__ __launch_bounds__(256) void gemm_f32_narrow_kernel(const float* __restrict__ A, long lda,
                                                              const float* __restrict__ B, long ldb,
                                                              float* __restrict__ slab, long slab_stride, int M, int N,
                                                              int K, int kchunk) {
  __shared__ __attribute__((aligned(16))) float lds[2][(GN_BM + GN_BN) * GN_BK];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int m0 = blockIdx.x * GN_BM, s = blockIdx.y;
  const int kbeg = s * kchunk, nk = (min(K, kbeg + kchunk) - kbeg) / GN_BK;
  // DMA map: chunk q (16 B) of the stage: A rows 0..127 (q < 1024), then B rows 0..47
  auto fill = [&](int kt, int st) {
    const int k0 = kbeg + kt * GN_BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = tid + 256 * i, row = q >> 3, pc = q & 7, c = pc ^ (row & 7);
      __builtin_amdgcn_global_load_lds((gf_glb_ptr_t)(A + (long)(m0 + row) * lda + k0 + 4 * c),
                                       (gf_lds_ptr_t)(&lds[st][0] + 4 * (w * 64 + 256 * i)), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i == 1 && w >= 2) break;  // 384 chunks of B: waves 0-1 issue a second one (wave-uniform)
      const int q = tid + 256 * i, row = q >> 3, pc = q & 7, c = pc ^ (row & 7);
      const int n = min(row, N - 1);  // padding columns read row N - 1 (their sums are not stored)
      __builtin_amdgcn_global_load_lds((gf_glb_ptr_t)(B + (long)n * ldb + k0 + 4 * c),
                                       (gf_lds_ptr_t)(&lds[st][GN_BM * GN_BK] + 4 * (w * 64 + 256 * i)), 16, 0, 0);
    }
  };
  f32x4 acc[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nk > 0) fill(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int st = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage st landed for every wave; stage st ^ 1 free
    if (kt + 1 < nk) fill(kt + 1, st ^ 1);
    const float* As = &lds[st][0];
    const float* Bs = &lds[st][GN_BM * GN_BK];
#pragma unroll
    for (int ks = 0; ks < GN_BK / 16; ++ks) {
      const int c = 4 * ks + lq;
      f32x4 a[2], b[3];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = 32 * w + 16 * i + lr;
        a[i] = *reinterpret_cast<const f32x4*>(As + row * GN_BK + 4 * (c ^ (row & 7)));
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int row = 16 * j + lr;
        b[j] = *reinterpret_cast<const f32x4*>(Bs + row * GN_BK + 4 * (c ^ (row & 7)));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
    }
  }
  // lane holds C[4 lq + v][lr] of each 16 x 16 block
  float* Cz = slab + (long)s * slab_stride;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int col = 16 * j + lr;
      if (col >= N) continue;
#pragma unroll
      for (int v = 0; v < 4; ++v) Cz[(long)(m0 + 32 * w + 16 * i + 4 * lq + v) * N + col] = acc[i][j][v];
    }
}
// the narrow kernel's plan: exact products, NT, N <= 48, whole 128-row tiles and 32-k steps; K
// chunks of at least 1024 over up to 32 slabs (c2: 24 row tiles x 32 slabs = 768 workgroups)
bool narrow_ok(int M, int N, int K, long lda, long ldb, int mode) {
  return mode == 0 && N <= GN_BN && M % GN_BM == 0 && K % GN_BK == 0 && K >= 4096 && lda % 4 == 0 &&
         ldb % 4 == 0;
}
int narrow_splitk(int K, int& kchunk) {
  const int sk = std::max(1, std::min(32, K / 1024));
  kchunk = ((K + sk - 1) / sk + GN_BK - 1) / GN_BK * GN_BK;
  return (K + kchunk - 1) / kchunk;
}

// ---- 256 x BN LDS-DMA tile (sv_gemm_f32_256.h) for the exact-fp32 NT GEMMs that tile exactly ----
int gf256_bn(int N) { return N % 256 == 0 ? 256 : 128; }
bool gf256_ok(int M, int N, int K, const float* C, long ldc, const float* b0, const float* b1) {
  return M % GF_BM == 0 && N % 128 == 0 && K % GF_BK == 0 && ldc % 4 == 0 &&
         !(((uintptr_t)C | (uintptr_t)b0 | (uintptr_t)b1) & 15);
}
// one workgroup per CU: split K only to fill the CUs (dW: 36 tiles x 7 slabs at c2)
GemmPlan plan_gf256(int M, int N, int K) {
  GemmPlan p;
  p.bm = GF_BM;
  p.bn = gf256_bn(N);
  const long tiles = (long)(M / GF_BM) * (N / p.bn);
  int sk = 1;
  if (tiles < 256) sk = (int)std::max(1L, std::min(256L / tiles, (long)K / 1024));
  p.kchunk = ((K + sk - 1) / sk + GF_BK - 1) / GF_BK * GF_BK;
  p.splitk = (K + p.kchunk - 1) / p.kchunk;
  return p;
}
template <int BN, int EPI>
void launch_gf256(dim3 grid, hipStream_t s, const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                  long slab, int M, int N, int K, int kchunk, const float* b0, const float* b1, float beta) {
  constexpr size_t lds = 2 * (size_t)(GF_BM + BN) * GF_BK * 4;
  hipLaunchKernelGGL((gemm_f32_256_kernel<BN, 32, EPI>), grid, dim3(512), lds, s, A, lda, B, ldb, C, ldc, slab,
                     M, N, K, kchunk, b0, b1, beta);
}
int gemm_f32_256(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N, int K,
                 const float* bias0, const float* bias1, float beta, float* workspace, hipStream_t stream) {
  const GemmPlan p = plan_gf256(M, N, K);
  const int tiles = (M / GF_BM) * (N / p.bn);
  if (p.splitk == 1) {
    const int cus = sv_stream_cus(stream);
    if (p.bn == 256 && beta == 0.f && cus > 0 && tiles > cus && K / GF_BK <= 32 &&
        K / GF_BK >= 2) {
      // more tiles than CUs, short K (K1; dx's 96 k-tiles measured slower persistent, 3.80 vs
      // 3.73 ms): the persistent form (each tile's k-tile 0 fetched during the previous tile)
      hipLaunchKernelGGL((gemm_f32_256p_kernel<256, 32>), dim3(cus), dim3(512),
                         2 * (size_t)(GF_BM + 256) * GF_BK * 4, stream, A, lda, B, ldb, C, ldc, M, N, K, bias0, bias1);
    } else if (p.bn == 256)
      launch_gf256<256, GF_STORE>(dim3(tiles, 1), stream, A, lda, B, ldb, C, ldc, 0L, M, N, K, p.kchunk, bias0, bias1,
                                  beta);
    else
      launch_gf256<128, GF_STORE>(dim3(tiles, 1), stream, A, lda, B, ldb, C, ldc, 0L, M, N, K, p.kchunk, bias0, bias1,
                                  beta);
    SV_LAUNCH_CHECK();
    return SV_OK;
  }
  if (!workspace) return SV_EARG;
  const long slab = (long)M * N;
  if (p.bn == 256)
    launch_gf256<256, GF_SLAB>(dim3(tiles, p.splitk), stream, A, lda, B, ldb, workspace, (long)N, slab, M, N, K,
                               p.kchunk, nullptr, nullptr, 0.f);
  else
    launch_gf256<128, GF_SLAB>(dim3(tiles, p.splitk), stream, A, lda, B, ldb, workspace, (long)N, slab, M, N, K,
                               p.kchunk, nullptr, nullptr, 0.f);
  SV_LAUNCH_CHECK();
  const int grid = (int)std::min<long>((slab + 255) / 256, 4096);
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(grid), dim3(256), 0, stream, workspace, p.splitk, slab, C, ldc, M, N, beta,
                     bias0, bias1);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // namespace

// dx = dG W_ih of the fp32 persistent backward with A read from its fragment-order hand-off
// (gemm_f32_256_kernel AF, GfAFrag): the recurrence then writes no row-major dG.  Exact products,
// whole 256-row tiles, whole 32-row groups per slot, one k-split; else -1 (use the row-major dG).
int dx_afrag_bn(int T, int B, int H, int Fl) {
  if (gemm_x() != 0 || B % 32 || H % 32 || ((long)T * B) % GF_BM) return -1;
  if ((unsigned long long)T * B * B >= (1ull << 32) || 4ull * H * H >= (1ull << 32)) return -1;  // gf_afrag's magic
  const int bn = gf256_bn(Fl);
  if (Fl % bn || plan_gf256(T * B, Fl, 4 * H).splitk != 1) return -1;
  return bn;
}
// stream-K scratch of the dx GEMM (gemm_f32_256sk_kernel): two partial slots of 512 threads x 128
// fp32 per workgroup (grid capped at GF_SK_GRID) + the stream-K tiles' arrival counters
constexpr int GF_SK_GRID = 256;
constexpr size_t GF_SK_SLOT = (size_t)512 * 128 * sizeof(float);
size_t gf_sk_bytes() { return 2 * GF_SK_GRID * GF_SK_SLOT + GF_SK_GRID * sizeof(unsigned) * 4; }
int gemm_f32_dx_afrag(int bn, const float* dgf, int T, int B, int H, const float* wihT, long ldw, int Fl, float* dx,
                      hipStream_t s, void* skws) {
  const long nrb = (B + 63) / 64, fs = nrb * 8 * (H / 8) * 256;
  const GfAFrag af = gf_afrag(dgf, fs, B, H);
  const int M = T * B, K = 4 * H, tiles = (M / GF_BM) * (Fl / bn);
  const size_t lds = 2 * (size_t)(GF_BM + bn) * GF_BK * 4;
  const int G = std::min(sv_stream_cus(s), GF_SK_GRID), nk = K / GF_BK;
  if (skws && bn == 256 && G > 0 && tiles > G && tiles % G) {
    // c2 dx: 1200 tiles on 256 CUs = 4 whole rounds + 176 tiles as 66 k-tiles per workgroup
    GfSK sk;
    sk.R = tiles / G;
    sk.rem = tiles % G;
    sk.L = (int)(((long)sk.rem * nk + G - 1) / G);
    if (sk.L * 3 >= nk) {  // <= GF_SK_MAXSEG pieces per tile
      sk.part = static_cast<float*>(skws);
      sk.cnt = reinterpret_cast<unsigned*>(static_cast<char*>(skws) + 2 * GF_SK_GRID * GF_SK_SLOT);
      hipError_t e = (hipError_t)sv_zero_counters(sk.cnt, 1, 0, sk.rem, s);
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL((gemm_f32_256sk_kernel<256, 1>), dim3(G), dim3(512), lds, s, nullptr, 0L, wihT, ldw, dx,
                         (long)Fl, M, Fl, K, sk, af);
      SV_LAUNCH_CHECK();
      return SV_OK;
    }
  }
  if (bn == 256)
    hipLaunchKernelGGL((gemm_f32_256_kernel<256, 32, GF_STORE, 1>), dim3(tiles, 1), dim3(512), lds, s, nullptr,
                       0L, wihT, ldw, dx, (long)Fl, 0L, M, Fl, K, K, nullptr, nullptr, 0.f, af);
  else
    hipLaunchKernelGGL((gemm_f32_256_kernel<128, 32, GF_STORE, 1>), dim3(tiles, 1), dim3(512), lds, s, nullptr,
                       0L, wihT, ldw, dx, (long)Fl, 0L, M, Fl, K, K, nullptr, nullptr, 0.f, af);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" size_t sv_gemm_f32_workspace(int M, int N, int K) {
  // the larger of the two kernels' split-K slabs (which one runs depends on pointers and mode)
  const GemmPlan p = plan_gemm(M, N, K), pf = plan_gemm(M, N, K, true);  // both plans (gemm_f32's `fine`)
  size_t ws = p.splitk > 1 ? (size_t)p.splitk * M * N * sizeof(float) : 0;
  if (pf.splitk > 1) ws = std::max(ws, (size_t)pf.splitk * M * N * sizeof(float));
  if (M % GF_BM == 0 && N % 128 == 0 && K % GF_BK == 0) {
    const GemmPlan q = plan_gf256(M, N, K);
    if (q.splitk > 1) ws = std::max(ws, (size_t)q.splitk * M * N * sizeof(float));
  }
  if (narrow_ok(M, N, K, K, K, 0)) {  // (the narrow kernel's slabs)
    int kchunk;
    ws = std::max(ws, (size_t)narrow_splitk(K, kchunk) * M * N * sizeof(float));
  }
  return ws;
}

extern "C" int sv_gemm_f32(int a_kcontig, int b_kcontig, int M, int N, int K, const float* A, long lda, const float* B,
                           long ldb, float* C, long ldc, const float* bias0, const float* bias1, float beta,
                           float* workspace, int products, hipStream_t stream) {
  if (products < 0 || products > 3) return SV_EARG;
  F32ProductScope scope(products);
  return gemm_f32(a_kcontig, b_kcontig, M, N, K, A, lda, B, ldb, C, ldc, bias0, bias1, beta, workspace, stream);
}

int gemm_f32(int a_kcontig, int b_kcontig, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
             float* C, long ldc, const float* bias0, const float* bias1, float beta, float* workspace,
             hipStream_t stream, bool fine) {
  if (M <= 0 || N <= 0 || K <= 0 || !A || !B || !C) return SV_EARG;
  if (a_kcontig ? (K % 4 || lda % 4) : (M % 4 || lda % 4)) return SV_EALIGN;
  if (b_kcontig ? (K % 4 || ldb % 4) : (N % 4 || ldb % 4)) return SV_EALIGN;
  if (((uintptr_t)A | (uintptr_t)B) & 15) return SV_EALIGN;
  if (a_kcontig && b_kcontig && gemm_x() == 0 && gf256_ok(M, N, K, C, ldc, bias0, bias1))
    return gemm_f32_256(A, lda, B, ldb, C, ldc, M, N, K, bias0, bias1, beta, workspace, stream);
  if (a_kcontig && b_kcontig && workspace && narrow_ok(M, N, K, lda, ldb, gemm_x())) {
    int kchunk;
    const int sk = narrow_splitk(K, kchunk);
    const long slab = (long)M * N;
    hipLaunchKernelGGL(gemm_f32_narrow_kernel, dim3(M / GN_BM, sk), dim3(256), 0, stream, A, lda, B, ldb, workspace,
                       slab, M, N, K, kchunk);
    SV_LAUNCH_CHECK();
    const int grid = (int)std::min<long>((slab + 255) / 256, 4096);
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(grid), dim3(256), 0, stream, workspace, sk, slab, C, ldc, M, N, beta, bias0,
                       bias1);
    SV_LAUNCH_CHECK();
    return SV_OK;
  }
  const GemmPlan p = plan_gemm(M, N, K, fine && workspace != nullptr);
  const bool ak = a_kcontig != 0, bk = b_kcontig != 0;
  if (p.splitk == 1) {
    if (p.bm == 64)
      return dispatch_layout<64, 64, EPI_STORE>(ak, bk, A, lda, B, ldb, C, ldc, 0, M, N, K, 1, p.kchunk, bias0, bias1, beta, stream);
    return dispatch_layout<128, 128, EPI_STORE>(ak, bk, A, lda, B, ldb, C, ldc, 0, M, N, K, 1, p.kchunk, bias0, bias1, beta, stream);
  }
  if (!workspace) return SV_EARG;
  const long slab = (long)M * N;
  int rc;
  if (p.bm == 64)
    rc = dispatch_layout<64, 64, EPI_SLAB>(ak, bk, A, lda, B, ldb, workspace, N, slab, M, N, K, p.splitk, p.kchunk, nullptr, nullptr, 0.f, stream);
  else
    rc = dispatch_layout<128, 128, EPI_SLAB>(ak, bk, A, lda, B, ldb, workspace, N, slab, M, N, K, p.splitk, p.kchunk, nullptr, nullptr, 0.f, stream);
  if (rc) return rc;
  const long total = slab;
  const int grid = (int)std::min<long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(grid), dim3(256), 0, stream, workspace, p.splitk, slab, C, ldc, M, N, beta,
                     bias0, bias1);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// the projection's split-K slabs summed and the rows normalised in one launch (one wave per row,
// P <= 256): y = sum_z slab[z] + bias in slab_reduce_kernel's order, emb = y / |y| and |y| in
// rownorm_fwd_kernel's (sv_misc.hip) -- the two launches' results bit for bit, one launch fewer
#define SR_NZ 8
__global__ __launch_bounds__(256) void slab_rownorm_kernel(const float* __restrict__ slab, int nz, long zstride, int B,
                                                           int P, const float* __restrict__ bias, float* __restrict__ y,
                                                           float* __restrict__ emb, float* __restrict__ ynorm) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= B) return;
  // every slab value of the lane's 4 columns loaded at once (nz <= SR_NZ: one round trip, where a
  // loop over z waited for each load in turn), then summed in z order
  float x[SR_NZ][4], bv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = lane + 64 * j;
    bv[j] = (bias && p < P) ? bias[p] : 0.f;
#pragma unroll
    for (int z = 0; z < SR_NZ; ++z) x[z][j] = (z < nz && p < P) ? slab[z * zstride + (long)r * P + p] : 0.f;
  }
  float v[4];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = lane + 64 * j;
    if (p < P) {
      float s = 0.f;
#pragma unroll
      for (int z = 0; z < SR_NZ; ++z)
        if (z < nz) s += x[z][j];
      if (bias) s += bv[j];
      v[j] = 0.f + s;  // (slab_reduce_kernel's store with beta = 0)
      y[(long)r * P + p] = v[j];
      ss += v[j] * v[j];
    }
  }
  const float n = sqrtf(wave_sum(ss));
  const float inv = 1.0f / n;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = lane + 64 * j;
    if (p < P) emb[(long)r * P + p] = v[j] * inv;
  }
  if (lane == 0) ynorm[r] = n;
}

// y = h W^T + b (h [B,K], W [P,K], both k-contiguous) with the row norm fused into the split-K
// reduce where gemm_f32 would take that form (P <= 256, P % 4 == 0); returns 1 if it ran, 0 if
// the caller should take gemm_f32 + its own norm
int proj_norm_fused(const float* h, int B, int K, int P, const float* W, const float* bias, float* y, float* emb,
                    float* ynorm, float* workspace, hipStream_t stream, int* rc) {
  *rc = SV_OK;
  if (!workspace || P > 256 || P % 4 || K % 4 || (((uintptr_t)h | (uintptr_t)W) & 15) || gemm_x() != 0) return 0;
  if (gf256_ok(B, P, K, y, P, bias, nullptr) || narrow_ok(B, P, K, K, K, 0)) return 0;
  const GemmPlan p = plan_gemm(B, P, K, true);
  if (p.splitk <= 1 || p.splitk > SR_NZ) return 0;
  const long slab = (long)B * P;
  if (p.bm == 64)
    *rc = dispatch_layout<64, 64, EPI_SLAB>(true, true, h, K, W, K, workspace, P, slab, B, P, K, p.splitk, p.kchunk,
                                            nullptr, nullptr, 0.f, stream);
  else
    *rc = dispatch_layout<128, 128, EPI_SLAB>(true, true, h, K, W, K, workspace, P, slab, B, P, K, p.splitk, p.kchunk,
                                              nullptr, nullptr, 0.f, stream);
  if (*rc) return 1;
  hipLaunchKernelGGL(slab_rownorm_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, workspace, p.splitk, slab, B, P, bias,
                     y, emb, ynorm);
  *rc = (int)hipGetLastError();
  return 1;
}

