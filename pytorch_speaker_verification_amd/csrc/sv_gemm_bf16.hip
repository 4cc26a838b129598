// The bf16 GEMMs of the library (operands bf16, both k-contiguous; fp32 accumulation on
// v_mfma_f32_32x32x16_bf16): the general kernel with its split-K planner, the 256 x 256 kernels'
// launchers (sv_gemm256.h), the narrow kernel for N <= 48, the fused pair and the whole-K launch of
// the weight gradients, the dx GEMM on the fragment-order hand-off, and the entry points
// sv_gemm_bf16 / sv_gemm_bf16_bf (include/sv_ge2e.h).  The bf16 LSTM glue (sv_bf16.hip) enqueues
// them through that ABI and sv_gemm_bf16.h.
#include <algorithm>
#include "sv_common.h"
#include "sv_gemm.h"
#include "../../include/sv_ge2e.h"
#include "sv_bf16.h"
#include "sv_gemm256.h"
#include "sv_persist_dev.h"
#include "sv_gemm_bf16.h"

// ============================================================================
// GEMM: C[M,N] fp32 = A[M,K] . B[N,K]^T (bf16, both k-contiguous) (+bias) / split-K slabs
// ============================================================================
enum { BEPI_STORE = 0, BEPI_SLAB = 1, BEPI_STORE_BF16 = 2 };

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(const bf16_t* __restrict__ A, long lda,
                                                        const bf16_t* __restrict__ B, long ldb, void* __restrict__ Cv,
                                                        long ldc, long slab, int M, int N, int K, int kchunk,
                                                        const float* __restrict__ bias0,
                                                        const float* __restrict__ bias1, float beta) {
  extern __shared__ __attribute__((aligned(16))) bf16_t ldsb[];
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
  gemm_mainloop_bf<BM, BN, 256, BBK, TM, TN>(A, lda, RowMapLinear{tm * BM, M}, B, ldb, RowMapLinear{tn * BN, N}, kbeg,
                                             kend, ldsb, tid, wm0, wn0, acc);
  float* Cz = reinterpret_cast<float*>(Cv) + (EPI == BEPI_SLAB ? (long)blockIdx.y * slab : 0);
  // bias sums of the lane's columns, loaded before any store (a load between stores waits for
  // every store issued before it)
  float bsum[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = tn * BN + wn0 + 32 * j + (lane & 31);
    float badd = 0.f;
    if (EPI != BEPI_SLAB && col < N) {
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
        if (EPI == BEPI_STORE_BF16) {
          reinterpret_cast<bf16_t*>(Cv)[(long)row * ldc + col] = to_bf(v + badd);
          continue;
        }
        float* dst = Cz + (long)row * ldc + col;
        if (EPI == BEPI_STORE) {
          v += badd;
          if (beta != 0.f) v += beta * *dst;
        }
        *dst = v;
      }
    }
}

__global__ void slab_reduce_bf_kernel(const float* __restrict__ slab, int nz, long zstride, float* __restrict__ out,
                                      long ldc, int M, int N, float beta, const float* __restrict__ bias0,
                                      const float* __restrict__ bias1, bf16_t* __restrict__ outb = nullptr,
                                      float* __restrict__ out2 = nullptr, long ldc2 = 0, int n1 = 0) {
  const long total = (long)M * N;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int row = (int)(e / N), col = (int)(e % N);
    float s = 0.f;
    for (int z = 0; z < nz; ++z) s += slab[z * zstride + e];
    if (out2 && col >= n1) {  // fused pair: columns past n1 belong to the second product
      out2[(long)row * ldc2 + col - n1] = s;
      continue;
    }
    if (bias0) s += bias0[col];
    if (bias1) s += bias1[col];
    if (outb) {  // bf16 output (beta unused)
      outb[(long)row * ldc + col] = to_bf(s);
      continue;
    }
    float* dst = out + (long)row * ldc + col;
    *dst = (beta != 0.f ? beta * *dst : 0.f) + s;
  }
}

namespace {

struct BPlan {
  int bm, bn, splitk, kchunk;
};

// the 256 x 256 tile's schedule: the 8-phase kernel (gemm_bf16_8q_kernel) where its 16-B
// epilogue stores are aligned (C rows, biases), else the two-stage gemm_bf16_256_kernel
bool g8_ok(const void* C, long ldc, const float* bias0, const float* bias1) {
  return !((((uintptr_t)C | (uintptr_t)bias0 | (uintptr_t)bias1) & 15) || ldc % 4);
}

// the 8-phase kernel with two LDS-DMA fills per phase.  Measured against one or two fill phases
// per k-tile (c3 shapes, us): dW 414 vs 445-446, dx 440 vs 471-480, K1 (bf16 out) 615 vs 626.
template <int EPI, int AF>
void launch_g8(dim3 grid, hipStream_t stream, const bf16_t* A, long lda, const bf16_t* B, long ldb, void* C, long ldc,
               long slab, int M, int N, int K, int kchunk, const float* bias0, const float* bias1, float beta,
               G256AFrag af = G256AFrag{}) {
  hipLaunchKernelGGL((gemm_bf16_8q_kernel<EPI, AF>), grid, dim3(512), G256_LDS, stream, A, lda, B, ldb, C, ldc, slab,
                     M, N, K, kchunk, bias0, bias1, beta, af);
}

template <int EPI, int AF>
void launch_g256(bool g8, dim3 grid, hipStream_t stream, const bf16_t* A, long lda, const bf16_t* B, long ldb, void* C,
                 long ldc, long slab, int M, int N, int K, int kchunk, const float* bias0, const float* bias1,
                 float beta, G256AFrag af = G256AFrag{}) {
  if (g8)
    launch_g8<EPI, AF>(grid, stream, A, lda, B, ldb, C, ldc, slab, M, N, K, kchunk, bias0, bias1, beta, af);
  else
    hipLaunchKernelGGL((gemm_bf16_256_kernel<EPI, AF>), grid, dim3(512), G256_LDS, stream, A, lda, B, ldb, (float*)C,
                       ldc, slab, M, N, K, kchunk, bias0, bias1, beta, af);
}

BPlan plan_bf16(int M, int N, int K) {
  BPlan p;
  if (gemm256_ok(M, N, K)) {  // one workgroup per CU: split K only to fill the 256 CUs
    // ... and only for the long weight-gradient reductions (K = T B): a dx GEMM (K = 4H) then sums
    // K in one order whether it runs per 32-step chunk (per-step schedule) or over all T (the
    // persistent schedule's fragment-order form), so the two schedules stay bit-identical
    const long tiles = (long)(M / G256_BM) * (N / G256_BM);
    int sk = 1;
    if (tiles < 256 && K >= 8192) sk = (int)std::max(1L, std::min(256L / tiles, (long)K / 1024));
    p.bm = p.bn = G256_BM;
    p.kchunk = ((K + sk - 1) / sk + G256_BK - 1) / G256_BK * G256_BK;
    p.splitk = (K + p.kchunk - 1) / p.kchunk;
    return p;
  }
  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
  const bool small = t128 < 128;
  p.bm = p.bn = small ? 64 : 128;
  const long tiles = (long)((M + p.bm - 1) / p.bm) * ((N + p.bn - 1) / p.bn);
  const long slots = small ? 1024 : 512;
  int sk = 1;
  if (tiles < slots) {  // the wave-quantised split-K model of plan_gemm (sv_gemm_f32.hip), at ~600 TF/s
    const double rate = 600e12 / (double)slots, hbm = 5e12;
    const int kmax = std::max(1, std::min(32, K / 1024));
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
  p.kchunk = ((K + sk - 1) / sk + BBK - 1) / BBK * BBK;
  p.splitk = (K + p.kchunk - 1) / p.kchunk;
  return p;
}

template <int BM, int BN, int EPI>
void launch_bf(const bf16_t* A, long lda, const bf16_t* B, long ldb, void* C, long ldc, long slab, int M, int N, int K,
               int splitk, int kchunk, const float* b0, const float* b1, float beta, hipStream_t s) {
  constexpr int LDS = 2 * (BM + BN) * (BBK + 8) * (int)sizeof(bf16_t);
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  hipLaunchKernelGGL((gemm_bf16_kernel<BM, BN, EPI>), dim3(tiles, splitk), dim3(256), LDS, s, A, lda, B, ldb, C, ldc,
                     slab, M, N, K, kchunk, b0, b1, beta);
}

// every layer's whole-K weight-gradient tiles in one launch (G8Full, sv_gemm_bf16.h)
__global__ __launch_bounds__(512, 1) void gemm_bf16_8qf_kernel(const G8Full q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 2, wc = w & 3;
  const G8FLayer& L2 = q.lay[2];
  const G8FLayer& L1 = q.lay[1];
  const G8FLayer& L0 = q.lay[0];
  const int P = L2.tiles + L1.tiles + L0.tiles;
  if ((int)blockIdx.x >= q.nsw + P) {  // the deferred bias finalize (the highest blocks: nobody waits on them)
    dbfin_run(q.fin, blockIdx.x - q.nsw - P);
    return;
  }
  // tile r (top layer first) -> its operands (field-wise selects: a dynamic index into the
  // kernel-argument struct would copy it to scratch)
  auto run = [&](int r, int kbeg, int nk, g8_f32x4 (&acc)[8][4], int& l, int& tm, int& tn) {
    l = r < L2.tiles ? 2 : r < L2.tiles + L1.tiles ? 1 : 0;
    const int tile = l == 2 ? r : l == 1 ? r - L2.tiles : r - L2.tiles - L1.tiles;
    const bf16_t* A = l == 2 ? L2.A : l == 1 ? L1.A : L0.A;
    const bf16_t* Bm = l == 2 ? L2.B : l == 1 ? L1.B : L0.B;
    const bf16_t* B2 = l == 2 ? L2.B2 : l == 1 ? L1.B2 : L0.B2;
    const long lda = l == 2 ? L2.lda : l == 1 ? L1.lda : L0.lda;
    const long ldb = l == 2 ? L2.ldb : l == 1 ? L1.ldb : L0.ldb;
    const long ldb2 = l == 2 ? L2.ldb2 : l == 1 ? L1.ldb2 : L0.ldb2;
    const int N = l == 2 ? L2.N : l == 1 ? L1.N : L0.N;
    const int n1 = l == 2 ? L2.n1 : l == 1 ? L1.n1 : L0.n1;
    const int f2 = l == 2 ? L2.f2 : l == 1 ? L1.f2 : L0.f2;
    const int tiles_n = N / G256_BM;
    tn = tile % tiles_n;
    tm = tile / tiles_n;
    g8_tile<0>(A, lda, Bm, ldb, G256AFrag{}, G256Dual{B2, ldb2, n1, f2}, tm, tn, kbeg, nk, smem, acc);
  };
  g8_f32x4 acc[8][4];
  int l, tm, tn;
  if ((int)blockIdx.x < q.nsw) {  // first pieces
    for (int j = blockIdx.x; j < P; j += q.nsw) {
      run(j, 0, q.S, acc, l, tm, tn);
      const __amdgpu_buffer_rsrc_t rp = sv_rsrc(q.part + (long)j * G256_BM * G256_BM, G256_BM * G256_BM * 4u);
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        const g8_f32x4 v = acc[i >> 2][i & 3];
        __builtin_amdgcn_raw_buffer_store_b128(
            u32x4_t{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])}, rp,
            (unsigned)(i * 512 + tid) * 16u, 0, 16 /* sc1 */);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) __hip_atomic_fetch_add(q.flag + j, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  // position after xcd_remap (nsw % 8 == 0, so blocks nsw + i keep i's XCD): each XCD owns a
  // contiguous run, so a row tile's column tiles (the same dG^T rows) share an L2
  const int r = xcd_remap((int)blockIdx.x - q.nsw, P);
  run(r, q.S * G256_BK, q.K / G256_BK - q.S, acc, l, tm, tn);
  if (q.S > 0) {
    if (tid == 0) persist_wait(q.flag + r, 1u, q.status, q.limit, 2u);
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rp = sv_rsrc(q.part + (long)r * G256_BM * G256_BM, G256_BM * G256_BM * 4u);
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const u32x4_t x = __builtin_amdgcn_raw_buffer_load_b128(rp, (unsigned)(i * 512 + tid) * 16u, 0, 16 /* sc1 */);
      acc[i >> 2][i & 3] += g8_f32x4{__uint_as_float(x[0]), __uint_as_float(x[1]), __uint_as_float(x[2]),
                                     __uint_as_float(x[3])};
    }
  }
  float* C1 = l == 2 ? L2.C1 : l == 1 ? L1.C1 : L0.C1;
  float* C2 = l == 2 ? L2.C2 : l == 1 ? L1.C2 : L0.C2;
  const long ldc1 = l == 2 ? L2.ldc1 : l == 1 ? L1.ldc1 : L0.ldc1;
  const long ldc2 = l == 2 ? L2.ldc2 : l == 1 ? L1.ldc2 : L0.ldc2;
  const int n1 = l == 2 ? L2.n1 : l == 1 ? L1.n1 : L0.n1;
  const int f2 = l == 2 ? L2.f2 : l == 1 ? L1.f2 : L0.f2;
  const bool second = tn * G256_BM >= n1;  // n1 % 256 == 0 (host): a tile is all C1 or all C2
  g8_epilogue<G8_STORE>(acc, second ? C2 : C1, second ? ldc2 : ldc1, 0, tm, second ? tn - n1 / G256_BM : tn, wr, wc,
                        lane, nullptr, nullptr, 0.f, second && f2 > 0 ? f2 : 1 << 30);
}

}  // namespace

int gemm_bf16_fullk(const G8Full& q, int P, hipStream_t stream) {
  hipLaunchKernelGGL(gemm_bf16_8qf_kernel, dim3(q.nsw + P + dbfin_blocks(q.fin, 512)), dim3(512), G256_LDS, stream, q);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ---- narrow bf16 NT GEMM (N <= 48): layer 0's dW_ih = dG^T x (M = 4H, N = F = 40, K = T B) ----
// The 64 x 64 tiles padded N = 40 to 64 and streamed dG^T (629 MB at c3) at 4.6 TB/s (138 us).  The
// fp32 narrow kernel's layout (sv_gemm_f32.hip) in bf16: a workgroup is 128 rows x 48 columns over a K
// chunk, v_mfma_f32_16x16x32_bf16 (B first: a lane's 4 accumulators are 4 consecutive C columns),
// each wave 32 rows (2 x 3 blocks); LDS images [rows][64 k] (128 B) with 16-B chunk c of row r at
// c ^ (r & 7), filled by LDS-DMA, two stages; split-K slabs reduced by slab_reduce_bf_kernel.
constexpr int GNB_BM = 128, GNB_BN = 48, GNB_BK = 64;
__global__ __launch_bounds__(256) void gemm_bf16_narrow_kernel(const bf16_t* __restrict__ A, long lda,
                                                               const bf16_t* __restrict__ B, long ldb,
                                                               float* __restrict__ slab, long slab_stride, int M,
                                                               int N, int K, int kchunk) {
  __shared__ __attribute__((aligned(16))) char lds[2][(GNB_BM + GNB_BN) * 128];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int m0 = blockIdx.x * GNB_BM, s = blockIdx.y;
  const int kbeg = s * kchunk, nk = (min(K, kbeg + kchunk) - kbeg) / GNB_BK;
  // DMA map: 16-B chunk q of the stage: A rows 0..127 (q < 1024), then B rows 0..47
  auto fill = [&](int kt, int st) {
    const int k0 = kbeg + kt * GNB_BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = tid + 256 * i, row = q >> 3, c = (q & 7) ^ (row & 7);
      __builtin_amdgcn_global_load_lds((glb_vptr_t)(A + (long)(m0 + row) * lda + k0 + 8 * c),
                                       (lds_vptr_t)(&lds[st][0] + 16 * (w * 64 + 256 * i)), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i == 1 && w >= 2) break;  // 384 chunks of B: waves 0-1 issue a second one (wave-uniform)
      const int q = tid + 256 * i, row = q >> 3, c = (q & 7) ^ (row & 7);
      const int n = min(row, N - 1);  // padding columns read row N - 1 (their sums are not stored)
      __builtin_amdgcn_global_load_lds((glb_vptr_t)(B + (long)n * ldb + k0 + 8 * c),
                                       (lds_vptr_t)(&lds[st][GNB_BM * 128] + 16 * (w * 64 + 256 * i)), 16, 0, 0);
    }
  };
  g8_f32x4 acc[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = g8_f32x4{0.f, 0.f, 0.f, 0.f};
  if (nk > 0) fill(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int st = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage st landed for every wave; stage st ^ 1 free
    if (kt + 1 < nk) fill(kt + 1, st ^ 1);
    const char* As = &lds[st][0];
    const char* Bs = &lds[st][GNB_BM * 128];
#pragma unroll
    for (int ks = 0; ks < GNB_BK / 32; ++ks) {
      const int c = 4 * ks + lq;  // lane group lq: k 8 lq .. 8 lq + 7 of the 32-k step
      bf16x8_t a[2], b[3];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = 32 * w + 16 * i + lr;
        a[i] = *reinterpret_cast<const bf16x8_t*>(As + row * 128 + 16 * (c ^ (row & 7)));
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int row = 16 * j + lr;
        b[j] = *reinterpret_cast<const bf16x8_t*>(Bs + row * 128 + 16 * (c ^ (row & 7)));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = mfma16_bf16(b[j], a[i], acc[i][j]);
    }
  }
  // lane holds C[16 i + lr][16 j + 4 lq .. + 3] of its wave's rows
  float* Cz = slab + (long)s * slab_stride;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int col = 16 * j + 4 * lq;
      if (col < N)
        *reinterpret_cast<g8_f32x4*>(Cz + (long)(m0 + 32 * w + 16 * i + lr) * N + col) = acc[i][j];
    }
}
// exact plan of the narrow kernel: N <= 48 in whole 4-column groups, whole 128-row tiles, 64-k steps,
// K chunks of at least 1024 over up to 32 slabs (c3: 24 row tiles x 32 slabs = 768 workgroups)
static bool narrow_bf_ok(int M, int N, int K, long lda, long ldb) {
  return N <= GNB_BN && N % 4 == 0 && M % GNB_BM == 0 && K % GNB_BK == 0 && K >= 4096 &&
         lda % 8 == 0 && ldb % 8 == 0;
}
static int narrow_bf_splitk(int K, int& kchunk) {
  const int sk = std::max(1, std::min(32, K / 1024));
  kchunk = ((K + sk - 1) / sk + GNB_BK - 1) / GNB_BK * GNB_BK;
  return (K + kchunk - 1) / kchunk;
}

extern "C" size_t sv_gemm_bf16_workspace(int M, int N, int K) {
  const BPlan p = plan_bf16(M, N, K);
  size_t nar = 0;
  if (narrow_bf_ok(M, N, K, K, K)) {  // (the narrow kernel's slabs)
    int kchunk;
    nar = (size_t)narrow_bf_splitk(K, kchunk) * M * N * sizeof(float);
  }
  if (p.splitk <= 1) return nar;
  return std::max(nar, (size_t)p.splitk * M * N * sizeof(float));
}

extern "C" int sv_gemm_bf16(int M, int N, int K, const bf16_t* A, long lda, const bf16_t* B, long ldb, float* C,
                            long ldc, const float* bias0, const float* bias1, float beta, float* workspace,
                            hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || !A || !B || !C) return SV_EARG;
  if (K % 8 || lda % 8 || ldb % 8 || (((uintptr_t)A | (uintptr_t)B) & 15)) return SV_EALIGN;
  if (workspace && !((uintptr_t)workspace & 15) && narrow_bf_ok(M, N, K, lda, ldb)) {
    int kchunk;
    const int sk = narrow_bf_splitk(K, kchunk);
    const long slab = (long)M * N;
    hipLaunchKernelGGL(gemm_bf16_narrow_kernel, dim3(M / GNB_BM, sk), dim3(256), 0, stream, A, lda, B, ldb, workspace,
                       slab, M, N, K, kchunk);
    SV_LAUNCH_CHECK();
    const int grid = (int)std::min<long>((slab + 255) / 256, 4096);
    hipLaunchKernelGGL(slab_reduce_bf_kernel, dim3(grid), dim3(256), 0, stream, workspace, sk, slab, C, ldc, M, N,
                       beta, bias0, bias1);
    SV_LAUNCH_CHECK();
    return SV_OK;
  }
  const BPlan p = plan_bf16(M, N, K);
  if (p.bm == G256_BM) {
    const int tiles = (M / G256_BM) * (N / G256_BM);
    const long slab = (long)M * N;
    if (p.splitk == 1) {
      launch_g256<G256_STORE, 0>(g8_ok(C, ldc, bias0, bias1), dim3(tiles, 1), stream, A, lda, B, ldb, C, ldc, 0L,
                                 M, N, K, p.kchunk, bias0, bias1, beta);
      SV_LAUNCH_CHECK();
      return SV_OK;
    }
    if (!workspace) return SV_EARG;
    launch_g256<G256_SLAB, 0>(g8_ok(workspace, N, nullptr, nullptr), dim3(tiles, p.splitk), stream, A, lda, B,
                              ldb, workspace, (long)N, slab, M, N, K, p.kchunk, nullptr, nullptr, 0.f);
    SV_LAUNCH_CHECK();
    const int grid = (int)std::min<long>((slab + 255) / 256, 4096);
    hipLaunchKernelGGL(slab_reduce_bf_kernel, dim3(grid), dim3(256), 0, stream, workspace, p.splitk, slab, C, ldc, M, N,
                       beta, bias0, bias1);
    SV_LAUNCH_CHECK();
    return SV_OK;
  }
  if (p.splitk == 1) {
    if (p.bm == 64)
      launch_bf<64, 64, BEPI_STORE>(A, lda, B, ldb, C, ldc, 0, M, N, K, 1, p.kchunk, bias0, bias1, beta, stream);
    else
      launch_bf<128, 128, BEPI_STORE>(A, lda, B, ldb, C, ldc, 0, M, N, K, 1, p.kchunk, bias0, bias1, beta, stream);
    SV_LAUNCH_CHECK();
    return SV_OK;
  }
  if (!workspace) return SV_EARG;
  const long slab = (long)M * N;
  if (p.bm == 64)
    launch_bf<64, 64, BEPI_SLAB>(A, lda, B, ldb, workspace, N, slab, M, N, K, p.splitk, p.kchunk, nullptr, nullptr, 0.f,
                                 stream);
  else
    launch_bf<128, 128, BEPI_SLAB>(A, lda, B, ldb, workspace, N, slab, M, N, K, p.splitk, p.kchunk, nullptr, nullptr,
                                   0.f, stream);
  SV_LAUNCH_CHECK();
  const int grid = (int)std::min<long>((slab + 255) / 256, 4096);
  hipLaunchKernelGGL(slab_reduce_bf_kernel, dim3(grid), dim3(256), 0, stream, workspace, p.splitk, slab, C, ldc, M, N,
                     beta, bias0, bias1);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// the fused pair of weight-gradient GEMMs (sv_gemm_bf16.h)
size_t sv_gemm_bf16_dual_workspace(int M, int N1, int N2, int K) {
  const BPlan p = plan_bf16(M, N1, K);
  size_t fused = p.splitk > 1 ? (size_t)p.splitk * M * (N1 + N2) * sizeof(float) : 0;
  return std::max(fused, std::max(sv_gemm_bf16_workspace(M, N1, K), sv_gemm_bf16_workspace(M, N2, K)));
}
int sv_gemm_bf16_dual(int M, int N1, int N2, int K, const bf16_t* A, long lda, const bf16_t* B1, long ldb1, float* C1,
                      long ldc1, const bf16_t* B2, long ldb2, float* C2, long ldc2, float* workspace,
                      hipStream_t stream) {
  const BPlan p = plan_bf16(M, N1, K);
  const bool fused = p.bm == G256_BM && p.splitk > 1 && gemm256_ok(M, N1 + N2, K) && N1 % G256_BM == 0 &&
                     N2 % G256_BM == 0 && workspace && g8_ok(workspace, N1 + N2, nullptr, nullptr) &&
                     ldb1 % 8 == 0 && ldb2 % 8 == 0 && lda % 8 == 0 && !(((uintptr_t)A | (uintptr_t)B1 | (uintptr_t)B2) & 15);
  if (!fused) {
    int rc = sv_gemm_bf16(M, N1, K, A, lda, B1, ldb1, C1, ldc1, nullptr, nullptr, 0.f, workspace, stream);
    if (rc) return rc;
    return sv_gemm_bf16(M, N2, K, A, lda, B2, ldb2, C2, ldc2, nullptr, nullptr, 0.f, workspace, stream);
  }
  const int N = N1 + N2;
  const int tiles = (M / G256_BM) * (N / G256_BM);
  const long slab = (long)M * N;
  hipLaunchKernelGGL((gemm_bf16_8q_kernel<G8_SLAB, 0>), dim3(tiles, p.splitk), dim3(512), G256_LDS, stream, A, lda, B1,
                     ldb1, (void*)workspace, (long)N, slab, M, N, K, p.kchunk, nullptr, nullptr, 0.f, G256AFrag{},
                     G256Dual{B2, ldb2, N1});
  SV_LAUNCH_CHECK();
  const int grid = (int)std::min<long>((slab + 255) / 256, 4096);
  hipLaunchKernelGGL(slab_reduce_bf_kernel, dim3(grid), dim3(256), 0, stream, workspace, p.splitk, slab, C1, ldc1, M, N,
                     0.f, nullptr, nullptr, nullptr, C2, ldc2, N1);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// C[M,N] bf16 = bf16(A . B^T + bias0 + bias1) (fp32 accumulation, one rounding): the bf16
// path's x-projection (K1), stored in the gates buffer the recurrence then overwrites with its
// bf16 activations.  The 8-phase 256 x 256 kernel where the shape tiles (no split-K), else the
// 128 x 128 / 64 x 64 kernel without split-K -- one kernel per shape, so every schedule that
// forms the same projection rounds it identically.
extern "C" int sv_gemm_bf16_bf(int M, int N, int K, const bf16_t* A, long lda, const bf16_t* B, long ldb, bf16_t* C,
                               long ldc, const float* bias0, const float* bias1, hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || !A || !B || !C) return SV_EARG;
  if (K % 8 || lda % 8 || ldb % 8 || (((uintptr_t)A | (uintptr_t)B) & 15)) return SV_EALIGN;
  const BPlan p = plan_bf16(M, N, K);
  if (p.bm == G256_BM && p.splitk == 1 && g8_ok(nullptr, 0, bias0, bias1) && ldc % 8 == 0 &&
      !((uintptr_t)C & 15) && (size_t)N * 4 <= G8P_BIAS_LDS) {
    // persistent form: one workgroup per CU walks the tiles, each tile's store tail overlapping
    // the next tile's first fill
    const int tiles = (M / G256_BM) * (N / G256_BM);
    const int cus = sv_stream_cus(stream);
    const int grid = std::min(tiles, cus > 0 ? cus : 256);
    const size_t lds = G256_LDS + ((bias0 || bias1) ? (size_t)N * 4 : 0);
    hipLaunchKernelGGL((gemm_bf16_8qp_kernel<G8_STORE_BF16>), dim3(grid), dim3(512), lds, stream, A, lda, B, ldb,
                       (void*)C, ldc, M, N, K, bias0, bias1, 0.f);
  } else if ((long)((M + 127) / 128) * ((N + 127) / 128) < 128) {
    launch_bf<64, 64, BEPI_STORE_BF16>(A, lda, B, ldb, C, ldc, 0, M, N, K, 1, ((K + BBK - 1) / BBK) * BBK, bias0,
                                       bias1, 0.f, stream);
  } else {
    launch_bf<128, 128, BEPI_STORE_BF16>(A, lda, B, ldb, C, ldc, 0, M, N, K, 1, ((K + BBK - 1) / BBK) * BBK, bias0,
                                         bias1, 0.f, stream);
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// dx = dG . W_ih with dG read from the persistent backward's fragment-order hand-off buffer
// (no row-major dG copy): M = T * B rows (t, b), K = 4H; needs B % 32, M % 256, N % 256, H % 64
bool gemm_afrag_ok(int T, int B, int N, int H) {
  return gemm256_ok(T * B, N, 4 * H) && B % 32 == 0 && H % G256_BK == 0 &&
         4 * H / G256_BK < 4096 && (unsigned long long)T * B * B < (1ull << 32);  // g256_af_koff / _rowoff exact
}
// (the split-K plan of sv_gemm_bf16 for the same shape)
// fin: a deferred bias finalize (sv_persist_bwd_bf16's `defer`) done by extra workgroups of the
// one-shot 8-phase launch, else by its own launch after the GEMM
int gemm_bf16_afrag(int T, int B, int H, int N, const bf16_t* dgf, int bm, const bf16_t* Bop, long ldb, float* C,
                    long ldc, float* workspace, hipStream_t stream, const DbFin& fin) {
  const int M = T * B, K = 4 * H;
  const int tiles = (M / G256_BM) * (N / G256_BM);
  const long fs = (long)((B + bm - 1) / bm) * bm * 4 * H;
  const G256AFrag af = g256_afrag(dgf, fs, B, bm, H);
  const BPlan p = plan_bf16(M, N, K);
  if (p.splitk == 1 && g8_ok(C, ldc, nullptr, nullptr)) {
    hipLaunchKernelGGL((gemm_bf16_8q_kernel<G256_STORE, 1>), dim3(tiles + dbfin_blocks(fin, 512)), dim3(512), G256_LDS,
                       stream, nullptr, 0L, Bop, ldb, (void*)C, ldc, 0L, M, N, K, p.kchunk, nullptr, nullptr, 0.f, af,
                       G256Dual{}, fin);
    SV_LAUNCH_CHECK();
    return SV_OK;
  }
  if (int rc = sv_dbfin_launch(fin, stream)) return rc;
  if (p.splitk == 1) {
    launch_g256<G256_STORE, 1>(false, dim3(tiles, 1), stream, nullptr, 0L, Bop, ldb, C, ldc, 0L, M, N, K, p.kchunk,
                               nullptr, nullptr, 0.f, af);
    SV_LAUNCH_CHECK();
    return SV_OK;
  }
  if (!workspace) return SV_EARG;
  const long slab = (long)M * N;
  launch_g256<G256_SLAB, 1>(g8_ok(workspace, N, nullptr, nullptr), dim3(tiles, p.splitk), stream, nullptr, 0L,
                            Bop, ldb, workspace, (long)N, slab, M, N, K, p.kchunk, nullptr, nullptr, 0.f, af);
  SV_LAUNCH_CHECK();
  const int grid = (int)std::min<long>((slab + 255) / 256, 4096);
  hipLaunchKernelGGL(slab_reduce_bf_kernel, dim3(grid), dim3(256), 0, stream, workspace, p.splitk, slab, C, ldc, M, N,
                     0.f, nullptr, nullptr);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
