// bf16-operand variant of the LSTM stack (BASELINE config c3: "gate GEMMs on MFMA", mixed
// precision).  GEMM operands (weights, h, dgates) are bf16 and feed v_mfma_f32_32x32x16_bf16
// with fp32 accumulation; cell state, activations, biases, gradients, the projection, the
// GE2E loss and the optimizer stay fp32.  Same algorithm, layouts and epilogues
// as sv_lstm.hip; transposed layouts use column blocks of Bp = B rounded up to 8 so every
// bf16 row stays 16-byte aligned.  This file: the cast / transpose / frames kernels, the per-step
// recurrent kernels and the host glue that enqueues one layer or the layer stack under the
// wavefront, persistent or per-step schedule; the GEMMs it enqueues are sv_gemm_bf16.hip's.
#include <algorithm>
#include "sv_common.h"
#include "sv_gemm.h"
#include "sv_lstm_stack.h"
#include "../../include/sv_ge2e.h"
#include "sv_bf16.h"
#include "sv_gemm_bf16.h"

// up to 8 casts / transpose-casts in ONE launch (the per-step weight copies of the bf16 path: at
// the c4 rank shape each of the 13 separate launches took ~5 us for ~1 us of traffic); the
// single-matrix entry points (sv_cast_bf16, sv_transpose_cast_bf16) are batches of one
struct CastBatch {
  const float* x[8];
  bf16_t* y[8];
  long start[9];  // element prefix sums
  int n;
};
// VEC: start[] counts groups of 4 elements (every count % 4 == 0, every pointer 16-B aligned):
// one float4 load and one 8-B store per thread-iteration
template <bool VEC>
__global__ void cast_bf16_batch_kernel(const CastBatch cb) {
  const long total = cb.start[cb.n];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int b = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k) b += (k < cb.n && i >= cb.start[k]) ? 1 : 0;
    const long j = i - cb.start[b];
    if constexpr (VEC) {
      const float4 v = reinterpret_cast<const float4*>(cb.x[b])[j];
      reinterpret_cast<uint2*>(cb.y[b])[j] = pack_bf4(v.x, v.y, v.z, v.w);
    } else {
      cb.y[b][j] = to_bf(cb.x[b][j]);
    }
  }
}
struct TCastBatch {
  const float* src[8];
  bf16_t* dst[8];   // transposed copy (null: none)
  bf16_t* dstr[8];  // row-major copy, row stride C (null: none; ABI v10, sv_lstm_weights_bf16)
  long lds[8], ldd[8];
  int R[8], C[8], tx[8];  // column tiles per matrix
  int tile0[9];           // 64 x 64 tile prefix sums
  int n;
  unsigned vec;           // bit b: matrix b takes the 16-B paths (lds % 4, ldd % 8, aligned bases)
};
// the frames' part of the bf16 stack's input preparation (sv_frames_to_bf16 / sv_lstm_prep_bf16):
// frames x [B,T,F] fp32 -> x_bf [T,B,F] and, when xT is given, xT [F][T Bp] with column t Bp + b =
// x[b,t,:] (padding columns b in [B, Bp) zero) -- layer 0's dW_ih operand.  Workgroup (t, 64 rows
// b): the tile goes through LDS so both stores coalesce.
struct FramesArgs {
  const float* x;
  bf16_t *x_bf, *xT;
  int B, T, F, Bp, nbx;  // nbx: 64-row blocks per timestep
};
__device__ __forceinline__ void frames_tile(const FramesArgs& fa, int bx, int t, float (*tile)[65]) {
  const int b0 = bx * 64, tid = threadIdx.x, B = fa.B, T = fa.T, F = fa.F, Bp = fa.Bp;
  // 16 predicated loads per thread, all in flight before the first LDS write (a rolled loop
  // waited for each load on its own); thread -> (row tid / 64 + 4 i, column tid % 64)
  float v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int b = (tid >> 6) + 4 * i, f = tid & 63;
    v[i] = (f < F && b0 + b < B) ? fa.x[((long)(b0 + b) * T + t) * F + f] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) tile[(tid >> 6) + 4 * i][tid & 63] = v[i];
  __syncthreads();
  for (int i = tid; i < 64 * F; i += 256) {
    const int b = i / F, f = i % F;
    if (b0 + b < B) fa.x_bf[((long)t * B + b0 + b) * F + f] = to_bf(tile[b][f]);
  }
  if (fa.xT)
    for (int i = tid; i < 64 * F; i += 256) {
      const int f = i / 64, b = i % 64;
      if (b0 + b < Bp) fa.xT[(long)f * T * Bp + (long)t * Bp + b0 + b] = to_bf(tile[b][f]);
    }
}

// 64 x 64 tiles: float4 loads along a source row (16 threads per row, 16 rows per pass) and 16-B
// bf16 stores along a destination row (8 threads per row, 32 rows per pass) where the matrix's
// leading dimensions and base pointers allow (tb.vec bit b), element-wise at the edges.
// The first nfr workgroups (fa.x given): the frames' part, beside the tiles in the same launch --
// dispatched first, so that these latency-bound workgroups overlap the tiles instead of forming
// the launch's tail (placed after the tiles, the launch took the two kernels' sum, 27 us at c4)
__global__ __launch_bounds__(256) void transpose_cast_batch_kernel(const TCastBatch tb, const FramesArgs fa, int nfr) {
  __shared__ float tile[64][65];
  if ((int)blockIdx.x < nfr) {
    frames_tile(fa, blockIdx.x % fa.nbx, blockIdx.x / fa.nbx, tile);
    return;
  }
  const int blk = blockIdx.x - nfr;
  int b = 0;
#pragma unroll
  for (int k = 1; k < 8; ++k) b += (k < tb.n && blk >= tb.tile0[k]) ? 1 : 0;
  const int t = blk - tb.tile0[b];
  const int R = tb.R[b], C = tb.C[b];
  const int c0 = (t % tb.tx[b]) * 64, r0 = (t / tb.tx[b]) * 64;
  const bool vec = (tb.vec >> b) & 1;
  const float* src = tb.src[b];
  {
    const int lc = (threadIdx.x & 15) * 4, lr = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + lr + 16 * i, c = c0 + lc;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (r < R) {
        if (vec && c + 3 < C) {
          const float4 q = *reinterpret_cast<const float4*>(src + (long)r * tb.lds[b] + c);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < C) v[e] = src[(long)r * tb.lds[b] + c + e];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) tile[lr + 16 * i][lc + e] = v[e];
      if (tb.dstr[b] && r < R) {  // the row-major copy straight from the registers
        bf16_t* d = tb.dstr[b] + (long)r * C + c;
        if (vec && c + 3 < C) {
          *reinterpret_cast<uint2*>(d) = pack_bf4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < C) d[e] = to_bf(v[e]);
        }
      }
    }
  }
  bf16_t* dst = tb.dst[b];
  if (!dst) return;  // uniform per workgroup: no barrier skipped by part of it
  __syncthreads();
  const int lr8 = (threadIdx.x & 7) * 8, lcr = threadIdx.x >> 3;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int cc = lcr + 32 * i, c = c0 + cc, r = r0 + lr8;
    if (c >= C) continue;
    bf16_t* d = dst + (long)c * tb.ldd[b] + r;
    if (vec && r + 7 < R) {
      const uint2 lo = pack_bf4(tile[lr8][cc], tile[lr8 + 1][cc], tile[lr8 + 2][cc], tile[lr8 + 3][cc]);
      const uint2 hi = pack_bf4(tile[lr8 + 4][cc], tile[lr8 + 5][cc], tile[lr8 + 6][cc], tile[lr8 + 7][cc]);
      *reinterpret_cast<uint4*>(d) = uint4{lo.x, lo.y, hi.x, hi.y};
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (r + e < R) d[e] = to_bf(tile[lr8 + e][cc]);
    }
  }
}

// row sums of a bf16 matrix, fp32 accumulation, one block per row, fixed order
__global__ __launch_bounds__(256) void rowsum_bf16_kernel(const bf16_t* __restrict__ X, long ld, int C,
                                                          float* __restrict__ out0, float* __restrict__ out1) {
  __shared__ float red[4];
  const bf16_t* x = X + (long)blockIdx.x * ld;
  float s = 0.f;
  const int C8 = C / 8;
  for (int c = threadIdx.x; c < C8; c += 256) {
    const bf16x8_t v = reinterpret_cast<const bf16x8_t*>(x)[c];
    float p = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) p += (float)v[j];
    s += p;
  }
  for (int c = C8 * 8 + threadIdx.x; c < C; c += 256) s += (float)*reinterpret_cast<const __bf16*>(x + c);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = (red[0] + red[1]) + (red[2] + red[3]);
    out0[blockIdx.x] = t;
    if (out1) out1[blockIdx.x] = t;
  }
}

// ============================================================================
// recurrent steps (same decomposition as the fp32 v2 kernels: 64 rows x 32 units, 8 waves)
// ============================================================================

template <int SC>
__global__ __launch_bounds__(512) void lstm_step_fwd_bf16_kernel(
    const bf16_t* __restrict__ hprev_bf, const bf16_t* __restrict__ whh_bf, bf16_t* __restrict__ gates,
    const float* __restrict__ cprev, float* __restrict__ cout, float* __restrict__ hout, bf16_t* __restrict__ hout_bf,
    bf16_t* __restrict__ hT, long ldhT, int t, int Bp, int B, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* ldsb = reinterpret_cast<bf16_t*>(smem);
  constexpr int BN = 4 * BF_U, LDP = BN + 4, LDH = BF_BM + 1;
  constexpr int PER = BF_BM * BF_U / 512;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j0 = blockIdx.x * BF_U, b0 = blockIdx.y * BF_BM;
  const int wm0 = (w >> 2) * 32, wn0 = (w & 3) * 32;
  const long G = 4L * H;
  float xg[PER][4], cpv[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = tid + 512 * k, b = e / BF_U, u = e % BF_U;
    const int gb = b0 + b, gj = j0 + u;
    const bool ok = gb < B && gj < H;
    const bf16_t* gp = gates + (long)gb * G + gj;
#pragma unroll
    for (int q = 0; q < 4; ++q) xg[k][q] = ok ? from_bf(gp[q * H]) : 0.f;
    cpv[k] = (ok && cprev) ? cprev[(long)gb * H + gj] : 0.f;
  }
  f32x16 acc[1][1];
  zero_acc(acc);
  if (hprev_bf)
    gemm_mainloop_step<BF_BM, BN, 512, SC, 1, 1>(hprev_bf + (long)b0 * H, H, RowMapLinear{0, B - b0}, whh_bf, H,
                                                 RowMapGates<BF_U>{j0, H}, 0, H, ldsb, tid, wm0, wn0, acc);
  float* pre = reinterpret_cast<float*>(smem);
  float* hs = pre + BF_BM * LDP;
#pragma unroll
  for (int r = 0; r < 16; ++r) pre[(wm0 + acc_row(r, lane)) * LDP + wn0 + (lane & 31)] = acc[0][0][r];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = tid + 512 * k, b = e / BF_U, u = e % BF_U;
    const int gb = b0 + b, gj = j0 + u;
    if (gb >= B || gj >= H) continue;
    bf16_t* gp = gates + (long)gb * G + gj;
    const float* pr = pre + b * LDP + u;
    const float pv[4] = {pr[0], pr[BF_U], pr[2 * BF_U], pr[3 * BF_U]};
    float av[4], h;
    const float c = lstm_cell_fwd(pv, xg[k], cpv[k], av, h);
    gp[0] = to_bf(av[0]);
    gp[H] = to_bf(av[1]);
    gp[2 * H] = to_bf(av[2]);
    gp[3 * H] = to_bf(av[3]);
    cout[(long)gb * H + gj] = c;
    hout[(long)gb * H + gj] = h;
    hout_bf[(long)gb * H + gj] = to_bf(h);
    hs[u * LDH + b] = h;
  }
  if (!hT) return;
  __syncthreads();
  for (int e = tid; e < BF_BM * BF_U; e += 512) {
    const int u = e / BF_BM, b = e % BF_BM;
    const int gb = b0 + b, gj = j0 + u;
    if (gb >= B || gj >= H) continue;
    bf16_t* row = hT + (long)gj * ldhT;
    row[(long)(t + 1) * Bp + gb] = to_bf(hs[u * LDH + b]);
    if (t == 0) row[gb] = 0;
  }
}

template <int SC>
__global__ __launch_bounds__(512) void lstm_step_bwd_bf16_kernel(
    const bf16_t* __restrict__ dgnext, const bf16_t* __restrict__ whhT, const float* __restrict__ dhup,
    const float* __restrict__ dcf_next, const bf16_t* __restrict__ acts, const float* __restrict__ c_t,
    const float* __restrict__ c_prev, bf16_t* __restrict__ dg, float* __restrict__ dcf, bf16_t* __restrict__ dgT,
    long lddgT, int t, int Bp, int B, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* ldsb = reinterpret_cast<bf16_t*>(smem);
  constexpr int GBUF = 2 * (BF_BM + BF_U) * (BBK + 8);
  constexpr int LDR = BF_U + 1;
  constexpr int LDT = BF_BM + 1;
  constexpr int PER = BF_BM * BF_U / 512;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int gate = w >> 1, gt = tid & 127;
  const int j0 = blockIdx.x * BF_U, b0 = blockIdx.y * BF_BM;
  const long G = 4L * H;
  float av[PER][4], cv[PER], cpv[PER], dcfv[PER], upv[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = tid + 512 * k, b = e / BF_U, u = e % BF_U;
    const int gb = b0 + b, gj = j0 + u;
    const bool ok = gb < B && gj < H;
    const long hi = (long)gb * H + gj;
    const bf16_t* ap = acts + (long)gb * G + gj;
#pragma unroll
    for (int q = 0; q < 4; ++q) av[k][q] = ok ? from_bf(ap[q * H]) : 0.f;
    cv[k] = ok ? c_t[hi] : 0.f;
    cpv[k] = (ok && c_prev) ? c_prev[hi] : 0.f;
    dcfv[k] = (ok && dcf_next) ? dcf_next[hi] : 0.f;
    upv[k] = (ok && dhup) ? dhup[hi] : 0.f;
  }
  f32x16 acc[1][1];
  zero_acc(acc);
  if (dgnext)
    gemm_mainloop_step<BF_BM, BF_U, 128, SC, 1, 1>(dgnext + (long)b0 * G, G, RowMapLinear{0, B - b0}, whhT, G,
                                                  RowMapLinear{j0, H}, gate * H, (gate + 1) * H, ldsb + gate * GBUF,
                                                  gt, (w & 1) * 32, 0, acc);
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);  // [4][64][LDR]
  float* gTs = red + 4 * BF_BM * LDR;           // [4*32][LDT]
#pragma unroll
  for (int r = 0; r < 16; ++r)
    red[(gate * BF_BM + (w & 1) * 32 + acc_row(r, lane)) * LDR + (lane & 31)] = acc[0][0][r];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = tid + 512 * k, b = e / BF_U, u = e % BF_U;
    const int gb = b0 + b, gj = j0 + u;
    if (gb >= B || gj >= H) continue;
    const long hi = (long)gb * H + gj;
    float dh = red[(0 * BF_BM + b) * LDR + u];
    dh += red[(1 * BF_BM + b) * LDR + u];
    dh += red[(2 * BF_BM + b) * LDR + u];
    dh += red[(3 * BF_BM + b) * LDR + u];
    dh += upv[k];
    float dd[4];
    dcf[hi] = lstm_cell_bwd(dh, av[k][0], av[k][1], av[k][2], av[k][3], cv[k], cpv[k], dcfv[k], dd);
    const float d0 = dd[0], d1 = dd[1], d2 = dd[2], d3 = dd[3];
    bf16_t* dp = dg + (long)gb * G + gj;
    dp[0] = to_bf(d0);
    dp[H] = to_bf(d1);
    dp[2 * H] = to_bf(d2);
    dp[3 * H] = to_bf(d3);
    gTs[(0 * BF_U + u) * LDT + b] = d0;
    gTs[(1 * BF_U + u) * LDT + b] = d1;
    gTs[(2 * BF_U + u) * LDT + b] = d2;
    gTs[(3 * BF_U + u) * LDT + b] = d3;
  }
  if (!dgT) return;
  __syncthreads();
  for (int e = tid; e < 4 * BF_U * BF_BM; e += 512) {
    const int gu = e / BF_BM, b = e % BF_BM;
    const int gte = gu / BF_U, u = gu % BF_U;
    const int gb = b0 + b, gj = j0 + u;
    if (gb >= B || gj >= H) continue;
    dgT[((long)gte * H + gj) * lddgT + (long)t * Bp + gb] = to_bf(gTs[gu * LDT + b]);
  }
}

// ============================================================================
// host side
// ============================================================================
namespace {

constexpr int BFWD_LDS_MAIN = 2 * (BF_BM + 4 * BF_U) * (BBK + 8) * 2;
constexpr int BFWD_LDS_EPI = (BF_BM * (4 * BF_U + 4) + BF_U * (BF_BM + 1)) * 4;
constexpr int BFWD_LDS = BFWD_LDS_MAIN > BFWD_LDS_EPI ? BFWD_LDS_MAIN : BFWD_LDS_EPI;
constexpr int BBWD_LDS_MAIN = 4 * 2 * (BF_BM + BF_U) * (BBK + 8) * 2;
constexpr int BBWD_LDS_EPI = (4 * BF_BM * (BF_U + 1) + 4 * BF_U * (BF_BM + 1)) * 4;
constexpr int BBWD_LDS = BBWD_LDS_MAIN > BBWD_LDS_EPI ? BBWD_LDS_MAIN : BBWD_LDS_EPI;

// per-step forward kernel: register prefetch in super-chunks of 3 k-tiles (measured against 4, 6,
// 12 and rolling prefetch depths 4 / 6 at c3: none faster)
void launch_fwd_bf16(dim3 grid, hipStream_t s, const bf16_t* hp, const bf16_t* whh, bf16_t* g, const float* cp,
                     float* c, float* h, bf16_t* hb, bf16_t* hT, long ldhT, int t, int Bp, int B, int H) {
  hipLaunchKernelGGL(lstm_step_fwd_bf16_kernel<3>, grid, dim3(512), BFWD_LDS, s, hp, whh, g, cp, c, h, hb, hT, ldhT,
                     t, Bp, B, H);
}

// bf16 stack schedule (the `schedule` flags of sv_lstm_stack_{fwd,bwd}_bf16, include/sv_ge2e.h):
// persistent recurrences (one launch per layer, W_hh held in registers, sv_persist.hip) at
// H = 768 (measured c3 21.5 vs 22.2 ms per-step) or wherever they fit with SV_SCHED_PERSIST;
// per-step launches, layer-pipelined, with SV_SCHED_PER_STEP (bit-identical results).
bool sched_persist(int schedule, int H) {
  return !(schedule & SV_SCHED_PER_STEP) && ((schedule & SV_SCHED_PERSIST) || H == 768);
}
// the layer wavefronts (every layer in one launch, sv_wave.hip / sv_persist3.hip) where all
// layers' grids fit co-resident, unless SV_SCHED_PER_LAYER (bf16-level different sums)
bool sched_wave(int schedule, int H) { return sched_persist(schedule, H) && !(schedule & SV_SCHED_PER_LAYER); }

// per-step backward kernel: register prefetch in super-chunks of 6 k-tiles (measured against
// 2, 3 and rolling depths 3 / 4 / 6 at c3)
void launch_bwd_bf16(dim3 grid, hipStream_t s, const bf16_t* dgn, const bf16_t* whhT, const float* up,
                     const float* dcfi, const bf16_t* acts, const float* ct, const float* cp, bf16_t* dg, float* dcfo,
                     bf16_t* dgT, long lddgT, int t, int Bp, int B, int H) {
  hipLaunchKernelGGL(lstm_step_bwd_bf16_kernel<6>, grid, dim3(512), BBWD_LDS, s, dgn, whhT, up, dcfi, acts, ct, cp,
                     dg, dcfo, dgT, lddgT, t, Bp, B, H);
}

}  // namespace

extern "C" int sv_cast_bf16_batch(int n, const float* const* x, bf16_t* const* y, const long* count,
                                  hipStream_t stream);
extern "C" int sv_cast_bf16(const float* x, bf16_t* y, long n, hipStream_t stream) {
  if (!x || !y || n <= 0) return SV_EARG;
  return sv_cast_bf16_batch(1, &x, &y, &n, stream);
}

extern "C" int sv_cast_bf16_batch(int n, const float* const* x, bf16_t* const* y, const long* count,
                                  hipStream_t stream) {
  if (n <= 0 || n > 8 || !x || !y || !count) return SV_EARG;
  CastBatch cb{};
  cb.n = n;
  bool vec = true;
  for (int i = 0; i < n; ++i) {
    if (!x[i] || !y[i] || count[i] <= 0) return SV_EARG;
    cb.x[i] = x[i];
    cb.y[i] = y[i];
    vec = vec && count[i] % 4 == 0 && !((uintptr_t)x[i] & 15) && !((uintptr_t)y[i] & 7);
  }
  for (int i = 0; i < n; ++i) cb.start[i + 1] = cb.start[i] + (vec ? count[i] / 4 : count[i]);
  const int grid = (int)std::min<long>((cb.start[n] + 255) / 256, 8192);
  if (vec)
    hipLaunchKernelGGL(cast_bf16_batch_kernel<true>, dim3(grid), dim3(256), 0, stream, cb);
  else
    hipLaunchKernelGGL(cast_bf16_batch_kernel<false>, dim3(grid), dim3(256), 0, stream, cb);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// the transpose-casts of up to 8 matrices in one launch (dst[c ldd + r] = bf16(src[r lds + c]));
// dstr (optional, per matrix): also the row-major cast dstr[r C + c], from the same read; a null
// dst[i] with a dstr[i]: the row-major cast alone
int transpose_cast_bf16_batch(int n, const float* const* src, const long* lds, const int* R, const int* C,
                              bf16_t* const* dst, const long* ldd, hipStream_t stream, bf16_t* const* dstr = nullptr,
                              const FramesArgs* frames = nullptr) {
  if (n <= 0 || n > 8) return SV_EARG;
  TCastBatch tb{};
  tb.n = n;
  for (int i = 0; i < n; ++i) {
    if (!src[i] || !(dst[i] || (dstr && dstr[i])) || R[i] <= 0 || C[i] <= 0) return SV_EARG;
    tb.src[i] = src[i];
    tb.dst[i] = dst[i];
    tb.dstr[i] = dstr ? dstr[i] : nullptr;
    tb.lds[i] = lds[i];
    tb.ldd[i] = ldd[i];
    tb.R[i] = R[i];
    tb.C[i] = C[i];
    tb.tx[i] = (C[i] + 63) / 64;
    tb.tile0[i + 1] = tb.tile0[i] + tb.tx[i] * ((R[i] + 63) / 64);
    const bool rv = !tb.dstr[i] || (C[i] % 4 == 0 && !((uintptr_t)tb.dstr[i] & 7));
    if (lds[i] % 4 == 0 && ldd[i] % 8 == 0 && !((uintptr_t)src[i] & 15) && !((uintptr_t)dst[i] & 15) && rv)
      tb.vec |= 1u << i;
  }
  const FramesArgs fa = frames ? *frames : FramesArgs{};
  const int nfr = frames ? fa.nbx * fa.T : 0;
  hipLaunchKernelGGL(transpose_cast_batch_kernel, dim3(nfr + tb.tile0[n]), dim3(256), 0, stream, tb, fa, nfr);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// the bf16 stack's input in one launch (ABI v10; was to_time_major + a cast + a transpose-cast, and
// T transpose-casts when B % 8 != 0): frames_tile above, one workgroup per (64 rows, timestep)
__global__ __launch_bounds__(256) void frames_to_bf16_kernel(const FramesArgs fa) {
  __shared__ float tile[64][65];  // [b][f], F <= 64
  frames_tile(fa, blockIdx.x, blockIdx.y, tile);
}
static FramesArgs frames_args(const float* x, int B, int T, int F, bf16_t* x_bf, bf16_t* xT, int Bp) {
  return FramesArgs{x, x_bf, xT, B, T, F, Bp, (std::max(B, xT ? Bp : B) + 63) / 64};
}
extern "C" int sv_frames_to_bf16(const float* x, int B, int T, int F, bf16_t* x_bf, bf16_t* xT, int Bp,
                                 hipStream_t stream) {
  if (!x || !x_bf || B <= 0 || T <= 0 || F <= 0 || F > 64 || (xT && Bp < B)) return SV_EARG;
  const FramesArgs fa = frames_args(x, B, T, F, x_bf, xT, Bp);
  hipLaunchKernelGGL(frames_to_bf16_kernel, dim3(fa.nbx, T), dim3(256), 0, stream, fa);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_transpose_cast_bf16(const float* src, long ld_src, int R, int C, bf16_t* dst, long ld_dst,
                                      hipStream_t stream) {
  if (!src || !dst || R <= 0 || C <= 0) return SV_EARG;
  return transpose_cast_bf16_batch(1, &src, &ld_src, &R, &C, &dst, &ld_dst, stream);
}

namespace {
// up to 8 transpose-casts gathered for one transpose_cast_bf16_batch launch: add() launches a
// full batch first, flush() what is left
struct TCastList {
  hipStream_t stream;
  const float* src[8];
  bf16_t *dst[8], *dstr[8];
  long lds[8], ldd[8];
  int R[8], C[8], n = 0;
  // W [R][C] fp32 -> its transpose wT [C][ld_wT] and / or its row-major cast w_bf (either may be NULL)
  int add(const float* w, int rows, int cols, bf16_t* wT, long ld_wT, bf16_t* w_bf) {
    if (n == 8)
      if (int rc = flush()) return rc;
    src[n] = w, dst[n] = wT, dstr[n] = w_bf;
    lds[n] = cols, ldd[n] = ld_wT;
    R[n] = rows, C[n] = cols;
    ++n;
    return SV_OK;
  }
  // frames: sv_frames_to_bf16's work in the same launch
  int flush(const FramesArgs* frames = nullptr) {
    const int rc = n ? transpose_cast_bf16_batch(n, src, lds, R, C, dst, ldd, stream, dstr, frames) : 0;
    n = 0;
    return rc;
  }
};

// up to SV_ZB_MAX zeroings gathered for one sv_zero_bytes_multi launch
struct ZeroList {
  hipStream_t stream;
  void* p[SV_ZB_MAX];
  size_t b[SV_ZB_MAX];
  int n = 0;
  // launches the gathered ones first unless k more fit
  int room(int k) { return n + k > SV_ZB_MAX ? flush() : SV_OK; }
  void add(void* q, size_t bytes) { p[n] = q, b[n++] = bytes; }
  int flush() {
    const int rc = sv_zero_bytes_multi(n, p, b, stream);
    n = 0;
    return rc;
  }
};

// One layer's forward sequences on the shared stack frame (sv_lstm_stack.h), batch padded to 8
struct BFwd : Stack<8> {
  const bf16_t* x_bf;
  const bf16_t *const *w_ih, *const *w_hh;
  const float *const *b_ih, *const *b_hh;
  bf16_t* const* gates;
  float *const *c_tm, *const *h_tm;
  bf16_t *const *h_bf, *const *hT;
  // K1 for t0 .. t1-1: gates = bf16(in W_ih^T + b_ih + b_hh); in = the frames or the layer below's
  // h_bf (slot t + 1 = h_t)
  int k1(int l, int t0, int t1, hipStream_t s) const {
    const bf16_t* in = l == 0 ? x_bf + (long)t0 * B * F : h_bf[l - 1] + (long)(t0 + 1) * BH;
    return sv_gemm_bf16_bf((t1 - t0) * B, 4 * H, Fl(l), in, Fl(l), w_ih[l], Fl(l), gates[l] + t0 * BG, 4L * H, b_ih[l],
                           b_hh[l], s);
  }
  // h_tm[0] = h_bf[0] = h_{-1} = 0; where B is padded, hT whole (its padding columns are GEMM operands)
  int reset(int l, hipStream_t s) const {
    int rc = sv_zero_bytes(h_tm[l], BH * sizeof(float), s);
    if (!rc) rc = sv_zero_bytes(h_bf[l], BH * sizeof(bf16_t), s);
    if (!rc && hT[l] && Bp != B) rc = sv_zero_bytes(hT[l], (size_t)H * ldhT * sizeof(bf16_t), s);
    return rc;
  }
  // the recurrent steps t0 .. t1-1
  int steps(int l, int t0, int t1, hipStream_t s) const {
    const dim3 grid((H + BF_U - 1) / BF_U, (B + BF_BM - 1) / BF_BM);
    for (int t = t0; t < t1; ++t) {
      launch_fwd_bf16(grid, s, t ? h_bf[l] + t * BH : nullptr, w_hh[l], gates[l] + t * BG,
                      t ? c_tm[l] + (t - 1) * BH : nullptr, c_tm[l] + t * BH, h_tm[l] + (t + 1) * BH,
                      h_bf[l] + (t + 1) * BH, hT[l], ldhT, t, Bp, B, H);
      SV_LAUNCH_CHECK();
    }
    return SV_OK;
  }
  // every layer's reset in one launch on `main` (the schedules that run there), and with it every
  // counter channel of the sync block: this forward's and the backward's that follows
  int zero_states() const {
    ZeroList z{main};
    for (int l = 0; l < L; ++l) {
      if (int rc = z.room(3)) return rc;
      z.add(h_tm[l], BH * sizeof(float));
      z.add(h_bf[l], BH * sizeof(bf16_t));
      if (hT[l] && Bp != B) z.add(hT[l], (size_t)H * ldhT * sizeof(bf16_t));
    }
    if (int rc = z.room(1)) return rc;
    z.add(sync + SV_SYNC_CNT, (size_t)SV_SYNC_CHANNELS * SV_PCNT_ROWS * SV_PCNT_STRIDE * sizeof(unsigned));
    return z.flush();
  }
};

// layer-wavefront schedule (sv_wave.hip): every layer's recurrence and input projection in one
// launch on `main`
int fwd_wave(const BFwd& a) {
  if (!a.sync || a.L > SV_SYNC_CHANNELS) return SV_EARG;
  if (int rc = a.zero_states()) return rc;
  hipEvent_t* pp = a.layer_probe(0);
  return sv_wave_fwd_bf16(a.L, a.T, a.B, a.F, a.H, a.x_bf, a.w_ih, a.w_hh, a.b_ih, a.b_hh, a.gates, a.c_tm, a.h_tm,
                          a.h_bf, a.hT, a.sync, a.main, sv_persist_limit(), sv_persist_fault(0), pp ? pp[0] : nullptr,
                          pp ? pp[1] : nullptr, 1);
}

// persistent schedule on `main`: per layer the whole-T K1 GEMM (layer 0's projection inside the
// recurrence where it can be), then one launch for the recurrence (sv_persist.hip); layers run one
// after another, layer l on counter channel l (zeroed, with the backward's, in the state-reset
// launch) where L <= SV_BWD_CH0, else all on channel 0, each launch zeroing it
int fwd_persist(const BFwd& a) {
  if (!a.sync) return SV_EARG;
  const bool own = a.L <= SV_BWD_CH0;
  int rc = a.zero_states();
  for (int l = 0; l < a.L && !rc; ++l) {
    const bool fuse = l == 0 && sv_persist_fwd_fusex_ok(a.H, a.F);
    if (!fuse && (rc = a.k1(l, 0, a.T, a.main))) return rc;
    hipEvent_t* pp = a.layer_probe(l);
    rc = sv_persist_fwd_bf16(a.T, a.B, a.H, a.w_hh[l], a.gates[l], a.c_tm[l], a.h_tm[l], a.h_bf[l], a.hT[l], a.main,
                             a.sync, own ? l : 0, fuse ? a.x_bf : nullptr, fuse ? a.F : 0, fuse ? a.w_ih[l] : nullptr,
                             fuse ? a.b_ih[l] : nullptr, fuse ? a.b_hh[l] : nullptr, pp ? pp[0] : nullptr,
                             pp ? pp[1] : nullptr, own);
  }
  return rc;
}
}  // namespace

extern "C" int sv_lstm_layer_fwd_bf16(const bf16_t* x_bf, int T, int B, int F, int H, const bf16_t* w_ih_bf,
                                      const bf16_t* w_hh_bf, const float* b_ih, const float* b_hh, bf16_t* gates,
                                      float* c_tm, float* h_tm, bf16_t* h_bf, bf16_t* hT, hipStream_t stream) {
  if (!x_bf || !w_ih_bf || !w_hh_bf || !gates || !c_tm || !h_tm || !h_bf) return SV_EARG;
  if (T <= 0 || B <= 0 || F <= 0 || H <= 0 || F % 8 || H % 8) return SV_ESHAPE;
  const BFwd a{{1, T, B, F, H, T, stream}, x_bf, &w_ih_bf, &w_hh_bf, &b_ih, &b_hh, &gates, &c_tm, &h_tm, &h_bf, &hT};
  int rc = a.k1(0, 0, T, stream);  // the all-timestep input projection
  if (!rc) rc = a.reset(0, stream);
  return rc ? rc : a.steps(0, 0, T, stream);
}

// Stack forward, bf16 operands.  `schedule` (include/sv_ge2e.h): the layer wavefront (one launch
// for every layer's recurrence and input projection, sv_wave.hip) where the grids fit; else per
// layer its K1 GEMM and one persistent recurrence launch (layer 0's projection in-kernel); else
// (SV_SCHED_PER_STEP, or H without a persistent kernel) the layer-pipelined per-step schedule
// (sv_lstm_stack.h).
extern "C" int sv_lstm_stack_fwd_bf16(int L, int T, int B, int F, int H, const bf16_t* x_bf,
                                      const bf16_t* const* w_ih_bf, const bf16_t* const* w_hh_bf,
                                      const float* const* b_ih, const float* const* b_hh, bf16_t* const* gates,
                                      float* const* c_tm, float* const* h_tm, bf16_t* const* h_bf,
                                      bf16_t* const* hT, int chunk, hipStream_t main, const hipStream_t* side,
                                      hipEvent_t* ev, void* sync_block, hipEvent_t* probe, int schedule) {
  if (L <= 0 || !x_bf || !w_ih_bf || !w_hh_bf || !gates || !c_tm || !h_tm || !h_bf || !side || !ev || chunk <= 0)
    return SV_EARG;
  if (schedule & ~SV_SCHED_MASK) return SV_EARG;
  unsigned* sync = reinterpret_cast<unsigned*>(sync_block);
  if (T <= 0 || B <= 0 || F <= 0 || H <= 0 || F % 8 || H % 8) return SV_ESHAPE;
  const BFwd a{{L, T, B, F, H, chunk, main, side, ev, probe, 0, schedule, sync},
               x_bf, w_ih_bf, w_hh_bf, b_ih, b_hh, gates, c_tm, h_tm, h_bf, hT};
  if (sched_wave(schedule, H) && sv_wave_fwd_fits(L, T, B, F, H, sv_stream_cus(main))) return fwd_wave(a);
  if (sched_persist(schedule, H) && sv_persist_fwd_fits(B, H, sv_stream_cus(main))) return fwd_persist(a);
  // per-step schedule: no counters of its own, but the backward's zeroed all the same (the
  // caller may pass SV_SCHED_CNT_READY to a persistent backward after any stack forward)
  if (sync)
    if (int rc = sv_zero_bytes(sync + SV_SYNC_CNT + (size_t)SV_BWD_CH0 * SV_PCNT_ROWS * SV_PCNT_STRIDE,
                               (size_t)(SV_SYNC_CHANNELS - SV_BWD_CH0) * SV_PCNT_ROWS * SV_PCNT_STRIDE *
                                   sizeof(unsigned),
                               main))
      return rc;
  return stack_fwd_per_step(a);
}

// Stack backward, bf16 operands (the per-step schedule: stack_bwd_per_step, sv_lstm_stack.h).
namespace {
// one layer's region of the workspace, and its transposed weights (bf16; written by prepare, read
// by the recurrence and the dx GEMM)
struct BBwdWs {
  float *dcf0, *dcf1, *gws;
  size_t gbytes, total;  // gws bytes; the region's
  const bf16_t *whhT, *wihT;
};
BBwdWs carve_bbwd(char* base, int T, int B, int F, int H) {
  BBwdWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) & ~size_t(255);
    return p;
  };
  w.dcf0 = (float*)take((size_t)B * H * 4);
  w.dcf1 = (float*)take((size_t)B * H * 4);
  const int TBp = T * ((B + 7) & ~7);
  size_t g = sv_gemm_bf16_workspace(4 * H, H, TBp);
  g = std::max(g, sv_gemm_bf16_workspace(4 * H, F, TBp));
  g = std::max(g, sv_gemm_bf16_workspace(T * B, F, 4 * H));
  g = std::max(g, sv_gemm_bf16_dual_workspace(4 * H, H, F, TBp));
  w.gws = (float*)take(g);
  w.gbytes = g;
  w.total = off;
  return w;
}
}  // namespace

// The bf16 weight transposes the stack backward reads live in a buffer of their own, `wt`
// (sv_lstm_wt_bf16_size bytes; independent of T and B): W_hh^T [H][4H] of every layer and W_ih^T
// [H][bf16_wiht_ld(H)] of layers >= 1, each piece 256-byte aligned.  wt_layer is the only place
// that knows the layout: layer l's two pointers (NULL where wt is NULL; wihT NULL for layer 0)
// and the offset at which the layer ends.
struct WtLayer {
  bf16_t *whhT, *wihT;
  size_t end;
};
static WtLayer wt_layer(void* wt, int l, int H) {
  const size_t hh = ((size_t)4 * H * H * 2 + 255) & ~size_t(255);
  const size_t ih = ((size_t)bf16_wiht_ld(H) * H * 2 + 255) & ~size_t(255);
  const size_t off = l ? hh + (size_t)(l - 1) * (hh + ih) : 0;
  char* p = wt ? (char*)wt + off : nullptr;
  return {(bf16_t*)p, (l && p) ? (bf16_t*)(p + hh) : nullptr, off + hh + (l ? ih : 0)};
}
extern "C" size_t sv_lstm_wt_bf16_size(int L, int F, int H) {
  return (L <= 0 || F <= 0 || H <= 0) ? 0 : wt_layer(nullptr, L - 1, H).end;
}

// W_hh^T of every layer and W_ih^T of layers >= 1 (bf16 [K, 4H]) into wt, in one or two launches
static int wbf_transposes(int L, int H, const float* const* w_ih, const float* const* w_hh, void* wt, hipStream_t s) {
  TCastList tc{s};
  for (int l = 0; l < L; ++l) {
    const WtLayer w = wt_layer(wt, l, H);
    int rc = tc.add(w_hh[l], 4 * H, H, w.whhT, 4L * H, nullptr);
    if (!rc && l > 0) rc = tc.add(w_ih[l], 4 * H, H, w.wihT, bf16_wiht_ld(H), nullptr);
    if (rc) return rc;
  }
  return tc.flush();
}

// Every layer's bf16 weights in one launch (transpose_cast_batch_kernel, each fp32 weight read
// once): the forward's row-major operands w_ih_bf / w_hh_bf and, when wt is given, the transposes
// the stack backward reads (wt_layer), so that sv_lstm_bwd with SV_SCHED_WT_READY on the same wt
// launches none (at the c4 rank shape: the forward's cast and the backward's transposes, 13 + 20 us,
// read every weight twice).  frames: sv_frames_to_bf16's work in the same (last) launch.
static int weights_bf16(int L, int F, int H, const float* const* w_ih, const float* const* w_hh,
                        bf16_t* const* w_ih_bf, bf16_t* const* w_hh_bf, void* wt, hipStream_t stream,
                        const FramesArgs* frames) {
  if (L <= 0 || !w_ih || !w_hh || !w_ih_bf || !w_hh_bf || ((uintptr_t)wt & 255)) return SV_EARG;
  if (F <= 0 || H <= 0 || F % 8 || H % 8) return SV_ESHAPE;
  TCastList tc{stream};
  for (int l = 0; l < L; ++l) {
    if (!w_ih[l] || !w_hh[l] || !w_ih_bf[l] || !w_hh_bf[l]) return SV_EARG;
    const WtLayer w = wt_layer(wt, l, H);
    int rc = tc.add(w_ih[l], 4 * H, l == 0 ? F : H, w.wihT, bf16_wiht_ld(H), w_ih_bf[l]);
    if (!rc) rc = tc.add(w_hh[l], 4 * H, H, w.whhT, 4L * H, w_hh_bf[l]);
    if (rc) return rc;
  }
  return tc.flush(frames);
}
extern "C" int sv_lstm_weights_bf16(int L, int F, int H, const float* const* w_ih, const float* const* w_hh,
                                    bf16_t* const* w_ih_bf, bf16_t* const* w_hh_bf, void* wt, hipStream_t stream) {
  return weights_bf16(L, F, H, w_ih, w_hh, w_ih_bf, w_hh_bf, wt, stream, nullptr);
}
// sv_frames_to_bf16 and sv_lstm_weights_bf16 as ONE launch (the frames' workgroups beside the weight
// tiles: at the c4 rank shape 10 + 17 us one after the other)
extern "C" int sv_lstm_prep_bf16(int L, int T, int B, int F, int H, const float* x, bf16_t* x_bf, bf16_t* xT, int Bp,
                                 const float* const* w_ih, const float* const* w_hh, bf16_t* const* w_ih_bf,
                                 bf16_t* const* w_hh_bf, void* wt, hipStream_t stream) {
  if (!x || !x_bf || F > 64 || (xT && Bp < B)) return SV_EARG;
  if (T <= 0 || B <= 0) return SV_ESHAPE;
  const FramesArgs fa = frames_args(x, B, T, F, x_bf, xT, Bp);
  return weights_bf16(L, F, H, w_ih, w_hh, w_ih_bf, w_hh_bf, wt, stream, &fa);
}

#ifndef SV_PERSIST_FULLK
#define SV_PERSIST_FULLK 1  // the persistent schedule's weight gradients as one whole-K launch (A/B)
#endif
// the stack backward's workspace: L per-layer regions (carve_bbwd), then the hand-off scratch shared
// by the layers (persistent or wavefront backward; the recurrences run one after another)
static size_t bbwd_scratch(int L, int T, int B, int H) {
  size_t scratch = sv_persist_bwd_fits(B, H, 1 << 30) ? sv_persist_bwd_scratch(T, B, H) : 0;
  if (sv_wave_bwd_fits(L, B, H, 1 << 30)) scratch = std::max(scratch, sv_wave_bwd_scratch(L, T, B, H));
  return (scratch + 255) & ~size_t(255);
}
extern "C" size_t sv_lstm_stack_bwd_bf16_workspace(int L, int T, int B, int F, int H) {
  const size_t per = (size_t)L * carve_bbwd(nullptr, T, B, std::max(F, H), H).total;
  return per + bbwd_scratch(L, T, B, H);
}

namespace {
// One layer's backward sequences on the shared stack frame (sv_lstm_stack.h), batch padded to 8
struct BBwd : Stack<8> {
  const bf16_t* const* xT;
  const long* ld_xT;
  const float *const *w_ih, *const *w_hh;
  const bf16_t* const* gates;
  const float* const* c_tm;
  const bf16_t* const* hT;
  const float* dh_last;  // dh into the top layer: [B,H] for t = T-1 alone, or -- top_full -- [T,B,H]
  int top_full;
  bf16_t *const *dg, *const *dgT;
  float *const *dx, *const *dw_ih, *const *dw_hh, *const *db_ih, *const *db_hh;
  char* workspace;
  void* wt;
  size_t per;     // bytes of one per-layer workspace region
  long ld_wihT;   // row stride of W_ih^T: bf16_wiht_ld(H) in wt, 4H in a single layer's caller's copy
  // the per-layer completion events (a caller's gradient buckets wait on them) of the persistent and
  // wavefront schedules; SV_SCHED_NO_EVENTS: nobody waits, record none (each record idles the GPU)
  bool evs() const { return !(schedule & SV_SCHED_NO_EVENTS); }
  // SV_SCHED_WT_READY: the caller filled wt (sv_lstm_weights_bf16): no transpose launches
  bool wt_ready() const { return schedule & SV_SCHED_WT_READY; }
  // SV_SCHED_CNT_READY: the stack forward zeroed the backward's counter channels and no backward
  // has used this sync block since (the caller tracks that): no zeroing launches here
  bool cnt_ready() const { return schedule & SV_SCHED_CNT_READY; }
  BBwdWs region(int l) const {
    BBwdWs ws = carve_bbwd(workspace + per * l, T, B, std::max(F, H), H);
    const WtLayer w = wt_layer(wt, l, H);
    ws.whhT = w.whhT, ws.wihT = w.wihT;
    return ws;
  }
  char* scratch() const { return workspace + per * L; }  // the recurrences' hand-off scratch
  // unless wt_ready: W_hh^T [H, 4H] and -- wih -- W_ih^T [H, ld_wihT] into wt; dgT (zero: the step
  // kernels will fill it) zeroed where B is padded
  int prepare(int l, const BBwdWs&, bool wih, bool zero, hipStream_t s) const {
    const WtLayer w = wt_layer(wt, l, H);
    int rc = wt_ready() ? 0 : sv_transpose_cast_bf16(w_hh[l], H, 4 * H, H, w.whhT, 4L * H, s);
    if (!rc && !wt_ready() && wih) rc = sv_transpose_cast_bf16(w_ih[l], Fl(l), 4 * H, Fl(l), w.wihT, ld_wihT, s);
    if (!rc && zero && Bp != B) rc = sv_zero_bytes(dgT[l], (size_t)4 * H * TBp * sizeof(bf16_t), s);
    return rc;
  }
  // the recurrent steps t1-1 .. t0; dh from above: dh_last for the top layer, else layer l + 1's
  // dx [T,B,H]  (the event pair of the fp32 schedule's probes: none here)
  int steps(int l, const BBwdWs& ws, int t0, int t1, hipStream_t s, hipEvent_t* = nullptr) const {
    const dim3 grid((H + BF_U - 1) / BF_U, (B + BF_BM - 1) / BF_BM);
    const float* up = l == L - 1 ? dh_last : dx[l + 1];
    const bool full = l < L - 1 || top_full;
    float* const dcf[2] = {ws.dcf0, ws.dcf1};  // ping-pong: step t writes dcf[t & 1], reads step t + 1's
    for (int t = t1 - 1; t >= t0; --t) {
      const bool last = t == T - 1;
      launch_bwd_bf16(grid, s, last ? nullptr : dg[l] + (t + 1) * BG, ws.whhT,
                      !up ? nullptr : full ? up + t * BH : last ? up : nullptr, last ? nullptr : dcf[~t & 1],
                      gates[l] + t * BG, c_tm[l] + t * BH, t ? c_tm[l] + (t - 1) * BH : nullptr, dg[l] + t * BG,
                      dcf[t & 1], dgT[l], (long)TBp, t, Bp, B, H);
      SV_LAUNCH_CHECK();
    }
    return SV_OK;
  }
  // dx = dG W_ih for t0 .. t1-1: A = dG [rows, 4H], B = W_ih^T [Fl, 4H] (ws.wihT)
  int dx_gemm(int l, const BBwdWs& ws, int t0, int t1, hipStream_t s) const {
    return sv_gemm_bf16((t1 - t0) * B, Fl(l), 4 * H, dg[l] + t0 * BG, 4L * H, ws.wihT, ld_wihT,
                        dx[l] + (long)t0 * B * Fl(l), Fl(l), nullptr, nullptr, 0.f, ws.gws, s);
  }
  // dW_hh = sum_t dG_t^T h_{t-1}: A = dG^T [4H, T Bp], B = hT[:, 0:T Bp] (column block t = h_{t-1});
  // dW_ih = sum_t dG_t^T x_t: B = x^T [Fl, T Bp]; db (where the recurrence has not summed the
  // biases itself): db_ih = db_hh (may be NULL) = row sums of dG^T
  int grads(int l, const BBwdWs& ws, bool db, hipStream_t s) const {
    int rc = sv_gemm_bf16(4 * H, H, TBp, dgT[l], TBp, hT[l], ldhT, dw_hh[l], H, nullptr, nullptr, 0.f, ws.gws, s);
    if (!rc)
      rc = sv_gemm_bf16(4 * H, Fl(l), TBp, dgT[l], TBp, xT[l], ld_xT[l], dw_ih[l], Fl(l), nullptr, nullptr, 0.f, ws.gws,
                        s);
    if (rc || !db) return rc;
    hipLaunchKernelGGL(rowsum_bf16_kernel, dim3(4 * H), dim3(256), 0, s, dgT[l], (long)TBp, TBp, db_ih[l],
                       db_hh ? db_hh[l] : nullptr);
    SV_LAUNCH_CHECK();
    return SV_OK;
  }
};

// every layer's whole-K weight-gradient tiles in one launch where they fit one round of the CUs
// (gemm_bf16_fullk; layer 0's N = F dW_ih after it on the narrow kernel), the split form
// (first pieces on the CUs the tiles leave free, their flags on channel SV_BWD_CH0 + WB_L) where
// at least 8 CUs are left over and the partials fit the GEMM scratch
bool plan_fullk(const BBwd& a, G8Full& f, int& fP) {
  const int L = a.L, F = a.F, H = a.H, TBp = a.TBp;
  const int cus = sv_stream_cus(a.main);
  f = G8Full{};
  fP = 0;
  if (!(L == WB_L && gemm256_ok(4 * H, H, TBp) && TBp % 8 == 0 && a.ldhT % 8 == 0)) return false;
  bool fullk = true;
  f.K = TBp;
  for (int l = 0; l < L; ++l) {
    // upper layers: dW_ih beside dW_hh (input width H, 3 column tiles); layer 0 too (x0 tile):
    // its F <= 256 columns as one partial column tile (x^T rows clamped, F columns stored) --
    // the narrow GEMM after the launch re-read all of dG^T_0 for them (c5 rank 76 + 10 us)
    const bool x0 = l == 0 && F <= G256_BM && F % 4 == 0;
    const bool dual = l > 0 || x0;
    G8FLayer& fl = f.lay[l];
    fl.A = a.dgT[l];
    fl.lda = TBp;
    fl.B = a.hT[l];
    fl.ldb = a.ldhT;
    fl.B2 = dual ? a.xT[l] : nullptr;
    fl.ldb2 = dual ? a.ld_xT[l] : 0;
    fl.C1 = a.dw_hh[l];
    fl.ldc1 = H;
    fl.C2 = dual ? a.dw_ih[l] : nullptr;
    fl.ldc2 = l > 0 ? H : F;
    fl.n1 = H;
    fl.N = l > 0 ? 2 * H : x0 ? H + G256_BM : H;
    fl.f2 = x0 ? F : 0;
    fl.tiles = (4 * H / G256_BM) * (fl.N / G256_BM);
    fP += fl.tiles;
    if (((uintptr_t)a.dgT[l] | (uintptr_t)a.hT[l] | (uintptr_t)a.dw_hh[l]) & 15) fullk = false;
    if (dual && ((((uintptr_t)a.xT[l] | (uintptr_t)a.dw_ih[l]) & 15) || a.ld_xT[l] % 8 || fl.ldc2 % 4)) fullk = false;
  }
  fullk = fullk && fP <= cus;
  const BBwdWs wsp = a.region(L - 1);
  const int KT = TBp / G256_BK;
  f.nsw = fullk ? (cus - fP) / 8 * 8 : 0;
  if (f.nsw > 0) {
    const int per_wg = (fP + f.nsw - 1) / f.nsw;  // first pieces per workgroup
    f.S = KT / (per_wg + 1) - 2;    // (their stores and prologues: a little less)
  }
  if (f.nsw <= 0 || f.S < 4 || (size_t)fP * G256_BM * G256_BM * 4 > wsp.gbytes) f.nsw = f.S = 0;
  if (f.S > 0) {
    f.part = wsp.gws;
    f.flag = a.sync + SV_SYNC_CNT + (size_t)(SV_BWD_CH0 + WB_L) * SV_PCNT_ROWS * SV_PCNT_STRIDE;
    f.status = a.sync;
    f.limit = sv_persist_limit();
  }
  return fullk;
}

// the whole-K launch plan_fullk planned, then layer 0's dW_ih and the layers' completion events
int run_fullk(const BBwd& a, const G8Full& f, int fP) {
  const int F = a.F, H = a.H, TBp = a.TBp;
  int rc = gemm_bf16_fullk(f, fP, a.main);
  for (int l = a.L - 1; l >= 1 && a.evs() && !rc; --l) rc = record(a.layer_done(l), a.main);
  if (rc) return rc;
  if (!f.lay[0].f2) {  // layer 0's dW_ih (F > 256) on its own
    if ((rc = sv_gemm_bf16(4 * H, F, TBp, a.dgT[0], TBp, a.xT[0], a.ld_xT[0], a.dw_ih[0], F, nullptr, nullptr, 0.f,
                           a.region(0).gws, a.main)))
      return rc;
  }
  return a.evs() ? record(a.layer_done(0), a.main) : SV_OK;
}

// layer-wavefront schedule: every layer's recurrence and upstream gradient dx in one launch
// (sv_persist3.hip, no dx GEMMs; bias gradients summed in the kernel), then per layer the
// weight gradients on `main`
int bwd_wave(const BBwd& a) {
  const int L = a.L, T = a.T, B = a.B, H = a.H, TBp = a.TBp;
  const bf16_t* whhT_l[WB_L];
  const bf16_t* wihT_l[WB_L];
  for (int l = 0; l < L; ++l) {
    const WtLayer w = wt_layer(a.wt, l, H);
    whhT_l[l] = w.whhT;
    wihT_l[l] = w.wihT;
  }
  int rc = a.wt_ready() ? 0 : wbf_transposes(L, H, a.w_ih, a.w_hh, a.wt, a.main);
  if (rc) return rc;
  G8Full f;
  int fP;
  const bool fullk = plan_fullk(a, f, fP);
  // with the whole-K launch after it, the bias finalize rides on that launch (G8Full::fin)
  hipEvent_t* pp = a.layer_probe(0);
  rc = sv_wave_bwd_bf16(L, T, B, H, whhT_l, wihT_l, a.gates, a.c_tm, a.dh_last, a.dx, a.dgT, a.scratch(), a.sync,
                        a.main, a.db_ih, a.db_hh, pp ? pp[0] : nullptr, pp ? pp[1] : nullptr, a.ld_wihT,
                        f.S > 0 ? fP : 0, SV_BWD_CH0, a.cnt_ready(), fullk ? &f.fin : nullptr);
  if (rc) return rc;
  if (fullk) return run_fullk(a, f, fP);
  for (int l = L - 1; l >= 0; --l) {
    if ((rc = sv_gemm_bf16_dual(4 * H, H, a.Fl(l), TBp, a.dgT[l], TBp, a.hT[l], a.ldhT, a.dw_hh[l], H, a.xT[l],
                                a.ld_xT[l], a.dw_ih[l], a.Fl(l), a.region(l).gws, a.main)))
      return rc;
    // layer l's gradients are complete: its all-reduce bucket (grad_ready) overlaps the lower
    // layers' weight-gradient GEMMs (the recurrences are all done)
    if (a.evs() && (rc = record(a.layer_done(l), a.main))) return rc;
  }
  return SV_OK;
}

// persistent schedule on `main`: per layer (top first) the whole-T recurrence in one launch
// (sv_persist.hip; bias gradients summed in the kernel), the whole-T dx GEMM straight from its
// fragment-order hand-off, then the layer's weight gradients (measured: on a side stream
// beside the next layer's recurrence 16.8 vs 16.6 ms at c3 -- the GEMM workgroups contend
// with the co-resident recurrence)
int bwd_persist(const BBwd& a) {
  const int L = a.L, T = a.T, B = a.B, H = a.H, TBp = a.TBp;
  hipStream_t main = a.main;
  // every layer's W_hh^T / W_ih^T (bf16) in one launch
  if (int rc = a.wt_ready() ? 0 : wbf_transposes(L, H, a.w_ih, a.w_hh, a.wt, main)) return rc;
  // the weight gradients of every layer after the last recurrence, as the layer wavefront's one
  // whole-K launch (plan_fullk), where it applies; else per layer, split-K, after its recurrence
  G8Full f;
  int fP;
  const bool fullk = SV_PERSIST_FULLK && plan_fullk(a, f, fP);
  if (fullk && f.S > 0 && !a.cnt_ready()) {  // the first pieces' flags (else zeroed by the forward)
    if (int rc = sv_zero_counters(f.flag, 1, 0, fP, main)) return rc;
  }
  for (int l = L - 1; l >= 0; --l) {
    const int Fl = a.Fl(l);
    const BBwdWs ws = a.region(l);
    int rc = 0;
    const float* up = l == L - 1 ? a.dh_last : a.dx[l + 1];
    bf16_t* dgf = (bf16_t*)a.scratch();
    const bool afr = l > 0 && gemm_afrag_ok(T, B, Fl, H);  // dx reads dgf: no row-major dG
    // layer l on channel SV_BWD_CH0 + l, pre-zeroed by the forward (cnt_ready) where the layers fit
    // the channels, else each launch zeroing its own
    const bool own = L <= SV_SYNC_CHANNELS - SV_BWD_CH0;
    // the bias-gradient finalize rides on the next launch (the dx GEMM; layer 0's: the whole-K
    // weight-gradient launch), before the next recurrence reuses the partials' slots in dgf
    DbFin fin{};
    hipEvent_t* pp = a.layer_probe(l);
    if ((rc = sv_persist_bwd_bf16(T, B, H, ws.whhT, a.gates[l], a.c_tm[l], up, l < L - 1,
                                  (afr || l == 0) ? nullptr : a.dg[l],  // layer 0 has no dx GEMM
                                  a.dgT[l], dgf, main, a.sync, a.db_ih[l], a.db_hh ? a.db_hh[l] : nullptr,
                                  pp ? pp[0] : nullptr, pp ? pp[1] : nullptr, SV_BWD_CH0 + (own ? l : 0),
                                  own && a.cnt_ready(), &fin)))
      return rc;
    // the completion events of layers >= 1 (grad_ready: a caller's bucketed all-reduce) fire once
    // the last recurrence is done, so collectives never share the device with a persistent launch
    // (whose grid must be co-resident; a concurrent RCCL kernel would hold CUs it waits for) but
    // overlap layer 0's weight-gradient GEMMs
    for (int k = 1; l == 0 && k < L && a.evs() && !fullk; ++k)
      if ((rc = record(a.layer_done(k), main))) return rc;
    if (afr) {
      if ((rc = gemm_bf16_afrag(T, B, H, Fl, dgf, sv_persist_bm(B, H, sv_stream_cus(main)), ws.wihT, a.ld_wihT,
                                a.dx[l], Fl, ws.gws, main, fin)))
        return rc;
    } else if (l == 0 && fullk) {
      f.fin = fin;
    } else {
      if ((rc = sv_dbfin_launch(fin, main))) return rc;
      if (l > 0 && (rc = a.dx_gemm(l, ws, 0, T, main))) return rc;
    }
    if (fullk) continue;
    // dW_hh and dW_ih in one pass over dG^T (falls back to two GEMMs for layer 0's F = 40)
    rc = sv_gemm_bf16_dual(4 * H, H, Fl, TBp, a.dgT[l], TBp, a.hT[l], a.ldhT, a.dw_hh[l], H, a.xT[l], a.ld_xT[l],
                           a.dw_ih[l], Fl, ws.gws, main);
    if (rc) return rc;
  }
  if (fullk) return run_fullk(a, f, fP);
  return a.evs() ? record(a.layer_done(0), main) : SV_OK;
}
}  // namespace

extern "C" size_t sv_lstm_layer_bwd_bf16_workspace(int T, int B, int F, int H) {
  const int TBp = T * ((B + 7) & ~7);
  size_t g = sv_gemm_bf16_workspace(4 * H, H, TBp);
  g = std::max(g, sv_gemm_bf16_workspace(4 * H, F, TBp));
  g = std::max(g, sv_gemm_bf16_workspace(T * B, F, 4 * H));
  return 2 * ((size_t)B * H * sizeof(float) + 256) + g + 256;
}

// unlike a stack layer: dh_up [T,B,H] if dh_up_full; the caller's own transposed weights (W_ih^T
// rows of 4H); the workspace carved with the caller's F (dcf0, dcf1, the GEMM scratch); dx = dG W_ih
// only where dx_tm is given, behind the weight gradients; db_hh may be NULL
extern "C" int sv_lstm_layer_bwd_bf16(int T, int B, int F, int H, const bf16_t* xT_bf, long ld_xT,
                                      const bf16_t* wihT_bf, const bf16_t* whhT_bf, const bf16_t* gates,
                                      const float* c_tm, const bf16_t* hT_bf, const float* dh_up, int dh_up_full,
                                      bf16_t* dg_bf, bf16_t* dgT_bf, float* dx_tm, float* dw_ih, float* dw_hh,
                                      float* db_ih, float* db_hh, float* workspace, hipStream_t stream) {
  if (!xT_bf || !wihT_bf || !whhT_bf || !gates || !c_tm || !hT_bf || !dg_bf || !dgT_bf || !dw_ih || !dw_hh || !db_ih ||
      !workspace)
    return SV_EARG;
  if (T <= 0 || B <= 0 || F <= 0 || H <= 0 || F % 8 || H % 8 || ld_xT % 8) return SV_ESHAPE;
  const BBwd a{{1, T, B, F, H, T, stream, nullptr, nullptr, nullptr, 0, SV_SCHED_WT_READY},
               &xT_bf, &ld_xT, nullptr, nullptr, &gates, &c_tm, &hT_bf, dh_up, dh_up_full, &dg_bf, &dgT_bf, &dx_tm,
               &dw_ih, &dw_hh, &db_ih, &db_hh, (char*)workspace, nullptr, 0, 4L * H};
  BBwdWs ws = carve_bbwd((char*)workspace, T, B, F, H);
  ws.whhT = whhT_bf, ws.wihT = wihT_bf;
  int rc = a.prepare(0, ws, false, true, stream);
  if (!rc) rc = a.steps(0, ws, 0, T, stream);
  if (!rc) rc = a.grads(0, ws, true, stream);
  return (rc || !dx_tm) ? rc : a.dx_gemm(0, ws, 0, T, stream);
}

// validates, fills BBwd and dispatches to the schedule that `schedule` and the device select
extern "C" int sv_lstm_stack_bwd_bf16(int L, int T, int B, int F, int H, const bf16_t* const* xT, const long* ld_xT,
                                      const float* const* w_ih, const float* const* w_hh, const bf16_t* const* gates,
                                      const float* const* c_tm, const bf16_t* const* hT, const float* dh_last,
                                      bf16_t* const* dg, bf16_t* const* dgT, float* const* dx, float* const* dw_ih,
                                      float* const* dw_hh, float* const* db_ih, float* const* db_hh, void* workspace,
                                      void* wt, int chunk, hipStream_t main, const hipStream_t* side, hipEvent_t* ev,
                                      void* sync_block, hipEvent_t* probe, int schedule) {
  if (L <= 0 || !xT || !ld_xT || !w_ih || !w_hh || !gates || !c_tm || !hT || !dh_last || !dg || !dgT || !dx ||
      !dw_ih || !dw_hh || !db_ih || !workspace || !wt || ((uintptr_t)wt & 255) || !side || !ev || chunk <= 0)
    return SV_EARG;
  if (schedule & ~SV_SCHED_MASK) return SV_EARG;
  if (T <= 0 || B <= 0 || F <= 0 || H <= 0 || F % 8 || H % 8) return SV_ESHAPE;
  const BBwd a{{L, T, B, F, H, chunk, main, side, ev, probe, 0, schedule, reinterpret_cast<unsigned*>(sync_block)},
               xT, ld_xT, w_ih, w_hh, gates, c_tm, hT, dh_last, 0, dg, dgT, dx, dw_ih, dw_hh, db_ih, db_hh,
               static_cast<char*>(workspace), wt, carve_bbwd(nullptr, T, B, std::max(F, H), H).total,
               bf16_wiht_ld(H)};
  if (sched_wave(schedule, H) && sv_wave_bwd_fits(L, B, H, sv_stream_cus(main))) return a.sync ? bwd_wave(a) : SV_EARG;
  if (sched_persist(schedule, H) && sv_persist_bwd_fits(B, H, sv_stream_cus(main)))
    return a.sync ? bwd_persist(a) : SV_EARG;
  return stack_bwd_per_step(a);
}
