// The fp32 SpeechEmbedder LSTM on gfx950: the per-timestep recurrent kernels (K2 forward, K3
// backward; gate nonlinearities and cell update fused into the epilogue), the layout movers around
// them (frames to time-major, transpose, bias row sums) and the host glue that enqueues one layer
// or the layer stack under either schedule -- per-step (layer-pipelined over side streams) or
// persistent (the recurrences of sv_persist_f32.hip).  The GEMMs it enqueues (K1 input projection,
// dx, dW) are the library's general fp32 GEMM, sv_gemm_f32.hip.
//
// Replaces the reference's nn.LSTM forward (speech_embedder_net.py:19,28) and its
// autograd backward (train_speech_embedder.py:62), SURVEY §8 rows a-B and a-H.
//
// HBM layout (time-major, so every timestep slice is one contiguous [B, *] block):
//   x_tm   [T, B, F]      layer input
//   gates  [T, B, 4H]     in: x W_ih^T + b_ih + b_hh (K1); out: activated i,f,g,o (K2)
//   c_tm   [T, B, H]      cell state c_t
//   h_tm   [T+1, B, H]    h_tm[0] = h_{-1} = 0, h_tm[t+1] = h_t
//   dgates [T, B, 4H]     dL/d(pre-activation gates)
#include <stdlib.h>
#include <algorithm>
#include "sv_common.h"
#include "sv_gemm.h"
#include "sv_lstm_stack.h"
#include "../../include/sv_ge2e.h"

// [B, T, F] (batch_first) -> [T, B, F]
__global__ void to_time_major_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int T, int F4) {
  const long total = (long)B * T * F4;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int f = (int)(e % F4);
    const long bt = e / F4;
    const int t = (int)(bt % T), b = (int)(bt / T);
    reinterpret_cast<f32x4*>(y)[((long)t * B + b) * F4 + f] = reinterpret_cast<const f32x4*>(x)[e];
  }
}

// row sums out[r] = sum_c X[r*ld + c], one block of RS_T threads per row, fixed order.
// 512-thread blocks: 4 per CU resident, so the 4H = 3072 rows of c2 run as 3 full rounds of
// 1024 blocks (256-thread blocks left a half-empty second round: 3072 / 2048)
#define RS_T 512
__global__ __launch_bounds__(RS_T) void rowsum_kernel(const float* __restrict__ X, long ld, int C,
                                                      float* __restrict__ out0, float* __restrict__ out1) {
  __shared__ float red[RS_T / 64];
  const float* x = X + (long)blockIdx.x * ld;
  // four independent 16-B loads in flight per thread per trip (a row is 400 KB at c2), summed
  // in a fixed order
  const int C4 = C / 4;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int c = threadIdx.x;
  for (; c + 3 * RS_T < C4; c += 4 * RS_T) {
    const f32x4 v0 = x4[c], v1 = x4[c + RS_T], v2 = x4[c + 2 * RS_T], v3 = x4[c + 3 * RS_T];
    s0 += (v0.x + v0.y) + (v0.z + v0.w);
    s1 += (v1.x + v1.y) + (v1.z + v1.w);
    s2 += (v2.x + v2.y) + (v2.z + v2.w);
    s3 += (v3.x + v3.y) + (v3.z + v3.w);
  }
  for (; c < C4; c += RS_T) {
    const f32x4 v = x4[c];
    s0 += (v.x + v.y) + (v.z + v.w);
  }
  float s = (s0 + s1) + (s2 + s3);
  for (int c1 = C4 * 4 + threadIdx.x; c1 < C; c1 += RS_T) s += x[c1];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < RS_T / 64; ++i) t += red[i];
    out0[blockIdx.x] = t;
    if (out1) out1[blockIdx.x] = t;
  }
}

// dst[c*ldd + r] = src[r*lds + c]  (R x C), 32x32 tiles through LDS
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ src, long lds_, int R, int C,
                                                        float* __restrict__ dst, long ldd) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < R && c < C) ? src[(long)r * lds_ + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + tx;
    if (c < C && r < R) dst[(long)c * ldd + r] = tile[tx][i];
  }
}

// ============================================================================
// K2: forward recurrent step.  Block = 64 batch rows x 32 hidden units (= 128 gate
// columns: i,f,g,o of those units), 4 waves in 2x2; K = H, k-major LDS tiles.
// Epilogue: + x-projection, sigmoid/tanh, c_t = f c_{t-1} + i g, h_t = o tanh(c_t);
// stores the activated gates (for BPTT), c_t, h_t and h_t^T (column block t+1 of
// hT[H, (T+1) B], the k-contiguous operand of the weight-gradient GEMMs).
// ============================================================================
#define FWD_BM 64
#define FWD_U 32

// ============================================================================
// K3: backward recurrent step at time t.  Block = 64 batch rows x 32 hidden units;
// wave w computes dG_{t+1}[:, gate w] . W_hh[gate w rows, units] (K = H each, an
// in-block split of K = 4H by gate) from W_hh^T [H, 4H] (k-contiguous), partials summed
// in LDS in fixed order.  Epilogue: dh = that + dh_up; dc = dc_{t+1} f_{t+1} + dh o
// (1 - tanh^2 c); dG_t = [dc g i(1-i), dc c_{t-1} f(1-f), dc i (1-g^2), dh tanh(c) o(1-o)],
// stored as dG[t] [B, 4H] and as column block t of dG^T [4H, T B].
// ============================================================================
#define BWD_BM 64
#define BWD_U 32
#define X3_GBUF_BYTES (12 * (BWD_BM + BWD_U) * (16 + 8))  // one gate group's X3 double buffer

// ============================================================================
// 8-wave variants of K2/K3 (512 threads, 2 waves per SIMD so one wave's MFMAs cover the
// other's LDS/global waits).
//   K2v2: the 64 x 128 gate tile is split 2 (rows) x 4 (gate) over 8 waves, one 32x32
//         accumulator each, all sharing the same staged A/B tiles.
//   K3v2: 4 groups of 2 waves, group = gate (its K range of W_hh^T), waves split the rows.
// ============================================================================
template <int BKX, int D = 1, bool X6 = false, bool X3 = false>
__global__ __launch_bounds__(512) void lstm_step_fwd_v2_kernel(const float* __restrict__ hprev,
                                                               const float* __restrict__ whh,
                                                               float* __restrict__ gates,
                                                               const float* __restrict__ cprev,
                                                               float* __restrict__ cout, float* __restrict__ hout,
                                                               float* __restrict__ hT, long ldhT, int t, int Bp, int B,
                                                               int H) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int BN = 4 * FWD_U, LDP = BN + 4, LDH = FWD_BM + 1;
  constexpr int PER = FWD_BM * FWD_U / 512;  // epilogue elements per thread
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j0 = blockIdx.x * FWD_U, b0 = blockIdx.y * FWD_BM;
  const int wm0 = (w >> 2) * 32, wn0 = (w & 3) * 32;
  const long G = 4L * H;
  // the epilogue's inputs do not depend on the GEMM: issue their loads first
  float xg[PER][4], cpv[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = tid + 512 * k, b = e / FWD_U, u = e % FWD_U;
    const int gb = b0 + b, gj = j0 + u;
    const bool ok = gb < B && gj < H;
    const float* gp = gates + (long)gb * G + gj;
#pragma unroll
    for (int q = 0; q < 4; ++q) xg[k][q] = ok ? gp[q * H] : 0.f;
    cpv[k] = (ok && cprev) ? cprev[(long)gb * H + gj] : 0.f;
  }
  f32x16 acc[1][1];
  zero_acc(acc);
  if (hprev) {
    if constexpr (X3)
      gemm_mainloop_x3<FWD_BM, BN, 512, 32, 2, 1, 1>(hprev + (long)b0 * H, H, RowMapLinear{0, B - b0}, whh, H,
                                                     RowMapGates<FWD_U>{j0, H}, 0, H, lds, tid, wm0, wn0, acc);
    else
      gemm_mainloop_km_d<FWD_BM, BN, 512, BKX, D, 1, 1, false, X6>(hprev + (long)b0 * H, H, RowMapLinear{0, B - b0},
                                                                  whh, H, RowMapGates<FWD_U>{j0, H}, 0, H, lds, tid,
                                                                  wm0, wn0, acc);
  }
  float* pre = lds;
  float* hs = lds + FWD_BM * LDP;
#pragma unroll
  for (int r = 0; r < 16; ++r) pre[(wm0 + acc_row(r, lane)) * LDP + wn0 + (lane & 31)] = acc[0][0][r];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = tid + 512 * k, b = e / FWD_U, u = e % FWD_U;
    const int gb = b0 + b, gj = j0 + u;
    if (gb >= B || gj >= H) continue;
    float* gp = gates + (long)gb * G + gj;
    const float* pr = pre + b * LDP + u;
    const float i = sv_sigmoid(pr[0] + xg[k][0]);
    const float f = sv_sigmoid(pr[FWD_U] + xg[k][1]);
    const float g = sv_tanh(pr[2 * FWD_U] + xg[k][2]);
    const float o = sv_sigmoid(pr[3 * FWD_U] + xg[k][3]);
    const float c = f * cpv[k] + i * g;
    const float h = o * sv_tanh(c);
    gp[0] = i;
    gp[H] = f;
    gp[2 * H] = g;
    gp[3 * H] = o;
    cout[(long)gb * H + gj] = c;
    hout[(long)gb * H + gj] = h;
    hs[u * LDH + b] = h;
  }
  if (!hT) return;
  __syncthreads();
  for (int e = tid; e < FWD_BM * FWD_U; e += 512) {
    const int u = e / FWD_BM, b = e % FWD_BM;
    const int gb = b0 + b, gj = j0 + u;
    if (gb >= B || gj >= H) continue;
    float* row = hT + (long)gj * ldhT;
    row[(long)(t + 1) * Bp + gb] = hs[u * LDH + b];
    if (t == 0) row[gb] = 0.f;
  }
}

template <int BKX, int D = 1, bool X6 = false, bool X3 = false>
__global__ __launch_bounds__(512) void lstm_step_bwd_v2_kernel(
    const float* __restrict__ dgnext, const float* __restrict__ whhT, const float* __restrict__ dhup,
    const float* __restrict__ dcf_next, const float* __restrict__ acts, const float* __restrict__ c_t,
    const float* __restrict__ c_prev, float* __restrict__ dg, float* __restrict__ dcf, float* __restrict__ dgT,
    long lddgT, int t, int Bp, int B, int H, unsigned long long* __restrict__ ts = nullptr) {
  // ts (timing sample, bench only): [start, end] of this launch on the 100 MHz real-time clock,
  // first workgroup start (min) and last workgroup end (max), vector atomics
  if (ts && threadIdx.x == 0) atomicMin(ts, (unsigned long long)__builtin_amdgcn_s_memrealtime());
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int GBUF = 2 * (BWD_BM + BWD_U) * (BKX + 4);
  constexpr int LDR = BWD_U + 1;
  constexpr int LDT = BWD_BM + 1;
  constexpr int PER = BWD_BM * BWD_U / 512;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int gate = w >> 1, gt = tid & 127;
  const int j0 = blockIdx.x * BWD_U, b0 = blockIdx.y * BWD_BM;
  const long G = 4L * H;
  // prefetch the epilogue's element-wise inputs (independent of the GEMM)
  float av[PER][4], cv[PER], cpv[PER], dcfv[PER], upv[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = tid + 512 * k, b = e / BWD_U, u = e % BWD_U;
    const int gb = b0 + b, gj = j0 + u;
    const bool ok = gb < B && gj < H;
    const long hi = (long)gb * H + gj;
    const float* ap = acts + (long)gb * G + gj;
#pragma unroll
    for (int q = 0; q < 4; ++q) av[k][q] = ok ? ap[q * H] : 0.f;
    cv[k] = ok ? c_t[hi] : 0.f;
    cpv[k] = (ok && c_prev) ? c_prev[hi] : 0.f;
    dcfv[k] = (ok && dcf_next) ? dcf_next[hi] : 0.f;
    upv[k] = (ok && dhup) ? dhup[hi] : 0.f;
  }
  f32x16 acc[1][1];
  zero_acc(acc);
  if (dgnext) {
    if constexpr (X3)
      gemm_mainloop_x3<BWD_BM, BWD_U, 128, 16, 2, 1, 1>(dgnext + (long)b0 * G, G, RowMapLinear{0, B - b0}, whhT, G,
                                                        RowMapLinear{j0, H}, gate * H, (gate + 1) * H,
                                                        reinterpret_cast<char*>(lds) + gate * X3_GBUF_BYTES, gt,
                                                        (w & 1) * 32, 0, acc);
    else
      gemm_mainloop_km_d<BWD_BM, BWD_U, 128, BKX, D, 1, 1, false, X6>(
          dgnext + (long)b0 * G, G, RowMapLinear{0, B - b0}, whhT, G, RowMapLinear{j0, H}, gate * H, (gate + 1) * H,
          lds + gate * GBUF, gt, (w & 1) * 32, 0, acc);
  }
  __syncthreads();
  float* red = lds;                    // [4][64][LDR]
  float* gT = lds + 4 * BWD_BM * LDR;  // [4*32][LDT]
#pragma unroll
  for (int r = 0; r < 16; ++r)
    red[(gate * BWD_BM + (w & 1) * 32 + acc_row(r, lane)) * LDR + (lane & 31)] = acc[0][0][r];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = tid + 512 * k, b = e / BWD_U, u = e % BWD_U;
    const int gb = b0 + b, gj = j0 + u;
    if (gb >= B || gj >= H) continue;
    const long hi = (long)gb * H + gj;
    float dh = red[(0 * BWD_BM + b) * LDR + u];
    dh += red[(1 * BWD_BM + b) * LDR + u];
    dh += red[(2 * BWD_BM + b) * LDR + u];
    dh += red[(3 * BWD_BM + b) * LDR + u];
    dh += upv[k];
    const float i = av[k][0], f = av[k][1], g = av[k][2], o = av[k][3];
    const float tc = sv_tanh(cv[k]);
    const float dc = dh * o * (1.f - tc * tc) + dcfv[k];
    const float d0 = dc * g * i * (1.f - i), d1 = dc * cpv[k] * f * (1.f - f);
    const float d2 = dc * i * (1.f - g * g), d3 = dh * tc * o * (1.f - o);
    float* dp = dg + (long)gb * G + gj;
    dp[0] = d0;
    dp[H] = d1;
    dp[2 * H] = d2;
    dp[3 * H] = d3;
    dcf[hi] = dc * f;
    gT[(0 * BWD_U + u) * LDT + b] = d0;
    gT[(1 * BWD_U + u) * LDT + b] = d1;
    gT[(2 * BWD_U + u) * LDT + b] = d2;
    gT[(3 * BWD_U + u) * LDT + b] = d3;
  }
  if (dgT) {
    __syncthreads();
    for (int e = tid; e < 4 * BWD_U * BWD_BM; e += 512) {
      const int gu = e / BWD_BM, b = e % BWD_BM;
      const int gte = gu / BWD_U, u = gu % BWD_U;
      const int gb = b0 + b, gj = j0 + u;
      if (gb >= B || gj >= H) continue;
      dgT[((long)gte * H + gj) * lddgT + (long)t * Bp + gb] = gT[gu * LDT + b];
    }
  }
  if (ts) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(ts + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
  }
}

extern "C" int sv_frames_to_time_major(const float* x, float* x_tm, int B, int T, int F, hipStream_t stream) {
  if (!x || !x_tm || B <= 0 || T <= 0 || F <= 0) return SV_EARG;
  if (F % 4 || (((uintptr_t)x | (uintptr_t)x_tm) & 15)) return SV_EALIGN;
  const long total = (long)B * T * (F / 4);
  const int grid = (int)std::min<long>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(to_time_major_kernel, dim3(grid), dim3(256), 0, stream, x, x_tm, B, T, F / 4);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_transpose(const float* src, long ld_src, int R, int C, float* dst, long ld_dst, hipStream_t stream) {
  if (!src || !dst || R <= 0 || C <= 0) return SV_EARG;
  hipLaunchKernelGGL(transpose_kernel, dim3((C + 31) / 32, (R + 31) / 32), dim3(256), 0, stream, src, ld_src, R, C, dst,
                     ld_dst);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

static bool lstm_dims_ok(int T, int B, int F, int H) {
  return T > 0 && B > 0 && F > 0 && H > 0 && F % 4 == 0 && H % 4 == 0;
}

namespace {
constexpr int FWD_LDS_MAIN = 2 * (FWD_BM + 4 * FWD_U) * (SV_BKM + 4);
constexpr int FWD_LDS_EPI = FWD_BM * (4 * FWD_U + 4) + FWD_U * (FWD_BM + 1);
constexpr int FWD_LDS = (FWD_LDS_MAIN > FWD_LDS_EPI ? FWD_LDS_MAIN : FWD_LDS_EPI) * (int)sizeof(float);
constexpr int BWD_LDS_MAIN = 4 * 2 * (BWD_BM + BWD_U) * (SV_BKM + 4);
constexpr int BWD_LDS_EPI = 4 * BWD_BM * (BWD_U + 1) + 4 * BWD_U * (BWD_BM + 1);
constexpr int BWD_LDS = (BWD_LDS_MAIN > BWD_LDS_EPI ? BWD_LDS_MAIN : BWD_LDS_EPI) * (int)sizeof(float);
// step-kernel main loops: pipelined local read (gemm_mainloop_km_plr; one barrier per k-tile, LDS
// writes issued behind the first k-group's MFMAs) with 1 register stage for K2 and 2 for K3.
// Measured at c2 against the rolling register prefetch of depth 2 (us): K2 35.1-35.6 vs 41.7,
// K3 37.2-38.0 vs 41.5; c2 step 69.3 -> 66.4-67.0 ms.  The x6 / x3 forms are the bf16x6 product
// mode's (`products`, F32ProductScope): K2 split at the LDS store (x3), K3 exact.
constexpr int FWD_X3_MAIN = 12 * (FWD_BM + 4 * FWD_U) * (32 + 8);
constexpr int FWD_X3_LDS = FWD_X3_MAIN > FWD_LDS ? FWD_X3_MAIN : FWD_LDS;
constexpr int BWD_X3_MAIN = 4 * X3_GBUF_BYTES;
constexpr int BWD_X3_LDS = BWD_X3_MAIN > BWD_LDS ? BWD_X3_MAIN : BWD_LDS;
dim3 fwd_step_grid(int B, int H) { return dim3((H + FWD_U - 1) / FWD_U, (B + FWD_BM - 1) / FWD_BM); }
void launch_fwd_step(dim3 grid, hipStream_t s, const float* hp, const float* whh, float* g, const float* cp, float* c,
                     float* h, float* hT, long ldhT, int t, int Bp, int B, int H) {
  if (k2_x() == 2)
    hipLaunchKernelGGL((lstm_step_fwd_v2_kernel<SV_BKM, 2, false, true>), grid, dim3(512), FWD_X3_LDS, s, hp, whh, g,
                       cp, c, h, hT, ldhT, t, Bp, B, H);
  else if (k2_x() == 1)
    hipLaunchKernelGGL((lstm_step_fwd_v2_kernel<SV_BKM, 2, true>), grid, dim3(512), FWD_LDS, s, hp, whh, g, cp, c, h,
                       hT, ldhT, t, Bp, B, H);
  else
    hipLaunchKernelGGL((lstm_step_fwd_v2_kernel<SV_BKM, SV_PLR + 1>), grid, dim3(512), FWD_LDS, s, hp, whh, g, cp, c, h,
                       hT, ldhT, t, Bp, B, H);
}
void launch_bwd_step(dim3 grid, hipStream_t s, const float* dgn, const float* whhT, const float* up, const float* dcfi,
                     const float* acts, const float* ct, const float* cp, float* dg, float* dcfo, float* dgT,
                     long lddgT, int t, int Bp, int B, int H, unsigned long long* ts = nullptr) {
  if (k3_x() == 2)
    hipLaunchKernelGGL((lstm_step_bwd_v2_kernel<SV_BKM, 2, false, true>), grid, dim3(512), BWD_X3_LDS, s, dgn, whhT, up,
                       dcfi, acts, ct, cp, dg, dcfo, dgT, lddgT, t, Bp, B, H, ts);
  else if (k3_x() == 1)
    hipLaunchKernelGGL((lstm_step_bwd_v2_kernel<SV_BKM, 2, true>), grid, dim3(512), BWD_LDS, s, dgn, whhT, up, dcfi,
                       acts, ct, cp, dg, dcfo, dgT, lddgT, t, Bp, B, H, ts);
  else
    hipLaunchKernelGGL((lstm_step_bwd_v2_kernel<SV_BKM, SV_PLR + 2>), grid, dim3(512), BWD_LDS, s, dgn, whhT, up, dcfi,
                       acts, ct, cp, dg, dcfo, dgT, lddgT, t, Bp, B, H, ts);
}
}  // namespace

extern "C" int sv_lstm_step_fwd(const float* h_prev, const float* w_hh, float* gates_t, const float* c_prev,
                                float* c_t, float* h_t, int B, int H, hipStream_t stream) {
  if (!w_hh || !gates_t || !c_t || !h_t || B <= 0 || H <= 0 || H % 4) return SV_EARG;
  const dim3 grid = fwd_step_grid(B, H);
  launch_fwd_step(grid, stream, h_prev, w_hh, gates_t, c_prev, c_t, h_t, nullptr, 0L, 0, B, B, H);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// one backward recurrent step (K3) on its own (timing / tests): dg_next may be NULL (t = T-1)
extern "C" int sv_lstm_step_bwd(const float* dg_next, const float* w_hhT, const float* dh_up, const float* dcf_next,
                                const float* acts_t, const float* c_t, const float* c_prev, float* dg_t, float* dcf_t,
                                int B, int H, hipStream_t stream) {
  if (!w_hhT || !acts_t || !c_t || !dg_t || !dcf_t || B <= 0 || H <= 0 || H % 4) return SV_EARG;
  const dim3 grid((H + BWD_U - 1) / BWD_U, (B + BWD_BM - 1) / BWD_BM);
  launch_bwd_step(grid, stream, dg_next, w_hhT, dh_up, dcf_next, acts_t, c_t, c_prev, dg_t, dcf_t, nullptr, 0L, 0, B, B,
                  H);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// Row stride (floats) of the library's own W_ih^T copies (fp32 [F][4H]), the dx GEMMs' B operand:
// 4H + 64.  A 12-KB row stride put the 256 rows of a k-tile fill on one L2 channel;
// 64 more floats spread them (the c2 dx GEMM 3707 -> 3654 us isolated, scripts/gemm_ld_ab.py).
static inline long f32_wiht_ld(int H) { return 4L * H + 64; }

namespace {
struct BwdWs {
  float *dcf0, *dcf1, *whhT, *wihT, *gws;
  size_t total;
};
size_t al4(size_t n) { return (n + 63) & ~size_t(63); }
size_t al256(size_t n) { return (n + 255) & ~size_t(255); }
BwdWs carve_bwd(float* base, int T, int B, int F, int H) {
  BwdWs w;
  size_t off = 0;
  auto take = [&](size_t n) {
    float* p = base ? base + off : nullptr;
    off += al4(n);
    return p;
  };
  w.dcf0 = take((size_t)B * H);
  w.dcf1 = take((size_t)B * H);
  w.whhT = take((size_t)4 * H * H);
  w.wihT = take((size_t)f32_wiht_ld(H) * F);
  const int TBp = T * ((B + 3) & ~3);
  size_t g = sv_gemm_f32_workspace(4 * H, H, TBp);
  g = std::max(g, sv_gemm_f32_workspace(4 * H, F, TBp));
  g = std::max(g, sv_gemm_f32_workspace(T * B, F, 4 * H));
  w.gws = take((g + 3) / 4);
  w.total = off * sizeof(float);
  return w;
}
// The stack backward's workspace: L regions of ws_per bytes (carve_bwd at the wider of F and H);
// behind them, at H = 768 (where the persistent recurrences can run), the persistent backward's
// fragment-order hand-off (ws_handoff bytes, shared by the layers, one after another) and the dx
// GEMM's stream-K scratch (gf_sk_bytes)
size_t ws_per(int T, int B, int F, int H) { return al256(carve_bwd(nullptr, T, B, std::max(F, H), H).total); }
size_t ws_handoff(int T, int B, int H) { return H == 768 ? al256(sv_persist_f32_bwd_scratch(T, B, H)) : 0; }
// One layer's sequences on the shared stack frame (sv_lstm_stack.h), batch padded to 4
struct Fwd : Stack<4> {
  const float* x_tm;
  const float *const *w_ih, *const *w_hh, *const *b_ih, *const *b_hh;
  float *const *gates, *const *c_tm, *const *h_tm, *const *hT;
  // K1 for t0 .. t1-1: gates = in W_ih^T + b_ih + b_hh; in = the frames or the layer below's h
  // (slot t + 1 = h_t)
  int k1(int l, int t0, int t1, hipStream_t s) const {
    const float* in = l == 0 ? x_tm + (long)t0 * B * F : h_tm[l - 1] + (long)(t0 + 1) * BH;
    return gemm_f32(1, 1, (t1 - t0) * B, 4 * H, Fl(l), in, Fl(l), w_ih[l], Fl(l), gates[l] + t0 * BG, 4L * H, b_ih[l],
                    b_hh[l], 0.f, nullptr, s);
  }
  // h_tm[0] = h_{-1} = 0; where B is padded, hT whole (its padding columns are GEMM operands)
  int reset(int l, hipStream_t s) const {
    int rc = sv_zero_bytes(h_tm[l], BH * sizeof(float), s);
    if (!rc && hT[l] && Bp != B) rc = sv_zero_bytes(hT[l], (size_t)H * ldhT * sizeof(float), s);
    return rc;
  }
  // K2 for t0 .. t1-1
  int steps(int l, int t0, int t1, hipStream_t s) const {
    for (int t = t0; t < t1; ++t) {
      launch_fwd_step(fwd_step_grid(B, H), s, t ? h_tm[l] + t * BH : nullptr, w_hh[l], gates[l] + t * BG,
                      t ? c_tm[l] + (t - 1) * BH : nullptr, c_tm[l] + t * BH, h_tm[l] + (t + 1) * BH, hT[l], ldhT, t,
                      Bp, B, H);
      SV_LAUNCH_CHECK();
    }
    return SV_OK;
  }
};

struct Bwd : Stack<4> {
  const float* const* xT;
  const long* ld_xT;
  const float *const *w_ih, *const *w_hh, *const *gates, *const *c_tm, *const *hT;
  const float* dh_last;  // dh into the top layer: [B,H] for t = T-1 alone, or -- top_full -- [T,B,H]
  int top_full;
  float *const *dgates, *const *dgT, *const *dx, *const *dw_ih, *const *dw_hh, *const *db_ih, *const *db_hh;
  char* workspace;
  unsigned long long* kstamp;
  size_t per;  // ws_per
  BwdWs region(int l) const { return carve_bwd((float*)(workspace + per * l), T, B, std::max(F, H), H); }
  float* handoff() const { return (float*)(workspace + per * L); }
  void* skws() const { return workspace + per * L + ws_handoff(T, B, H); }
  // W_hh^T [H, 4H] and -- wih -- W_ih^T [Fl, 4H] into ws; dgT (zero: the step kernels will fill it)
  // zeroed where B is padded
  int prepare(int l, const BwdWs& ws, bool wih, bool zero, hipStream_t s) const {
    int rc = sv_transpose(w_hh[l], H, 4 * H, H, ws.whhT, 4L * H, s);
    if (!rc && wih) rc = wih_transpose(l, ws, s);
    if (!rc && zero && Bp != B) rc = sv_zero_bytes(dgT[l], (size_t)4 * H * TBp * sizeof(float), s);
    return rc;
  }
  int wih_transpose(int l, const BwdWs& ws, hipStream_t s) const {
    return sv_transpose(w_ih[l], Fl(l), 4 * H, Fl(l), ws.wihT, f32_wiht_ld(H), s);
  }
  // K3 for t1-1 .. t0; dh from above: dh_last for the top layer, else layer l + 1's dx [T,B,H].
  // pp (or NULL): an event pair around one launch, the range's second (behind a running K3 on its
  // stream; the first if the range has one).  kstamp (or NULL): [L][T][2] start / end stamps.
  int steps(int l, const BwdWs& ws, int t0, int t1, hipStream_t s, hipEvent_t* pp = nullptr) const {
    const dim3 grid((H + BWD_U - 1) / BWD_U, (B + BWD_BM - 1) / BWD_BM);
    const int tp = t1 - t0 > 1 ? t1 - 2 : t0;
    const float* up = l == L - 1 ? dh_last : dx[l + 1];
    const bool full = l < L - 1 || top_full;
    float* const dcf[2] = {ws.dcf0, ws.dcf1};  // ping-pong: step t writes dcf[t & 1], reads step t + 1's
    int rc;
    for (int t = t1 - 1; t >= t0; --t) {
      const bool last = t == T - 1;
      if (pp && t == tp && (rc = record(pp[0], s))) return rc;
      launch_bwd_step(grid, s, last ? nullptr : dgates[l] + (t + 1) * BG, ws.whhT,
                      !up ? nullptr : full ? up + t * BH : last ? up : nullptr, last ? nullptr : dcf[~t & 1],
                      gates[l] + t * BG, c_tm[l] + t * BH, t ? c_tm[l] + (t - 1) * BH : nullptr, dgates[l] + t * BG,
                      dcf[t & 1], dgT[l], (long)TBp, t, Bp, B, H, kstamp ? kstamp + 2 * ((long)l * T + t) : nullptr);
      SV_LAUNCH_CHECK();
      if (pp && t == tp && (rc = record(pp[1], s))) return rc;
    }
    return SV_OK;
  }
  // dx = dG W_ih for t0 .. t1-1: A = dG [rows, 4H], B = W_ih^T [Fl, 4H] (ws.wihT)
  int dx_gemm(int l, const BwdWs& ws, int t0, int t1, hipStream_t s) const {
    return gemm_f32(1, 1, (t1 - t0) * B, Fl(l), 4 * H, dgates[l] + t0 * BG, 4L * H, ws.wihT, f32_wiht_ld(H),
                    dx[l] + (long)t0 * B * Fl(l), Fl(l), nullptr, nullptr, 0.f, ws.gws, s);
  }
  // dW_hh = sum_t dG_t^T h_{t-1}: A = dG^T [4H, T Bp], B = hT[:, 0:T Bp] (column block t = h_{t-1});
  // dW_ih = sum_t dG_t^T x_t: B = x^T [Fl, T Bp]; db (where the recurrence has not summed the
  // biases itself): db_ih = db_hh (may be NULL) = row sums of dG^T
  int grads(int l, const BwdWs& ws, bool db, hipStream_t s) const {
    int rc = gemm_f32(1, 1, 4 * H, H, TBp, dgT[l], TBp, hT[l], ldhT, dw_hh[l], H, nullptr, nullptr, 0.f, ws.gws, s);
    if (!rc)
      rc = gemm_f32(1, 1, 4 * H, Fl(l), TBp, dgT[l], TBp, xT[l], ld_xT[l], dw_ih[l], Fl(l), nullptr, nullptr, 0.f, ws.gws,
                    s);
    if (rc || !db) return rc;
    hipLaunchKernelGGL(rowsum_kernel, dim3(4 * H), dim3(RS_T), 0, s, dgT[l], (long)TBp, TBp, db_ih[l],
                       db_hh ? db_hh[l] : nullptr);
    return (int)hipGetLastError();
  }
};
}  // namespace

extern "C" int sv_lstm_layer_fwd(const float* x_tm, int T, int B, int F, int H, const float* w_ih, const float* w_hh,
                                 const float* b_ih, const float* b_hh, float* gates, float* c_tm, float* h_tm,
                                 float* hT, hipStream_t stream) {
  if (!x_tm || !w_ih || !w_hh || !gates || !c_tm || !h_tm) return SV_EARG;
  if (!lstm_dims_ok(T, B, F, H)) return SV_ESHAPE;
  const Fwd a{{1, T, B, F, H, T, stream}, x_tm, &w_ih, &w_hh, &b_ih, &b_hh, &gates, &c_tm, &h_tm, &hT};
  int rc = a.k1(0, 0, T, stream);  // the all-timestep input projection
  if (!rc) rc = a.reset(0, stream);
  return rc ? rc : a.steps(0, 0, T, stream);
}

extern "C" size_t sv_lstm_layer_bwd_workspace(int T, int B, int F, int H) { return carve_bwd(nullptr, T, B, F, H).total; }

// unlike a stack layer: dh_up [T,B,H] if dh_up_full; the workspace carved with the caller's F;
// W_ih^T and dx = dG W_ih only where dx_tm is given, behind the weight gradients; db_hh may be NULL
extern "C" int sv_lstm_layer_bwd(int T, int B, int F, int H, const float* xT, long ld_xT, const float* w_ih,
                                 const float* w_hh, const float* gates, const float* c_tm, const float* hT,
                                 const float* dh_up, int dh_up_full, float* dgates, float* dgT, float* dx_tm,
                                 float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, float* workspace,
                                 hipStream_t stream) {
  if (!xT || !w_ih || !w_hh || !gates || !c_tm || !hT || !dgates || !dgT || !dw_ih || !dw_hh || !db_ih || !workspace)
    return SV_EARG;
  if (!lstm_dims_ok(T, B, F, H) || ld_xT % 4) return SV_ESHAPE;
  const Bwd a{{1, T, B, F, H, T, stream}, &xT, &ld_xT, &w_ih, &w_hh, &gates, &c_tm, &hT, dh_up, dh_up_full,
              &dgates, &dgT, &dx_tm, &dw_ih, &dw_hh, &db_ih, &db_hh, (char*)workspace, nullptr, 0};
  const BwdWs ws = carve_bwd(workspace, T, B, F, H);
  int rc = a.prepare(0, ws, false, true, stream);
  if (!rc) rc = a.steps(0, ws, 0, T, stream);
  if (!rc) rc = a.grads(0, ws, true, stream);
  if (rc || !dx_tm) return rc;
  rc = a.wih_transpose(0, ws, stream);
  return rc ? rc : a.dx_gemm(0, ws, 0, T, stream);
}

// The layer stack under two schedules.  Per-step, layer-pipelined: layer l runs on side[l], its
// timesteps in chunks of `chunk`, and waits only for its neighbour layer to finish the same chunk,
// so up to L layers' kernels run at once and one layer's latency-bound step kernels overlap
// another's GEMMs (each step block leaves room for a second resident block per CU); joins back
// into `main`.  Persistent: the fp32 W-stationary recurrences (sv_persist_f32.hip), one layer after
// another on `main` (their grid needs the whole chip) -- never under SV_SCHED_PER_STEP; where they
// fit co-resident, under SV_SCHED_PERSIST always, under SV_SCHED_AUTO when the grid fills at least
// 3/4 of the device (c2: 240 of 256 CUs; a half-empty grid leaves the chip to per-step kernels that
// share it with the GEMMs).  Host arrays (length L) carry the per-layer device pointers.
static bool f32_persist(int schedule, int B, int H, hipStream_t s) {
  if (schedule & SV_SCHED_PER_STEP) return false;
  const int cus = sv_stream_cus(s);
  if (!sv_persist_f32_fits(B, H, cus)) return false;
  return (schedule & SV_SCHED_PERSIST) || 4L * (H / 32) * ((B + 63) / 64) >= 3L * cus;
}

extern "C" int sv_lstm_f32_persist_ok(int B, int H, int schedule) { return f32_persist(schedule, B, H, nullptr); }

static int fwd_persist(const Fwd& a) {
  for (int l = 0; l < a.L; ++l) {
    int rc = a.reset(l, a.main);
    if (rc) return rc;
    // layer 0 at F = 40: the input projection inside the recurrence (c2 layer 0:
    // the K=40 GEMM wrote 1.26 GB that the recurrence read back)
    // (exact fp32 products only: the bf16x6 mode keeps the GEMM, whose products it splits; and 16-B
    // aligned x_tm / W_ih only: the kernel reads them by LDS-DMA / f32x4 -- else the GEMM path
    // rejects the misaligned pointer with SV_EALIGN)
    const bool fuse = l == 0 && a.F == 40 && a.products == 0 && !(((uintptr_t)a.x_tm | (uintptr_t)a.w_ih[0]) & 15);
    if (!fuse && (rc = a.k1(l, 0, a.T, a.main))) return rc;
    hipEvent_t* pp = a.layer_probe(l);
    rc = sv_persist_fwd_f32(a.T, a.B, a.H, a.w_hh[l], a.gates[l], a.c_tm[l], a.h_tm[l], a.hT[l], a.main, a.sync, 0,
                            pp ? pp[0] : nullptr, pp ? pp[1] : nullptr, fuse ? a.x_tm : nullptr, a.F, a.w_ih[l],
                            a.b_ih[l], a.b_hh[l]);
    if (rc) return rc;
  }
  return SV_OK;
}

extern "C" int sv_lstm_stack_fwd(int L, int T, int B, int F, int H, const float* x_tm, const float* const* w_ih,
                                 const float* const* w_hh, const float* const* b_ih, const float* const* b_hh,
                                 float* const* gates, float* const* c_tm, float* const* h_tm, float* const* hT,
                                 int chunk, hipStream_t main, const hipStream_t* side, hipEvent_t* ev,
                                 int products, int schedule, unsigned* sync, hipEvent_t* probe) {
  if (L <= 0 || !x_tm || !w_ih || !w_hh || !gates || !c_tm || !h_tm || !side || !ev || chunk <= 0) return SV_EARG;
  if (products < 0 || products > 3 || schedule < 0 || schedule > SV_SCHED_MASK) return SV_EARG;
  F32ProductScope scope(products);
  if (!lstm_dims_ok(T, B, F, H)) return SV_ESHAPE;
  const Fwd a{{L, T, B, F, H, chunk, main, side, ev, probe, products, schedule, sync},
              x_tm, w_ih, w_hh, b_ih, b_hh, gates, c_tm, h_tm, hT};
  if (f32_persist(schedule, B, H, main)) return sync ? fwd_persist(a) : SV_EARG;
  return stack_fwd_per_step(a);
}

// Stack backward, top layer first in issue order.  Per-step: layer l's timesteps in reverse chunks
// (K3 steps, then -- for l > 0 -- the chunk's dx = dG W_ih GEMM, the next-lower layer's dh_up for
// those timesteps), then its whole-T weight-gradient GEMMs and bias row sums behind the recurrence
// on the same stream; layer l-1 waits only for layer l's dx of the same chunk, so one layer's
// recurrence overlaps the upper layers' GEMMs.  Persistent: per layer ONE launch for the
// recurrence, then the whole-T dx GEMM (the next layer's dh_up) and the dW GEMMs.
//   xT[l], ld_xT[l]: layer input transposed (layer 0: the frames; l > 0: hT[l-1] + Bp cols)
//   dx[l] [T,B,H] for l > 0 (dh_up of layer l-1); dx[0] may be NULL
//   workspace: sv_lstm_stack_bwd_workspace bytes; side: L streams
//   ev: L*ceil(T/chunk) + L + 1 caller-created events; probe, kstamp (or NULL): Bwd::steps
extern "C" size_t sv_lstm_stack_bwd_workspace(int L, int T, int B, int F, int H) {
  return (size_t)L * ws_per(T, B, F, H) + (H == 768 ? ws_handoff(T, B, H) + gf_sk_bytes() : 0);
}

static int bwd_persist(const Bwd& a) {
  const int L = a.L, T = a.T, B = a.B, H = a.H;
  const bool events = !(a.schedule & SV_SCHED_NO_EVENTS);
  int rc;
  for (int l = L - 1; l >= 0; --l) {
    const BwdWs ws = a.region(l);
    if ((rc = a.prepare(l, ws, l > 0, false, a.main))) return rc;
    // the row-major dG only where a dx GEMM needs it and cannot read the fragment-order hand-off
    // (layer 0 computes no dx here)
    const int abn = l > 0 ? dx_afrag_bn(T, B, H, a.Fl(l)) : 0;
    hipEvent_t* pp = a.layer_probe(l);
    rc = sv_persist_bwd_f32(T, B, H, ws.whhT, a.gates[l], a.c_tm[l], l == L - 1 ? a.dh_last : a.dx[l + 1], l < L - 1,
                            abn < 0 ? a.dgates[l] : nullptr, a.dgT[l], a.handoff(), a.main, a.sync,
                            pp ? pp[0] : nullptr, pp ? pp[1] : nullptr, a.db_ih[l], a.db_hh ? a.db_hh[l] : nullptr);
    // the completion events of layers >= 1 (grad_ready: a caller's bucketed all-reduce) fire once
    // the last recurrence is done, so a collective never shares the device with a persistent
    // launch (a concurrent RCCL kernel would hold CUs its grid waits for) but overlaps layer 0's
    // weight-gradient GEMMs
    for (int k = 1; l == 0 && k < L && events && !rc; ++k) rc = record(a.layer_done(k), a.main);
    if (rc) return rc;
    if (abn > 0)
      rc = gemm_f32_dx_afrag(abn, a.handoff(), T, B, H, ws.wihT, f32_wiht_ld(H), a.Fl(l), a.dx[l], a.main, a.skws());
    else if (abn < 0)
      rc = a.dx_gemm(l, ws, 0, T, a.main);
    // (bias gradients: summed inside the persistent recurrence, finalized after it)
    if (rc || (rc = a.grads(l, ws, false, a.main))) return rc;
  }
  return events ? record(a.layer_done(0), a.main) : SV_OK;
}

extern "C" int sv_lstm_stack_bwd(int L, int T, int B, int F, int H, const float* const* xT, const long* ld_xT,
                                 const float* const* w_ih, const float* const* w_hh, const float* const* gates,
                                 const float* const* c_tm, const float* const* hT, const float* dh_last,
                                 float* const* dgates, float* const* dgT, float* const* dx, float* const* dw_ih,
                                 float* const* dw_hh, float* const* db_ih, float* const* db_hh, float* workspace,
                                 int chunk, hipStream_t main, const hipStream_t* side, hipEvent_t* ev,
                                 int products, hipEvent_t* probe, unsigned long long* kstamp, int schedule,
                                 unsigned* sync) {
  if (L <= 0 || !xT || !ld_xT || !w_ih || !w_hh || !gates || !c_tm || !hT || !dh_last || !dgates || !dgT || !dx ||
      !dw_ih || !dw_hh || !db_ih || !workspace || !side || !ev || chunk <= 0)
    return SV_EARG;
  if (products < 0 || products > 3 || schedule < 0 || schedule > SV_SCHED_MASK) return SV_EARG;
  F32ProductScope scope(products);
  if (!lstm_dims_ok(T, B, F, H)) return SV_ESHAPE;
  const Bwd a{{L, T, B, F, H, chunk, main, side, ev, probe, products, schedule, sync}, xT, ld_xT, w_ih, w_hh,
              gates, c_tm, hT, dh_last, 0, dgates, dgT, dx, dw_ih, dw_hh, db_ih, db_hh, (char*)workspace, kstamp,
              ws_per(T, B, F, H)};
  if (f32_persist(schedule, B, H, main)) return sync ? bwd_persist(a) : SV_EARG;
  return stack_bwd_per_step(a);
}
