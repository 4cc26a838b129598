// Spectral diarization of d-vector sequences (the sv_diar_* entry points of the C ABI): the
// refinement chain of Wang et al., "Speaker Diarization with LSTM" (arXiv 1710.10468), the products
// of a block subspace iteration for the top SV_DIAR_M eigenpairs, and k-means, for a ragged batch
// of F files.  File f owns the rows row_off[f] .. row_off[f + 1] of every [sum n][.] array and an
// n_f x n_f matrix with leading dimension ld_f = (n_f + 3) & ~3 at element mat_off[f] of every packed
// matrix buffer; every kernel that writes a matrix writes zeros into the columns n_f .. ld_f - 1.
// Every launch is a (blocks of the largest file, F) grid whose surplus workgroups leave at once;
// no kernel waits for another workgroup, and every loop bound is n, ld, r, k <= 16 or max_iter.
//   crop + blur   row pass, one workgroup per row staged in LDS (32 KB at n = 8192): the diagonal
//                 takes the largest other element of its row, then C = A' W^T over the in-range taps,
//                 written over A.  Column pass: B = W C, one thread per element, the 2 r + 1 rows
//                 of a column read coalesced along j.  The normalisers c_i are sums of the taps.
//   row select    one workgroup per row: the row's order-preserving keys (sv_snorm.hip's key) in
//                 LDS, an MSD radix select with 8-bit digits -- 4 passes of a 256-bin LDS histogram
//                 and a 256-thread scan -- gives the element of ascending rank q exactly.
//   thresh + sym  32 x 32 tiles; the mirrored tile goes through LDS so that both reads are
//                 coalesced: Y_ij = fmaxf(T_ij, T_ji), T_ij = B_ij >= tau_i ? B_ij : mult * B_ij.
//   row norm      one wave per row for d_i = max_j Z_ij and r_i = 1 / sqrt(d_i) in fp64; then one
//                 thread per element, S_ij = Z_ij (r_i r_j) with the product in fp64, rounded once.
//   spmm          P = S (W T): a workgroup of four waves owns 32 rows of S, two groups of 16 rows
//                 times two halves of every 64-wide k chunk.  The chunk of Q = W T (fp64 products,
//                 rounded to fp32) is built in LDS by all 256 threads; a lane loads two float4 of
//                 its row of S (32 consecutive floats per row and wave: whole 128-byte lines) and
//                 feeds 8 v_mfma_f32_16x16x4_f32 into two accumulators.  The two k halves meet in
//                 LDS in a fixed order.  S is read once.
//   gram          G = X^T Y in fp64: 256-row blocks staged in LDS, one thread per (i, j), the
//                 blocks' partial sums in a workspace, summed per file in block order by a second
//                 kernel (the same kernel sums rmul's residual partials).
//   rmul          Y = X T (fp64 products, rounded once); with P and lam also the squared column
//                 norms of P T - Y diag(lam), per 64-row block and then per file in block order.
//   kmeans        one workgroup per file, the k <= 16 centres in LDS, farthest-first start and the
//                 whole Lloyd loop inside the launch; the centre sums are fp64 over the rows in
//                 ascending order, staged through LDS in chunks of 256 rows.
#include "sv_common.h"
#include "../../include/sv_ge2e.h"

#include <algorithm>

namespace {

constexpr int DM = SV_DIAR_M;
constexpr int DN_MAX = SV_DIAR_MAX_N;
constexpr int DR_MAX = SV_DIAR_MAX_R;
constexpr int D_MAX_F = 65535;  // grid.y
static_assert(DM == 16, "the MFMA tile and the thread maps below are written for 16 columns");

struct Tables {
  const int* row_off;
  const long* mat_off;
};

struct File {
  int r0, n, ld;
};

__device__ __forceinline__ File file_of(const int* __restrict__ row_off, int f) {
  const int r0 = row_off[f], n = row_off[f + 1] - r0;
  return {r0, n, (n + 3) & ~3};
}

__device__ __forceinline__ unsigned diar_key(float s) {
  const unsigned u = __float_as_uint(s);
  return s != s ? 0xffffffffu : (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float diar_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? k & 0x7fffffffu : ~k);
}

// ------------------------------------------------------------------ crop + blur
struct Taps {
  float g[DR_MAX + 1];
  int r;
};

// sum of the taps that fall inside [0, n) around position i, in the order of the blur's own sum
__device__ __forceinline__ float tap_norm(const Taps& t, int i, int n) {
  float c = 0.0f;
  for (int d = -t.r; d <= t.r; ++d)
    if (i + d >= 0 && i + d < n) c += t.g[d < 0 ? -d : d];
  return c;
}

__global__ __launch_bounds__(256) void diar_crop_rowblur_kernel(float* __restrict__ A, Tables tb, Taps t) {
  __shared__ float row[DN_MAX];
  __shared__ float wmax[4];
  const File fl = file_of(tb.row_off, blockIdx.y);
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i >= fl.n || fl.n > DN_MAX) return;
  float* a = A + tb.mat_off[blockIdx.y] + (long)i * fl.ld;
  float m = -INFINITY;
  for (int j = tid; j < fl.n; j += 256) {
    const float v = a[j];
    row[j] = v;
    if (j != i) m = fmaxf(m, v);
  }
  m = wave_max(m);
  if ((tid & 63) == 0) wmax[tid >> 6] = m;
  __syncthreads();
  if (tid == 0 && fl.n > 1) row[i] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  __syncthreads();
  for (int j = tid; j < fl.ld; j += 256) {
    float acc = 0.0f;
    if (j < fl.n) {
      for (int d = -t.r; d <= t.r; ++d)
        if (j + d >= 0 && j + d < fl.n) acc += t.g[d < 0 ? -d : d] * row[j + d];
      acc /= tap_norm(t, j, fl.n);
    }
    a[j] = acc;
  }
}

__global__ __launch_bounds__(256) void diar_colblur_kernel(const float* __restrict__ C, float* __restrict__ B, Tables tb,
                                                           Taps t) {
  const File fl = file_of(tb.row_off, blockIdx.z);
  const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (i >= fl.n || j >= fl.ld) return;
  const long base = tb.mat_off[blockIdx.z];
  float acc = 0.0f;
  for (int d = -t.r; d <= t.r; ++d)
    if (i + d >= 0 && i + d < fl.n) acc += t.g[d < 0 ? -d : d] * C[base + (long)(i + d) * fl.ld + j];
  B[base + (long)i * fl.ld + j] = j < fl.n ? acc / tap_norm(t, i, fl.n) : 0.0f;
}

// ------------------------------------------------------------------ row select
__global__ __launch_bounds__(256) void diar_row_select_kernel(const float* __restrict__ B, Tables tb,
                                                              const int* __restrict__ q, float* __restrict__ tau) {
  __shared__ unsigned keys[DN_MAX];
  __shared__ unsigned hist[256], scan[256];
  __shared__ unsigned prefix_s, want_s;
  const File fl = file_of(tb.row_off, blockIdx.y);
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i >= fl.n || fl.n > DN_MAX) return;
  const float* b = B + tb.mat_off[blockIdx.y] + (long)i * fl.ld;
  for (int j = tid; j < fl.n; j += 256) keys[j] = diar_key(b[j]);
  if (tid == 0) {
    prefix_s = 0;
    want_s = (unsigned)min(max(q[blockIdx.y], 0), fl.n - 1);
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned fixed = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    hist[tid] = 0;
    __syncthreads();  // the keys, the zeroed bins, the last pass's prefix and want
    const unsigned pre = prefix_s, want = want_s;
    for (int j = tid; j < fl.n; j += 256) {
      const unsigned k = keys[j];
      if (((k ^ pre) & fixed) == 0) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    const unsigned c = hist[tid];
    scan[tid] = c;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // inclusive scan over the bins, ascending
      const unsigned v = tid >= off ? scan[tid - off] : 0u;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const unsigned incl = scan[tid], excl = incl - c;
    // the matching keys are more than `want` (n > q at the start, afterwards the chosen bin's count),
    // so exactly one bin holds the rank
    if (excl <= want && want < incl) {
      prefix_s = pre | ((unsigned)tid << shift);
      want_s = want - excl;
    }
    __syncthreads();
  }
  if (tid == 0) tau[fl.r0 + i] = diar_unkey(prefix_s);
}

// ------------------------------------------------------------------ threshold + symmetrise
__global__ __launch_bounds__(256) void diar_thresh_sym_kernel(const float* __restrict__ B, const float* __restrict__ tau,
                                                              float mult, float* __restrict__ Y, Tables tb) {
  __shared__ float tile[32][33];
  const File fl = file_of(tb.row_off, blockIdx.z);
  const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
  if (i0 >= fl.n || j0 >= fl.ld) return;
  const long base = tb.mat_off[blockIdx.z];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  // the mirrored tile: rows j0 .. j0 + 31, columns i0 .. i0 + 31, thresholded by its own rows' tau
  for (int y = ty; y < 32; y += 8) {
    const int r = j0 + y, c = i0 + tx;
    float v = 0.0f;
    if (r < fl.n && c < fl.n) {
      const float b = B[base + (long)r * fl.ld + c];
      v = b >= tau[fl.r0 + r] ? b : __fmul_rn(mult, b);
    }
    tile[y][tx] = v;
  }
  __syncthreads();
  for (int y = ty; y < 32; y += 8) {
    const int r = i0 + y, c = j0 + tx;
    if (r < fl.n && c < fl.ld) {
      float v = 0.0f;
      if (c < fl.n) {
        const float b = B[base + (long)r * fl.ld + c];
        v = fmaxf(b >= tau[fl.r0 + r] ? b : __fmul_rn(mult, b), tile[tx][y]);
      }
      Y[base + (long)r * fl.ld + c] = v;
    }
  }
}

// ------------------------------------------------------------------ row-max normalisation
__global__ __launch_bounds__(256) void diar_rowmax_kernel(const float* __restrict__ Z, Tables tb, float* __restrict__ d,
                                                          double* __restrict__ rs) {
  const File fl = file_of(tb.row_off, blockIdx.y);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= fl.n) return;
  const float* z = Z + tb.mat_off[blockIdx.y] + (long)i * fl.ld;
  float m = -INFINITY;
  for (int j = lane; j < fl.n; j += 64) m = fmaxf(m, z[j]);
  m = wave_max(m);
  if (lane == 0) {
    d[fl.r0 + i] = m;
    rs[fl.r0 + i] = m > 0.0f ? 1.0 / sqrt((double)m) : 0.0;
  }
}

__global__ __launch_bounds__(256) void diar_rownorm_kernel(const float* __restrict__ Z, const double* __restrict__ rs,
                                                           float* __restrict__ S, Tables tb) {
  const File fl = file_of(tb.row_off, blockIdx.z);
  const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (i >= fl.n || j >= fl.ld) return;
  const long at = tb.mat_off[blockIdx.z] + (long)i * fl.ld + j;
  S[at] = j < fl.n ? (float)((double)Z[at] * (rs[fl.r0 + i] * rs[fl.r0 + j])) : 0.0f;
}

// ------------------------------------------------------------------ P = S (W T)
constexpr int SP_BM = 32, SP_KC = 64;

__global__ __launch_bounds__(256) void diar_spmm_kernel(const float* __restrict__ S, const float* __restrict__ W,
                                                        const double* __restrict__ T, float* __restrict__ P, Tables tb) {
  __shared__ double Ts[DM * DM];
  __shared__ float Qs[SP_KC * DM];   // row of k = kh * 32 + g * 8 + m at ((kh * 8 + m) * 4 + g) * 16
  __shared__ float red[2 * 64 * 4];  // the upper k half's accumulators
  const File fl = file_of(tb.row_off, blockIdx.y);
  const int i0 = blockIdx.x * SP_BM;
  if (i0 >= fl.n) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rg = wave & 1, kh = wave >> 1, g = lane >> 4, col = lane & 15;
  Ts[tid] = T[(long)blockIdx.y * DM * DM + tid];
  const float* w = W + (long)fl.r0 * DM;
  const float* srow = S + tb.mat_off[blockIdx.y] + (long)min(i0 + rg * 16 + col, fl.n - 1) * fl.ld;
  // this thread's entries of the Q chunk: row kq, columns c4 .. c4 + 3
  const int kq = tid >> 2, c4 = (tid & 3) * 4;
  const int qpos = (((kq >> 5) * 8 + (kq & 7)) * 4 + ((kq >> 3) & 3)) * DM + c4;
  f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = acc0;
  for (int k0 = 0; k0 < fl.ld; k0 += SP_KC) {
    __syncthreads();  // Ts; the last chunk's reads of Qs
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    if (k0 + kq < fl.n) {
      const f32x4* wr = reinterpret_cast<const f32x4*>(w + (long)(k0 + kq) * DM);
#pragma unroll
      for (int m4 = 0; m4 < 4; ++m4) {
        const f32x4 wv = wr[m4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int c = 0; c < 4; ++c) q[c] = fma((double)wv[e], Ts[(m4 * 4 + e) * DM + c4 + c], q[c]);
      }
    }
    *reinterpret_cast<f32x4*>(Qs + qpos) = f32x4{(float)q[0], (float)q[1], (float)q[2], (float)q[3]};
    __syncthreads();
    const int kb = k0 + kh * 32 + g * 8;  // a multiple of 4, as ld is: a float4 is inside the row or past it
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    const f32x4 s0 = kb + 4 <= fl.ld ? *reinterpret_cast<const f32x4*>(srow + kb) : zero;
    const f32x4 s1 = kb + 8 <= fl.ld ? *reinterpret_cast<const f32x4*>(srow + kb + 4) : zero;
    const float* qs = Qs + (kh * 8 * 4 + g) * DM + col;
#pragma unroll
    for (int m = 0; m < 4; m += 2) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(s0[m], qs[m * 4 * DM], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(s0[m + 1], qs[(m + 1) * 4 * DM], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int m = 0; m < 4; m += 2) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(s1[m], qs[(m + 4) * 4 * DM], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(s1[m + 1], qs[(m + 5) * 4 * DM], acc1, 0, 0, 0);
    }
  }
  f32x4 acc = acc0 + acc1;
  if (kh == 1) *reinterpret_cast<f32x4*>(red + (rg * 64 + lane) * 4) = acc;
  __syncthreads();
  if (kh == 0) {
    acc += *reinterpret_cast<const f32x4*>(red + (rg * 64 + lane) * 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // C/D of the 16 x 16 tile: column lane & 15, row 4 (lane >> 4) + r
      const int row = i0 + rg * 16 + 4 * g + r;
      if (row < fl.n) P[(long)(fl.r0 + row) * DM + col] = acc[r];
    }
  }
}

// ------------------------------------------------------------------ G = X^T Y, fp64
constexpr int GR_ROWS = 256;

__global__ __launch_bounds__(256) void diar_gram_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                        double* __restrict__ ws, const int* __restrict__ row_off,
                                                        int nb_max) {
  __shared__ float Xs[GR_ROWS * DM], Ys[GR_ROWS * DM];
  const File fl = file_of(row_off, blockIdx.y);
  const int b0 = blockIdx.x * GR_ROWS, tid = threadIdx.x;
  if (b0 >= fl.n) return;
  const int m = min(GR_ROWS, fl.n - b0);
  const long at = (long)(fl.r0 + b0) * DM;
  for (int e = tid; e < m * DM; e += 256) {
    Xs[e] = X[at + e];
    Ys[e] = Y[at + e];
  }
  __syncthreads();
  const int i = tid >> 4, j = tid & 15;
  double s = 0.0;
  for (int r = 0; r < m; ++r) s = fma((double)Xs[r * DM + i], (double)Ys[r * DM + j], s);
  ws[((long)blockIdx.y * nb_max + blockIdx.x) * (DM * DM) + tid] = s;
}

// out[f][t] = the sum over the file's blocks of `rows` rows, in order, of ws[f][block][t]; blockDim = width
__global__ void diar_block_sum_kernel(const double* __restrict__ ws, double* __restrict__ out,
                                      const int* __restrict__ row_off, int nb_max, int rows) {
  const File fl = file_of(row_off, blockIdx.x);
  const int width = blockDim.x, nb = min((fl.n + rows - 1) / rows, nb_max);
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += ws[((long)blockIdx.x * nb_max + b) * width + threadIdx.x];
  out[(long)blockIdx.x * width + threadIdx.x] = s;
}

// ------------------------------------------------------------------ Y = X T (+ residual norms)
constexpr int RM_ROWS = 64;

__global__ __launch_bounds__(256) void diar_rmul_kernel(const float* __restrict__ X, const double* __restrict__ T,
                                                        float* __restrict__ Y, const float* __restrict__ P,
                                                        const double* __restrict__ lam, double* __restrict__ ws,
                                                        const int* __restrict__ row_off, int nb_max) {
  __shared__ double Ts[DM * DM];
  __shared__ double sq[RM_ROWS * DM];
  const File fl = file_of(row_off, blockIdx.y);
  const int b0 = blockIdx.x * RM_ROWS, tid = threadIdx.x;
  if (b0 >= fl.n) return;
  Ts[tid] = T[(long)blockIdx.y * DM * DM + tid];
  __syncthreads();
  const int rl = tid >> 2, row = b0 + rl, c4 = (tid & 3) * 4;
  double e2[4] = {0.0, 0.0, 0.0, 0.0};
  if (row < fl.n) {
    const long at = (long)(fl.r0 + row) * DM;
    double y[4] = {0.0, 0.0, 0.0, 0.0}, pv[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m = 0; m < DM; ++m) {
      const double x = (double)X[at + m];
#pragma unroll
      for (int c = 0; c < 4; ++c) y[c] = fma(x, Ts[m * DM + c4 + c], y[c]);
    }
    const f32x4 yf = {(float)y[0], (float)y[1], (float)y[2], (float)y[3]};
    *reinterpret_cast<f32x4*>(Y + at + c4) = yf;
    if (P) {
      for (int m = 0; m < DM; ++m) {
        const double p = (double)P[at + m];
#pragma unroll
        for (int c = 0; c < 4; ++c) pv[c] = fma(p, Ts[m * DM + c4 + c], pv[c]);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double e = pv[c] - lam[(long)blockIdx.y * DM + c4 + c] * (double)yf[c];
        e2[c] = e * e;
      }
    }
  }
  if (!P) return;  // (uniform)
#pragma unroll
  for (int c = 0; c < 4; ++c) sq[rl * DM + c4 + c] = e2[c];
  __syncthreads();
  if (tid < DM) {
    double s = 0.0;
    for (int r = 0; r < RM_ROWS; ++r) s += sq[r * DM + tid];
    ws[((long)blockIdx.y * nb_max + blockIdx.x) * DM + tid] = s;
  }
}

// ------------------------------------------------------------------ k-means
__device__ __forceinline__ float dist2(const float* __restrict__ e, const float* c) {
  float s = 0.0f;
#pragma unroll
  for (int d = 0; d < DM; ++d) {
    const float t = e[d] - c[d];
    s += t * t;
  }
  return s;
}

__global__ __launch_bounds__(256) void diar_kmeans_kernel(const float* __restrict__ E, const int* __restrict__ row_off,
                                                          const int* __restrict__ ks, int max_iter,
                                                          int* __restrict__ labels, int* __restrict__ iters) {
  __shared__ float C[DM * DM];
  __shared__ float Es[256 * DM];
  __shared__ int ls[256];
  __shared__ float bval[256];
  __shared__ int bidx[256];
  __shared__ int flag;
  const File fl = file_of(row_off, blockIdx.x);
  const int tid = threadIdx.x, n = fl.n;
  if (n < 1) {
    if (tid == 0) iters[blockIdx.x] = 0;
    return;
  }
  const int k = min(min(max(ks[blockIdx.x], 1), DM), n);
  const float* e = E + (long)fl.r0 * DM;
  int* lab = labels + fl.r0;
  if (tid < DM) C[tid] = e[tid];
  for (int c = 1; c < k; ++c) {  // farthest-first: the row farthest from the centres chosen so far
    __syncthreads();
    float best = -1.0f;
    int bi = 0x7fffffff;
    for (int r = tid; r < n; r += 256) {
      float md = INFINITY;
      for (int cc = 0; cc < c; ++cc) md = fminf(md, dist2(e + (long)r * DM, C + cc * DM));
      if (md > best) {
        best = md;
        bi = r;
      }
    }
    bval[tid] = best;
    bidx[tid] = bi;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
      if (tid < s) {
        const float v = bval[tid + s];
        const int ix = bidx[tid + s];
        if (v > bval[tid] || (v == bval[tid] && ix < bidx[tid])) {
          bval[tid] = v;
          bidx[tid] = ix;
        }
      }
      __syncthreads();
    }
    const int pick = min(max(bidx[0], 0), n - 1);
    if (tid < DM) C[c * DM + tid] = e[(long)pick * DM + tid];
  }
  for (int r = tid; r < n; r += 256) lab[r] = -1;
  int it = 0;
  while (it < max_iter) {
    __syncthreads();  // the centres; the last pass's read of flag
    if (tid == 0) flag = 0;
    __syncthreads();
    bool changed = false;
    for (int r = tid; r < n; r += 256) {
      float best = INFINITY;
      int bc = 0;
      for (int c = 0; c < k; ++c) {
        const float dd = dist2(e + (long)r * DM, C + c * DM);
        if (dd < best) {
          best = dd;
          bc = c;
        }
      }
      if (bc != lab[r]) {
        lab[r] = bc;
        changed = true;
      }
    }
    if (changed) flag = 1;
    __syncthreads();
    ++it;
    if (!flag) break;  // (uniform: read after the barrier, rewritten only after the next one)
    // centre c, coordinate d: the fp64 sum over the rows of label c in ascending order
    const int c = tid >> 4, d = tid & 15;
    double sum = 0.0;
    int cnt = 0;
    for (int ch = 0; ch < n; ch += 256) {
      __syncthreads();  // the last chunk's reads
      const int m = min(256, n - ch);
      if (tid < m) {
        const f32x4* src = reinterpret_cast<const f32x4*>(e + (long)(ch + tid) * DM);
#pragma unroll
        for (int v = 0; v < 4; ++v) *reinterpret_cast<f32x4*>(Es + tid * DM + v * 4) = src[v];
        ls[tid] = lab[ch + tid];  // written by this same thread
      }
      __syncthreads();
      for (int r = 0; r < m; ++r)
        if (ls[r] == c) {
          sum += (double)Es[r * DM + d];
          ++cnt;
        }
    }
    if (c < k && cnt > 0) C[c * DM + d] = (float)(sum / (double)cnt);  // an empty cluster keeps its centre
  }
  if (tid == 0) iters[blockIdx.x] = it;
}

inline bool off16(const void* p) { return ((uintptr_t)p & 15) != 0; }
inline bool off8(const void* p) { return ((uintptr_t)p & 7) != 0; }
inline bool off4(const void* p) { return ((uintptr_t)p & 3) != 0; }

// the checks every entry point shares, in the header's order; 0 = go on
inline int check_batch(bool null, int F, int n_max, bool misaligned) {
  if (null || F < 1 || n_max < 1) return SV_EARG;
  if (misaligned) return SV_EALIGN;
  if (F > D_MAX_F || n_max > DN_MAX) return SV_ESHAPE;
  return SV_OK;
}

}  // namespace

extern "C" int sv_diar_crop_blur(float* A, float* B, const int* row_off, const long* mat_off, int F, int n_max,
                                 const float* taps, int r, hipStream_t stream) {
  if (r < 0) return SV_EARG;
  if (int rc = check_batch(!A || !B || !row_off || !mat_off || !taps || A == B, F, n_max,
                           off16(A) || off16(B) || off4(row_off) || off8(mat_off)))
    return rc;
  if (r > DR_MAX) return SV_ESHAPE;
  Taps t{};
  t.r = r;
  for (int d = 0; d <= r; ++d) t.g[d] = taps[d];
  const Tables tb{row_off, mat_off};
  const int ld_max = (n_max + 3) & ~3;
  hipLaunchKernelGGL(diar_crop_rowblur_kernel, dim3(n_max, F), dim3(256), 0, stream, A, tb, t);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(diar_colblur_kernel, dim3((ld_max + 255) / 256, n_max, F), dim3(256), 0, stream, A, B, tb, t);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_diar_row_select(const float* B, const int* row_off, const long* mat_off, int F, int n_max,
                                  const int* q, float* tau, hipStream_t stream) {
  if (int rc = check_batch(!B || !row_off || !mat_off || !q || !tau, F, n_max,
                           off16(B) || off4(row_off) || off8(mat_off) || off4(q) || off4(tau)))
    return rc;
  hipLaunchKernelGGL(diar_row_select_kernel, dim3(n_max, F), dim3(256), 0, stream, B, Tables{row_off, mat_off}, q, tau);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_diar_thresh_sym(const float* B, const float* tau, float mult, float* Y, const int* row_off,
                                  const long* mat_off, int F, int n_max, hipStream_t stream) {
  if (int rc = check_batch(!B || !tau || !Y || !row_off || !mat_off || B == Y, F, n_max,
                           off16(B) || off16(Y) || off4(tau) || off4(row_off) || off8(mat_off)))
    return rc;
  const int tiles = (((n_max + 3) & ~3) + 31) / 32;
  hipLaunchKernelGGL(diar_thresh_sym_kernel, dim3(tiles, tiles, F), dim3(256), 0, stream, B, tau, mult, Y,
                     Tables{row_off, mat_off});
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_diar_row_norm(const float* Z, float* S, float* d, double* r, const int* row_off, const long* mat_off,
                                int F, int n_max, hipStream_t stream) {
  if (int rc = check_batch(!Z || !S || !d || !r || !row_off || !mat_off, F, n_max,
                           off16(Z) || off16(S) || off4(d) || off8(r) || off4(row_off) || off8(mat_off)))
    return rc;
  const Tables tb{row_off, mat_off};
  hipLaunchKernelGGL(diar_rowmax_kernel, dim3((n_max + 3) / 4, F), dim3(256), 0, stream, Z, tb, d, r);
  SV_LAUNCH_CHECK();
  const int ld_max = (n_max + 3) & ~3;
  hipLaunchKernelGGL(diar_rownorm_kernel, dim3((ld_max + 255) / 256, n_max, F), dim3(256), 0, stream, Z, r, S, tb);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_diar_spmm(const float* S, const float* W, const double* T, float* P, const int* row_off,
                            const long* mat_off, int F, int n_max, hipStream_t stream) {
  if (int rc = check_batch(!S || !W || !T || !P || !row_off || !mat_off || W == P, F, n_max,
                           off16(S) || off16(W) || off8(T) || off16(P) || off4(row_off) || off8(mat_off)))
    return rc;
  hipLaunchKernelGGL(diar_spmm_kernel, dim3((n_max + SP_BM - 1) / SP_BM, F), dim3(256), 0, stream, S, W, T, P,
                     Tables{row_off, mat_off});
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" size_t sv_diar_workspace(int F, int n_max) {
  if (F < 1 || n_max < 1 || F > D_MAX_F || n_max > DN_MAX) return 0;
  const size_t gram = (size_t)((n_max + GR_ROWS - 1) / GR_ROWS) * DM * DM;
  const size_t rmul = (size_t)((n_max + RM_ROWS - 1) / RM_ROWS) * DM;
  return (size_t)F * std::max(gram, rmul) * sizeof(double);
}

extern "C" int sv_diar_gram(const float* X, const float* Y, double* G, double* workspace, const int* row_off, int F,
                            int n_max, hipStream_t stream) {
  if (int rc = check_batch(!X || !Y || !G || !workspace || !row_off, F, n_max,
                           off4(X) || off4(Y) || off8(G) || off8(workspace) || off4(row_off)))
    return rc;
  const int nb_max = (n_max + GR_ROWS - 1) / GR_ROWS;
  hipLaunchKernelGGL(diar_gram_kernel, dim3(nb_max, F), dim3(256), 0, stream, X, Y, workspace, row_off, nb_max);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(diar_block_sum_kernel, dim3(F), dim3(DM * DM), 0, stream, workspace, G, row_off, nb_max, GR_ROWS);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_diar_rmul(const float* X, const double* T, float* Y, const float* P, const double* lam, double* res2,
                            double* workspace, const int* row_off, int F, int n_max, hipStream_t stream) {
  const bool res = P != nullptr;
  if (int rc = check_batch(!X || !T || !Y || !row_off || X == Y || (res && (!lam || !res2 || !workspace || P == Y)), F,
                           n_max, off16(X) || off8(T) || off16(Y) || off4(P) || off8(lam) || off8(res2) ||
                                      off8(workspace) || off4(row_off)))
    return rc;
  const int nb_max = (n_max + RM_ROWS - 1) / RM_ROWS;
  hipLaunchKernelGGL(diar_rmul_kernel, dim3(nb_max, F), dim3(256), 0, stream, X, T, Y, P, lam, workspace, row_off,
                     nb_max);
  SV_LAUNCH_CHECK();
  if (res) {
    hipLaunchKernelGGL(diar_block_sum_kernel, dim3(F), dim3(DM), 0, stream, workspace, res2, row_off, nb_max, RM_ROWS);
    SV_LAUNCH_CHECK();
  }
  return SV_OK;
}

extern "C" int sv_diar_kmeans(const float* E, const int* row_off, const int* k, int F, int max_iter, int* labels,
                              int* iters, hipStream_t stream) {
  if (!E || !row_off || !k || !labels || !iters || F < 1 || max_iter < 1) return SV_EARG;
  if (off16(E) || off4(row_off) || off4(k) || off4(labels) || off4(iters)) return SV_EALIGN;
  if (F > D_MAX_F) return SV_ESHAPE;
  hipLaunchKernelGGL(diar_kmeans_kernel, dim3(F), dim3(256), 0, stream, E, row_off, k, max_iter, labels, iters);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
