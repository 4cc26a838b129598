// Log-mel front end (sv_logmel of the C ABI): a ragged batch of waveform segments to log-mel
// frames [n_frames][nmels] in one launch.
//   kernel   logmel_kernel: a workgroup (4 waves) takes 64 consecutive frames of the batch (they may
//            belong to several segments; every frame row carries its own segment's bounds, so a row
//            never reads a neighbouring segment) and computes
//              S^T [bin][frame] = wbasis^T [bin][tap] x frames^T [tap][frame]
//            on v_mfma_f32_32x32x2_f32 (exact fp32 products, a tap-ordered fmaf chain per element).
//            Both operands are staged in LDS LM_KC taps at a time, double-buffered, the next chunk's
//            global loads in flight during the current chunk's MFMAs: the A operand is LM_KC rows of
//            wbasis (L2-resident; a lane's cos and sin of one bin are one 8-byte LDS read), the B
//            operand the frames, reflect-indexed from the waveform.  The transposed orientation
//            leaves the accumulators [bin][frame] with the frame on the lane, so the power spectrum
//            P = re^2 + im^2 is the B operand of the mel product
//              out^T [mel][frame] = melfb [mel][bin] x P [bin][frame]
//            as it stands: no LDS round trip and no spectrum in memory.  log10(. + 1e-6) and a
//            transpose through LDS finish the tile's [64][nmels] rows, which are contiguous in out.
//   bins     the DC bin's sine column is identically zero, so its slot carries the Nyquist bin's
//            cosine column: nfft / 2 bin pairs instead of nfft / 2 + 1 (256 at nfft = 512: 8 whole
//            tiles of 32, all held in one pass of accumulators; nfft = 1024 takes two passes)
//   order    every output element's sums run in a fixed order that does not depend on the frame's
//            row in its tile, so a segment's frames are bit-identical alone or in a batch
// Magnitude / dB mode (sv_meldb of the C ABI, the same kernel's second instantiation): a segment is
// a virtual signal (seg_start, seg_valid, seg_len) -- seg_valid samples of y from seg_start, then
// zeros up to seg_len, reflected against seg_len -- so trim, zero padding and truncation are index
// arithmetic on the one uploaded buffer.  The spectrum's magnitude sqrt(re^2 + im^2) takes the
// power's place as the mel product's operand; the epilogue writes 20 log10(max(x, amin)) and folds
// the raw mel sums x of every valid frame row into seg_max[its segment] by an unsigned integer
// atomic max on the float's bits (x >= 0: exact, and independent of the order of arrival).
// meldb_clip_kernel then lifts every element to its own segment's maximum - top_db.
// Range mode (sv_logmel_ranges of the C ABI, the third instantiation): the power epilogue on
// segments given as (seg_start, seg_len) ranges of the one uploaded buffer -- they may touch, overlap
// or leave gaps, so the voiced ranges of many files are framed without re-packing the audio.  A
// frame row's origin, length and tap 0 are the only things read from the tables, so a range's frames
// are bit-identical to sv_logmel's of a packed copy of it.
#include "sv_common.h"
#include "../../include/sv_ge2e.h"

namespace {

constexpr int LM_BM = 64;                   // frames per workgroup
constexpr int LM_KC = 8;                    // taps per staged chunk (16 measured the same)
constexpr int LM_FT = LM_BM * LM_KC / 256;  // frames a thread stages per chunk
constexpr int LM_FS = 256 / LM_KC;          // their spacing
constexpr int LM_FLD = LM_BM + 1;           // row stride of a staged frame chunk [tap][frame]
constexpr int LM_PASS = 256;                // bins per pass: 2 wave groups x 4 tiles of 32
constexpr int LM_BLD = 2 * LM_PASS;         // row stride of a staged basis chunk [tap][cos, sin of 256 bins]
constexpr int LM_BT = LM_KC * LM_BLD / 4 / 256;  // 16-byte pieces of it a thread stages per chunk
constexpr int LM_MT = 4;                    // at most 4 mel tiles of 32 rows (nmels <= 128)

constexpr int LM_POWER = 0;  // |.|^2, log10(. + 1e-6); segments from seg_off (sv_logmel)
constexpr int LM_MAGDB = 1;  // |.|, 20 log10(max(., amin)), per-segment maximum; virtual segments (sv_meldb)
constexpr int LM_RANGES = 2;  // LM_POWER's epilogue; segments from seg_start and seg_len (sv_logmel_ranges)

// NMT: mel tiles of 32 rows, (nmels + 31) / 32
// MODE: LM_POWER (seg_off [n_seg + 1]; seg_valid, seg_len, amin, seg_max unused), LM_MAGDB
//       (seg_off is seg_start [n_seg]) or LM_RANGES (seg_off is seg_start [n_seg], seg_len [n_seg];
//       seg_valid, amin, seg_max unused)
template <int NMT, int MODE>
__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ y, const int* __restrict__ seg_off,
                                                     const int* __restrict__ frame_off, int n_seg, int n_frames,
                                                     int nfft, int win, int hop, int nmels,
                                                     const float* __restrict__ wb, int ldw,
                                                     const float* __restrict__ melfb, float* __restrict__ out,
                                                     const int* __restrict__ seg_valid,
                                                     const int* __restrict__ seg_len, float amin,
                                                     unsigned* __restrict__ seg_max) {
  constexpr bool MAG = MODE == LM_MAGDB;
  __shared__ __attribute__((aligned(16))) float Bs[2 * LM_KC * LM_BLD];  // basis chunks; after the last chunk `red`
  __shared__ float Fs[2 * LM_KC * LM_FLD];                               // frame chunks
  // per frame row: its segment's sample offset and length, its tap 0's sample index; MAG: also the
  // segment's count of real samples and its index
  __shared__ int rows[(MAG ? 5 : 3) * LM_BM];
  float* red = Bs;                 // cross-wave mel sums [2][NMT][16][64], then the output tile [64][nmels]
  static_assert(2 * LM_MT * 16 * 64 <= 2 * LM_KC * LM_BLD, "red fits in Bs");
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const int fh = w & 1, bg = w >> 1;  // the wave's frame half and bin group (4 tiles of 32 bins)
  const int g0 = blockIdx.x * LM_BM;
  const int nh = nfft / 2, nb = nh + 1, lpad = (nfft - win) / 2;

  // segment s under the MODE: its origin in y, its length and (MAG) its count of real samples
  auto segment = [&](int s, int& y0, int& n, int& nv) {
    y0 = seg_off[s];
    n = MODE == LM_POWER ? seg_off[s + 1] - y0 : seg_len[s];
    if constexpr (MAG) nv = seg_valid[s];
  };
  if (tid < LM_BM) {
    const int g = g0 + tid;
    int y0 = 0, n = 1, base = 0;  // rows past n_frames read y[0]; their columns are never stored
    int nv = 0, sg = 0;
    if (g < n_frames) {
      sg = seg_of_frame(frame_off, n_seg, g);
      segment(sg, y0, n, nv);
      base = (g - frame_off[sg]) * hop + lpad - nh;  // sample index of tap 0 before reflection
    }
    rows[tid] = y0;
    rows[LM_BM + tid] = n;
    rows[2 * LM_BM + tid] = base;
    if constexpr (MAG) {
      rows[3 * LM_BM + tid] = nv;
      rows[4 * LM_BM + tid] = sg;
    }
  }
  __syncthreads();

  // Staging is branch-free: every load is clamped into its segment / table and what lies outside
  // (a tap past the window, a column past the bins) is zeroed by a select -- at the LDS store, after
  // the chunk's MFMAs, so that nothing waits for the loads before them.
  // frames: thread -> tap tid % LM_KC of frames tid / LM_KC + LM_FS i
  const int tap_l = tid & (LM_KC - 1);
  int ry0[LM_FT], rn[LM_FT], rbase[LM_FT], rv[MAG ? LM_FT : 1];
#pragma unroll
  for (int i = 0; i < LM_FT; ++i) {
    const int f = tid / LM_KC + LM_FS * i;
    ry0[i] = rows[f];
    rn[i] = rows[LM_BM + f];
    rbase[i] = rows[2 * LM_BM + f];
    if constexpr (MAG) rv[i] = rows[3 * LM_BM + f];
  }
  // MAG: bit i of fz says that sample i of the chunk lies in the segment's zero padding (the load
  // is clamped into its real samples, [0, max(valid, 1) - 1]; stage zeroes the value)
  auto gather = [&](int c, float (&fv)[LM_FT], unsigned& fz) {
    const int tap = c * LM_KC + tap_l;
    if constexpr (MAG) fz = 0u;
#pragma unroll
    for (int i = 0; i < LM_FT; ++i) {
      int idx = reflect_clamp(rbase[i] + tap, rn[i]);
      if constexpr (MAG) {
        fz |= idx >= rv[i] ? 1u << i : 0u;
        idx = min(idx, max(rv[i], 1) - 1);
      }
      fv[i] = y[(long)ry0[i] + idx];
    }
  };
  auto stage = [&](int c, const float (&fv)[LM_FT], unsigned fz) {
    const bool on = c * LM_KC + tap_l < win;
#pragma unroll
    for (int i = 0; i < LM_FT; ++i) {
      bool keep = on;
      if constexpr (MAG) keep = on && !(fz >> i & 1u);
      Fs[((c & 1) * LM_KC + tap_l) * LM_FLD + tid / LM_KC + LM_FS * i] = keep ? fv[i] : 0.f;
    }
  };
  // basis: thread -> 16-byte piece tid % 128 of rows tid / 128 + 2 i of the pass's 512 columns
  const int bcol = 4 * (tid & 127), brow = tid >> 7;
  // (bn: Nyquist's cosine, for DC's sine slot in column 1)
  auto load_basis = [&](int c, int pass, f32x4 (&bv)[LM_BT], float (&bn)[LM_BT]) {
    const int col = pass * LM_BLD + bcol;
#pragma unroll
    for (int i = 0; i < LM_BT; ++i) {
      const int tap = c * LM_KC + brow + 2 * i;
      const unsigned roff = (unsigned)min(tap, win - 1) * (unsigned)ldw;
      bv[i] = *reinterpret_cast<const f32x4*>(wb + (roff + (unsigned)min(col, ldw - 4)));
      bn[i] = wb[roff + (unsigned)nfft];
    }
  };
  auto stage_basis = [&](int c, int pass, const f32x4 (&bv)[LM_BT], const float (&bn)[LM_BT]) {
    const int col = pass * LM_BLD + bcol;
#pragma unroll
    for (int i = 0; i < LM_BT; ++i) {
      const bool on = c * LM_KC + brow + 2 * i < win && col < nfft;
      f32x4 v = bv[i];
      v[1] = col == 0 ? bn[i] : v[1];
      *reinterpret_cast<f32x4*>(&Bs[((c & 1) * LM_KC + brow + 2 * i) * LM_BLD + bcol]) =
          on ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

  f32x16 macc[NMT];
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) macc[mt][r] = 0.f;

  const int nchunk = (win + LM_KC - 1) / LM_KC;
  const int npass = (nh + LM_PASS - 1) / LM_PASS;
  for (int pass = 0; pass < npass; ++pass) {
    const int bin0 = pass * LM_PASS + bg * 128;               // the wave's first bin of this pass
    const int ntile = min(4, max(0, (nh - bin0 + 31) / 32));  // its tiles that hold bins (wave-uniform)
    const bool nyq = bin0 == 0;                               // tile 0 holds DC (and Nyquist in its sine slot)
    f32x16 are[4], aim[4];
#pragma unroll
    for (int bt = 0; bt < 4; ++bt)
#pragma unroll
      for (int r = 0; r < 16; ++r) are[bt][r] = aim[bt][r] = 0.f;

    float fv[LM_FT], bn[LM_BT];
    f32x4 bv[LM_BT];
    unsigned fz = 0u;
    gather(0, fv, fz);
    load_basis(0, pass, bv, bn);
    __syncthreads();  // (the previous pass's reads of the stages are done)
    stage(0, fv, fz);
    stage_basis(0, pass, bv, bn);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
      const int cur = c & 1;
      const bool more = c + 1 < nchunk;
      if (more) {
        gather(c + 1, fv, fz);
        load_basis(c + 1, pass, bv, bn);
      }
      // a wave or tile without bins multiplies zeros (it has its own SIMD and would otherwise wait
      // at the barrier): the loop stays straight-line
      const float* F = Fs + cur * LM_KC * LM_FLD + 32 * fh + l31;
      const float* B = Bs + cur * LM_KC * LM_BLD + 2 * (bg * 128 + l31);
      // the chunk's operands first, then its MFMAs
      float f[LM_KC / 2];
      float2 b[LM_KC / 2][4];
#pragma unroll
      for (int ks = 0; ks < LM_KC / 2; ++ks) {
        f[ks] = F[(2 * ks + h) * LM_FLD];
#pragma unroll
        for (int bt = 0; bt < 4; ++bt)
          b[ks][bt] = *reinterpret_cast<const float2*>(B + (2 * ks + h) * LM_BLD + 64 * bt);
      }
#pragma unroll
      for (int ks = 0; ks < LM_KC / 2; ++ks)
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) {
          are[bt] = mfma32x32x2(b[ks][bt].x, f[ks], are[bt]);
          aim[bt] = mfma32x32x2(b[ks][bt].y, f[ks], aim[bt]);
        }
      if (more) {
        stage(c + 1, fv, fz);
        stage_basis(c + 1, pass, bv, bn);
      }
      __syncthreads();
    }

    // power (MAG: magnitude) and mel: accumulator r of lane (l31, h) is bin (tile base +
    // acc_row(r, lane)) of frame l31, which is P [k = h][j = l31] of the k pair (b_r, b_r + 4),
    // b_r = acc_row(r, 0)
    // The mel weights of a (tile, mel tile) are loaded as a batch before its 16 MFMAs, masked by a
    // multiply (a select lets the compiler move each load into a branch of its own, one L2 round
    // trip per MFMA); every load is clamped into the table
#pragma unroll
    for (int bt = 0; bt < 4; ++bt) {
      if (bt >= ntile) continue;
      const int tb = bin0 + 32 * bt;
      float p[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float re = are[bt][r], im = aim[bt][r];
        const bool dc = nyq && bt == 0 && r == 0 && h == 0;  // DC: its sine slot is Nyquist's cosine
        if constexpr (MAG)
          p[r] = dc ? fabsf(re) : sqrtf(re * re + im * im);
        else
          p[r] = dc ? re * re : re * re + im * im;
      }
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt) {
        const int m = 32 * mt + l31;
        const float* wrow = melfb + (long)min(m, nmels - 1) * nb;
        const float mrow = m < nmels ? 1.f : 0.f;
        float wv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int bin = tb + acc_row(r, lane);
          wv[r] = wrow[min(bin, nh - 1)] * (bin < nh ? mrow : 0.f);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) macc[mt] = mfma32x32x2(wv[r], p[r], macc[mt]);
      }
      if (bt == 0 && nyq) {  // the Nyquist bin: k = 0 of one more k pair, k = 1 empty
        const float im = aim[0][0];
        const float pn = h == 0 ? (MAG ? fabsf(im) : im * im) : 0.f;
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
          const int m = 32 * mt + l31;
          const float wl = melfb[(long)min(m, nmels - 1) * nb + nh] * ((m < nmels && h == 0) ? 1.f : 0.f);
          macc[mt] = mfma32x32x2(wl, pn, macc[mt]);
        }
      }
    }
  }

  // sum the two bin groups of each frame half (group 0 + group 1), log10, transpose through LDS
  // (MAG: 20 log10(max(., amin)), and the largest raw sum of every frame row into its segment's
  // seg_max)
  if (bg == 1) {
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[((fh * NMT + mt) * 16 + r) * 64 + lane] = macc[mt][r];
  }
  __syncthreads();
  if (bg == 0) {
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) macc[mt][r] += red[((fh * NMT + mt) * 16 + r) * 64 + lane];
  }
  __syncthreads();
  if (bg == 0) {
    float rmax = 0.f;  // (the sums are >= 0)
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = 32 * mt + acc_row(r, lane);
        if constexpr (MAG) {
          if (m < nmels) {
            red[(32 * fh + l31) * nmels + m] = 20.f * log10f(fmaxf(macc[mt][r], amin));
            rmax = fmaxf(rmax, macc[mt][r]);
          }
        } else {
          if (m < nmels) red[(32 * fh + l31) * nmels + m] = log10f(macc[mt][r] + 1e-6f);
        }
      }
    if constexpr (MAG) {
      // the lane pair (l31, h = 0 / 1) holds frame row 32 fh + l31's mels; lanes h = 0 fold.  A
      // wave whose valid rows all belong to one segment (most do) folds them first: one atomic
      rmax = fmaxf(rmax, __shfl_xor(rmax, 32, 64));
      const int f = 32 * fh + l31;
      const bool valid = h == 0 && g0 + f < n_frames;
      const int sg = rows[4 * LM_BM + f];
      const int sg0 = rows[4 * LM_BM + 32 * fh];  // (row 32 fh is valid if any row of the wave is)
      const bool one = __builtin_amdgcn_ballot_w64(valid && sg != sg0) == 0;
      if (one) {
        const float wmax = wave_max_dpp(valid ? rmax : 0.f);
        if (lane == 0 && g0 + f < n_frames) atomicMax(seg_max + sg0, __float_as_uint(wmax));
      } else if (valid) {
        atomicMax(seg_max + sg, __float_as_uint(rmax));
      }
    }
  }
  __syncthreads();
  const int nvalid = min(LM_BM, n_frames - g0) * nmels;
  float* dst = out + (long)g0 * nmels;
  for (int i = tid; i < nvalid; i += 256) dst[i] = red[i];
}

// out[f][:] = max(out[f][:], 20 log10(max(seg_max[segment of f], amin)) - top_db): a workgroup takes
// the 64 frame rows of one tile of the main kernel (contiguous in out)
__global__ __launch_bounds__(256) void meldb_clip_kernel(const int* __restrict__ frame_off, int n_seg, int n_frames,
                                                         int nmels, const float* __restrict__ seg_max, float amin,
                                                         float top_db, float* __restrict__ out) {
  __shared__ float level[LM_BM];
  const int tid = threadIdx.x;
  const int g0 = blockIdx.x * LM_BM;
  if (tid < LM_BM) {
    const int g = g0 + tid;
    float lv = 0.f;
    if (g < n_frames) lv = 20.f * log10f(fmaxf(seg_max[seg_of_frame(frame_off, n_seg, g)], amin)) - top_db;
    level[tid] = lv;
  }
  __syncthreads();
  const int nvalid = min(LM_BM, n_frames - g0) * nmels;
  float* dst = out + (long)g0 * nmels;
  for (int i = tid; i < nvalid; i += 256) dst[i] = fmaxf(dst[i], level[i / nmels]);
}

// The argument checks the three entry points share, in their order: the configuration, the basis
// table's row stride, alignment (tabs: the addresses of the entry point's 4-byte tables, or-ed
// together) and the stride's limit.
int lm_check(int nfft, int win, int hop, int nmels, long ld_wbasis, const float* y, const float* wbasis,
             const float* melfb, const float* out, uintptr_t tabs) {
  if (nfft < 2 || nfft > 1024 || nfft % 2 || win < 1 || win > nfft || hop < 1 || nmels < 1 || nmels > 32 * LM_MT)
    return SV_ESHAPE;
  if (ld_wbasis < nfft + 2) return SV_EARG;
  if (ld_wbasis % 4 || (((uintptr_t)y | (uintptr_t)wbasis | (uintptr_t)melfb | (uintptr_t)out) & 15) || (tabs & 3))
    return SV_EALIGN;
  if (ld_wbasis > (1L << 20)) return SV_EARG;  // (the kernel indexes the table with 32-bit offsets)
  return SV_OK;
}

// logmel_kernel<(nmels + 31) / 32, MODE> on 64 frames per workgroup
template <int MODE>
int lm_launch(hipStream_t stream, const float* y, const int* seg_off, const int* frame_off, int n_seg, int n_frames,
              int nfft, int win, int hop, int nmels, const float* wbasis, long ld_wbasis, const float* melfb,
              float* out, const int* seg_valid, const int* seg_len, float amin, unsigned* seg_max) {
  const dim3 grid((n_frames + LM_BM - 1) / LM_BM);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, y, seg_off, frame_off, n_seg, n_frames, nfft, win, hop,
                       nmels, wbasis, (int)ld_wbasis, melfb, out, seg_valid, seg_len, amin, seg_max);
  };
  switch ((nmels + 31) / 32) {
    case 1: launch(logmel_kernel<1, MODE>); break;
    case 2: launch(logmel_kernel<2, MODE>); break;
    case 3: launch(logmel_kernel<3, MODE>); break;
    default: launch(logmel_kernel<4, MODE>); break;
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // namespace

extern "C" size_t sv_logmel_workspace(int n_frames, int nfft, int win, int nmels) {
  (void)n_frames, (void)nfft, (void)win, (void)nmels;
  return 0;  // the fused kernel keeps the spectrum in registers
}

extern "C" int sv_logmel(const float* y, const int* seg_off, const int* frame_off, int n_seg, int n_frames, int nfft,
                         int win, int hop, int nmels, const float* wbasis, long ld_wbasis, const float* melfb,
                         float* out, void* workspace, hipStream_t stream) {
  (void)workspace;
  if (!y || !seg_off || !frame_off || !wbasis || !melfb || !out || n_seg < 1 || n_frames < n_seg) return SV_EARG;
  const int rc = lm_check(nfft, win, hop, nmels, ld_wbasis, y, wbasis, melfb, out,
                          (uintptr_t)seg_off | (uintptr_t)frame_off);
  if (rc) return rc;
  return lm_launch<LM_POWER>(stream, y, seg_off, frame_off, n_seg, n_frames, nfft, win, hop, nmels, wbasis, ld_wbasis,
                             melfb, out, nullptr, nullptr, 0.f, nullptr);
}

extern "C" int sv_logmel_ranges(const float* y, const int* seg_start, const int* seg_len, const int* frame_off,
                                int n_seg, int n_frames, int nfft, int win, int hop, int nmels, const float* wbasis,
                                long ld_wbasis, const float* melfb, float* out, void* workspace, hipStream_t stream) {
  (void)workspace;
  if (!y || !seg_start || !seg_len || !frame_off || !wbasis || !melfb || !out || n_seg < 1 || n_frames < n_seg)
    return SV_EARG;
  const int rc = lm_check(nfft, win, hop, nmels, ld_wbasis, y, wbasis, melfb, out,
                          (uintptr_t)seg_start | (uintptr_t)seg_len | (uintptr_t)frame_off);
  if (rc) return rc;
  return lm_launch<LM_RANGES>(stream, y, seg_start, frame_off, n_seg, n_frames, nfft, win, hop, nmels, wbasis,
                              ld_wbasis, melfb, out, nullptr, seg_len, 0.f, nullptr);
}

extern "C" size_t sv_meldb_workspace(int n_frames, int nfft, int win, int nmels) {
  (void)n_frames, (void)nfft, (void)win, (void)nmels;
  return 0;  // the per-segment maxima live in the caller's seg_max
}

extern "C" int sv_meldb(const float* y, const int* seg_start, const int* seg_valid, const int* seg_len,
                        const int* frame_off, int n_seg, int n_frames, int nfft, int win, int hop, int nmels,
                        const float* wbasis, long ld_wbasis, const float* melfb, float amin, float top_db, float* out,
                        float* seg_max, void* workspace, hipStream_t stream) {
  (void)workspace;
  if (!y || !seg_start || !seg_valid || !seg_len || !frame_off || !wbasis || !melfb || !out || !seg_max || n_seg < 1 ||
      n_frames < n_seg || !(amin > 0.f))
    return SV_EARG;
  int rc = lm_check(nfft, win, hop, nmels, ld_wbasis, y, wbasis, melfb, out,
                    (uintptr_t)seg_start | (uintptr_t)seg_valid | (uintptr_t)seg_len | (uintptr_t)frame_off |
                        (uintptr_t)seg_max);
  if (rc) return rc;
  rc = sv_zero_bytes(seg_max, (size_t)n_seg * sizeof(float), stream);
  if (rc) return rc;
  rc = lm_launch<LM_MAGDB>(stream, y, seg_start, frame_off, n_seg, n_frames, nfft, win, hop, nmels, wbasis, ld_wbasis,
                           melfb, out, seg_valid, seg_len, amin, reinterpret_cast<unsigned*>(seg_max));
  if (rc) return rc;
  if (top_db >= 0.f) {
    hipLaunchKernelGGL(meldb_clip_kernel, dim3((n_frames + LM_BM - 1) / LM_BM), dim3(256), 0, stream, frame_off, n_seg,
                       n_frames, nmels, (const float*)seg_max, amin, top_db, out);
    SV_LAUNCH_CHECK();
  }
  return SV_OK;
}
