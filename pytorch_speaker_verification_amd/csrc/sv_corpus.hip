// Training batches cut out of a device-resident corpus (sv_corpus_batch / sv_corpus_batch_bf16 of the
// C ABI): x[b][t][f] = corpus[utt[b]][f][start[b] + t] is never materialised; one launch writes the
// LSTM stack's layer-0 operands x_tm [T][B][F] and xT [F][T Bp] straight from the stored utterances.
//   corpus   [n_utt][F][Tc] fp32, the layout of the speakerK.npy files (mel-major, frames contiguous)
//   tile     one workgroup = 16 rows b x 16 frames t x up to 40 mels f.  The read runs along the frame
//            axis: 16 lanes take the 16 consecutive frames of one (utterance, mel) row (64 B; dword
//            loads, since start[b] may be odd), all of a thread's up to 48 loads in flight before
//            the first LDS store.  The tile lands in LDS as [t][b][f] with odd strides (41 per row, 657 per
//            frame: the store's 16 t-lanes fall on 16 different banks) and both outputs are written
//            from it: x_tm with consecutive lanes along (b, f) -- for one t the tile's rows are one
//            contiguous run of 16 F floats -- and xT with 16 lanes along b.  42 KB of LDS: three
//            workgroups per CU.
//   bounds   utt is clamped into [0, n_utt - 1] and start into [0, Tc - T] before any address is
//            formed; offsets are 64-bit.  Rows b in [B, Bp) load nothing and put zeros into xT's
//            padding columns.  No workspace, no atomics; the grid depends on the shape only.
#include "sv_bf16.h"
#include "../../include/sv_ge2e.h"

namespace {

constexpr int CB_R = 16, CB_T = 16, CB_F = 40;              // rows, frames, mels of a workgroup's tile
constexpr int CB_FP = CB_F + 1, CB_S = CB_R * CB_FP + 1;    // LDS strides of a row and of a frame
constexpr int CB_NK = (CB_F + 15) / 16;                     // passes of 16 mels over a row

struct CorpusArgs {
  const float* corpus;
  long n_utt;
  const int *utt, *start;
  int F, Tc, B, T, Bp;
};

// BF: bf16 outputs (the RNE cast of to_bf / pack_bf2), two elements per 4-byte store
template <bool BF>
__global__ __launch_bounds__(256) void corpus_batch_kernel(const CorpusArgs a, void* __restrict__ x_out,
                                                           void* __restrict__ xT_out) {
  __shared__ float tile[CB_T * CB_S];
  __shared__ long rowbase[CB_R];  // corpus offset of (row b, mel f0, frame t0); -1: no such row
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * CB_T, b0 = blockIdx.y * CB_R, f0 = blockIdx.z * CB_F;
  const int fcn = min(CB_F, a.F - f0);
  if (tid < CB_R) {
    long base = -1;
    if (b0 + tid < a.B) {
      const long u = min(max((long)a.utt[b0 + tid], 0L), a.n_utt - 1);
      const int s = min(max(a.start[b0 + tid], 0), a.Tc - a.T);
      base = (u * a.F + f0) * a.Tc + s + t0;
    }
    rowbase[tid] = base;
  }
  __syncthreads();
  {
    const int lt = tid & 15, lf = tid >> 4;  // 16 lanes along the frames of one (row, mel)
    const bool t_ok = t0 + lt < a.T;
    // the whole tile in flight before the first LDS store: 3 passes of 16 mels for each of the 16
    // rows, 48 predicated loads per thread
    float v[CB_R * CB_NK];
#pragma unroll
    for (int j = 0; j < CB_R * CB_NK; ++j) {
      const int b = j / CB_NK, f = (j % CB_NK) * 16 + lf;
      const long base = rowbase[b];
      v[j] = (t_ok && f < fcn && base >= 0) ? a.corpus[base + (long)f * a.Tc + lt] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < CB_R * CB_NK; ++j) {
      const int b = j / CB_NK, f = (j % CB_NK) * 16 + lf;
      if (f < fcn) tile[lt * CB_S + b * CB_FP + f] = v[j];
    }
  }
  __syncthreads();
  {  // x_tm: a wave per frame, its lanes along (row, mel) in steps of V elements
    constexpr int V = BF ? 2 : 1;
    const int nb = min(CB_R, a.B - b0), fu = fcn / V;
    const int lane = tid & 63;
    for (int t = tid >> 6; t < CB_T && t0 + t < a.T; t += 4) {
      int b = lane / fu, f = lane - b * fu;
      while (b < nb) {
        const float* src = tile + t * CB_S + b * CB_FP + f * V;
        const long o = ((long)(t0 + t) * a.B + b0 + b) * a.F + f0 + f * V;
        if constexpr (BF)
          *reinterpret_cast<unsigned*>(static_cast<bf16_t*>(x_out) + o) = pack_bf2(src[0], src[1]);
        else
          static_cast<float*>(x_out)[o] = src[0];
        f += 64;
        while (f >= fu) {
          f -= fu;
          ++b;
        }
      }
    }
  }
  if (xT_out) {  // xT: 16 lanes along the rows of one (mel, frame); bf16 pairs two rows per store
    const int b = tid & 15, t = tid >> 4;
    const bool ok = t0 + t < a.T && b0 + b < a.Bp;
    const long ldf = (long)a.T * a.Bp;
    const long o = (long)f0 * ldf + (long)(t0 + t) * a.Bp + b0 + b;
    const float* src = tile + t * CB_S + b * CB_FP;
    for (int f = 0; f < fcn; ++f) {
      if constexpr (BF) {
        const unsigned lo = to_bf(src[f]);
        const unsigned hi = __shfl_down(lo, 1, 64);  // row b + 1 (Bp % 8 == 0: inside Bp with b)
        if (ok && !(b & 1)) *reinterpret_cast<unsigned*>(static_cast<bf16_t*>(xT_out) + o + f * ldf) = lo | (hi << 16);
      } else {
        if (ok) static_cast<float*>(xT_out)[o + f * ldf] = src[f];
      }
    }
  }
}

template <bool BF>
int corpus_batch(const float* corpus, long n_utt, int F, int Tc, const int* utt, const int* start, int B, int T,
                 void* x, void* xT, int Bp, hipStream_t stream) {
  constexpr int V = BF ? 8 : 4;
  if (!corpus || !utt || !start || !x || n_utt < 1 || B < 1 || T < 1 || F < 1 || (xT && Bp < B)) return SV_EARG;
  if (T > Tc || F > 128 || F % V || Bp % V) return SV_ESHAPE;
  if ((((uintptr_t)corpus | (uintptr_t)x | (uintptr_t)xT) & 15) || (((uintptr_t)utt | (uintptr_t)start) & 3))
    return SV_EALIGN;
  const long rows = xT ? std::max(B, Bp) : B;
  const long nrb = (rows + CB_R - 1) / CB_R;
  if (nrb > 65535) return SV_ESHAPE;  // (the grid's y dimension)
  const CorpusArgs a{corpus, n_utt, utt, start, F, Tc, B, T, Bp};
  hipLaunchKernelGGL(corpus_batch_kernel<BF>, dim3((T + CB_T - 1) / CB_T, (unsigned)nrb, (F + CB_F - 1) / CB_F),
                     dim3(256), 0, stream, a, x, xT);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // namespace

extern "C" int sv_corpus_batch(const float* corpus, long n_utt, int F, int Tc, const int* utt, const int* start, int B,
                               int T, float* x_tm, float* xT, int Bp, hipStream_t stream) {
  return corpus_batch<false>(corpus, n_utt, F, Tc, utt, start, B, T, x_tm, xT, Bp, stream);
}

extern "C" int sv_corpus_batch_bf16(const float* corpus, long n_utt, int F, int Tc, const int* utt, const int* start,
                                    int B, int T, sv_bf16* x_bf, sv_bf16* xT, int Bp, hipStream_t stream) {
  return corpus_batch<true>(corpus, n_utt, F, Tc, utt, start, B, T, x_bf, xT, Bp, stream);
}
