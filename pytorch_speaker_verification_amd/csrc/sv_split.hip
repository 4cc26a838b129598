// Framed energy of a ragged batch of waveforms (sv_frame_energy of the C ABI): the only part of
// librosa.effects.split / trim that touches every sample (feature.rms(center=True,
// pad_mode='reflect') ** 2).  The dB threshold and the interval bookkeeping are a few lines of
// numpy on the host (features.split).
//   kernel   frame_energy_kernel: one wave per frame, 4 frames per workgroup, no LDS and no barrier.
//            The wave finds its frame's segment by a bisection of frame_off (wave-uniform), then its
//            lanes stride the frame: sample j of the frame goes to lane j % 64, partial sum
//            (j / 64) % 4, in increasing j -- fmaf(v, v, acc) in fp32.  A frame that lies wholly
//            inside its segment (all but frame_length / hop of a waveform's frames) reads
//            consecutive dwords, 256 contiguous bytes per load instruction; an edge frame reflects
//            every index once and then clamps it into the segment.  The four partial sums are added
//            pairwise, the 64 lanes by DPP (wave_sum_dpp), and lane 0 stores sum * (1 / frame_length).
//   order    lane, partial sum and position in the chain depend on j alone, and the interior and the
//            edge path differ only in how they form the address: a frame's mse is bit-identical
//            wherever the frame sits in the batch
//   bound    the waveforms of one speaker sit in L2 and every sample is read frame_length / hop
//            times from there; there is nothing for an MFMA to do
#include "sv_common.h"
#include "../../include/sv_ge2e.h"

namespace {

constexpr int FE_WAVES = 4;         // frames per workgroup
constexpr int FE_ACC = 4;           // independent partial sums (and loads in flight) per lane
constexpr int FE_MAX_FL = 1 << 20;  // frame_length limit of the entry point

__global__ __launch_bounds__(64 * FE_WAVES) void frame_energy_kernel(const float* __restrict__ y,
                                                                    const int* __restrict__ seg_off,
                                                                    const int* __restrict__ frame_off, int n_seg,
                                                                    int n_frames, int fl, int hop, float inv_fl,
                                                                    float* __restrict__ mse) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long g = (long)blockIdx.x * FE_WAVES + w;
  if (g >= n_frames) return;
  const int lo = seg_of_frame(frame_off, n_seg, g);
  const int y0 = seg_off[lo], n = seg_off[lo + 1] - y0;
  if (n < 1) {  // an empty segment's one frame: nothing to read
    if (lane == 0) mse[g] = 0.f;
    return;
  }
  const float* ys = y + y0;
  const long base = (g - frame_off[lo]) * (long)hop - fl / 2;  // sample index of j = 0 before reflection
  float acc[FE_ACC];
#pragma unroll
  for (int k = 0; k < FE_ACC; ++k) acc[k] = 0.f;
  if (base >= 0 && base + fl <= n) {
    const float* yf = ys + base;
    for (int j0 = 0; j0 < fl; j0 += 64 * FE_ACC) {
      float v[FE_ACC];
#pragma unroll
      for (int k = 0; k < FE_ACC; ++k) {
        const int j = j0 + 64 * k + lane;
        v[k] = yf[min(j, fl - 1)];
        v[k] = j < fl ? v[k] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < FE_ACC; ++k) acc[k] = fmaf(v[k], v[k], acc[k]);
    }
  } else {
    for (int j0 = 0; j0 < fl; j0 += 64 * FE_ACC) {
      float v[FE_ACC];
#pragma unroll
      for (int k = 0; k < FE_ACC; ++k) {
        const int j = j0 + 64 * k + lane;
        v[k] = ys[reflect_clamp(base + j, n)];
        v[k] = j < fl ? v[k] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < FE_ACC; ++k) acc[k] = fmaf(v[k], v[k], acc[k]);
    }
  }
  const float s = wave_sum_dpp((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if (lane == 0) mse[g] = s * inv_fl;
}

}  // namespace

extern "C" int sv_frame_energy(const float* y, const int* seg_off, const int* frame_off, int n_seg, int n_frames,
                               int frame_length, int hop, float* mse, hipStream_t stream) {
  if (!y || !seg_off || !frame_off || !mse || n_seg < 1 || n_frames < n_seg) return SV_EARG;
  if (frame_length < 2 || frame_length > FE_MAX_FL || frame_length % 2 || hop < 1) return SV_ESHAPE;
  if ((((uintptr_t)y | (uintptr_t)mse) & 15) || (((uintptr_t)seg_off | (uintptr_t)frame_off) & 3)) return SV_EALIGN;
  const dim3 grid((unsigned)(((long)n_frames + FE_WAVES - 1) / FE_WAVES));
  hipLaunchKernelGGL(frame_energy_kernel, grid, dim3(64 * FE_WAVES), 0, stream, y, seg_off, frame_off, n_seg,
                     n_frames, frame_length, hop, 1.0f / (float)frame_length, mse);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
