// align_embeddings on the device (sv_dvec_align of the C ABI; dvector_create.py:55-73): the window
// embeddings of a batch of files averaged over the host's ~0.4 s partitions, in one launch.
//   kernel   dvec_align_kernel: a thread owns V consecutive columns of one partition (V = 4 where
//            P % 4 == 0: 16-byte loads, else 1), neighbouring threads neighbouring columns, so every
//            row read and the output row are coalesced.  It adds the partition's rows in their order
//            in fp32, starting from the first row, divides once by (float)count -- an IEEE divide,
//            never a reciprocal multiply -- and widens to double: what np.average does along axis 0
//            of a float32 [k, P] array (a sequential fp32 add of whole rows, one true divide), so
//            the result equals dvector.align_embeddings of the same embeddings exactly.
//   bounds   part_off is clamped into [0, S]: a bad table never reads outside emb.  An empty
//            partition writes zeros.  No atomics, no LDS, no workspace.
#include "sv_common.h"
#include "../../include/sv_ge2e.h"

namespace {

template <int V>
__global__ __launch_bounds__(256) void dvec_align_kernel(const float* __restrict__ emb, int S, int P,
                                                         const int* __restrict__ part_off, int n_parts,
                                                         double* __restrict__ out) {
  const int pv = P / V;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)n_parts * pv) return;
  const int p = (int)(i / pv), c = V * (int)(i % pv);
  const int a = min(max(part_off[p], 0), S), b = min(max(part_off[p + 1], a), S);
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  for (int r = a; r < b; ++r) {
    const float* src = emb + (long)r * P + c;
    float v[V];
    if constexpr (V == 4) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = x[j];
    } else {
      v[0] = src[0];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = r == a ? v[j] : acc[j] + v[j];
  }
  const float cnt = (float)(b - a);
  double* dst = out + (long)p * P + c;
#pragma unroll
  for (int j = 0; j < V; ++j) dst[j] = b > a ? (double)(acc[j] / cnt) : 0.0;
}

}  // namespace

extern "C" int sv_dvec_align(const float* emb, int S, int P, const int* part_off, int n_parts, double* out,
                             hipStream_t stream) {
  if (!emb || !part_off || !out || S < 1 || P < 1 || n_parts < 1) return SV_EARG;
  if ((((uintptr_t)emb | (uintptr_t)out) & 15) || ((uintptr_t)part_off & 3)) return SV_EALIGN;
  if ((long)n_parts * P >= (1L << 31) * 256) return SV_ESHAPE;  // (the grid's x dimension)
  if (P % 4 == 0) {
    const long n = (long)n_parts * (P / 4);
    hipLaunchKernelGGL(dvec_align_kernel<4>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, emb, S, P, part_off,
                       n_parts, out);
  } else {
    const long n = (long)n_parts * P;
    hipLaunchKernelGGL(dvec_align_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, emb, S, P, part_off,
                       n_parts, out);
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}
