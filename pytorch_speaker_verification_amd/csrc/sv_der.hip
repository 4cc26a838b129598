// Diarization scoring on a frame grid (sv_seg_raster, sv_der_count of the C ABI): segment tables
// to per-frame speaker bit masks, and the masks to the integers of the diarization error rate, for a
// ragged batch of F files.  File f owns the frames frame_off[f] .. frame_off[f + 1] of every
// per-frame array; frame i of a file has its centre at sample i * step + step / 2.  Everything
// here is integer arithmetic: the results do not depend on the order of the atomics.
//   raster   one wave per table row (the host splits long rows into pieces of a fixed number of
//            frames, so rows are an even load): the row's first and one-past-last covered frame
//            from two divisions, clamped to the file's own frames and to the array, then the 64
//            lanes OR the row's bits into consecutive words (global_atomic_or, no return value:
//            256 contiguous bytes per wave instruction).
//   count    a (blocks of the largest file, F) grid, 8192 frames per workgroup, surplus workgroups
//            leave at once.  A lane reads one uint4 of every array per step (a wave: 1 KB of
//            consecutive frames per array; files start at any frame, so the grid of uint4 groups is
//            aligned to the arrays, and a group that straddles a file's edge is read word by
//            word).  total / miss / fa / both are popcounts summed in registers.  The 32 x 32
//            pair counts go through run-length merging before they touch LDS: the pair of an
//            unscored frame is (0, 0), which counts nothing; a lane whose four frames carry one
//            pair compares it with the lane below, the lanes where a run starts are collected by a
//            ballot, and the first lane of a run adds the run's whole length (4 x its lanes) to the
//            LDS histogram, once per set bit pair.  A lane with mixed frames merges its own four.
//            A wave in the middle of a speaker turn so does one LDS atomic per 256 frames instead
//            of 256 on one address.  The workgroup's 4 + 1024 counters are flushed with 64-bit
//            global atomic adds (zero counters are skipped).
#include "sv_common.h"
#include "../../include/sv_ge2e.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int DER_THREADS = 256;
constexpr int DER_STEPS = 8;                             // uint4 groups per lane
constexpr int DER_CHUNK = DER_THREADS * 4 * DER_STEPS;   // frames per workgroup: 8192
constexpr int DER_OUT = 4 + 32 * 32;
constexpr int DER_MAX_F = 65535;                         // grid.y

// ------------------------------------------------------------------ raster
__global__ __launch_bounds__(256) void seg_raster_kernel(const int* __restrict__ seg_start,
                                                         const int* __restrict__ seg_end,
                                                         const unsigned* __restrict__ seg_bits,
                                                         const int* __restrict__ seg_file, int n_seg,
                                                         const int* __restrict__ frame_off, int F, int step, int n_total,
                                                         unsigned* __restrict__ mask) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n_seg) return;
  const int lane = threadIdx.x & 63;
  const int f = seg_file[k];
  if (f < 0 || f >= F) return;
  const long s = seg_start[k], e = seg_end[k];
  const unsigned bits = seg_bits[k];
  if (e <= s || bits == 0u) return;
  const long off = frame_off[f];
  const long nf = (long)frame_off[f + 1] - off;
  if (off < 0 || nf <= 0) return;
  // frame i is covered iff s <= i * step + h < e: i in [ceil((s - h) / step), ceil((e - h) / step))
  const long h = step / 2;
  long lo = s <= h ? 0 : (s - h + step - 1) / step;
  long hi = e <= h ? 0 : (e - h + step - 1) / step;
  hi = hi < nf ? hi : nf;
  const long room = (long)n_total - off;  // whatever the tables say, nothing is written past the array
  hi = hi < room ? hi : room;
  for (long i = lo + lane; i < hi; i += 64) atomicOr(mask + off + i, bits);
}

// ------------------------------------------------------------------ count
__device__ __forceinline__ void pair_add(unsigned* __restrict__ hist, unsigned r, unsigned h, unsigned n) {
  while (r) {
    const int i = __ffs(r) - 1;
    r &= r - 1;
    unsigned hh = h;
    while (hh) {
      const int j = __ffs(hh) - 1;
      hh &= hh - 1;
      atomicAdd(hist + i * 32 + j, n);
    }
  }
}

struct Sums {
  unsigned total, miss, fa, both;
};

// one frame: the scalar sums, and the frame's pair with (0, 0) for a frame that is not scored
__device__ __forceinline__ void frame(unsigned& r, unsigned& h, unsigned ns, unsigned u, int skip_overlap, Sums& a) {
  const int nr = __popc(r), nh = __popc(h);
  const bool scored = ns == 0u && u != 0u && !(skip_overlap && nr > 1);
  if (scored) {
    a.total += nr;
    a.miss += nr > nh ? nr - nh : 0;
    a.fa += nh > nr ? nh - nr : 0;
    a.both += nr < nh ? nr : nh;
  } else {
    r = 0u;
    h = 0u;
  }
}

__global__ __launch_bounds__(DER_THREADS) void der_count_kernel(const unsigned* __restrict__ ref,
                                                                const unsigned* __restrict__ hyp,
                                                                const unsigned* __restrict__ noscore,
                                                                const unsigned* __restrict__ uem,
                                                                const int* __restrict__ frame_off, int n_total,
                                                                int skip_overlap, unsigned long long* __restrict__ out) {
  __shared__ unsigned hist[32 * 32];
  __shared__ unsigned scal[4];
  const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  long base = frame_off[f], end = frame_off[f + 1];
  base = base < 0 ? 0 : base;
  end = end < n_total ? end : n_total;
  const long first = (base & ~3L) + (long)blockIdx.x * DER_CHUNK;  // aligned to the arrays' uint4 groups
  if (first >= end) return;                                        // past this file's frames
  for (int i = tid; i < 32 * 32; i += DER_THREADS) hist[i] = 0u;
  if (tid < 4) scal[tid] = 0u;
  __syncthreads();

  Sums a{0u, 0u, 0u, 0u};
  for (int it = 0; it < DER_STEPS; ++it) {
    const long g = first + ((long)it * DER_THREADS + tid) * 4;
    if (first + (long)it * DER_THREADS * 4 >= end) break;  // uniform over the workgroup
    unsigned r[4] = {0u, 0u, 0u, 0u}, h[4] = {0u, 0u, 0u, 0u};
    if (g >= base && g + 4 <= end) {
      const u32x4 rv = *reinterpret_cast<const u32x4*>(ref + g);
      const u32x4 hv = *reinterpret_cast<const u32x4*>(hyp + g);
      const u32x4 nv = *reinterpret_cast<const u32x4*>(noscore + g);
      u32x4 uv = {1u, 1u, 1u, 1u};
      if (uem) uv = *reinterpret_cast<const u32x4*>(uem + g);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        r[v] = rv[v];
        h[v] = hv[v];
        frame(r[v], h[v], nv[v], uv[v], skip_overlap, a);
      }
    } else {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const long i = g + v;
        if (i >= base && i < end) {
          r[v] = ref[i];
          h[v] = hyp[i];
          frame(r[v], h[v], noscore[i], uem ? uem[i] : 1u, skip_overlap, a);
        }
      }
    }
    // run-length merge: inside the lane, then across the wave's lanes
    const bool plain = r[0] == r[1] && r[0] == r[2] && r[0] == r[3] && h[0] == h[1] && h[0] == h[2] && h[0] == h[3];
    const unsigned pr = __shfl_up(r[0], 1), ph = __shfl_up(h[0], 1);
    const int pplain = __shfl_up((int)plain, 1);
    const bool head = !plain || lane == 0 || !pplain || pr != r[0] || ph != h[0];
    const unsigned long long heads = __ballot(head);
    if (plain) {
      if (head && r[0] != 0u && h[0] != 0u) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int lanes = above ? __ffsll((long long)above) : 64 - lane;
        pair_add(hist, r[0], h[0], 4u * (unsigned)lanes);
      }
    } else {
      unsigned n = 1u;
#pragma unroll
      for (int v = 1; v <= 4; ++v) {
        if (v < 4 && r[v] == r[v - 1] && h[v] == h[v - 1]) {
          ++n;
        } else {
          if (r[v - 1] != 0u && h[v - 1] != 0u) pair_add(hist, r[v - 1], h[v - 1], n);
          n = 1u;
        }
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    a.total += __shfl_xor(a.total, d);
    a.miss += __shfl_xor(a.miss, d);
    a.fa += __shfl_xor(a.fa, d);
    a.both += __shfl_xor(a.both, d);
  }
  if (lane == 0) {
    atomicAdd(scal + 0, a.total);
    atomicAdd(scal + 1, a.miss);
    atomicAdd(scal + 2, a.fa);
    atomicAdd(scal + 3, a.both);
  }
  __syncthreads();
  unsigned long long* o = out + (long)f * DER_OUT;
  if (tid < 4 && scal[tid]) atomicAdd(o + tid, (unsigned long long)scal[tid]);
  for (int i = tid; i < 32 * 32; i += DER_THREADS)
    if (hist[i]) atomicAdd(o + 4 + i, (unsigned long long)hist[i]);
}

inline bool off16(const void* p) { return ((uintptr_t)p & 15) != 0; }
inline bool off8(const void* p) { return ((uintptr_t)p & 7) != 0; }
inline bool off4(const void* p) { return ((uintptr_t)p & 3) != 0; }

}  // namespace

extern "C" int sv_seg_raster(const int* seg_start, const int* seg_end, const unsigned* seg_bits, const int* seg_file,
                             int n_seg, const int* frame_off, int F, int step, int n_total, unsigned* mask,
                             hipStream_t stream) {
  if (!seg_start || !seg_end || !seg_bits || !seg_file || !frame_off || !mask || F < 1 || step < 1 || n_seg < 0 ||
      n_total < 0)
    return SV_EARG;
  if (off4(seg_start) || off4(seg_end) || off4(seg_bits) || off4(seg_file) || off4(frame_off) || off4(mask))
    return SV_EALIGN;
  if (n_seg == 0 || n_total == 0) return SV_OK;
  hipLaunchKernelGGL(seg_raster_kernel, dim3((n_seg + 3) / 4), dim3(256), 0, stream, seg_start, seg_end, seg_bits,
                     seg_file, n_seg, frame_off, F, step, n_total, mask);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_der_count(const unsigned* ref, const unsigned* hyp, const unsigned* noscore, const unsigned* uem,
                            const int* frame_off, int F, int max_frames, int n_total, int skip_overlap,
                            unsigned long long* out, hipStream_t stream) {
  if (!ref || !hyp || !noscore || !frame_off || !out || F < 1 || max_frames < 0 || n_total < 0) return SV_EARG;
  if (off16(ref) || off16(hyp) || off16(noscore) || off16(uem) || off4(frame_off) || off8(out)) return SV_EALIGN;
  if (F > DER_MAX_F) return SV_ESHAPE;
  if (hipError_t e = hipMemsetAsync(out, 0, sizeof(unsigned long long) * DER_OUT * (size_t)F, stream)) return (int)e;
  if (max_frames == 0 || n_total == 0) return SV_OK;
  // (+ 3: a file may start up to three frames into its first uint4 group)
  const int blocks = (int)(((long)max_frames + 3 + DER_CHUNK - 1) / DER_CHUNK);
  hipLaunchKernelGGL(der_count_kernel, dim3(blocks, F), dim3(DER_THREADS), 0, stream, ref, hyp, noscore, uem, frame_off,
                     n_total, skip_overlap, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
