// The sync block and the small launches around the persistent recurrences: the per-device CU count,
// the zeroing kernels (counters, state buffers), the sync block's size and counter channels, the
// status word's kernels (poison, report to pinned host memory, data-parallel agreement) and the
// deferred bias-gradient finalize as its own launch.  The recurrences are in sv_persist.hip,
// sv_persist3.hip, sv_wave.hip and sv_persist_f32.hip.
#include <algorithm>
#include <atomic>
#include "sv_bf16.h"
#include "../../include/sv_ge2e.h"

namespace {
// CU count per device, cached (device attributes do not change while the process runs)
std::atomic<int> g_cus[64];
int device_cus(int dev) {
  if (dev < 0 || dev >= 64) return 0;
  int n = g_cus[dev].load(std::memory_order_relaxed);
  if (n > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  g_cus[dev].store(n, std::memory_order_relaxed);
  return n;
}
int current_cus() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess ? device_cus(dev) : 0;
}
}  // namespace

int sv_stream_cus(hipStream_t stream) {
  int dev = -1;
  if (stream && hipStreamGetDevice(stream, &dev) == hipSuccess) return device_cus(dev);
  return current_cus();
}

extern "C" size_t sv_sync_size(void) { return (size_t)SV_SYNC_WORDS * sizeof(unsigned); }
// counter channel `chan` of a sync block
unsigned* sv_sync_cnt(unsigned* sync, int chan) {
  return sync + SV_SYNC_CNT + (size_t)chan * SV_PCNT_ROWS * SV_PCNT_STRIDE;
}

__global__ void sv_zero_counters_kernel(unsigned* cnt, int nchan, long chan_stride, int words) {
  for (int i = threadIdx.x; i < nchan * words; i += blockDim.x) cnt[(i / words) * chan_stride + i % words] = 0u;
}

int sv_zero_counters(unsigned* cnt, int nchan, long chan_stride, int words, hipStream_t stream) {
  if (!cnt || nchan <= 0 || words <= 0) return SV_EARG;
  hipLaunchKernelGGL(sv_zero_counters_kernel, dim3(1), dim3(256), 0, stream, cnt, nchan, chan_stride, words);
  return (int)hipGetLastError();
}

// head bytes up to 16-B alignment, 16-B body, tail bytes
__global__ void sv_zero_bytes_kernel(char* p, size_t head, size_t n16, size_t tail) {
  const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  if (i0 < head) p[i0] = 0;
  uint4* b = reinterpret_cast<uint4*>(p + head);
  for (size_t i = i0; i < n16; i += stride) b[i] = make_uint4(0u, 0u, 0u, 0u);
  if (i0 < tail) p[head + 16 * n16 + i0] = 0;
}

int sv_zero_bytes(void* p, size_t bytes, hipStream_t stream) {
  if (!bytes) return SV_OK;
  if (!p) return SV_EARG;
  const size_t head = std::min(bytes, (size_t)((16 - ((uintptr_t)p & 15)) & 15));
  const size_t n16 = (bytes - head) / 16, tail = bytes - head - 16 * n16;
  const size_t blocks = std::max<size_t>(1, std::min<size_t>(2048, (n16 + 255) / 256));
  hipLaunchKernelGGL(sv_zero_bytes_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (char*)p, head, n16, tail);
  return (int)hipGetLastError();
}

// up to SV_ZB_MAX zeroings in one launch (blockIdx.y = buffer): the per-step state resets of the
// bf16 stack (and, for the layer wavefront, its counter channels)
struct ZeroBatch {
  char* p[SV_ZB_MAX];
  size_t head[SV_ZB_MAX], n16[SV_ZB_MAX], tail[SV_ZB_MAX];
};
__global__ void sv_zero_bytes_multi_kernel(const ZeroBatch zb) {
  const int b = blockIdx.y;
  char* p = zb.p[b];
  const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  if (i0 < zb.head[b]) p[i0] = 0;
  uint4* q = reinterpret_cast<uint4*>(p + zb.head[b]);
  for (size_t i = i0; i < zb.n16[b]; i += stride) q[i] = make_uint4(0u, 0u, 0u, 0u);
  if (i0 < zb.tail[b]) p[zb.head[b] + 16 * zb.n16[b] + i0] = 0;
}
int sv_zero_bytes_multi(int n, void* const* ptrs, const size_t* bytes, hipStream_t stream) {
  if (n <= 0) return SV_OK;
  if (n > SV_ZB_MAX) return SV_EARG;
  ZeroBatch zb{};
  size_t most = 0;
  for (int i = 0; i < n; ++i) {
    if (!ptrs[i] && bytes[i]) return SV_EARG;
    char* p = static_cast<char*>(ptrs[i]);
    zb.p[i] = p;
    zb.head[i] = std::min(bytes[i], (size_t)((16 - ((uintptr_t)p & 15)) & 15));
    zb.n16[i] = (bytes[i] - zb.head[i]) / 16;
    zb.tail[i] = bytes[i] - zb.head[i] - 16 * zb.n16[i];
    most = std::max(most, zb.n16[i]);
  }
  const size_t blocks = std::max<size_t>(1, std::min<size_t>(2048, (most + 255) / 256));
  hipLaunchKernelGGL(sv_zero_bytes_multi_kernel, dim3((unsigned)blocks, n), dim3(256), 0, stream, zb);
  return (int)hipGetLastError();
}

__global__ void dbfin_kernel(const DbFin f) { dbfin_run(f, blockIdx.x); }
int sv_dbfin_launch(const DbFin& f, hipStream_t stream) {
  if (f.n <= 0) return SV_OK;
  hipLaunchKernelGGL(dbfin_kernel, dim3(dbfin_blocks(f, 256)), dim3(256), 0, stream, f);
  return (int)hipGetLastError();
}

// (status guard) loss := NaN when the sync block's status is set: a training step whose
// recurrences timed out reports a NaN loss instead of a finite wrong one
__global__ void status_poison_kernel(const unsigned* __restrict__ status, float* __restrict__ x, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) x[i] = __builtin_nanf("");
}
extern "C" int sv_status_poison(const void* sync, float* x, int n, hipStream_t stream) {
  if (!sync || !x || n <= 0) return SV_EARG;
  hipLaunchKernelGGL(status_poison_kernel, dim3((n + 255) / 256), dim3(256), 0, stream,
                     reinterpret_cast<const unsigned*>(sync), x, n);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// sv_status_poison + the status word reported to the host without a copy or an event (ABI v9):
// thread 0 stores ((seq << 32) | status) into a slot of caller-owned pinned host memory mapped into
// the device's address space (system scope, release), so the host reads the outcome of step `seq`
// by comparing the slot's high word -- the device->pinned copy and the event it needed idled the
// GPU ~10 us per step
__global__ void status_report_kernel(const unsigned* __restrict__ status, float* __restrict__ x, int n,
                                     unsigned long long* slot, unsigned seq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned s = __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (i < n && s) x[i] = __builtin_nanf("");
  if (i == 0)
    __hip_atomic_store(slot, ((unsigned long long)seq << 32) | s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
extern "C" int sv_status_report(const void* sync, float* x, int n, void* host_slot_dev, unsigned seq,
                                hipStream_t stream) {
  if (!sync || !host_slot_dev || n < 0 || (n > 0 && !x) || ((uintptr_t)host_slot_dev & 7)) return SV_EARG;
  hipLaunchKernelGGL(status_report_kernel, dim3(n > 0 ? (n + 255) / 256 : 1), dim3(256), 0, stream,
                     reinterpret_cast<const unsigned*>(sync), x, n,
                     reinterpret_cast<unsigned long long*>(host_slot_dev), seq);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
// the device address of pinned host memory (hipHostGetDevicePointer), for sv_status_report's slot
extern "C" int sv_host_device_ptr(void* host, void** dev) {
  if (!host || !dev) return SV_EARG;
  return (int)hipHostGetDevicePointer(dev, host, 0);
}

// data-parallel status agreement: flag[0..1] := the status's forward / backward bits as floats
// (two words of the SUM-reduced gradient buffer: a sum over ranks stays nonzero iff any rank set
// the bit), then status |= the reduced bits on every rank
__global__ void status_to_flag_kernel(const unsigned* __restrict__ status, float* __restrict__ flag) {
  if (threadIdx.x == 0) {
    const unsigned s = __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag[0] = (s & 1u) ? 1.f : 0.f;
    flag[1] = (s & 2u) ? 1.f : 0.f;
  }
}
__global__ void status_merge_kernel(unsigned* __restrict__ status, const float* __restrict__ flag) {
  if (threadIdx.x == 0) {
    const unsigned bits = (flag[0] != 0.f ? 1u : 0u) | (flag[1] != 0.f ? 2u : 0u);
    if (bits) __hip_atomic_fetch_or(status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
extern "C" int sv_status_to_flag(const void* sync, float* flag, hipStream_t stream) {
  if (!sync || !flag) return SV_EARG;
  hipLaunchKernelGGL(status_to_flag_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<const unsigned*>(sync), flag);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
extern "C" int sv_status_merge(void* sync, const float* flag, hipStream_t stream) {
  if (!sync || !flag) return SV_EARG;
  hipLaunchKernelGGL(status_merge_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<unsigned*>(sync), flag);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
