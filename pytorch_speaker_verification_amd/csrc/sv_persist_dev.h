// Device helpers shared by the persistent-recurrence kernels (sv_persist.hip, sv_persist3.hip,
// sv_wave.hip; sv_persist_f32.hip takes the tile order, the bounded wait and the prefetch): the
// hand-off protocol, the tile order, the W-stationary weight loads, the elementwise pieces of the
// bf16 backward and forward steps, the phase stamps and the LDS-DMA tile image.  Each formula is
// written once (a kernel whose loop a helper would change keeps its own text, with a comment);
// every kernel keeps its own step skeleton -- the order of wait, staging, k-loop, exchange, cell,
// hand-off, publish and off-chain work, with every barrier and s_waitcnt in the kernel's own text
// or in a helper named for it.
#pragma once
#include "sv_bf16.h"

constexpr int SV_LDS_BYTES = 160 * 1024;  // LDS of a CU (gfx950): the bound of every kernel's layout

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;


__device__ __forceinline__ __amdgpu_buffer_rsrc_t sv_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// Tile order of the W-stationary kernels (1-D grid of nub x nrb workgroups).  Workgroup i is
// dispatched to XCD i % 8; with xcd = 1 each XCD gets a contiguous range of logical tiles, so
// the workgroups that share a row block (and read the same handed-off rows) sit mostly on one
// XCD and the second and later readers hit that XCD's L2 instead of the fabric.
// n: the compute workgroups (blocks past them, if any, are helper workgroups)
__device__ __forceinline__ int persist_tile_index(int xcd, int n) {
  const int i = blockIdx.x;
  int L = i;
  if (xcd) {
    const int x = i & 7, q = n >> 3, r = n & 7;
    L = x * q + min(x, r) + (i >> 3);
  }
  return L;
}
__device__ __forceinline__ void persist_tile(int xcd, int nub, int& ub, int& rb, int ncomp = 0) {
  const int L = persist_tile_index(xcd, ncomp ? ncomp : gridDim.x);
  ub = L % nub;
  rb = L / nub;
}
// the layered form (the layer wavefronts: L x nrb x nub workgroups, always XCD-grouped)
__device__ __forceinline__ void persist_tile_layered(int nub, int nrb, int& ub, int& rb, int& l) {
  const int L = persist_tile_index(1, gridDim.x);
  ub = L % nub;
  rb = (L / nub) % nrb;
  l = L / (nub * nrb);
}

// lane 0 of the workgroup: wait until *c >= target.  Bounded: after `limit` polls the wait sets
// `code` in the sync block's status word and returns; once the status is nonzero every wait on
// the block returns at once, so a broken launch drains instead of hanging the GPU.
__device__ __forceinline__ void persist_wait(unsigned* c, unsigned target, unsigned* status, unsigned limit,
                                             unsigned code) {
  unsigned spins = 0;
  while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
    if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    __builtin_amdgcn_s_sleep(2);
    if (++spins > limit) {
      __hip_atomic_fetch_or(status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  }
}
// test-only fault injection (SV_PERSIST_FAULT=1, read by the host): workgroup 0 withholds its
// first arrival, so its row block's consumers time out (short spin limit) and the status is set
__device__ __forceinline__ bool persist_arrive_ok(int fault, int first) { return !(fault && first && blockIdx.x == 0); }

// Publish a step (hand-off table row 1): every wave drains its stores (the hand-off's sc1 stores
// among them), the workgroup barrier, then ONE lane arrives on the row block's counter.
__device__ __forceinline__ void persist_drain() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
__device__ __forceinline__ void persist_arrive(unsigned* cnt, int fault, bool first) {
  if (threadIdx.x == 0 && persist_arrive_ok(fault, first))
    __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void persist_publish(unsigned* cnt, int fault, bool first) {
  persist_drain();
  persist_arrive(cnt, fault, first);
}
// The overlapped drain of the backward kernels: between persist_behind_begin() and
// persist_behind_drain<N>() the kernel issues N plain stores per thread (the step's dG^T pieces)
// behind the hand-off stores, and the wait counts them -- vmcnt(N): this wave's older (hand-off)
// stores done -- with a raw barrier (__syncthreads' fence would drain the N too).  The fence and
// the scheduling barriers keep the N stores younger than the hand-off's.  (Two calls, not one
// taking the stores as a lambda: a lambda that captured t by reference turned an LDS-DMA
// descriptor of lstm_persist2_bwd_bf16_kernel into VALU arithmetic with a waterfall loop.)
__device__ __forceinline__ void persist_behind_begin() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int N>
__device__ __forceinline__ void persist_behind_drain() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// ---- W-stationary weights: this lane's MFMA B fragments (16 k per step, 8 bf16 at wrow + 16 s),
// held for the whole launch ----
// one array, pinned to AGPRs (MFMA reads B from them directly: the VGPRs stay free for the A
// stream and the step's operands)
template <int NS>
__device__ __forceinline__ void wstat_load(const bf16_t* wrow, bool ok, bf16x8_t (&w)[NS]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    bf16x8_t z = {};
    w[s] = ok ? *reinterpret_cast<const bf16x8_t*>(wrow + 16 * s) : z;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) asm volatile("" : "+a"(w[s]));
}
// two slices per wave (the wide tiles' two unit halves, the wavefront backward's W_hh^T and
// W_ih^T): wa[NS] and the first NS - NL fragments of the second slice in registers (all of wa and
// 64 - NS of wb pinned to the 256 AGPRs), its last NL in LDS, wl [4 waves][NL][64 lanes][16 B]
template <int NS, int NL>
__device__ __forceinline__ void wstat_load_split(const bf16_t* ra, const bf16_t* rbp, bool oka, bool okb, char* wl,
                                                 int g, int lane, bf16x8_t (&wa)[NS], bf16x8_t (&wb)[NS - NL]) {
  constexpr int NR = NS - NL;
  const bf16x8_t z = {};
#pragma unroll
  for (int s = 0; s < NS; ++s) wa[s] = oka ? *reinterpret_cast<const bf16x8_t*>(ra + 16 * s) : z;
#pragma unroll
  for (int s = 0; s < NR; ++s) wb[s] = okb ? *reinterpret_cast<const bf16x8_t*>(rbp + 16 * s) : z;
#pragma unroll
  for (int s = NR; s < NS; ++s)
    *reinterpret_cast<bf16x8_t*>(wl + ((g * NL + s - NR) * 64 + lane) * 16) =
        okb ? *reinterpret_cast<const bf16x8_t*>(rbp + 16 * s) : z;
#pragma unroll
  for (int s = 0; s < NS; ++s) asm volatile("" : "+a"(wa[s]));
#pragma unroll
  for (int s = 0; s < 64 - NS; ++s) asm volatile("" : "+a"(wb[s]));  // the AGPRs left: 64 - NS fragments
}
// LDS-resident fragment j (0 .. NL - 1) of wave g's second slice
template <int NL>
__device__ __forceinline__ bf16x8_t wstat_wl_read(const char* wl, int g, int lane, int j) {
  return *reinterpret_cast<const bf16x8_t*>(wl + ((g * NL + j) * 64 + lane) * 16);
}
constexpr int wstat_wl_bytes(int NL) { return 4 * NL * 64 * 16; }

// ---- elementwise pieces of the bf16 backward step ----
// step tt's upstream dh: dhup [T][B][H] (up_full) or [B][H] at t = T - 1 only, else none
__device__ __forceinline__ const float* persist_dhup(const float* dhup, int up_full, int tt, int T, long BH) {
  return dhup ? (up_full ? dhup + (long)tt * BH : (tt == T - 1 ? dhup : nullptr)) : nullptr;
}
// 4 fp32 of a row (16-B buffer load; offsets past the range read zeros)
__device__ __forceinline__ float4 persist_ld_f4(__amdgpu_buffer_rsrc_t rs, long off_elems) {
  const u32x4_t x = __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)(off_elems * 4), 0, 0);
  return float4{__uint_as_float(x.x), __uint_as_float(x.y), __uint_as_float(x.z), __uint_as_float(x.w)};
}
// dh of 4 units: the four per-gate partials summed in gate order 0..3 (the per-step kernel's
// order), then the upstream dh
__device__ __forceinline__ float4 persist_gate_sum(float4 r0, float4 r1, float4 r2, float4 r3, float4 up) {
  float4 dh4 = r0;  // (elementwise, the scalar order)
  dh4 += r1;
  dh4 += r2;
  dh4 += r3;
  dh4 += up;
  return dh4;
}
// the hand-off stores of a step's dG tile dgs [32 KR rows][LDG] (4 gates x U units) in MFMA
// A-fragment order -- [row block][gate][row half m][k-step][lane][8], FRAG elements per (row
// block, gate, row half) -- as contiguous KB pieces (gate, row half, k-step), 16-B sc1 stores:
// KR U / 16 per thread
template <int KR, int U, int LDG, int FRAG>
__device__ __forceinline__ void persist_dgf_store(const bf16_t* dgs, __amdgpu_buffer_rsrc_t rw, int rb, int j0,
                                                  int tid) {
  constexpr int S = U / 16;  // k-steps of the tile's units
#pragma unroll
  for (int i = 0; i < KR * S; ++i) {
    const int p = tid + 256 * i, c = p >> 6, l = p & 63;
    const int gq = c / (KR * S), m = (c / S) % KR, sl = c % S;
    const uint4 v = *reinterpret_cast<const uint4*>(dgs + (32 * m + (l & 31)) * LDG + gq * U + 16 * sl + 8 * (l >> 5));
    const unsigned off =
        ((unsigned)((rb * 4 + gq) * KR + m) * (unsigned)FRAG + (unsigned)(j0 / 16 + sl) * 512u + (unsigned)l * 8u) * 2u;
    __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{v.x, v.y, v.z, v.w}, rw, off, 0, 16 /* sc1 */);
  }
}
// bias gradients (the tail after the time loop; dsum reuses the partial-exchange region, between
// two barriers of the kernel's): a thread's partial sums over t of its 4 units x 4 gates into
// dsum [ROWS][4 U] ...
template <int U>
__device__ __forceinline__ void persist_db_put(float* dsum, int row, int u4, const float (&dbs)[4][4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
    *reinterpret_cast<float4*>(dsum + row * (4 * U) + q * U + u4) = float4{dbs[q][0], dbs[q][1], dbs[q][2], dbs[q][3]};
}
// ... and its column sums (rows in order), one partial per row block; sv_persist_db_finalize adds
// the row blocks in order
template <int ROWS, int U>
__device__ __forceinline__ void persist_db_colsum(const float* dsum, int tid, int j0, int H, int rb, float* dbp) {
  if (4 * U == 256 || tid < 4 * U) {
    const int q = tid / U, gj = j0 + tid % U;
    float sum = 0.f;
    for (int b = 0; b < ROWS; ++b) sum += dsum[b * (4 * U) + tid];
    if (gj < H) dbp[(long)rb * (4L * H) + (long)q * H + gj] = sum;
  }
}

// ---- pieces of the bf16 forward step ----
// bf16(x W_ih^T + b) of a row (K1's output in `gates`, rx = step t's slice): 4 units at column ju
// of each gate, 8-B buffer loads; gbv = the row, or an offset past the slice for rows past B (zeros)
__device__ __forceinline__ void persist_load_xg(__amdgpu_buffer_rsrc_t rx, long gbv, long G, int H, int ju,
                                                uint2 (&xg)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u32x2_t x = __builtin_amdgcn_raw_buffer_load_b64(rx, (unsigned)((gbv * G + q * H + ju) * 2), 0, 0);
    xg[q] = uint2{x.x, x.y};
  }
}
// the hand-off: h_t bf16 from the LDS tile hsb [BM][LDB] (U units), BM rows x U / 8 chunks of 8
// units, one 16-B sc1 store per thread (of the first BM U / 8)
template <int BM, int U, int LDB>
__device__ __forceinline__ void persist_h_store(const bf16_t* hsb, __amdgpu_buffer_rsrc_t rw, int b0, int j0, int B,
                                                int H, int tid) {
  constexpr int C = U / 8;
  if (BM * C >= 256 || tid < BM * C) {
    const int row = tid / C, c = tid % C, gb = b0 + row;
    if (gb < B && j0 + 8 * c < H) {
      const uint4 v = *reinterpret_cast<const uint4*>(hsb + row * LDB + 8 * c);
      __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{v.x, v.y, v.z, v.w}, rw,
                                             ((unsigned)gb * (unsigned)H + (unsigned)(j0 + 8 * c)) * 2u, 0,
                                             16 /* sc1 */);
    }
  }
}
// off the critical chain: a row's 4 units of the activated gates (bf16), c, and -- at the last step
// only: the projection reads h_{T-1}; the next layer and the backward take the bf16 copies -- h
__device__ __forceinline__ void persist_row_store(bf16_t* gates_t, float* c_t, float* h_next, bool last, long gb, int ju,
                                                  int H, const uint2 (&act)[4], float4 cv, float4 hv) {
  bf16_t* gp = gates_t + gb * (4L * H) + ju;
#pragma unroll
  for (int q = 0; q < 4; ++q) *reinterpret_cast<uint2*>(gp + q * H) = act[q];
  *reinterpret_cast<float4*>(c_t + gb * H + ju) = cv;
  if (last) *reinterpret_cast<float4*>(h_next + gb * H + ju) = hv;
}
// h^T: 8 batch columns of unit row j (16 B from the transposed LDS tile) into hT [H][(T+1) Bp]
// slot t + 1 (padding columns get zeros; slot 0 is zeroed at t = 0)
__device__ __forceinline__ void persist_hT_store(bf16_t* hT, long ldhT, int j, int t, int Bp, int gb,
                                                 const bf16_t* chunk) {
  bf16_t* row = hT + (long)j * ldhT;
  *reinterpret_cast<uint4*>(row + (long)(t + 1) * Bp + gb) = *reinterpret_cast<const uint4*>(chunk);
  if (t == 0) *reinterpret_cast<uint4*>(row + gb) = uint4{0u, 0u, 0u, 0u};
}

// ---- phase stamps (profiling builds): s_memtime cycles per phase, summed over the steps; each
// kernel has its own way of switching them on, and stamps only where that switch is set ----
template <int N>
struct PhaseStamps {
  unsigned long long ph[N] = {}, tlast = 0;
  __device__ __forceinline__ void start() { tlast = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void mark(int i, bool count = true) {
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    if (count) ph[i] += now - tlast;
    tlast = now;
  }
};

// LDS-DMA image of one 32-row x H bf16 tile (H = 768; sv_wave.hip's wave3 forward and
// sv_persist3.hip's wide forward), two regions:
//   A: units [0, 512) as 32 rows of 1024 B + 16 B pad (a 1040-B row stride);
//   B: units [512, 768) as 32 rows of 512 B, unpadded, the 16-B chunk c of row r at slot
//      c ^ (r & 15) (an XOR swizzle in place of a pad: one DMA instruction fills two whole rows).
// Fragment reads (lanes 0-15 = rows 0-15 at one k offset) are conflict-free in both; every DMA
// instruction reads whole 128-B lines (one 1 KB row piece, or two 512-B ones).
constexpr int W3_RA = 1040, W3_RB = 512;
constexpr int W3_TILE = 32 * (W3_RA + W3_RB);
constexpr int W3_DMA = 12;  // DMA instructions per wave per tile (8 A + 4 B)

// stage a 32-row tile of slot `ts` of `ra` (a [T+1][B][H] bf16 buffer, H = 768; the descriptor is
// built once, outside the time loop, so it stays scalar): wave w stages rows 8 w .. 8 w + 7; rows
// past B read zeros.  The wave index goes through an opaque SGPR copy: the 24 per-instruction
// addresses are not hoisted out of the time loop (held live across it they pushed weight fragments
// into scratch) yet stay scalar -- a row's base is SALU arithmetic passed as soffset (region A) or
// one select per lane (region B) -- where an opaque VGPR zero made every address a VALU chain with
// a quarter-rate v_mul_lo_u32 and a v_readfirstlane for M0
struct W3Dma {
  __amdgpu_buffer_rsrc_t ra;
  unsigned slot, vl, xs, h2;
  int B, H, b0, g;
  char* tile;
  __device__ __forceinline__ W3Dma(__amdgpu_buffer_rsrc_t ra_, int ts, int B_, int H_, int b0_, char* tile_, int g_,
                                   int lane)
      : ra(ra_), B(B_), H(H_), b0(b0_), tile(tile_) {
    int gz = __builtin_amdgcn_readfirstlane(g_);  // (wave-uniform)
    asm volatile("" : "+s"(gz));
    g = gz;
    slot = (unsigned)ts * (unsigned)B * (unsigned)H * 2u;
    vl = 16u * (unsigned)lane;
    const unsigned hh = (unsigned)lane >> 5;
    xs = ((unsigned)lane & 31u) ^ hh;  // (sl ^ ((2 p + hh) & 15)) = xs ^ (2 p & 14)
    h2 = hh;
  }
  __device__ __forceinline__ unsigned row_base(int row) const {
    return b0 + row < B ? slot + (unsigned)(b0 + row) * (unsigned)H * 2u : 0xFFFFE000u;
  }
  __device__ __forceinline__ void piece(int i) const {
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    if (i < 8) {  // region A: row g 8 + i, one 1-KB row per instruction
      const int row = g * 8 + i;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_ptr_t)(tile + row * W3_RA), 16, vl, row_base(row), 0,
                                               16 /* sc1 */);
    } else {  // region B: rows 2 p, 2 p + 1 (lane halves), 512 B each, chunk c at c ^ (row & 15)
      const int p = g * 4 + (i - 8);
      const unsigned r0 = row_base(2 * p), r1 = row_base(2 * p + 1);
      const unsigned c = 64u + (xs ^ (unsigned)((2 * p) & 14));
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_ptr_t)(tile + 32 * W3_RA + p * 1024), 16,
                                               (h2 ? r1 : r0) + 16u * c, 0, 0, 16 /* sc1 */);
    }
  }
};
__device__ __forceinline__ void w3_dma(__amdgpu_buffer_rsrc_t ra, int ts, int B, int H, int b0, char* tile, int g,
                                       int lane) {
  const W3Dma d(ra, ts, B, H, b0, tile, g, lane);
#pragma unroll
  for (int i = 0; i < W3_DMA; ++i) d.piece(i);
}

// piece i (0 .. W3_DMA - 1) of w3_dma alone (the same addresses), for issue spread over a k-loop
__device__ __forceinline__ void w3_dma_piece(__amdgpu_buffer_rsrc_t ra, int ts, int B, int H, int b0, char* tile, int g,
                                             int lane, int i) {
  W3Dma(ra, ts, B, H, b0, tile, g, lane).piece(i);
}

// byte offset of A fragment s (k-step, 16 bf16) of lane (r, hh) in a w3_dma tile image
struct W3Frag {
  const char* pa;
  const char* pb;
  unsigned fb;
  __device__ __forceinline__ W3Frag(const char* tile, int lane) {
    const int r = lane & 31, hh = lane >> 5;
    pa = tile + r * W3_RA + hh * 16;
    fb = (unsigned)(((r & 15) ^ hh) << 4);
    pb = tile + 32 * W3_RA + r * W3_RB;
  }
  __device__ __forceinline__ bf16x8_t operator()(int s) const {
    if (s < 32) return *reinterpret_cast<const bf16x8_t*>(pa + 32 * s);
    return *reinterpret_cast<const bf16x8_t*>(pb + ((unsigned)(32 * (s - 32)) ^ fb));
  }
};

// The logical tiles [l0, l1) that persist_tile (xcd = 1) gives the blocks of XCD group x (blocks
// b with b % 8 == x) of an n-block grid
__device__ __forceinline__ void persist_xcd_tiles(int x, int n, int& l0, int& l1) {
  const int q = n >> 3, r = n & 7;
  l0 = x * q + min(x, r);
  l1 = l0 + q + (x < r ? 1 : 0);
}

// Operand prefetch by the helper workgroups of a persistent grid (blocks ncomp .. ncomp + npf - 1,
// npf a multiple of 8, so every XCD group gets npf / 8 of them): pull 16-B pieces of the bytes the
// XCD group's compute workgroups will DMA a few steps later into that XCD's L2 (and the
// Infinity Cache) by LDS-DMA into a scratch LDS slot -- no registers, no waits on the compute
// waves' in-order vmcnt.  Speed only: nothing reads the scratch slot, and a prefetch that comes
// late (or never) changes no result.
__device__ __forceinline__ void persist_prefetch16(const void* p, char* lds_scratch) {
  typedef __attribute__((address_space(1))) void* glb_ptr_t;
  __builtin_amdgcn_global_load_lds((glb_ptr_t)p, (lds_ptr_t)lds_scratch, 16, 0, 0);
}
