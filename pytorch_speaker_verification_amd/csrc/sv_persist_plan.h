// The tile plan of the bf16 persistent recurrences: which kernel runs a layer's forward and
// backward recurrence for a batch of B rows at H hidden units on a device of `cus` CUs, with its
// row-block size and grid (host only; DESIGN §3.4 has the table).  One derivation for
// sv_persist_fwd_bf16, sv_persist_bwd_bf16 and sv_persist_bm: the backward's row block fixes the
// layout of the fragment-order hand-off that the dx GEMM reads.
#pragma once
#include "sv_bf16.h"

enum PersistTileKind {
  PT_LDS,     // LDS-staged forward, 64 rows x 32 units (H != 768): lstm_persist_fwd_bf16_kernel
  PT_U32x32,  // W-stationary, 32 units x 32 rows: lstm_persist2_{fwd,bwd}_bf16_kernel
  PT_U32x64,  // W-stationary, 32 units x 64 rows: lstm_persist2_bwd_bf16_kernel at H = 64 / 96 only
  PT_WIDE,    // wide tile, 64 units x 32 rows: lstm_persist3_{fwd,bwd}_bf16_kernel
  PT_FWD16    // 16-row wide forward, 64 units x 16 rows: lstm_persist16_fwd_bf16_kernel
};
struct PersistTile {
  PersistTileKind kind;
  int bm, nub, nrb;  // rows per block; the grid is nub unit blocks x nrb row blocks
};
struct PersistPlan {
  PersistTile fwd, bwd;
};

inline PersistPlan persist_plan(int B, int H, int cus) {
  const auto tile = [B](PersistTileKind kind, int bm, int nub) { return PersistTile{kind, bm, nub, (B + bm - 1) / bm}; };
  const int nub32 = (H + BF_U - 1) / BF_U, nrb32 = (B + 31) / 32;
  const bool rows32 = nrb32 <= SV_PCNT_ROWS;  // one counter per row block
  // 32 rows when twice the 64-row grid still fits on the device (B <= 320 at H = 768: c5's per-GPU
  // batch; measured 13.4 -> 10.1 ms at the c5 rank shape), else 64
  const PersistTile u32 = rows32 && (long)nub32 * nrb32 <= cus ? tile(PT_U32x32, 32, nub32) : tile(PT_U32x64, 64, nub32);
  // the wide pair: H = 768, (H / 64) x (B / 32) co-resident, and only where the 32-unit tile would
  // need 64-row blocks (B > 320 on 256 CUs: c3); at smaller B the 32 x 32 tile's twice-as-many
  // workgroups win (c5 rank 8.30 vs 9.48 ms, c4 rank 4.36 vs 5.65)
  const bool wide = H == 768 && u32.bm == 64 && rows32 && (long)(H / 64) * nrb32 <= cus;
  // the 16-row wide forward: H = 768, whole 16-row blocks, B > 256 (below, the 32 x 32 tile keeps its
  // bit-identity with the per-step schedule), (B / 16) x (H / 64) co-resident
  const bool fwd16 = H == 768 && !wide && B % 16 == 0 && B > 256 && B / 16 <= SV_PCNT_ROWS &&
                     (long)(B / 16) * (H / 64) <= cus;
  PersistPlan p;
  p.bwd = wide ? tile(PT_WIDE, 32, H / 64) : u32;
  // W_hh in registers at H = 768, else the LDS-staged forward
  p.fwd = H != 768 ? tile(PT_LDS, BF_BM, nub32) : wide ? p.bwd : fwd16 ? tile(PT_FWD16, 16, H / 64) : u32;
  return p;
}
