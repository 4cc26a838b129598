// What the bf16 LSTM glue (sv_bf16.hip) needs from the bf16 GEMMs (sv_gemm_bf16.hip) beyond the C ABI
// of include/sv_ge2e.h: the fused pair of weight-gradient GEMMs, the dx GEMM that reads the
// persistent backward's fragment-order hand-off, and the whole-K weight-gradient launch with its plan.
#pragma once
#include "sv_bf16.h"
#include "sv_gemm256.h"

// 256 x 256 kernels (sv_gemm256.h) for shapes they tile exactly
inline bool gemm256_ok(int M, int N, int K) { return M % G256_BM == 0 && N % G256_BM == 0 && K % G256_BK == 0; }

// C1 = A . B1^T and C2 = A . B2^T (fp32 out, no bias / beta) in one launch over the shared A:
// the split-K plan of sv_gemm_bf16(M, N1, K), so each product sums exactly as the single GEMM
// does (bit-identical); falls back to two calls where the fused form does not apply.
// workspace: sv_gemm_bf16_dual_workspace bytes
size_t sv_gemm_bf16_dual_workspace(int M, int N1, int N2, int K);
int sv_gemm_bf16_dual(int M, int N1, int N2, int K, const bf16_t* A, long lda, const bf16_t* B1, long ldb1, float* C1,
                      long ldc1, const bf16_t* B2, long ldb2, float* C2, long ldc2, float* workspace,
                      hipStream_t stream);

// dx = dG . W_ih with dG read from the persistent backward's fragment-order hand-off buffer, where
// gemm_afrag_ok; fin: a deferred bias finalize riding on the launch (sv_gemm_bf16.hip)
bool gemm_afrag_ok(int T, int B, int N, int H);
int gemm_bf16_afrag(int T, int B, int H, int N, const bf16_t* dgf, int bm, const bf16_t* Bop, long ldb, float* C,
                    long ldc, float* workspace, hipStream_t stream, const DbFin& fin);

// ---- the layer wavefront's weight gradients as whole-K tiles in one launch (c4 rank) ----
// After the wavefront every layer's dG^T is final.  The per-layer split-K plan (c4 rank: K = T Bp =
// 12800 in 7 slabs of 29 k-tiles; 504 workgroups per dual GEMM, two rounds) writes 129 MB of fp32
// slabs per layer and reads them back in a reduce launch; the three layers' 256 x 256 tiles
// together (72 + 72 dual, 36 for layer 0's dW_hh) fit the CUs as ONE round of whole-K tiles, each
// stored straight into dW_hh / dW_ih.  Another fp32 summation order than the slabs' (one
// accumulator over the k-tiles): agreement with the per-layer schedule at fp32 level.
// Split form (S > 0): the CUs the tiles leave free (nsw workgroups, a multiple of 8, blocks
// 0 .. nsw - 1) compute every tile's first S k-tiles (tiles b, b + nsw, ...) and store the fp32
// partial (sc1, per-thread order) and a flag; the tile's own workgroup (block nsw + position)
// computes k-tiles S .. K/64 - 1, waits for the flag, adds the partial (its own sum first: one
// fixed order) and stores C.  The waiters are dispatched after every workgroup they wait for.
struct G8FLayer {
  const bf16_t* A;    // dG^T [4H][T Bp]
  const bf16_t* B;    // h^T (time-shifted)
  const bf16_t* B2;   // x^T (dual: columns past n1), or null
  float* C1;          // dW_hh
  float* C2;          // dW_ih (dual)
  long lda, ldb, ldb2, ldc1, ldc2;
  int N, n1, tiles;
  int f2;             // dW_ih columns (rows of x^T): layer 0's F = 40 in one partial 256-wide tile
};
struct G8Full {
  G8FLayer lay[WB_L];
  int K;             // T Bp
  int nsw, S;        // split form: first-piece workgroups and k-tiles (S = 0: whole-K tiles only)
  float* part;       // [P][256 x 256] fp32 first-piece partials
  unsigned* flag;    // [P], zero before the launch
  unsigned* status;  // the sync block's status word
  unsigned limit;
  DbFin fin;         // a deferred bias finalize: workgroups past the tiles (dbfin_blocks(fin, 512))
};
// the launch (gemm_bf16_8qf_kernel): P = the layers' tiles; the caller plans q (plan_fullk, sv_bf16.hip)
int gemm_bf16_fullk(const G8Full& q, int P, hipStream_t stream);
