/* C ABI of libsv_ge2e.so -- the MI355X (gfx950) GE2E speaker-embedding training path.
 *
 * The reference (hwidong-na/PyTorch_Speaker_Verification) is pure Python over PyTorch and
 * has no FFI of its own; each entry point below replaces the device work PyTorch launches
 * implicitly at the cited reference line (SURVEY.md §2 "implicit op" table, §8 b).
 *
 * Conventions (all entry points):
 *   - every pointer is a caller-owned, contiguous, row-major DEVICE buffer (fp32), 16-byte
 *     aligned; scalars such as w, b, gloss are device pointers to one float (no host sync);
 *   - nothing is allocated, no global state is kept, no pointer is retained after return;
 *     scratch comes from a caller workspace of the size the matching *_workspace* returns;
 *     modes are explicit arguments (`products`, `schedule`; the library reads no environment
 *     variables), cross-workgroup counters live in a caller sync block (sv_sync_size), so calls
 *     with distinct buffers may run concurrently;
 *   - every launch goes to `stream` (pass the current stream of the tensor's device: the
 *     *_bwd functions are called from the autograd engine's worker thread);
 *   - return 0 on success, a hipError_t (> 0) from a failed launch, or a negative
 *     argument error (SV_EARG -1, SV_EALIGN -2, SV_ESHAPE -3).  Functions are reentrant.
 */
#ifndef SV_GE2E_H
#define SV_GE2E_H

#include <stddef.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SV_ABI_VERSION 12
int sv_abi_version(void);

/* ---- fp32 product modes (`products` argument of sv_gemm_f32 / sv_lstm_stack_fwd / _bwd; every
 * other fp32 entry point runs mode 0):
 *   0 exact fp32 MFMA products (v_mfma_f32_32x32x2_f32);
 *   1 "bf16x6": each fp32 operand split into three bf16 terms, six bf16 MFMA products per fp32
 *     product, fp32 accumulation -- products carried to ~2^-25 relative, measured GEMM error vs
 *     fp64 at or below the exact-MFMA path's (scripts/emu_check.py) -- on the NT GEMMs and K2;
 *   2 / 3 diagnostics (split at LDS store / in registers everywhere). */
#define SV_F32_EXACT 0
#define SV_F32_BF16X6 1

/* ---- schedule flags (`schedule` argument of the stack entry points; 0 = the measured default).
 * fp32 (sv_lstm_stack_fwd / _bwd): the W-stationary persistent recurrences (one launch per layer,
 * W_hh in registers, H = 768) under SV_SCHED_AUTO where their grid fills >= 3/4 of the device and
 * under SV_SCHED_PERSIST wherever it fits; SV_SCHED_PER_STEP keeps the layer-pipelined per-step
 * kernels (K2 / K3).  The two agree to fp32 rounding (different summation order).
 * bf16 (sv_lstm_stack_fwd_bf16 / _bwd_bf16):
 *   SV_SCHED_AUTO       the layer wavefront (all layers in one launch) where every layer's grid
 *                       fits co-resident, else one persistent recurrence launch per layer at
 *                       H = 768, else per-step launches;
 *   SV_SCHED_PER_LAYER  never the layer wavefront (it sums the upper layers' products in another
 *                       order: results agree at bf16 level, not bit for bit);
 *   SV_SCHED_PER_STEP   per-step launches, layer-pipelined over the side streams (bit-identical
 *                       to the persistent per-layer schedule);
 *   SV_SCHED_PERSIST    persistent per-layer recurrences for any H they support (64, 96, 768),
 *                       not only H = 768.
 * Both precisions:
 *   SV_SCHED_NO_EVENTS  (ABI v9) the stack backward's persistent / wavefront schedules record no
 *                       per-layer completion events into `ev` (set it when nothing waits on them,
 *                       i.e. no data-parallel gradient buckets: each event record leaves the GPU
 *                       idle for ~6 us between two kernels); the per-step schedule, whose side
 *                       streams synchronise through the events, ignores it.
 * bf16 stack backward only:
 *   SV_SCHED_WT_READY   the `wt` buffer is already filled: sv_lstm_weights_bf16 / sv_lstm_prep_bf16
 *                       (below) wrote the bf16 weight transposes into it from the same weights, so
 *                       the backward launches no transposes (the fp32 backward ignores it).
 *   SV_SCHED_CNT_READY  (ABI v11) the sync block's backward counter channels are still as the last
 *                       bf16 stack forward on it left them (it zeroes them) -- no backward has run
 *                       on the block since: the persistent / wavefront backward launches no
 *                       counter zeroing (the caller tracks this; passing it wrongly makes the
 *                       hand-off waits pass early). */
#define SV_SCHED_AUTO 0
#define SV_SCHED_PER_LAYER 1
#define SV_SCHED_PER_STEP 2
#define SV_SCHED_PERSIST 4
#define SV_SCHED_NO_EVENTS 8
#define SV_SCHED_WT_READY 16
#define SV_SCHED_CNT_READY 32
#define SV_SCHED_MASK 63

/* ---- dense fp32 MFMA GEMM (used by every op below; exported for tests) -----------------
 * C[M,N] = op(A) op(B) (+ bias0[n] + bias1[n]) (+ beta C).
 * a_kcontig: A element (m,k) at A[m*lda+k], else at A[k*lda+m].
 * b_kcontig: B element (k,n) at B[n*ldb+k], else at B[k*ldb+n].  */
size_t sv_gemm_f32_workspace(int M, int N, int K);
int sv_gemm_f32(int a_kcontig, int b_kcontig, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                float* C, long ldc, const float* bias0, const float* bias1, float beta, float* workspace,
                int products, hipStream_t stream);

/* column sums of X[R,C] (deterministic two-level reduction) */
size_t sv_colsum_workspace(int R, int C);
int sv_colsum(const float* X, int R, int C, float* out, float* workspace, hipStream_t stream);

/* ---- SpeechEmbedder LSTM stack (replaces nn.LSTM fwd, speech_embedder_net.py:19,28, and its
 * autograd backward via train_speech_embedder.py:62).  Time-major layouts:
 *   x_tm [T,B,F], gates [T,B,4H] (activated i,f,g,o), c_tm [T,B,H], h_tm [T+1,B,H] (h_tm[0]=0). */
int sv_frames_to_time_major(const float* x, float* x_tm, int B, int T, int F, hipStream_t stream);
/* dst[c*ld_dst + r] = src[r*ld_src + c] for an R x C matrix */
int sv_transpose(const float* src, long ld_src, int R, int C, float* dst, long ld_dst, hipStream_t stream);
/* Transposed layouts use column blocks of Bp = (B + 3) & ~3 (padding columns zero).
 * hT [H, (T+1)Bp] (may be NULL): h_t^T as column block t+1, block 0 = 0 -- the k-contiguous
 * operand of the weight-gradient GEMMs (block t = h_{t-1}) and of the next layer's dW_ih. */
int sv_lstm_layer_fwd(const float* x_tm, int T, int B, int F, int H, const float* w_ih, const float* w_hh,
                      const float* b_ih, const float* b_hh, float* gates, float* c_tm, float* h_tm, float* hT,
                      hipStream_t stream);
/* one forward recurrent step (K2): on entry gates_t [B,4H] = x_t W_ih^T + b_ih + b_hh, on exit the
 * activated gates; h_prev / c_prev may be NULL (t = 0). */
int sv_lstm_step_fwd(const float* h_prev, const float* w_hh, float* gates_t, const float* c_prev, float* c_t,
                     float* h_t, int B, int H, hipStream_t stream);
/* one backward recurrent step (K3): dg_t [B,4H] = dL/d(gates_t) from dg_next [B,4H] (NULL at
 * t = T-1), W_hh^T [H,4H], dh_up [B,H] (may be NULL), dcf_next = dc_{t+1} f_{t+1} (may be NULL),
 * the activated gates, c_t, c_{t-1} (NULL at t = 0); writes dcf_t = dc_t f_t. */
int sv_lstm_step_bwd(const float* dg_next, const float* w_hhT, const float* dh_up, const float* dcf_next,
                     const float* acts_t, const float* c_t, const float* c_prev, float* dg_t, float* dcf_t, int B,
                     int H, hipStream_t stream);
/* Whole stack.  Per-step schedule: layer-pipelined over streams, layer l on side[l] in chunks of
 * `chunk` timesteps (chunk input-projection GEMM, then its steps), waiting only for layer l-1's
 * same chunk, so the layers' kernels overlap.  Persistent schedule (`schedule`, above): per layer on
 * `main`, the whole-T input projection, then one persistent recurrence launch (needs `sync`, the
 * caller's sync block below; probe (may be NULL): 2*L caller events recorded around layer l's
 * launch, probe[2l] before, [2l+1] after).  Per-layer pointers come in host arrays of length L
 * (layer 0 input width F, others H); ev = L*ceil(T/chunk)+1 caller-created events.  Starts after
 * and joins back into `main` (all work ordered before the next op on `main`). */
int sv_lstm_stack_fwd(int L, int T, int B, int F, int H, const float* x_tm, const float* const* w_ih,
                      const float* const* w_hh, const float* const* b_ih, const float* const* b_hh,
                      float* const* gates, float* const* c_tm, float* const* h_tm, float* const* hT, int chunk,
                      hipStream_t main, const hipStream_t* side, hipEvent_t* ev, int products, int schedule,
                      unsigned* sync, hipEvent_t* probe);
/* 1 if the fp32 stack functions take the persistent recurrences for this batch under `schedule`
 * on the current device */
int sv_lstm_f32_persist_ok(int B, int H, int schedule);
size_t sv_lstm_layer_bwd_workspace(int T, int B, int F, int H);
/* Whole-stack backward (top layer first).  Per-step schedule, layer-pipelined over streams: each
 * layer's reverse chunks of steps on side[l], then (l > 0) the chunk's dx = dG W_ih GEMM that feeds
 * layer l-1; then the layer's whole-T dW_hh / dW_ih GEMMs and bias row sums on side[l].  side: L
 * streams.  Persistent schedule (`schedule`, `sync` as sv_lstm_stack_fwd): per layer on `main`, one
 * persistent recurrence launch (probe[2l] / [2l+1] around it; kstamp unused), then the whole-T dx,
 * dW GEMMs and row sums; ev[L*nch + l] recorded after layer l's gradients.
 * xT/ld_xT: per-layer transposed inputs; dx[l] [T,B,H] for l > 0;
 * ev = L*ceil(T/chunk) + L + 1 caller events (ev[L*nch + l] = layer l's gradients done);
 * joins back into `main`.  probe (may be NULL): 2*L*ceil(T/chunk) caller events recorded on the
 * layer's stream around ONE recurrent-step (K3) launch of each chunk (its second),
 * probe[2(l nch + c)] before, [+1] after (stream view: includes any wait for CUs); kstamp (may be
 * NULL): 2*L*T u64, each pair preset by the caller to {UINT64_MAX, 0}, which K3 launch (l, t)
 * sets to its first-workgroup start / last-workgroup end on the GPU's 100 MHz real-time clock
 * (the kernel's own execution span, as a profiler measures it) -- the bench's in-step roofline. */
size_t sv_lstm_stack_bwd_workspace(int L, int T, int B, int F, int H);
int sv_lstm_stack_bwd(int L, int T, int B, int F, int H, const float* const* xT, const long* ld_xT,
                      const float* const* w_ih, const float* const* w_hh, const float* const* gates,
                      const float* const* c_tm, const float* const* hT, const float* dh_last, float* const* dgates,
                      float* const* dgT, float* const* dx, float* const* dw_ih, float* const* dw_hh,
                      float* const* db_ih, float* const* db_hh, float* workspace, int chunk, hipStream_t main,
                      const hipStream_t* side, hipEvent_t* ev, int products, hipEvent_t* probe,
                      unsigned long long* kstamp, int schedule, unsigned* sync);
/* xT: the layer input transposed, [F, >= T*Bp] with row stride ld_xT (layer 0: the frames;
 * layer l > 0: hT of layer l-1 offset by Bp columns).  hT: this layer's [H, (T+1)Bp] from the fwd.
 * dh_up: gradient w.r.t. this layer's outputs; dh_up_full=1 -> [T,B,H], 0 -> [B,H] for t=T-1 only.
 * Outputs dgates [T,B,4H], dgT [4H, T*Bp] (its transpose), dx_tm [T,B,F] (may be NULL),
 * dw_ih [4H,F], dw_hh [4H,H], db_ih [4H] and db_hh [4H] (may be NULL; both = sum dgates). */
int sv_lstm_layer_bwd(int T, int B, int F, int H, const float* xT, long ld_xT, const float* w_ih, const float* w_hh,
                      const float* gates, const float* c_tm, const float* hT, const float* dh_up, int dh_up_full,
                      float* dgates, float* dgT, float* dx_tm, float* dw_ih, float* dw_hh, float* db_ih,
                      float* db_hh, float* workspace, hipStream_t stream);

/* ---- projection + L2 norm (speech_embedder_net.py:30-32) --------------------------------- */
size_t sv_proj_norm_workspace(int B, int H, int P);
int sv_proj_norm_fwd(const float* h_last, int B, int H, int P, const float* w_p, const float* b_p, float* y,
                     float* emb, float* ynorm, float* workspace, hipStream_t stream);
int sv_proj_norm_bwd(const float* demb, const float* emb, const float* ynorm, const float* h_last, int B, int H, int P,
                     const float* w_p, float* dw_p, float* db_p, float* dh_last, float* workspace,
                     hipStream_t stream);

/* ---- GE2E loss (speech_embedder_net.py:43-49; utils.py:27-132) -----------------------------
 * E is the local block [N_local, M, D] of a batch of N speakers; its first speaker is global
 * speaker spk_offset.  ssum_all [N,D] = per-speaker sums (all-gathered when sharded).
 * D % 4 == 0 and M >= 2.  dchat buffers are [Np, D] with Np = (N + 3) & ~3.
 * The workspace carries state from fwd to bwd: keep it alive and untouched in between. */
size_t sv_ge2e_workspace_size(int N_local, int M, int D, int N);
int sv_ge2e_speaker_sums(const float* E, int N_local, int M, int D, float* ssum_local, hipStream_t stream);
int sv_ge2e_fwd_rows(const float* E, int N_local, int M, int D, int spk_offset, int N, const float* ssum_all,
                     const float* w, const float* b, float* per, float* loss_local, float* workspace,
                     hipStream_t stream);
int sv_ge2e_fwd(const float* E, int N, int M, int D, const float* w, const float* b, float* loss, float* per,
                float* workspace, float* ssum, hipStream_t stream);
/* dchat_partial [Np,D] and beta_partial [N]: this shard's contribution (sum over ranks before
 * finalize); dwdb [2] = this shard's (dL/dw, dL/db).  gloss = upstream dL (NULL -> 1). */
int sv_ge2e_bwd_rows(int N_local, int M, int D, int spk_offset, int N, const float* w, const float* b,
                     const float* gloss, float* dchat_partial, float* beta_partial, float* dwdb, float* workspace,
                     hipStream_t stream);
int sv_ge2e_bwd_finalize(int N_local, int M, int D, int spk_offset, int N, const float* dchat, const float* beta,
                         float* dE, float* workspace, hipStream_t stream);
int sv_ge2e_bwd(int N, int M, int D, const float* w, const float* b, const float* gloss, float* dE, float* dwdb,
                float* dchat, float* beta, float* workspace, hipStream_t stream);

/* fused single-GPU training form (all N speakers local, gloss = 1): forward + closed-form
 * backward in three launches (per-speaker prep; a wave per row with the centroids staged in LDS,
 * fp32, in one tile up to 128 speakers and two tiles of 128 above: cosines, shuffle softmax, row
 * backward; a workgroup per (speaker, 64-wide d slice): centroid gradients and the speaker's dE).
 * Needs N <= 256, 2 <= M <= 16, D <= 256, D % 4 == 0 (sv_ge2e_train_ok);
 * workspace: sv_ge2e_workspace_size(N, M, D, N). */
int sv_ge2e_train_ok(int N, int M, int D);
int sv_ge2e_train(const float* E, int N, int M, int D, const float* w, const float* b, float* loss, float* per,
                  float* dE, float* dwdb, float* workspace, hipStream_t stream);

/* the fused kernels in the speaker-sharded form (data parallel; same shape limits as
 * sv_ge2e_train_ok(N, M, D) for the GLOBAL N):
 *   sv_ge2e_shard_prep      this shard's per-speaker sums ssum_local [N_local, D] (all-gather them
 *                           into ssum_all [N, D]) and its rows' normalised state (workspace);
 *   sv_ge2e_shard_rows      rows against all N centroids, softmax, row backward, then this shard's
 *                           contribution to red [Np*D + N] (dC^ before the norm Jacobian, beta;
 *                           SUM-all-reduce it) and its loss / (dw, db) partials;
 *   sv_ge2e_shard_finalize  this shard's dE from the reduced red.
 * workspace: sv_ge2e_workspace_size(N_local, M, D, N), kept across the three calls. */
int sv_ge2e_shard_prep(const float* E, int N_local, int M, int D, float* ssum_local, float* workspace,
                       hipStream_t stream);
int sv_ge2e_shard_rows(int N_local, int M, int D, int spk_offset, int N, const float* ssum_all, const float* w,
                       const float* b, float* per, float* red, float* loss_local, float* dwdb_local, float* workspace,
                       hipStream_t stream);
int sv_ge2e_shard_finalize(int N_local, int M, int D, int spk_offset, int N, const float* red, float* dE,
                           float* workspace, hipStream_t stream);

/* stand-alone helpers (utils.py): C = E.mean(1) [N,D]; cos [N,M,Nc] = get_cossim(E, C) with the
 * diagonal from E's own leave-one-out centroids (utils.py:75,91,113), +1e-6; calc_loss on S [N,M,K]. */
int sv_ge2e_centroids(const float* E, int N, int M, int D, float* C, hipStream_t stream);
size_t sv_ge2e_cossim_workspace(int N, int M, int D, int Nc);
int sv_ge2e_cossim(const float* E, int N, int M, int D, const float* C, int Nc, float* cos, float* workspace,
                   hipStream_t stream);
int sv_ge2e_calc_loss(const float* S, int N, int M, int K, float* per, float* loss, hipStream_t stream);
/* their backward passes (the autograd of utils.py:28, :72-115, :126-132):
 *   dE = dC / M broadcast over the M utterances;
 *   cossim: dE [N,M,D], dC [Nc,D] from dcos [N,M,Nc] -- gradient through the cosines against C_k
 *   (k != j) and, on the diagonal, through E's own leave-one-out centroid U_ji = (sum_i' E_ji' -
 *   E_ji) / (M - 1), as index_put's backward routes it (the overwritten entries give C nothing);
 *   calc_loss: dS [N,M,K] from gloss (device scalar, NULL = 0) and gper [N,M] (NULL = 0):
 *   dS_jik = (gloss + gper_ji) (e^{S_jik} / (sum_k e^{S_jik} + 1e-6) - [k == j]). */
int sv_ge2e_centroids_bwd(const float* dC, int N, int M, int D, float* dE, hipStream_t stream);
size_t sv_ge2e_cossim_bwd_workspace(int N, int M, int D, int Nc);
int sv_ge2e_cossim_bwd(const float* E, int N, int M, int D, const float* C, int Nc, const float* dcos, float* dE,
                       float* dC, float* workspace, hipStream_t stream);
int sv_ge2e_calc_loss_bwd(const float* S, int N, int M, int K, const float* gloss, const float* gper, float* dS,
                          hipStream_t stream);
/* EER sweep (train_speech_embedder.py:134-149): per threshold, #{S > thr} over all of S [N,M2,Nc]
 * and over its diagonal k == j (exact integer counts, returned as float). */
int sv_eer_counts(const float* S, int N, int M2, int Nc, const float* thresholds, int n_thr, float* cnt_all,
                  float* cnt_diag, hipStream_t stream);

/* ---- GE2E contrast loss (added under v12; additive): eq. 7 of the GE2E paper (arXiv 1710.10467, the
 * text-dependent loss) beside the softmax loss (eq. 6) the entry points above compute.  On the same
 * cos and S = w (cos + 1e-6) + b:
 *   per[j,i] = 1 - sigma(S[j,i,j]) + max_{k != j} sigma(S[j,i,k]),   loss = sum per.
 * The maximum is taken where S is largest over k != j (sigma is monotone: a negative w selects the
 * smallest cosine), ties to the lowest k (torch.max(dim)'s index).  Row backward with p = sigma(S_jj),
 * q = sigma(S_jk*): dS[j] = -p (1 - p), dS[k*] = q (1 - q), every other dS exactly 0, all scaled by the
 * upstream gloss.  sigma is evaluated from e^{-|x|}, so it neither overflows nor loses the small tail.
 * Each `_as` entry point is its namesake with a leading `loss` argument: SV_GE2E_SOFTMAX runs exactly
 * the namesake (which forwards here), SV_GE2E_CONTRAST swaps the row step only -- the fused
 * path's rows kernel (one kernel over the whole sv_ge2e_train_ok domain, local or sharded) or the
 * split path's row-loss / row-backward / diagonal kernels; prep, centroids, GEMMs, the column step
 * and finalize are shared, and so are the workspace (sv_ge2e_workspace_size; the split forward keeps
 * each row's k* in it for the backward), sv_ge2e_speaker_sums, sv_ge2e_bwd_finalize,
 * sv_ge2e_shard_prep and sv_ge2e_shard_finalize.  An unknown `loss` is SV_EARG and the contrast loss
 * with N < 2 speakers (no negative) SV_ESHAPE, both before any launch. */
enum sv_ge2e_loss_kind { SV_GE2E_SOFTMAX = 0, SV_GE2E_CONTRAST = 1 };
int sv_ge2e_fwd_rows_as(int loss, const float* E, int N_local, int M, int D, int spk_offset, int N,
                        const float* ssum_all, const float* w, const float* b, float* per, float* loss_local,
                        float* workspace, hipStream_t stream);
int sv_ge2e_fwd_as(int loss_kind, const float* E, int N, int M, int D, const float* w, const float* b, float* loss,
                   float* per, float* workspace, float* ssum, hipStream_t stream);
int sv_ge2e_bwd_rows_as(int loss, int N_local, int M, int D, int spk_offset, int N, const float* w, const float* b,
                        const float* gloss, float* dchat_partial, float* beta_partial, float* dwdb, float* workspace,
                        hipStream_t stream);
int sv_ge2e_bwd_as(int loss, int N, int M, int D, const float* w, const float* b, const float* gloss, float* dE,
                   float* dwdb, float* dchat, float* beta, float* workspace, hipStream_t stream);
int sv_ge2e_train_as(int loss_kind, const float* E, int N, int M, int D, const float* w, const float* b, float* loss,
                     float* per, float* dE, float* dwdb, float* workspace, hipStream_t stream);
int sv_ge2e_shard_rows_as(int loss, int N_local, int M, int D, int spk_offset, int N, const float* ssum_all,
                          const float* w, const float* b, float* per, float* red, float* loss_local, float* dwdb_local,
                          float* workspace, hipStream_t stream);
/* the contrast loss on a given S [N,M,K], K >= N and K >= 2 (else SV_ESHAPE): the positive is column
 * j, the maximum runs over every k != j, k < K; mirrors sv_ge2e_calc_loss / _bwd:
 * dS from gloss (device scalar, NULL = 0) and gper [N,M] (NULL = 0). */
int sv_ge2e_calc_contrast(const float* S, int N, int M, int K, float* per, float* loss, hipStream_t stream);
int sv_ge2e_calc_contrast_bwd(const float* S, int N, int M, int K, const float* gloss, const float* gper, float* dS,
                              hipStream_t stream);

/* ---- bf16 mixed-precision variant (BASELINE config c3) ---------------------------------------
 * GEMM operands (weights, h, dgates) in bf16 (RNE casts), bf16 MFMA with fp32 accumulation;
 * the stored x-projection (K1 output incl. biases) and the saved activated gates are bf16 (ABI
 * v3: `gates` is sv_bf16 [T,B,4H] -- in: bf16(x W_ih^T + b_ih + b_hh), out: bf16 activations;
 * the cell update itself runs on the fp32 sums and fp32 activations); cell state, biases,
 * gradients and outputs fp32.  Same layouts as the fp32 entry points, except transposed layouts
 * use column blocks of Bp = (B + 7) & ~7 and F, H, K and every bf16 leading dimension must be
 * multiples of 8.  sv_bf16 = raw bf16 bits. */
typedef unsigned short sv_bf16;
size_t sv_gemm_bf16_workspace(int M, int N, int K);
/* C[M,N] (fp32) = A[M,K] . B[N,K]^T (+ bias0 + bias1) (+ beta C); both operands k-contiguous */
int sv_gemm_bf16(int M, int N, int K, const sv_bf16* A, long lda, const sv_bf16* B, long ldb, float* C, long ldc,
                 const float* bias0, const float* bias1, float beta, float* workspace, hipStream_t stream);
/* C[M,N] (bf16) = bf16(A[M,K] . B[N,K]^T + bias0 + bias1): fp32 accumulation, one rounding (the
 * x-projection store of the bf16 LSTM); ldc % 4 == 0 for the 256 x 256 kernel, else a slower one */
int sv_gemm_bf16_bf(int M, int N, int K, const sv_bf16* A, long lda, const sv_bf16* B, long ldb, sv_bf16* C,
                    long ldc, const float* bias0, const float* bias1, hipStream_t stream);
int sv_cast_bf16(const float* x, sv_bf16* y, long n, hipStream_t stream);
/* n <= 8 such casts in one launch (y[i] = bf16(x[i]), count[i] elements each; host arrays) */
int sv_cast_bf16_batch(int n, const float* const* x, sv_bf16* const* y, const long* count, hipStream_t stream);
int sv_transpose_cast_bf16(const float* src, long ld_src, int R, int C, sv_bf16* dst, long ld_dst,
                           hipStream_t stream);
/* (ABI v10) the bf16 stack's input in one launch: frames x [B,T,F] (F <= 64) -> x_bf [T,B,F] and,
 * if xT != NULL, xT [F][T*Bp] (column t*Bp + b = x[b,t,:], columns b in [B, Bp) zero) */
int sv_frames_to_bf16(const float* x, int B, int T, int F, sv_bf16* x_bf, sv_bf16* xT, int Bp, hipStream_t stream);
/* `wt`: the buffer of bf16 weight transposes that the bf16 stack backward reads -- W_hh^T [H][4H]
 * of every layer and W_ih^T of layers >= 1 (rows padded by the library), each piece 256-byte
 * aligned.  sv_lstm_wt_bf16_size bytes (independent of T and B; 0 for a non-positive argument);
 * the caller allocates it 256-byte aligned, the library alone knows its layout. */
size_t sv_lstm_wt_bf16_size(int L, int F, int H);
/* every layer's bf16 weights in one launch, each fp32 weight read once: w_ih_bf[l] / w_hh_bf[l] =
 * bf16(w_ih[l]) / bf16(w_hh[l]) (row-major, the stack forward's operands) and, if wt != NULL, the
 * transposes into wt: pass it to sv_lstm_bwd with SV_SCHED_WT_READY and the backward launches no
 * transposes.  wt == NULL: the row-major copies only. */
int sv_lstm_weights_bf16(int L, int F, int H, const float* const* w_ih, const float* const* w_hh,
                         sv_bf16* const* w_ih_bf, sv_bf16* const* w_hh_bf, void* wt, hipStream_t stream);
/* sv_frames_to_bf16 (frames x [B,T,F] -> x_bf, xT) and sv_lstm_weights_bf16 in ONE launch: the bf16
 * stack forward's whole operand preparation. */
int sv_lstm_prep_bf16(int L, int T, int B, int F, int H, const float* x, sv_bf16* x_bf, sv_bf16* xT, int Bp,
                      const float* const* w_ih, const float* const* w_hh, sv_bf16* const* w_ih_bf,
                      sv_bf16* const* w_hh_bf, void* wt, hipStream_t stream);
/* x_bf [T,B,F]; writes gates (bf16), c_tm/h_tm (fp32) plus h_bf [T+1,B,H] and hT [H,(T+1)Bp] (bf16) */
int sv_lstm_layer_fwd_bf16(const sv_bf16* x_bf, int T, int B, int F, int H, const sv_bf16* w_ih_bf,
                           const sv_bf16* w_hh_bf, const float* b_ih, const float* b_hh, sv_bf16* gates, float* c_tm,
                           float* h_tm, sv_bf16* h_bf, sv_bf16* hT, hipStream_t stream);
/* stack forward in bf16 (as sv_lstm_stack_fwd; h_bf per layer [T+1,B,H]; of the fp32 h_tm only
 * slot T = h_{T-1}, the projection's input, is guaranteed -- the persistent schedules write no
 * other slot, the next layer and the backward read the bf16 copies) under `schedule`
 * (SV_SCHED_*).  sync: the caller's sync block (below; required when the persistent recurrences run).
 * probe (may be NULL): 2*L caller events recorded around each layer's persistent recurrence
 * launch (before / after; only when the persistent schedule runs) -- in-step kernel timing. */
int sv_lstm_stack_fwd_bf16(int L, int T, int B, int F, int H, const sv_bf16* x_bf, const sv_bf16* const* w_ih_bf,
                           const sv_bf16* const* w_hh_bf, const float* const* b_ih, const float* const* b_hh,
                           sv_bf16* const* gates, float* const* c_tm, float* const* h_tm, sv_bf16* const* h_bf,
                           sv_bf16* const* hT, int chunk, hipStream_t main, const hipStream_t* side,
                           hipEvent_t* ev, void* sync, hipEvent_t* probe, int schedule);
size_t sv_lstm_layer_bwd_bf16_workspace(int T, int B, int F, int H);
/* wihT_bf [F,4H], whhT_bf [H,4H]; dg_bf [T,B,4H] and dgT_bf [4H,T*Bp] are bf16 outputs */
int sv_lstm_layer_bwd_bf16(int T, int B, int F, int H, const sv_bf16* xT_bf, long ld_xT, const sv_bf16* wihT_bf,
                           const sv_bf16* whhT_bf, const sv_bf16* gates, const float* c_tm, const sv_bf16* hT_bf,
                           const float* dh_up, int dh_up_full, sv_bf16* dg_bf, sv_bf16* dgT_bf, float* dx_tm,
                           float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, float* workspace,
                           hipStream_t stream);

/* stack backward in bf16 under `schedule` (as sv_lstm_stack_bwd, L side streams; dg/dgT per layer
 * bf16).  workspace: sv_lstm_stack_bwd_bf16_workspace bytes of scratch (per-layer GEMM scratch and
 * the recurrences' hand-off; nothing in it outlives the call).  wt (required, sv_lstm_wt_bf16_size
 * bytes): the bf16 weight transposes -- already filled under SV_SCHED_WT_READY, else the backward
 * fills it from the fp32 master weights w_ih / w_hh.  probe: as the bf16 stack forward's, around
 * each layer's persistent backward recurrence. */
size_t sv_lstm_stack_bwd_bf16_workspace(int L, int T, int B, int F, int H);
int sv_lstm_stack_bwd_bf16(int L, int T, int B, int F, int H, const sv_bf16* const* xT, const long* ld_xT,
                           const float* const* w_ih, const float* const* w_hh, const sv_bf16* const* gates,
                           const float* const* c_tm, const sv_bf16* const* hT, const float* dh_last,
                           sv_bf16* const* dg, sv_bf16* const* dgT, float* const* dx, float* const* dw_ih,
                           float* const* dw_hh, float* const* db_ih, float* const* db_hh, void* workspace, void* wt,
                           int chunk, hipStream_t main, const hipStream_t* side, hipEvent_t* ev, void* sync,
                           hipEvent_t* probe, int schedule);

/* ---- dtype-enum form of the stack entry points (SURVEY.md §8 b: `lstm_fwd` = K1 + K2 and
 * `lstm_bwd` = K3 + K4 with a dtype argument; replaces the nn.LSTM forward / autograd backward at
 * speech_embedder_net.py:28 and train_speech_embedder.py:62).  One entry point per direction:
 *   SV_DTYPE_F32   -> sv_lstm_stack_fwd / _bwd: the `void` operands are float; h_bf is ignored
 *                     (pass NULL);
 *   SV_DTYPE_BF16  -> sv_lstm_stack_fwd_bf16 / _bwd_bf16: the `void` operands are sv_bf16
 *                     (x, w_ih, w_hh, gates, h_bf, hT; in the backward xT, gates, hT, dg, dgT);
 *                     `products` and `kstamp` are ignored (pass 0 / NULL); the backward's `wt`
 *                     (sv_lstm_wt_bf16_size bytes) is required (NULL: SV_EARG).  fp32 ignores `wt`.
 * Every other argument means what it means in the dtype-specific entry point; the backward takes
 * the fp32 master weights in both dtypes.  An unknown dtype returns SV_EARG. */
#define SV_DTYPE_F32 0
#define SV_DTYPE_BF16 1
int sv_lstm_fwd(int dtype, int L, int T, int B, int F, int H, const void* x, const void* const* w_ih,
                const void* const* w_hh, const float* const* b_ih, const float* const* b_hh, void* const* gates,
                float* const* c_tm, float* const* h_tm, void* const* h_bf, void* const* hT, int chunk,
                hipStream_t main, const hipStream_t* side, hipEvent_t* ev, int products, int schedule, void* sync,
                hipEvent_t* probe);
size_t sv_lstm_bwd_workspace(int dtype, int L, int T, int B, int F, int H);
int sv_lstm_bwd(int dtype, int L, int T, int B, int F, int H, const void* const* xT, const long* ld_xT,
                const float* const* w_ih, const float* const* w_hh, const void* const* gates, const float* const* c_tm,
                const void* const* hT, const float* dh_last, void* const* dg, void* const* dgT, float* const* dx,
                float* const* dw_ih, float* const* dw_hh, float* const* db_ih, float* const* db_hh, void* workspace,
                void* wt, int chunk, hipStream_t main, const hipStream_t* side, hipEvent_t* ev, int products,
                hipEvent_t* probe, unsigned long long* kstamp, int schedule, void* sync);

/* ---- persistent recurrences (one launch per layer for all T; sv_persist.hip).  The bf16 stack
 * forward uses them (by default when H = 768: W_hh held in registers) when the grid is
 * co-resident on the device of `main` (sv_persist_fwd_ok answers for the current device); the
 * bf16 stack backward likewise (H in {64, 96, 768}; by default when H = 768), handing dG off
 * through a fragment-order scratch of sv_persist_bwd_scratch(T, B, H) bytes that
 * sv_lstm_stack_bwd_bf16_workspace includes.
 * Sync block: caller-owned device memory of sv_sync_size() bytes, zeroed once before first use;
 * it holds the recurrences' arrival counters and, in its first u32 word, a STICKY status:
 *   0 ok; bit 0 / bit 1 set = a forward / backward hand-off wait timed out (a co-residency
 *   failure: another kernel or process held the CUs).  A timed-out launch drains instead of
 *   hanging; every later wait on the same block returns at once; all outputs written since are
 *   invalid.  The caller reads the word (async copy) and clears it.
 * Calls that share one block must be ordered (one stream); distinct blocks may run concurrently.
 * sv_status_poison: x[0..n) := NaN if the block's status is set (stream-ordered, no host sync). */
size_t sv_sync_size(void);
int sv_persist_fwd_ok(int B, int H);
int sv_persist_bwd_ok(int B, int H);
/* the bf16 layer-wavefront schedule (all L layers in one forward and one backward launch) fits
 * B rows on the current device (L = 3, F = 40, H = 768: B <= 96 on 256 CUs) */
int sv_wave_ok(int L, int T, int B, int F, int H);
size_t sv_persist_bwd_scratch(int T, int B, int H);
int sv_status_poison(const void* sync, float* x, int n, hipStream_t stream);
/* (ABI v9) sv_status_poison's poisoning of x[0..n) (n may be 0) plus a report of the status word
 * to the host without a copy: one 8-byte store of ((seq << 32) | status) into host_slot_dev, the
 * device address (sv_host_device_ptr = hipHostGetDevicePointer) of a caller-owned, 8-byte aligned
 * slot of pinned host memory; the host knows step `seq` is done when the slot's high word equals
 * seq.  Replaces the device->pinned copy + event of the old check. */
int sv_status_report(const void* sync, float* x, int n, void* host_slot_dev, unsigned seq, hipStream_t stream);
int sv_host_device_ptr(void* host, void** dev);
/* data-parallel status agreement (a rank whose recurrence timed out must stop every rank's
 * update): sv_status_to_flag writes the status's forward / backward bits as 0/1 floats into
 * flag[0..1], two words of the gradient buffer that the SUM all-reduce carries; sv_status_merge
 * ORs the bits whose reduced flag is nonzero back into the block's status, so sv_clip_sgd_step
 * skips the update on every rank alike. */
int sv_status_to_flag(const void* sync, float* flag, hipStream_t stream);
int sv_status_merge(void* sync, const float* flag, hipStream_t stream);

/* ---- large-batch d-vector inference (dvector_create.py:96-101; SpeechEmbedder.forward of every
 * 24-frame window of a file, speech_embedder_net.py:27-33), bf16 GEMM operands / fp32 accumulation
 * and state as the c3 forward (the input projection rounded to bf16 with its biases).  One launch per
 * timestep and layer: the 256 x 256 bf16 GEMM over [x_t | h_{t-1}] . [W_ih | W_hh]^T with the LSTM
 * cell in its epilogue, so no co-residency requirement at any B.  x [B][T][F] fp32 (batch-first
 * windows; F <= 64), layer l's w_ih [4H][F_l] (F_0 = F, else H), w_hh [4H][H], b_ih / b_hh [4H]
 * (the arrays of b_ih / b_hh may be NULL), w_p [P][H], b_p [P] (may be NULL), all fp32 device
 * pointers; emb [B][P] = normalize(h_{T-1} w_p^T + b_p).  H % 64 == 0, 4H % 256 == 0; workspace
 * of sv_dvector_bf16_workspace bytes, 256-B aligned.  Replaces embedder_net(windows) at
 * dvector_create.py:100 for the bf16 precision of embed_windows (dvector.py). */
size_t sv_dvector_bf16_workspace(int B, int T, int F, int H, int L, int P);
int sv_dvector_embed_bf16(int B, int T, int F, int H, int L, const float* x, const float* const* w_ih,
                          const float* const* w_hh, const float* const* b_ih, const float* const* b_hh,
                          const float* w_p, const float* b_p, int P, float* emb, void* workspace,
                          hipStream_t stream);

/* ---- log-mel front end (added under v12; additive): a ragged batch of waveform segments to
 * log-mel frames in one launch (librosa.stft(center=True, pad_mode='reflect') -> |.|^2 -> mel ->
 * log10(. + 1e-6): data_preprocess.py:41-47, dvector_create.py:38-47).
 *   y          all segments back to back, fp32
 *   seg_off    [n_seg + 1] sample offsets into y (device int32)
 *   frame_off  [n_seg + 1] frame offsets into out (device int32); segment s has 1 + len_s / hop
 *              frames and frame_off[n_seg] == n_frames (the host computes both arrays)
 *   wbasis     [win][ld_wbasis] fp32, the periodic Hann window w (length win, centred in nfft:
 *              lpad = (nfft - win) / 2) folded into the real-DFT basis, bins k = 0 .. nfft / 2:
 *                column 2k     = w[j] cos(2 pi k (j + lpad) / nfft)
 *                column 2k + 1 = w[j] sin(2 pi k (j + lpad) / nfft)
 *              nfft + 2 <= ld_wbasis <= 2^20, a multiple of 4
 *   melfb      [nmels][nfft / 2 + 1] fp32, dense
 *   out        [n_frames][nmels] fp32, time-major: out[f][i] = log10(sum_k melfb[i][k] P[f][k] + 1e-6),
 *              P[f][k] = |sum_j wbasis-row-j terms of frame f|^2; frame f of a segment covers the
 *              reflect-padded samples [f hop, f hop + nfft)
 * One fused kernel (frames x wbasis on the exact fp32 MFMA, power, mel and log10 in its epilogue;
 * the spectrum never goes to memory).  Limits: nfft even, 2 <= nfft <= 1024, 1 <= win <= nfft,
 * hop >= 1, 1 <= nmels <= 128 (else SV_ESHAPE); y, wbasis, melfb, out 16-byte aligned (SV_EALIGN).
 * Every segment must hold at least nfft / 2 + 1 samples (one reflection); the lengths live on the
 * device, so that check is the caller's (features.logmel raises ValueError) -- the kernel clamps
 * every sample index into its own segment, so a shorter segment gives meaningless frames but never
 * a read outside it.  Needs no scratch: sv_logmel_workspace returns 0 and workspace may be NULL. */
size_t sv_logmel_workspace(int n_frames, int nfft, int win, int nmels);
int sv_logmel(const float* y, const int* seg_off, const int* frame_off, int n_seg, int n_frames, int nfft, int win,
              int hop, int nmels, const float* wbasis, long ld_wbasis, const float* melfb, float* out,
              void* workspace, hipStream_t stream);

/* ---- mel magnitude in dB (added under v12; additive): the raw-waveform training feature of
 * utils.mfccs_and_spec(wav_process=True) (utils.py:138-158) for a ragged batch of virtual segments:
 * librosa.stft(center=True, pad_mode='reflect') -> |.| -> mel -> amplitude_to_db (ref 1, amin,
 * top_db), time-major.  wbasis, ld_wbasis, melfb, frame_off, n_seg, n_frames and the limits as in
 * sv_logmel.  Instead of seg_off, three device int32 arrays of n_seg entries describe segment s as
 * the virtual signal z[i] = i < seg_valid[s] ? y[seg_start[s] + i] : 0, i = 0 .. seg_len[s] - 1:
 *   seg_start  the segment's first sample in y
 *   seg_valid  how many real samples follow it (0 <= seg_valid; seg_start + max(seg_valid, 1) must
 *              lie inside y: with seg_valid = 0 the kernel still loads y[seg_start], and drops it)
 *   seg_len    the virtual length L_s; the segment has 1 + L_s / hop frames and the STFT's
 *              reflection is taken against L_s, so librosa.effects.trim (a start and a count),
 *              librosa.util.fix_length's zero padding (seg_valid < L_s) and its truncation
 *              (seg_valid = L_s < the count) are index arithmetic: y is never copied or re-packed.
 *              L_s >= nfft / 2 + 1 is the caller's check, as for sv_logmel (a shorter segment gives
 *              meaningless frames, never a read outside its real samples).  Segments may overlap in y.
 *   out        [n_frames][nmels] fp32: with x[f][i] = sum_k melfb[i][k] |STFT[f][k]|,
 *              db[f][i] = 20 log10(max(amin, x[f][i])), and for top_db >= 0
 *              out[f][i] = max(db[f][i], 20 log10(max(amin, seg_max[s])) - top_db), s the segment of
 *              f; top_db < 0: no clip, out = db
 *   seg_max    [n_seg] fp32, output: the largest x of the segment's frames (>= 0)
 * The fused kernel of sv_logmel in a second instantiation (magnitude in place of power as the mel
 * product's operand; IEEE sqrt, no fast-math), whose epilogue folds every valid frame row's largest
 * x into seg_max[its segment] with an unsigned integer atomic max on the float's bits (exact and
 * independent of order for x >= 0; seg_max is zeroed on the stream first), then one elementwise
 * kernel for the clip.  A segment's out and seg_max are bit-identical alone or in any batch.  No
 * host synchronisation, no allocation, graph-capturable; sv_meldb_workspace returns 0 and workspace
 * may be NULL.  Errors as sv_logmel, plus SV_EARG for amin <= 0 (or NaN) and a null seg_max, and
 * SV_EALIGN for a seg_* / seg_max pointer off a 4-byte boundary; all checks return before any
 * launch. */
size_t sv_meldb_workspace(int n_frames, int nfft, int win, int nmels);
int sv_meldb(const float* y, const int* seg_start, const int* seg_valid, const int* seg_len, const int* frame_off,
             int n_seg, int n_frames, int nfft, int win, int hop, int nmels, const float* wbasis, long ld_wbasis,
             const float* melfb, float amin, float top_db, float* out, float* seg_max, void* workspace,
             hipStream_t stream);

/* ---- framed energy (added under v12; additive): the per-sample half of librosa.effects.split /
 * trim (data_preprocess.py:35), feature.rms(center=True, pad_mode='reflect') ** 2, for a ragged
 * batch of waveforms in one launch.  y, seg_off, frame_off, n_seg, n_frames as in sv_logmel:
 * packed fp32 samples, device int32 tables of n_seg + 1 entries, waveform s has 1 + len_s / hop
 * frames and frame_off[n_seg] == n_frames.
 *   mse        [n_frames] fp32: mse[f] = (1 / frame_length) sum_j y[r(f hop - frame_length / 2 + j)]^2,
 *              j = 0 .. frame_length - 1, f counted within the waveform, r(i) = -i for i < 0,
 *              2 (len - 1) - i for i >= len (one reflection), then clamped into the waveform
 * One wave per frame: fp32 squares and partial sums in an order that depends on j alone (a
 * waveform's mse is bit-identical alone or in a batch), one multiply by 1 / frame_length.  No
 * workspace, nothing allocated or retained.  The dB threshold against each waveform's own maximum
 * and the interval bookkeeping are the host's (features.split).  Limits: frame_length even,
 * 2 <= frame_length <= 2^20, hop >= 1 (else SV_ESHAPE); y and mse 16-byte aligned, the tables 4-byte
 * (SV_EALIGN); null pointers, n_seg < 1 or n_frames < n_seg are SV_EARG.  Every waveform must hold
 * at least frame_length / 2 + 1 samples; as for sv_logmel that check is the caller's
 * (features.frame_energy raises ValueError) and a shorter one never reads outside itself (an empty
 * one reads nothing and gives 0). */
int sv_frame_energy(const float* y, const int* seg_off, const int* frame_off, int n_seg, int n_frames,
                    int frame_length, int hop, float* mse, hipStream_t stream);

/* ---- corpus d-vector export (added under v12; additive): the three device steps of
 * dvector.embed_files, which turns the voiced ranges of many files into uis-rnn sequences
 * (dvector_create.py:84-122) with one log-mel launch, one embedding pass and one averaging launch
 * per batch of files.
 *
 * sv_logmel_ranges: sv_logmel on ranges of ONE uploaded buffer.  Instead of seg_off, two device int32
 * arrays of n_seg entries give segment s as y[seg_start[s] .. seg_start[s] + seg_len[s]); ranges may
 * touch, overlap or leave gaps, and y is never re-packed.  frame_off, wbasis, melfb, out, the limits,
 * the alignment rules (the tables 4-byte), the error codes and "all checks return before any launch"
 * as in sv_logmel.  seg_len[s] >= nfft / 2 + 1 and seg_start[s] + seg_len[s] inside y are the caller's
 * checks (features.logmel_ranges raises ValueError); the kernel never reads outside
 * [seg_start, seg_start + seg_len).  The fused kernel of sv_logmel in a third instantiation that
 * differs only in where a frame row's origin and length come from: a range's frames are
 * bit-identical to sv_logmel's of a packed copy of that range, alone or in any batch. */
int sv_logmel_ranges(const float* y, const int* seg_start, const int* seg_len, const int* frame_off, int n_seg,
                     int n_frames, int nfft, int win, int hop, int nmels, const float* wbasis, long ld_wbasis,
                     const float* melfb, float* out, void* workspace, hipStream_t stream);

/* sv_dvector_embed_bf16_frames: sv_dvector_embed_bf16 reading its windows in place.  Instead of x,
 * frames [n_rows][F] fp32 (time-major log-mel rows, 16-byte aligned) and a device int32 win_start[B]:
 * window b, step t is row win_start[b] + t, clamped into [0, n_rows - 1] (a bad table never reads
 * outside frames).  Only the kernel that builds the padded bf16 x operand differs; the per-step
 * kernels, the workspace (sv_dvector_bf16_workspace) and the projection are shared, so emb is
 * bit-identical to sv_dvector_embed_bf16 on the materialised windows at the same B.  SV_EARG for a
 * null frames / win_start or n_rows < 1, SV_EALIGN for a misaligned one, before any launch. */
int sv_dvector_embed_bf16_frames(int B, int T, int F, int H, int L, const float* frames, int n_rows,
                                 const int* win_start, const float* const* w_ih, const float* const* w_hh,
                                 const float* const* b_ih, const float* const* b_hh, const float* w_p,
                                 const float* b_p, int P, float* emb, void* workspace, hipStream_t stream);

/* sv_dvec_align: align_embeddings (dvector_create.py:55-73) of a batch of files in one launch.
 * emb [S][P] fp32; part_off [n_parts + 1] device int32 row offsets (dvector.partitions per file,
 * concatenated over the files); out [n_parts][P] fp64.  Per element: rows part_off[p] ..
 * part_off[p + 1] - 1 added in that order in fp32 starting from the first row, one IEEE fp32
 * division by (float)count, widened to double -- np.average along axis 0 of a float32 array, so out
 * equals dvector.align_embeddings exactly.  An empty partition gives zeros; offsets are clamped
 * into [0, S].  Any P >= 1; emb and out 16-byte aligned, part_off 4-byte (SV_EALIGN); null
 * pointers or S, P, n_parts < 1 are SV_EARG.  No atomics, no workspace. */
int sv_dvec_align(const float* emb, int S, int P, const int* part_off, int n_parts, double* out, hipStream_t stream);

/* ---- training batches from a device-resident corpus (added under v12; additive): the LSTM stack's
 * layer-0 operands cut straight out of the stored utterances, in one launch.  The batch
 *   x[b][t][f] = corpus[utt[b]][f][start[b] + t],  b < B, t < T, f < F
 * is never materialised.
 *   corpus  [n_utt][F][Tc] fp32: utterance-major, then mel, frames contiguous -- the layout of the
 *           preprocessed speakerK.npy files (data_preprocess.py:46-54), all speakers concatenated
 *   utt     device int32 [B]: the utterance of row b, clamped into [0, n_utt - 1]
 *   start   device int32 [B]: its first frame, clamped into [0, Tc - T]; a bad table never forms an
 *           address outside corpus, and every offset is 64-bit (n_utt F Tc may pass 2^31)
 *   x_tm    [T][B][F] (fp32), x_bf likewise in bf16
 *   xT      [F][T Bp]: column t Bp + b holds x[b][t][:], the padding columns b in [B, Bp) are written
 *           as zeros (the buffer needs no zeroing); may be NULL (a forward that saves no state)
 * These are the operands sv_frames_to_time_major + sv_transpose (fp32) and sv_frames_to_bf16 (bf16)
 * make of the materialised batch, bit for bit: the fp32 outputs are copies, the bf16 ones the same
 * round-to-nearest-even cast.  One launch on `stream`, whose grid depends on (B, T, F, Bp) only; no
 * workspace, no atomics, no host synchronisation, graph-capturable.  It belongs on the stream of the
 * step it feeds, ahead of the forward: never on a side stream beside a persistent recurrence, whose
 * grid must have the CUs to itself (the sync block's status word reports exactly that failure).
 * SV_EARG: a null corpus, utt, start or x_tm / x_bf; n_utt, B, T or F < 1; xT given with Bp < B.
 * SV_ESHAPE: T > Tc; F > 128 (the front end's nmels limit); F % 4 or Bp % 4 (fp32), F % 8 or Bp % 8
 * (bf16; Bp is checked whether or not xT is given); more than 2^20 - 16 rows.  SV_EALIGN: corpus or
 * an output off a 16-byte boundary, a table off a 4-byte one.  All checks return before any launch. */
int sv_corpus_batch(const float* corpus, long n_utt, int F, int Tc, const int* utt, const int* start, int B, int T,
                    float* x_tm, float* xT, int Bp, hipStream_t stream);
int sv_corpus_batch_bf16(const float* corpus, long n_utt, int F, int Tc, const int* utt, const int* start, int B,
                         int T, sv_bf16* x_bf, sv_bf16* xT, int Bp, hipStream_t stream);

/* ---- verification trials (added under v12; additive): every pair of rows of two embedding
 * matrices scored and binned in one launch, for a ROC over a whole held-out set (verification.py).
 * The score matrix is never written: U utterances give U^2 / 2 scores, 20 GB at U = 100 000.
 *   A [Na][lda], B [Nb][ldb] fp32 rows of D values, taken as they are (the caller normalises);
 *   lab_a [Na], lab_b [Nb] device int32.  Pair (i, j) has the score s = sum_d A[i][d] B[j][d], fp32
 *   products and sums on the exact fp32 MFMA.  A row with a negative label takes part in no pair; a
 *   pair is a target when its two labels are equal, else a non-target.
 *   symmetric != 0: B, ldb, lab_b, Nb must repeat A, lda, lab_a, Na; only the pairs i < j count.
 *   Slot of a score, with q = floorf((s - lo) * inv_width) in two separately rounded fp32 operations:
 *       slot 0             if !(q >= 0)     (below lo, or NaN)
 *       slot n_bins + 1    if q >= n_bins
 *       slot 1 + (int)q    otherwise
 *   hist [2][n_bins + 2] unsigned 64-bit, sv_trial_hist_size(n_bins) bytes: row 0 non-targets, row 1
 *   targets.  The kernel ADDS to it (64-bit atomics): the caller zeroes it, two calls accumulate.
 *   Counts are integers, so the result depends neither on `grid` nor on arrival order.
 *   grid: workgroups of the persistent launch, 0 = chosen from the device and the LDS footprint.
 * One launch on `stream`, no workspace, nothing retained (sv_trials.hip has the tile plan).
 * SV_EARG: a null pointer; Na, Nb, D or n_bins < 1; grid < 0; symmetric with different operands.
 * SV_EALIGN: A or B off a 16-byte boundary (a label table off a 4-byte, hist off an 8-byte one);
 * lda, ldb or D not a multiple of 4; lda or ldb < D.  SV_ESHAPE: n_bins > 8192; D > 1024.  Checked in
 * that order, all before any launch. */
size_t sv_trial_hist_size(int n_bins);
int sv_trial_hist(const float* A, long lda, const int* lab_a, int Na, const float* B, long ldb, const int* lab_b,
                  int Nb, int D, int symmetric, float lo, float inv_width, int n_bins, unsigned long long* hist,
                  int grid, hipStream_t stream);

/* ---- adaptive score normalisation (AS-norm; added under v12; additive): the two device steps of
 *     z(e, t) = 1/2 ((s - mu_e) / sigma_e + (s - mu_t) / sigma_t),
 * mu_x, sigma_x the mean and standard deviation of the top_k largest scores of x against a cohort.
 *
 * sv_cohort_topk_stats: for every row i of X [N][ldx] the scores s_c = sum_d X[i][d] C[c][d] over the
 * Nc rows of C [Nc][ldc], on the exact fp32 MFMA with sv_trial_hist's tile (a pair of rows scores the
 * same bits in both); mean[i] = the mean of the top_k largest of them, std[i] = their population
 * standard deviation (divisor top_k), both computed in fp64 from the fp32 scores and rounded once.
 * The selection is exact, ties included: the top_k values are a multiset, so which of several equal
 * scores is taken cannot matter.  It is a radix select (8-bit digits, 4 passes) on the order-preserving
 * key of a score -- all 32 bits flipped if the sign bit is set, else the sign bit flipped -- plus one
 * pass for the sums; each pass recomputes the scores, none is written, there is no workspace
 * (sv_snorm.hip has the plan).  A NaN score takes the largest key, above +inf: a row of X with a NaN
 * score gets NaN mean and std, and no other row is touched (a NaN row of C reaches every row).
 *   grid: workgroups striding over the 128-row blocks of X, 0 = one per CU; the results do not depend
 *   on it (the sums are combined in a fixed order).
 * SV_EARG: a null pointer; N, Nc, D or top_k < 1; top_k > Nc; grid < 0.  SV_EALIGN: X or C off a
 * 16-byte boundary (mean or std off a 4-byte one); ldx, ldc or D not a multiple of 4; ldx or ldc < D.
 * SV_ESHAPE: Nc > 65 535 (16-bit bin counters); D > 1024.  Checked in that order, before the launch. */
int sv_cohort_topk_stats(const float* X, long ldx, int N, const float* C, long ldc, int Nc, int D, int top_k,
                         float* mean, float* std, int grid, hipStream_t stream);

/* sv_trial_hist_norm: sv_trial_hist -- the same kernel, tiles, masks, labels, flush and `hist` -- with
 * one step between the score s of pair (i, j) and the slot rule, five separately rounded fp32
 * operations (no contraction):
 *     za = (s - mu_a[i]) * inv_a[i];   zb = (s - mu_b[j]) * inv_b[j];   z = 0.5f * (za + zb);
 * and the slot is sv_trial_hist's slot rule on z.  mu_a, inv_a [Na], mu_b, inv_b [Nb] device fp32 (inv
 * is the caller's 1 / sigma, floored as the caller sees fit).  symmetric != 0 also requires
 * mu_b == mu_a and inv_b == inv_a.  Errors as sv_trial_hist, in its order, with: a null mu / inv
 * pointer or symmetric with different ones SV_EARG; one off a 4-byte boundary SV_EALIGN. */
int sv_trial_hist_norm(const float* A, long lda, const int* lab_a, int Na, const float* B, long ldb, const int* lab_b,
                       int Nb, int D, int symmetric, float lo, float inv_width, int n_bins, const float* mu_a,
                       const float* inv_a, const float* mu_b, const float* inv_b, unsigned long long* hist, int grid,
                       hipStream_t stream);

/* ---- spectral diarization (added under v12; additive): the device steps of Wang et al., "Speaker
 * Diarization with LSTM" (arXiv 1710.10468) on a ragged batch of F files of unit d-vectors
 * (diarization.py has the pipeline; sv_diar.hip the kernel plans).
 *   Layout: file f owns the rows row_off[f] .. row_off[f + 1] (device int32 [F + 1], n_f rows) of every
 *   [sum n][.] array, and an n_f x n_f fp32 matrix with leading dimension ld_f = (n_f + 3) & ~3 at
 *   element mat_off[f] (device 64-bit [F], multiples of 4) of every packed matrix buffer.  Every
 *   function that writes a matrix writes zeros into its columns n_f .. ld_f - 1, so the matrix is a
 *   k-contiguous sv_gemm_f32 operand with K = ld_f.  n_max: an upper bound of the n_f, given by the
 *   host; it sizes the grids, and rows past it are not processed.
 *   No function waits between workgroups; every stage boundary is a launch boundary on `stream`.
 *
 * sv_diar_crop_blur: A_ii := max_{j != i} A_ij, then B = W A W^T with W_ij = g(|i - j|) / c_i for
 *   |i - j| <= r, c_i the sum of row i's in-range taps (edges renormalise, nothing is padded).
 *   taps: HOST pointer to the r + 1 values g(0) .. g(r); r = 0 with g(0) = 1 is W = I.  A is overwritten
 *   (it holds the row pass's result).  |B - exact| <= ((2 r + 1)^2 + 8) 2^-24 max|A|.
 * sv_diar_row_select: tau[row_off[f] + i] = the element of ascending rank q[f] (0-based, device int32
 *   [F], clamped to [0, n_f - 1]) of row i of B: an exact radix select on the order-preserving key of
 *   sv_cohort_topk_stats, ties included; a NaN sorts above +inf.
 * sv_diar_thresh_sym: Y_ij = fmaxf(T_ij, T_ji) with T_ij = B_ij >= tau_i ? B_ij : mult * B_ij (one fp32
 *   multiplication).  Y must not be B.
 * sv_diar_row_norm: d_i = max_j Z_ij (exact), r_i = 1 / sqrt(d_i) in fp64, or 0 if d_i <= 0, and
 *   S_ij = Z_ij (r_i r_j), the product formed in fp64 and rounded once: |S - exact| <= 2^-24 |S|, S is
 *   symmetric bit for bit where Z is, and a row with d_i <= 0 gives a zero row and column.  r: [sum n]
 *   doubles (output).  S may be Z.
 * sv_diar_spmm: P = S (W T) for W, P [sum n][SV_DIAR_M] fp32 and T [F][16][16] fp64 row-major: the
 *   operand Q = W T is formed on the fly (fp64 products, rounded to fp32), the products S Q on the
 *   exact fp32 MFMA in a fixed order.  S is read once.  P must not be W.
 * sv_diar_gram: G[f] = X_f^T Y_f, [F][16][16] fp64, from fp32 X, Y [sum n][16]: fp64 products and sums,
 *   256-row blocks and then the blocks in ascending order through `workspace` (sv_diar_workspace bytes;
 *   no floating-point atomics: the same input gives the same bits).
 * sv_diar_rmul: Y = X T (fp64 products, rounded once).  With P != NULL also res2[f][j] = the squared
 *   norm of column j of P_f T_f - Y_f diag(lam[f]) ([F][16] fp64 each), summed in the same two levels;
 *   P NULL: lam, res2 and workspace are not used.  Y must be neither X nor P.
 * sv_diar_kmeans: Lloyd's algorithm on the rows of E [sum n][16] (unused columns zero), one workgroup
 *   per file, k[f] (device int32, clamped to [1, min(16, n_f)]) centres.  Start: row 0, then
 *   repeatedly the row whose fp32 squared distance to the nearest chosen centre is largest (ties: the
 *   lowest row).  A pass assigns every row to its nearest centre (ties: the lowest centre); if a
 *   label changed, every non-empty cluster's centre becomes the mean of its rows (fp64 sum in row
 *   order, rounded once; an empty cluster keeps its centre) and the next pass runs, up to max_iter
 *   passes.  labels [sum n] int32 (centre indices), iters [F] the passes that ran.
 * SV_EARG: a null pointer (P of sv_diar_rmul may be NULL); F or n_max < 1; r < 0; max_iter < 1; an
 * output that must not alias an input and does.  SV_EALIGN: a matrix, W, P, X / Y of sv_diar_rmul or E
 * off a 16-byte boundary; a 64-bit table or fp64 array off an 8-byte, anything else off a 4-byte one.
 * SV_ESHAPE: n_max > SV_DIAR_MAX_N (a row is staged in LDS); F > 65 535; r > SV_DIAR_MAX_R.  Checked in
 * that order, all before any launch. */
#define SV_DIAR_M 16
#define SV_DIAR_MAX_N 8192
#define SV_DIAR_MAX_R 8
int sv_diar_crop_blur(float* A, float* B, const int* row_off, const long* mat_off, int F, int n_max,
                      const float* taps, int r, hipStream_t stream);
int sv_diar_row_select(const float* B, const int* row_off, const long* mat_off, int F, int n_max, const int* q,
                       float* tau, hipStream_t stream);
int sv_diar_thresh_sym(const float* B, const float* tau, float mult, float* Y, const int* row_off, const long* mat_off,
                       int F, int n_max, hipStream_t stream);
int sv_diar_row_norm(const float* Z, float* S, float* d, double* r, const int* row_off, const long* mat_off, int F,
                     int n_max, hipStream_t stream);
int sv_diar_spmm(const float* S, const float* W, const double* T, float* P, const int* row_off, const long* mat_off,
                 int F, int n_max, hipStream_t stream);
size_t sv_diar_workspace(int F, int n_max);
int sv_diar_gram(const float* X, const float* Y, double* G, double* workspace, const int* row_off, int F, int n_max,
                 hipStream_t stream);
int sv_diar_rmul(const float* X, const double* T, float* Y, const float* P, const double* lam, double* res2,
                 double* workspace, const int* row_off, int F, int n_max, hipStream_t stream);
int sv_diar_kmeans(const float* E, const int* row_off, const int* k, int F, int max_iter, int* labels, int* iters,
                   hipStream_t stream);

/* ---- diarization scoring on a frame grid (added under v12; additive): segment tables to per-frame
 * speaker bit masks, and the masks to the integers of the diarization error rate (diarization.der has
 * the pipeline; sv_der.hip the kernel plans).  Every result is an integer and independent of the order
 * in which workgroups run.
 *   Grid: `step` samples per frame; frame i of a file has its centre at c_i = i * step + step / 2, and
 *   a segment [s, e) in samples covers frame i iff s <= c_i < e.  File f owns the frames frame_off[f] ..
 *   frame_off[f + 1] (device int32 [F + 1]) of every per-frame array; n_total is the length of those
 *   arrays in frames (frame_off[F] for a packed batch), and nothing past it is read or written.
 *
 * sv_seg_raster: mask[frame_off[f] + i] |= seg_bits[k] for every frame i that row k = (seg_start[k],
 *   seg_end[k], seg_bits[k], f = seg_file[k]) covers (device tables of n_seg rows; samples are int32),
 *   clamped to the file's own frames.  A row with seg_file outside [0, F) or seg_end <= seg_start writes
 *   nothing.  The caller zeroes mask (uint32 [n_total]).  One wave per row: the host keeps rows short
 *   (diarization.split_rows); n_seg = 0 is no launch.
 * sv_der_count: out [F][4 + 32 * 32] uint64, overwritten: per file, over its scored frames, with
 *   Nr = popcount(ref), Nh = popcount(hyp): total = sum Nr, miss = sum max(0, Nr - Nh),
 *   fa = sum max(0, Nh - Nr), both = sum min(Nr, Nh), then C[i][j] = the number of scored frames with
 *   bit i of ref and bit j of hyp set.  A frame is scored iff noscore == 0, uem != 0 (uem may be NULL:
 *   every frame) and, with skip_overlap != 0, Nr <= 1.  max_frames: an upper bound of the files' frame
 *   counts, given by the host; it sizes the grid, and frames past it are not counted.
 * SV_EARG: a null pointer (uem may be NULL); F < 1; step < 1; n_seg, max_frames or n_total < 0.
 * SV_EALIGN: a per-frame array of sv_der_count off a 16-byte boundary, out off an 8-byte, anything else
 * off a 4-byte one.  SV_ESHAPE: F > 65 535 (sv_der_count).  All before any launch. */
int sv_seg_raster(const int* seg_start, const int* seg_end, const unsigned* seg_bits, const int* seg_file, int n_seg,
                  const int* frame_off, int F, int step, int n_total, unsigned* mask, hipStream_t stream);
int sv_der_count(const unsigned* ref, const unsigned* hyp, const unsigned* noscore, const unsigned* uem,
                 const int* frame_off, int F, int max_frames, int n_total, int skip_overlap, unsigned long long* out,
                 hipStream_t stream);

/* ---- clip_grad_norm_ + SGD step over one flat parameter group (train_speech_embedder.py:63-65)
 * p -= lr * min(1, max_norm / (|g|_2 + 1e-6)) * g; write_grad=1 also scales g in place.
 * sync (may be NULL): a persistent-recurrence sync block; if its status is set the step is
 * skipped (p and g untouched, total_norm_out = NaN): never a step on invalid gradients. */
size_t sv_clip_sgd_workspace(void);
int sv_clip_sgd_step(float* params, float* grads, long n, float max_norm, float lr, int write_grad,
                     float* total_norm_out, const void* sync, float* workspace, hipStream_t stream);
/* the reference's two parameter groups in one pair of launches (ABI v8): the network's
 * (clip_grad_norm_(net, 3.0), train_speech_embedder.py:63) and the GE2E loss's {w, b}
 * (clip_grad_norm_(ge2e, 1.0), :64), each exactly as sv_clip_sgd_step computes it (bit-identical);
 * total_norm_out (may be NULL): float[2]; workspace: sv_clip_sgd_workspace() * 2 bytes */
int sv_clip_sgd_step2(float* params0, float* grads0, long n0, float max_norm0, float* params1, float* grads1,
                      long n1, float max_norm1, float lr, int write_grad, float* total_norm_out, const void* sync,
                      float* workspace, hipStream_t stream);
/* (ABI v11) sv_clip_sgd_step2 with the training step's status report in its update launch: as
 * sv_status_report(sync, report_x, report_n, host_slot_dev, seq) after it, one launch fewer */
int sv_clip_sgd_step2_report(float* params0, float* grads0, long n0, float max_norm0, float* params1, float* grads1,
                             long n1, float max_norm1, float lr, int write_grad, float* total_norm_out,
                             const void* sync, float* workspace, float* report_x, int report_n, void* host_slot_dev,
                             unsigned seq, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SV_GE2E_H */
