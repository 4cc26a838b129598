// The LSTM layer stack's host-side frame, shared by the fp32 glue (sv_lstm.hip) and the bf16 glue
// (sv_bf16.hip): the validated arguments with what every schedule derives from them, and the
// per-step, layer-pipelined schedule of either direction.  A precision's Fwd / Bwd struct derives
// from Stack and adds one layer's sequences (k1 / reset / steps; region / prepare / steps / dx_gemm /
// grads), each written once and run on the stream it is given; the single-layer entry points run
// those on a stack of one layer.
#pragma once
#include <algorithm>
#include "sv_common.h"

inline int record(hipEvent_t e, hipStream_t s) { return (int)hipEventRecord(e, s); }
inline int stream_wait(hipStream_t s, hipEvent_t e) { return (int)hipStreamWaitEvent(s, e, 0); }

// The shape and scheduling arguments of a stack entry point (named as in the signatures).
// PAD: the batch padding of the transposed layouts (4 for fp32, 8 for bf16: 16-byte rows).
template <int PAD>
struct Stack {
  int L, T, B, F, H, chunk;
  hipStream_t main;
  const hipStream_t* side;
  hipEvent_t *ev, *probe;
  int products, schedule;
  unsigned* sync;
  // derived: chunks; B rounded up to PAD, the column block of hT [H, (T+1) Bp] and dgT [4H, T Bp]
  int nch = (T + chunk - 1) / chunk, Bp = (B + PAD - 1) & ~(PAD - 1), TBp = T * Bp;
  long BH = (long)B * H, BG = 4L * B * H, ldhT = (long)(T + 1) * Bp;
  int Fl(int l) const { return l == 0 ? F : H; }
  int t0(int c) const { return c * chunk; }
  int t1(int c) const { return std::min(T, (c + 1) * chunk); }
  // ev: chunk c of layer l done | the forward's fork from main | backward layer l done | the
  // backward's fork (forward L nch + 1 events, backward L nch + L + 1)
  hipEvent_t chunk_done(int l, int c) const { return ev[l * nch + c]; }
  hipEvent_t fwd_start() const { return ev[L * nch]; }
  hipEvent_t layer_done(int l) const { return ev[L * nch + l]; }
  hipEvent_t bwd_start() const { return ev[L * nch + L]; }
  // probe (or NULL) in pairs: persistent, 2 L events, pair l around layer l's launch; per-step
  // fp32 backward, 2 L nch events, pair (l, c) around one K3 launch of layer l's chunk c
  hipEvent_t* layer_probe(int l) const { return probe ? probe + 2 * l : nullptr; }
  hipEvent_t* chunk_probe(int l, int c) const { return probe ? probe + 2 * (l * nch + c) : nullptr; }
};

// Per-step forward, layer-pipelined: layer l runs on side[l], its timesteps in chunks of `chunk`,
// and waits only for the layer below to finish the same chunk, so up to L layers' kernels run at
// once and one layer's latency-bound step kernels overlap another's GEMMs; joins back into `main`.
template <class F>
int stack_fwd_per_step(const F& a) {
  int rc = record(a.fwd_start(), a.main);
  for (int l = 0; l < a.L && !rc; ++l)
    if (!(rc = stream_wait(a.side[l], a.fwd_start()))) rc = a.reset(l, a.side[l]);
  if (rc) return rc;
  // wavefront issue order: chunk c of layer l after chunk c of layer l-1 on the host too
  for (int d = 0; d < a.nch + a.L - 1; ++d)
    for (int l = 0; l < a.L; ++l) {
      const int c = d - l;
      if (c < 0 || c >= a.nch) continue;
      hipStream_t s = a.side[l];
      if (l > 0 && (rc = stream_wait(s, a.chunk_done(l - 1, c)))) return rc;
      if ((rc = a.k1(l, a.t0(c), a.t1(c), s)) || (rc = a.steps(l, a.t0(c), a.t1(c), s))) return rc;
      if ((rc = record(a.chunk_done(l, c), s))) return rc;
    }
  for (int l = 0; l < a.L && !rc; ++l) rc = stream_wait(a.main, a.chunk_done(l, a.nch - 1));
  return rc;
}

// Per-step backward, top layer first in issue order: layer l's timesteps in reverse chunks (the
// recurrent steps, then -- for l > 0 -- the chunk's dx = dG W_ih GEMM, the next-lower layer's dh_up
// for those timesteps), then its whole-T weight-gradient GEMMs and bias row sums behind the
// recurrence on the same stream; layer l-1 waits only for layer l's dx of the same chunk, so one
// layer's recurrence overlaps the upper layers' GEMMs.
template <class B>
int stack_bwd_per_step(const B& a) {
  int rc = record(a.bwd_start(), a.main);
  for (int l = a.L - 1; l >= 0 && !rc; --l) {
    hipStream_t s = a.side[l];
    const auto ws = a.region(l);
    if ((rc = stream_wait(s, a.bwd_start())) || (rc = a.prepare(l, ws, l > 0, true, s))) return rc;
    for (int c = a.nch - 1; c >= 0; --c) {
      if (l < a.L - 1 && (rc = stream_wait(s, a.chunk_done(l + 1, c)))) return rc;
      rc = a.steps(l, ws, a.t0(c), a.t1(c), s, a.chunk_probe(l, c));
      if (!rc && l > 0) rc = a.dx_gemm(l, ws, a.t0(c), a.t1(c), s);  // dh_up of layer l-1 for this chunk
      if (rc || (rc = record(a.chunk_done(l, c), s))) return rc;
    }
    // whole-T weight gradients and bias row sums behind the recurrence, on its stream
    if (!(rc = a.grads(l, ws, true, s))) rc = record(a.layer_done(l), s);
  }
  for (int l = 0; l < a.L && !rc; ++l) rc = stream_wait(a.main, a.layer_done(l));
  return rc;
}
