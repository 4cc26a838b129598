"""Torch-facing wrappers over the C ABI (include/sv_ge2e.h).

PyTorch supplies device memory (caching allocator), the current HIP stream and autograd
plumbing; every FLOP of the path runs in the HIP kernels of libsv_ge2e.so.

  embedder_forward / embedder_backward   SpeechEmbedder.forward (speech_embedder_net.py:27-33)
                                         and its backward: 3-layer LSTM + Linear + L2 norm
  embedder_forward_bf16 / _backward_bf16 the same with bf16 GEMM operands
  embedder_fwd / embedder_bwd            either pair, chosen by a `precision` argument
  ge2e_forward / ge2e_backward           GE2ELoss.forward (speech_embedder_net.py:43-49)
  EmbedderFunction, GE2EFunction         autograd.Function glue (loss.backward() works)
  clip_sgd_step_                         clip_grad_norm_ + SGD.step (train_speech_embedder.py:63-65)
  clip_sgd_step2_                        the same over both parameter groups in one launch pair
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import (SV_DTYPE_BF16, SV_DTYPE_F32, SV_SCHED_CNT_READY, SV_SCHED_NO_EVENTS, SV_SCHED_WT_READY,
                   PersistStatus, call, call_as, lib, loss_id, ptr, require_device, schedule_flags, stream_of)
from .data_load import CorpusBatch

# timesteps per chunk of the layer-pipelined schedules (measured at c2: 16 / 24 / 32 / 48 / 64 ->
# 69.3 / 69.7 / 69.1 / 69.5 / 69.6 ms per step)
PIPELINE_CHUNK = 32

# how the fp32 path forms its products (the `products` argument of the C ABI, include/sv_ge2e.h):
# "mfma_f32" (default, exact fp32 MFMA) or "bf16x6" (three-way bf16 split, six bf16 MFMA products
# per fp32 product, fp32 accumulation).  Per call, never process-wide.
F32_PRODUCT_MODES = {"mfma_f32": 0, "bf16x6": 1}


def _products(mode):
    try:
        return F32_PRODUCT_MODES[mode or "mfma_f32"]
    except KeyError:
        raise ValueError(f"unknown fp32 product mode {mode!r} (expected one of {sorted(F32_PRODUCT_MODES)})") from None


# sync blocks of bf16 calls made without a caller-owned one (autograd path): their status is
# checked (non-blocking) at the next call and by check_persistent_status()
_UNCHECKED = []


def _own_status(status, device):
    if status is not None:
        return status, False
    check_persistent_status()
    return PersistStatus(device), True


def _release_status(st, own):
    if own:
        st.arm()
        _UNCHECKED.append(st)


def check_persistent_status(wait=False):
    """Raise PersistentRecurrenceError if a persistent recurrence of an earlier call (made
    without a caller-owned sync block) timed out; wait=True waits for all of them first."""
    global _UNCHECKED
    pending = _UNCHECKED
    _UNCHECKED = []
    err = None
    for st in pending:
        try:
            st.poll(wait=wait)
        except RuntimeError as e:
            err = err or e
        if st._pending:
            _UNCHECKED.append(st)
    if err:
        raise err


class _StreamPool:
    """Side streams + events for the layer-pipelined schedules, one set per (device, role): the
    forward and the backward of a step keep separate sets, and a set only ever grows -- an event
    a call recorded is never destroyed while later work on `main` may still wait on it."""
    _pools = {}

    @classmethod
    def get(cls, device, role, n_streams, n_events):
        key = (device.index, role, n_streams)
        p = cls._pools.get(key)
        if p is None:
            p = ([torch.cuda.Stream(device=device) for _ in range(n_streams)], [])
            cls._pools[key] = p
        streams, events = p
        if len(events) < n_events:
            with torch.cuda.device(device):
                for _ in range(n_events - len(events)):
                    e = torch.cuda.Event()
                    e.record()  # materialise the native event
                    events.append(e)
        return p


def _parr(ts):
    return (ctypes.c_void_p * len(ts))(*[ptr(t) if t is not None else None for t in ts])


def _evarr(events):
    """Host array of native HIP events (timing probes), or NULL."""
    if not events:
        return None
    return (ctypes.c_void_p * len(events))(*[e.cuda_event for e in events])


def _ws(nbytes, device):
    """Workspace of at least nbytes (fp32 storage, 256-byte aligned by the allocator)."""
    n = max(1, (int(nbytes) + 3) // 4)
    return torch.empty(n, dtype=torch.float32, device=device)


# ----------------------------------------------------------------------------- LSTM stack
class EmbedderState:
    """Activations saved by the forward for the backward (all time-major; fp32, under bf16 the GEMM
    operands x_tm / gates / hT / xT0 in bf16)."""

    def __init__(self):
        self.x_tm = []      # per layer input [T,B,F_l]
        self.gates = []     # per layer [T,B,4H] activated i,f,g,o
        self.c_tm = []      # per layer [T,B,H]
        self.h_tm = []      # per layer [T+1,B,H]
        self.hT = []        # per layer [H,(T+1)B]  (h^T, column block t+1 = h_t, block 0 = 0)
        self.xT0 = None     # layer-0 input transposed [F, T*B]
        self.y = self.emb = self.ynorm = self.h_last = None
        self.T = self.B = self.H = self.P = 0
        self.bf16 = False
        self.wt = None      # bf16, L > 1: the stack backward's weight transposes (sv_lstm_wt_bf16_size bytes)


def _f32(shape, dev):
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _bf(shape, dev):
    return torch.empty(shape, dtype=torch.bfloat16, device=dev)


def _proj_norm_fwd(st, h_last, w_p, b_p, s):
    """Projection + L2 norm of h_last [B,H] (sv_proj_norm_fwd), saved into st; returns emb [B,P]."""
    B, H, P, dev = st.B, st.H, st.P, h_last.device
    y, emb, ynorm = _f32((B, P), dev), _f32((B, P), dev), _f32((B,), dev)
    ws = _ws(lib().sv_proj_norm_workspace(B, H, P), dev)
    call("sv_proj_norm_fwd", ptr(h_last), B, H, P, ptr(w_p), ptr(b_p), ptr(y), ptr(emb), ptr(ynorm), ptr(ws), s)
    st.y, st.emb, st.ynorm, st.h_last = y, emb, ynorm, h_last
    return emb


def _proj_norm_bwd(st, demb, layers, w_p, grads, s):
    """Backward of _proj_norm_fwd into the projection's two of ``grads`` (allocated here if None, in
    parameter order [w_ih, w_hh, b_ih, b_hh]*L + [w_p, b_p]); returns (grads, dh_last [B,H])."""
    B, H, P, L, dev = st.B, st.H, st.P, len(layers), demb.device
    if grads is None:
        grads = [torch.empty_like(t) for l in layers for t in l] + [torch.empty_like(w_p), _f32((P,), dev)]
    dh_last = _f32((B, H), dev)
    ws = _ws(lib().sv_proj_norm_workspace(B, H, P), dev)
    call("sv_proj_norm_bwd", ptr(demb), ptr(st.emb), ptr(st.ynorm), ptr(st.h_last), B, H, P, ptr(w_p),
         ptr(grads[4 * L]), ptr(grads[4 * L + 1]), ptr(dh_last), ptr(ws), s)
    return grads, dh_last


def _side(dev, role, L, nev):
    """The (device, role) pool's L side streams and first nev events as host arrays, and its events."""
    streams, events = _StreamPool.get(dev, role, L, nev)
    sp = (ctypes.c_void_p * L)(*[st_.cuda_stream for st_ in streams])
    ep = (ctypes.c_void_p * nev)(*[e.cuda_event for e in events[:nev]])
    return sp, ep, events


def _stack_fwd(dtype, x_tm, w_ih, w_hh, layers, gs, cs, hs, hbs, hTs, prod, sched, status, probe, s):
    """sv_lstm_fwd of L > 1 layers: x_tm, w_ih, w_hh, gs, hTs (and hbs, bf16 only) in ``dtype``."""
    T, B, F = x_tm.shape
    L, H, dev = len(layers), cs[0].shape[2], x_tm.device
    nch = (T + PIPELINE_CHUNK - 1) // PIPELINE_CHUNK
    sp, ep, _ = _side(dev, "fwd", L, L * nch + 1)
    sync, own = _own_status(status, dev)
    call("sv_lstm_fwd", dtype, L, T, B, F, H, ptr(x_tm), _parr(w_ih), _parr(w_hh), _parr([l[2] for l in layers]),
         _parr([l[3] for l in layers]), _parr(gs), _parr(cs), _parr(hs), _parr(hbs) if hbs else None, _parr(hTs),
         PIPELINE_CHUNK, s, sp, ep, prod, sched, sync.ptr(), _evarr(probe))
    if dtype == SV_DTYPE_BF16:  # (the bf16 stack forward zeroes the backward's channels, every schedule)
        sync.bwd_counters_clean = True
    _release_status(sync, own)


def _stack_bwd(dtype, st, layers, grads, dh_last, dgs, dgTs, ws, wt, prod, sched, status, probe, kstamp, grad_ready,
               late_head, s):
    """sv_lstm_bwd of L > 1 layers (no input gradient): dgs / dgTs [4H, T*Bp] in ``dtype``, ws its
    scratch, wt the bf16 weight transposes (None for fp32).  Then the layers' grad_ready calls, each
    behind the event the library recorded for it; late_head: the projection's too."""
    T, B, H, L, dev = st.T, st.B, st.H, len(layers), dh_last.device
    F0 = st.x_tm[0].shape[2]
    Bp, esz = dgTs[0].shape[1] // T, dgTs[0].element_size()
    dxs = [None] + [_f32((T, B, H), dev) for _ in range(L - 1)]
    # layer l's input transposed: x^T, then the layer below's h^T from column block 1 (= h_0 .. h_{T-1})
    xT = [ptr(st.xT0)] + [ptr(st.hT[l - 1]) + Bp * esz for l in range(1, L)]
    ld = [T * Bp] + [(T + 1) * Bp] * (L - 1)
    nch = (T + PIPELINE_CHUNK - 1) // PIPELINE_CHUNK
    sp, ep, events = _side(dev, "bwd", L, L * nch + L + 1)
    sync, own = _own_status(status, dev)
    if dtype == SV_DTYPE_BF16:
        if sync.bwd_counters_clean:  # the forward zeroed the backward's counters, none used since
            sched |= SV_SCHED_CNT_READY
        sync.bwd_counters_clean = False
    call("sv_lstm_bwd", dtype, L, T, B, F0, H, (ctypes.c_void_p * L)(*xT), (ctypes.c_long * L)(*ld),
         _parr([l[0] for l in layers]), _parr([l[1] for l in layers]), _parr(st.gates), _parr(st.c_tm),
         _parr(st.hT), ptr(dh_last), _parr(dgs), _parr(dgTs), _parr(dxs),
         _parr([grads[4 * l] for l in range(L)]), _parr([grads[4 * l + 1] for l in range(L)]),
         _parr([grads[4 * l + 2] for l in range(L)]), _parr([grads[4 * l + 3] for l in range(L)]), ptr(ws), ptr(wt),
         PIPELINE_CHUNK, s, sp, ep, prod, _evarr(probe), ptr(kstamp), sched, sync.ptr())
    _release_status(sync, own)
    if grad_ready:
        if late_head:
            # behind the event the library records right after the last recurrence (the status word
            # is final there, and with the persistent recurrences a collective must not run beside
            # them), not behind all of main: the buckets then overlap layer 0's dx / dW GEMMs
            grad_ready(L, events[L * nch + L - 1])
        for l in range(L - 1, -1, -1):
            grad_ready(l, events[L * nch + l])


def _dx_batch_first(dx, s):
    """dx [T,B,F] time-major -> [B,T,F]."""
    T, B, F = dx.shape
    dxb = _f32((B, T, F), dx.device)
    call("sv_frames_to_time_major", ptr(dx), ptr(dxb), T, B, F, s)
    return dxb


def _corpus_batch(x):
    """x if it is a data_load.CorpusBatch (a batch still in the resident corpus), None for a tensor."""
    return x if isinstance(x, CorpusBatch) else None


def _corpus_prep(entry, cb, x_out, xT, Bp, s):
    """sv_corpus_batch / sv_corpus_batch_bf16: layer 0's operands x_out [T,B,F] and xT [F, T*Bp] (or
    None) of the batch cb, cut out of its corpus in one launch on the step's stream s."""
    data = cb.corpus.data
    require_device(data)
    _check_i32_table(cb.utt, "utt")
    _check_i32_table(cb.start, "start")
    if cb.utt.shape != cb.start.shape or cb.utt.device != data.device or cb.start.device != data.device:
        raise RuntimeError("CorpusBatch: utt and start must be [B] tables on the corpus' device")
    B, T, F = cb.shape
    call(entry, ptr(data), data.shape[0], F, data.shape[2], ptr(cb.utt), ptr(cb.start), B, T, ptr(x_out), ptr(xT), Bp,
         s)


def embedder_forward(x, layers, w_p, b_p, save=True, products="mfma_f32", status=None, probe=None, schedule="auto"):
    """x [B,T,F] float32 (batch_first), or a data_load.CorpusBatch of that shape (its operands are
    then cut out of the resident corpus by sv_corpus_batch, bit-identical to those of
    x = batch.frames()); layers = [(w_ih, w_hh, b_ih, b_hh)] * L.
    Returns (emb [B,P], state).  products: fp32 product mode of the stack (F32_PRODUCT_MODES).
    schedule: 'auto' (the persistent recurrences where they fill the device, sv_lstm_f32_persist_ok),
    'per_step' (layer-pipelined K2 steps) or 'persist'; status: the caller's PersistStatus (sync
    block of the persistent recurrences; None = a fresh one, checked at the next call / by
    check_persistent_status()); probe: 2*L events around the layers' persistent launches."""
    prod = _products(products)
    sched = schedule_flags(schedule)
    cb = _corpus_batch(x)
    require_device(None if cb else x, w_p, b_p, *[t for l in layers for t in l])
    B, T, F = x.shape
    H = layers[0][1].shape[1]
    L = len(layers)
    dev = x.device
    s = stream_of(x)
    if prod and L == 1:
        raise ValueError("the bf16x6 product mode runs on the layer-pipelined stack only (L > 1)")
    st = EmbedderState()
    st.T, st.B, st.H, st.P = T, B, H, w_p.shape[0]
    x_tm = _f32((T, B, F), dev)
    Bp = (B + 3) // 4 * 4
    if cb:  # x_tm and x^T from the corpus in one launch (the padding columns are the kernel's)
        st.xT0 = _f32((F, T * Bp), dev) if save else None
        _corpus_prep("sv_corpus_batch", cb, x_tm, st.xT0, Bp, s)
    else:
        call("sv_frames_to_time_major", ptr(x), ptr(x_tm), B, T, F, s)
    if save and not cb:  # layer-0 input transposed, [F, T*Bp] (column block t = x_t^T, padding columns zero)
        if Bp == B:
            st.xT0 = _f32((F, T * B), dev)
            call("sv_transpose", ptr(x_tm), F, T * B, F, ptr(st.xT0), T * B, s)
        else:
            st.xT0 = torch.zeros((F, T * Bp), dtype=torch.float32, device=dev)
            for t in range(T):
                call("sv_transpose", ptr(x_tm[t]), F, B, F, ptr(st.xT0) + 4 * t * Bp, T * Bp, s)
    gs = [_f32((T, B, 4 * H), dev) for _ in range(L)]
    cs = [_f32((T, B, H), dev) for _ in range(L)]
    hs = [_f32((T + 1, B, H), dev) for _ in range(L)]
    hTs = [_f32((H, (T + 1) * Bp), dev) if save else None for _ in range(L)]
    if L > 1:
        _stack_fwd(SV_DTYPE_F32, x_tm, [l[0] for l in layers], [l[1] for l in layers], layers, gs, cs, hs, None, hTs,
                   prod, sched, status, probe, s)
    else:
        w_ih, w_hh, b_ih, b_hh = layers[0]
        call("sv_lstm_layer_fwd", ptr(x_tm), T, B, F, H, ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), ptr(gs[0]),
             ptr(cs[0]), ptr(hs[0]), ptr(hTs[0]), s)
    if save:
        st.x_tm = [x_tm] + [h[1:] for h in hs[:-1]]
        st.gates, st.c_tm, st.h_tm, st.hT = gs, cs, hs, hTs
    return _proj_norm_fwd(st, hs[-1][T], w_p, b_p, s), st


def embedder_backward(st, demb, layers, w_p, grads=None, need_dx=False, grad_ready=None, products="mfma_f32",
                      probe=None, kstamp=None, status=None, schedule="auto"):
    """Backward of embedder_forward.  ``grads`` (optional) is a list of preallocated
    output tensors in parameter order [w_ih, w_hh, b_ih, b_hh]*L + [w_p, b_p]; returns it
    (and dx [B,T,F] if need_dx).

    ``grad_ready(k, event)`` (optional) is called as soon as a gradient group is enqueued:
    k = L for the projection, then k = L-1 .. 0 for the LSTM layers; ``event`` is the HIP
    event that completes it (None: the current stream).  The data-parallel trainer hangs its
    per-layer all-reduce buckets on it so communication overlaps the rest of the BPTT.

    ``probe`` (optional): 2*L*ceil(T/chunk) timing events recorded around one recurrent-step
    launch per chunk; ``kstamp`` (optional): int64 device tensor of 2*L*T slots, pairs preset
    to (-1, 0), set by every recurrent-step launch (l, t) to its start / end on the GPU's 100 MHz
    real-time clock (include/sv_ge2e.h, sv_lstm_stack_bwd).  Under the persistent schedule
    (``schedule``, ``status`` as embedder_forward) probe[2l] / [2l+1] bracket layer l's launch and
    kstamp is not written."""
    prod = _products(products)
    # no grad_ready: nothing waits on the per-layer completion events, so the persistent
    # schedule records none (include/sv_ge2e.h SV_SCHED_NO_EVENTS)
    sched = schedule_flags(schedule) | (0 if grad_ready else SV_SCHED_NO_EVENTS)
    demb = demb.contiguous()
    require_device(demb)
    T, B, H = st.T, st.B, st.H
    dev = demb.device
    s = stream_of(demb)
    L = len(layers)
    grads, dh_last = _proj_norm_bwd(st, demb, layers, w_p, grads, s)
    stacked = L > 1 and not need_dx
    # under the persistent schedule the projection bucket is enqueued behind the stack backward
    # (a collective must not run beside a persistent launch); else it overlaps the BPTT
    with torch.cuda.device(dev):  # (the library answers for the current device)
        late_head = stacked and bool(lib().sv_lstm_f32_persist_ok(B, H, sched))
    if grad_ready and not late_head:
        grad_ready(L, None)
    if prod and not stacked:
        raise ValueError("the bf16x6 product mode runs on the layer-pipelined stack only")
    Bp = (B + 3) // 4 * 4
    if stacked:
        ws = _ws(lib().sv_lstm_bwd_workspace(SV_DTYPE_F32, L, T, B, st.x_tm[0].shape[2], H), dev)
        dgs = [_f32((T, B, 4 * H), dev) for _ in range(L)]
        dgTs = [_f32((4 * H, T * Bp), dev) for _ in range(L)]
        _stack_bwd(SV_DTYPE_F32, st, layers, grads, dh_last, dgs, dgTs, ws, None, prod, sched, status, probe, kstamp,
                   grad_ready, late_head, s)
        return grads
    Fmax = max(st.x_tm[l].shape[2] for l in range(L))
    ws = _ws(lib().sv_lstm_layer_bwd_workspace(T, B, Fmax, H), dev)
    dgates = _f32((T, B, 4 * H), dev)
    dgT = _f32((4 * H, T * Bp), dev)
    dh_up, full = dh_last, 0
    for l in range(L - 1, -1, -1):
        w_ih, w_hh, _, _ = layers[l]
        Fl = st.x_tm[l].shape[2]
        dx = _f32((T, B, Fl), dev) if (l > 0 or need_dx) else None
        if l == 0:
            xT, ld_xT = ptr(st.xT0), T * Bp
        else:  # previous layer's h^T, column blocks 1..T (= h_0 .. h_{T-1})
            xT, ld_xT = ptr(st.hT[l - 1]) + Bp * 4, (T + 1) * Bp
        call("sv_lstm_layer_bwd", T, B, Fl, H, xT, ld_xT, ptr(w_ih), ptr(w_hh), ptr(st.gates[l]),
             ptr(st.c_tm[l]), ptr(st.hT[l]), ptr(dh_up), full, ptr(dgates), ptr(dgT), ptr(dx), ptr(grads[4 * l]),
             ptr(grads[4 * l + 1]), ptr(grads[4 * l + 2]), ptr(grads[4 * l + 3]), ptr(ws), s)
        if grad_ready:
            grad_ready(l, None)
        dh_up, full = dx, 1
    return (grads, _dx_batch_first(dh_up, s)) if need_dx else grads


# ----------------------------------------------------------------------------- bf16 operands
def embedder_forward_bf16(x, layers, w_p, b_p, save=True, status=None, probe=None, schedule="auto"):
    """Mixed-precision forward (BASELINE config c3): bf16 GEMM operands, fp32 accumulation,
    bf16 storage of the x-projection and of the activated gates saved for the backward, fp32
    cell state / projection / norm.  Same outputs as embedder_forward.
    status: the caller's PersistStatus (sync block of the persistent recurrences); None = a
    fresh one, checked at the next call / check_persistent_status().  probe: 2*L timing events
    around the layers' persistent recurrences (include/sv_ge2e.h).  schedule: 'auto' (default),
    'per_layer', 'per_step' or 'persist' (the SV_SCHED_* flags of include/sv_ge2e.h).
    x may be a data_load.CorpusBatch: sv_corpus_batch_bf16 then writes x_bf and x^T from the resident
    corpus (bit-identical to the frames' part on batch.frames()), followed by sv_lstm_weights_bf16."""
    sched = schedule_flags(schedule)
    cb = _corpus_batch(x)
    require_device(None if cb else x, w_p, b_p, *[t for l in layers for t in l])
    B, T, F = x.shape
    H = layers[0][1].shape[1]
    dev = x.device
    s = stream_of(x)
    Bp = (B + 7) // 8 * 8
    st = EmbedderState()
    st.T, st.B, st.H, st.P, st.bf16 = T, B, H, w_p.shape[0], True
    x_bf = _bf((T, B, F), dev)
    L = len(layers)
    # x -> time-major bf16 and x^T: in the weights' launch below (sv_lstm_prep_bf16)
    fused_x = F <= 64 and not cb
    if save:  # layer 0's dW_ih operand x^T [F][T Bp] (padding columns zero)
        st.xT0 = (torch.empty if cb or fused_x or Bp == B else torch.zeros)((F, T * Bp), dtype=torch.bfloat16,
                                                                           device=dev)
    if cb:
        _corpus_prep("sv_corpus_batch_bf16", cb, x_bf, st.xT0, Bp, s)
    elif not fused_x:
        x_tm = _f32((T, B, F), dev)
        call("sv_frames_to_time_major", ptr(x), ptr(x_tm), B, T, F, s)
        if save:
            if Bp == B:
                call("sv_transpose_cast_bf16", ptr(x_tm), F, T * B, F, ptr(st.xT0), T * B, s)
            else:
                for t in range(T):
                    call("sv_transpose_cast_bf16", ptr(x_tm[t]), F, B, F, ptr(st.xT0) + 2 * t * Bp, T * Bp, s)
        call("sv_cast_bf16", ptr(x_tm), ptr(x_bf), x_tm.numel(), s)
    # every layer's bf16 weights in one launch (sv_lstm_weights_bf16); when the stacked backward
    # follows, also its weight transposes, into the buffer st.wt it will be handed
    # (SV_SCHED_WT_READY: the backward launches no transposes)
    wbf = [(_bf(w_ih.shape, dev), _bf(w_hh.shape, dev)) for (w_ih, w_hh, _, _) in layers]
    if save and L > 1:
        st.wt = _ws(lib().sv_lstm_wt_bf16_size(L, F, H), dev)
    wargs = (_parr([l[0] for l in layers]), _parr([l[1] for l in layers]), _parr([w[0] for w in wbf]),
             _parr([w[1] for w in wbf]), ptr(st.wt), s)
    if fused_x:  # the frames' part in the same launch
        call("sv_lstm_prep_bf16", L, T, B, F, H, ptr(x), ptr(x_bf), ptr(st.xT0), Bp, *wargs)
    else:
        call("sv_lstm_weights_bf16", L, F, H, *wargs)
    gs = [_bf((T, B, 4 * H), dev) for _ in range(L)]  # bf16 x-projection in, bf16 activations out
    cs = [_f32((T, B, H), dev) for _ in range(L)]
    hs = [_f32((T + 1, B, H), dev) for _ in range(L)]
    hbs = [_bf((T + 1, B, H), dev) for _ in range(L)]
    hTs = [_bf((H, (T + 1) * Bp), dev) if save else None for _ in range(L)]
    if L > 1:
        _stack_fwd(SV_DTYPE_BF16, x_bf, [w[0] for w in wbf], [w[1] for w in wbf], layers, gs, cs, hs, hbs, hTs, 0,
                   sched, status, probe, s)
    else:
        call("sv_lstm_layer_fwd_bf16", ptr(x_bf), T, B, F, H, ptr(wbf[0][0]), ptr(wbf[0][1]), ptr(layers[0][2]),
             ptr(layers[0][3]), ptr(gs[0]), ptr(cs[0]), ptr(hs[0]), ptr(hbs[0]), ptr(hTs[0]), s)
    if save:
        st.x_tm = [x_bf] + [h[1:] for h in hbs[:-1]]
        st.gates, st.c_tm, st.h_tm, st.hT = gs, cs, hs, hTs
    return _proj_norm_fwd(st, hs[-1][T], w_p, b_p, s), st


def _dvec_bf16(entry, src, B, T, F, layers, w_p, b_p):
    """The shared body of the two sv_dvector_embed_bf16* wrappers: `src` is the entry point's input
    arguments (between L and the weight arrays), a tuple of tensors and ints whose first member
    gives the device and the stream."""
    require_device(src[0], w_p, *[t for l in layers for t in l if t is not None])
    H = layers[0][1].shape[1]
    P = w_p.shape[0]
    L = len(layers)
    emb = torch.empty((B, P), dtype=torch.float32, device=src[0].device)
    ws = _ws(lib().sv_dvector_bf16_workspace(B, T, F, H, L, P), src[0].device)
    ts = [[l[i].contiguous() if l[i] is not None else None for l in layers] for i in range(4)]  # kept alive
    wih, whh, bih, bhh = (_parr(t) for t in ts)
    call(entry, B, T, F, H, L, *[ptr(a) if torch.is_tensor(a) else a for a in src], wih, whh, bih, bhh,
         ptr(w_p.contiguous()), ptr(b_p) if b_p is not None else None, P, ptr(emb), ptr(ws), stream_of(src[0]))
    return emb


def embedder_forward_dvec_bf16(x, layers, w_p, b_p):
    """Embeddings [B, P] of B windows x [B, T, F] (fp32, batch-first) by sv_dvector_embed_bf16:
    the c3 forward's numerics (bf16 GEMM operands, bf16 input projection with its biases, fp32
    accumulation / state / projection) as one 256 x 256 GEMM launch per timestep and layer with the
    LSTM cell in its epilogue -- the large-batch d-vector path (dvector_create.py:96-101), no
    activations saved and no co-residency requirement."""
    B, T, F = x.shape
    return _dvec_bf16("sv_dvector_embed_bf16", (x.contiguous(),), B, T, F, layers, w_p, b_p)


def _check_i32_table(t, name):
    if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 1:
        raise RuntimeError(f"{name} must be a contiguous 1-D int32 tensor on the GPU")


def embedder_forward_dvec_bf16_frames(frames, win_start, layers, w_p, b_p):
    """embedder_forward_dvec_bf16 with the windows read in place (sv_dvector_embed_bf16_frames):
    frames [n_rows, F] fp32 are time-major log-mel rows (features.logmel's out), win_start [B]
    int32 on the same device the first row of every window; window b, step t is row
    win_start[b] + t (T = dvector.WIN rows, clamped into frames).  No [B, T, F] window tensor is
    built; the embeddings [B, P] are bit-identical to embedder_forward_dvec_bf16 on the
    materialised windows at the same B."""
    from .dvector import WIN
    _check_i32_table(win_start, "win_start")
    n_rows, F = frames.shape
    return _dvec_bf16("sv_dvector_embed_bf16_frames", (frames, n_rows, win_start), win_start.shape[0], WIN, F, layers,
                      w_p, b_p)


def dvec_align(emb, part_off):
    """Rows part_off[p] : part_off[p + 1] of emb [S, P] (fp32) averaged into out [n_parts, P]
    float64 on the device (sv_dvec_align; part_off a device int32 tensor of n_parts + 1 offsets):
    equal to np.average of each float32 row block, i.e. to dvector.align_embeddings, exactly."""
    require_device(emb)
    _check_i32_table(part_off, "part_off")
    S, P = emb.shape
    n_parts = part_off.shape[0] - 1
    out = torch.empty((n_parts, P), dtype=torch.float64, device=emb.device)
    call("sv_dvec_align", ptr(emb), S, P, ptr(part_off), n_parts, ptr(out), stream_of(emb))
    return out


def embedder_backward_bf16(st, demb, layers, w_p, grads=None, grad_ready=None, status=None, probe=None,
                           schedule="auto", need_dx=False):
    """Backward of embedder_forward_bf16 (same ``grads`` / ``grad_ready`` contract as
    embedder_backward; ``status`` and ``schedule`` as embedder_forward_bf16).  need_dx: also the
    input gradient dx [B,T,F] (returns (grads, dx)), formed by the per-layer kernels, whose layer-0
    step adds the dx = dG W_ih GEMM (bf16 operands, fp32 accumulation) the stacked schedules skip;
    the per-layer per-step kernels are bit-identical to the persistent ones."""
    sched = schedule_flags(schedule) | (0 if grad_ready else SV_SCHED_NO_EVENTS)  # (as embedder_backward)
    demb = demb.contiguous()
    require_device(demb)
    T, B, H = st.T, st.B, st.H
    dev = demb.device
    s = stream_of(demb)
    L = len(layers)
    Bp = (B + 7) // 8 * 8
    grads, dh_last = _proj_norm_bwd(st, demb, layers, w_p, grads, s)
    if L > 1 and not need_dx:
        F0 = st.x_tm[0].shape[2]
        ws = _ws(lib().sv_lstm_bwd_workspace(SV_DTYPE_BF16, L, T, B, F0, H), dev)
        wt = st.wt
        if wt is not None:  # the forward wrote the weight transposes into it (sv_lstm_weights_bf16)
            sched |= SV_SCHED_WT_READY
        else:               # the backward transposes into it itself
            wt = _ws(lib().sv_lstm_wt_bf16_size(L, F0, H), dev)
        dgs = [_bf((T, B, 4 * H), dev) for _ in range(L)]
        dgTs = [_bf((4 * H, T * Bp), dev) for _ in range(L)]
        # the projection bucket too is enqueued behind the stack backward (late_head), for every schedule
        _stack_bwd(SV_DTYPE_BF16, st, layers, grads, dh_last, dgs, dgTs, ws, wt, 0, sched, status, probe, None,
                   grad_ready, True, s)
        st.dgT = dgTs  # the weight-gradient GEMMs' A operands (tests check dW against them)
        return grads
    if grad_ready:
        grad_ready(L, None)
    Fmax = max(st.x_tm[l].shape[2] for l in range(L))
    ws = _ws(lib().sv_lstm_layer_bwd_bf16_workspace(T, B, Fmax, H), dev)
    dg = _bf((T, B, 4 * H), dev)
    dgT = _bf((4 * H, T * Bp), dev)
    whhT = _bf((H, 4 * H), dev)
    dh_up, full = dh_last, 0
    for l in range(L - 1, -1, -1):
        w_ih, w_hh, _, _ = layers[l]
        Fl = st.x_tm[l].shape[2]
        wihT = _bf((Fl, 4 * H), dev)
        call("sv_transpose_cast_bf16", ptr(w_ih), Fl, 4 * H, Fl, ptr(wihT), 4 * H, s)
        call("sv_transpose_cast_bf16", ptr(w_hh), H, 4 * H, H, ptr(whhT), 4 * H, s)
        dx = _f32((T, B, Fl), dev) if (l > 0 or need_dx) else None
        if l == 0:
            xT, ld_xT = ptr(st.xT0), T * Bp
        else:
            xT, ld_xT = ptr(st.hT[l - 1]) + 2 * Bp, (T + 1) * Bp
        call("sv_lstm_layer_bwd_bf16", T, B, Fl, H, xT, ld_xT, ptr(wihT), ptr(whhT), ptr(st.gates[l]),
             ptr(st.c_tm[l]), ptr(st.hT[l]), ptr(dh_up), full, ptr(dg), ptr(dgT), ptr(dx), ptr(grads[4 * l]),
             ptr(grads[4 * l + 1]), ptr(grads[4 * l + 2]), ptr(grads[4 * l + 3]), ptr(ws), s)
        if grad_ready:
            grad_ready(l, None)
        dh_up, full = dx, 1
    return (grads, _dx_batch_first(dh_up, s)) if need_dx else grads


def embedder_fwd(precision, x, layers, w_p, b_p, products="mfma_f32", **kw):
    """embedder_forward_bf16 (precision "bf16") or embedder_forward (any other; ``products`` is its)."""
    if precision == "bf16":
        return embedder_forward_bf16(x, layers, w_p, b_p, **kw)
    return embedder_forward(x, layers, w_p, b_p, products=products, **kw)


def embedder_bwd(precision, st, demb, layers, w_p, products="mfma_f32", kstamp=None, **kw):
    """embedder_backward_bf16 (precision "bf16") or embedder_backward (any other; ``products`` and
    ``kstamp`` are its)."""
    if precision == "bf16":
        return embedder_backward_bf16(st, demb, layers, w_p, **kw)
    return embedder_backward(st, demb, layers, w_p, products=products, kstamp=kstamp, **kw)


def _flat_grads(params, dev):
    """Gradient tensors shaped like params, as views of one flat buffer (returned last)."""
    n = sum(p.numel() for p in params)
    flat = torch.empty(n, dtype=torch.float32, device=dev)
    out, off = [], 0
    for p in params:
        out.append(flat[off:off + p.numel()].view(p.shape))
        off += p.numel()
    return out, flat


class EmbedderFunction(torch.autograd.Function):
    """emb = SpeechEmbedder.forward(x) with params (w_ih, w_hh, b_ih, b_hh)*L, w_p, b_p.

    The forward and backward share one sync block; if a persistent recurrence of either timed
    out, every returned gradient is NaN (sv_status_poison), so an optimizer step on them
    cannot pass unnoticed, and check_persistent_status() raises."""

    @staticmethod
    def forward(ctx, x, num_layers, precision, products, schedule, *params):
        L = num_layers
        layers = [tuple(params[4 * l:4 * l + 4]) for l in range(L)]
        w_p, b_p = params[4 * L], params[4 * L + 1]
        # earlier calls' completed checks: raise on a timeout there, drop the finished entries (so
        # a forward-only loop keeps _UNCHECKED bounded)
        check_persistent_status()
        ctx.status = PersistStatus(x.device)
        emb, st = embedder_fwd(precision, x.contiguous(), layers, w_p, b_p, products=products, save=True,
                               status=ctx.status, schedule=schedule)
        # checked even if no backward follows (eval, d-vectors, anything under no_grad): a hand-off
        # timeout in this forward raises at the next call / check_persistent_status()
        ctx.status.arm()
        _UNCHECKED.append(ctx.status)
        ctx.precision, ctx.products, ctx.schedule = precision, products, schedule
        ctx.st = st
        ctx.L = L
        ctx.save_for_backward(*params)
        return emb

    @staticmethod
    def backward(ctx, demb):
        params = ctx.saved_tensors
        L = ctx.L
        layers = [tuple(params[4 * l:4 * l + 4]) for l in range(L)]
        need_dx = ctx.needs_input_grad[0]
        grads, flat = _flat_grads(params, demb.device)
        out = embedder_bwd(ctx.precision, ctx.st, demb, layers, params[4 * L], products=ctx.products, grads=grads,
                           need_dx=need_dx, status=ctx.status, schedule=ctx.schedule)
        call("sv_status_poison", ctx.status.ptr(), ptr(flat), flat.numel(), stream_of(flat))
        ctx.status.arm()
        if ctx.status not in _UNCHECKED:
            _UNCHECKED.append(ctx.status)
        ctx.status = None
        ctx.st = None
        if need_dx:
            grads, dx = out
        else:
            grads, dx = out, None
        return (dx, None, None, None, None, *grads)


# ----------------------------------------------------------------------------- GE2E
class Ge2eState:
    pass


def _pad_d(E):
    D = E.shape[-1]
    if D % 4 == 0:
        return E.contiguous(), D
    Dp = (D + 3) // 4 * 4
    Ep = torch.zeros(E.shape[:-1] + (Dp,), dtype=E.dtype, device=E.device)
    Ep[..., :D] = E
    return Ep, D


def _loss_kind(loss_method, N):
    """The C ABI's loss id of a method name; the contrast loss needs a negative (N >= 2)."""
    kind = loss_id(loss_method)
    if loss_method == "contrast" and N < 2:
        raise ValueError("the GE2E contrast loss needs N >= 2 speakers (max over k != j)")
    return kind


def ge2e_forward(E, w, b, loss_method="softmax"):
    """GE2E loss of E [N,M,D] with device scalars w, b.  Returns (loss 0-dim, per [N,M], state).
    loss_method: 'softmax' (eq. 6 of the GE2E paper, the reference's) or 'contrast' (eq. 7)."""
    require_device(E, w, b)
    if E.dim() != 3 or E.shape[1] < 2:
        raise ValueError("GE2E expects embeddings [N, M, D] with M >= 2 (leave-one-out centroids)")
    kind = _loss_kind(loss_method, E.shape[0])
    Ep, D0 = _pad_d(E)
    N, M, D = Ep.shape
    dev = E.device
    s = stream_of(E)
    st = Ge2eState()
    st.ws = _ws(lib().sv_ge2e_workspace_size(N, M, D, N), dev)
    st.ssum = torch.empty((N, D), dtype=torch.float32, device=dev)
    st.N, st.M, st.D, st.D0 = N, M, D, D0
    st.loss_method = loss_method
    loss = torch.empty((), dtype=torch.float32, device=dev)
    per = torch.empty((N, M), dtype=torch.float32, device=dev)
    call_as("sv_ge2e_fwd", kind, ptr(Ep), N, M, D, ptr(w.contiguous()), ptr(b.contiguous()), ptr(loss), ptr(per),
            ptr(st.ws), ptr(st.ssum), s)
    return loss, per, st


def ge2e_backward(st, w, b, gloss=None, loss_method=None):
    """Returns (dE [N,M,D0], dw 0-dim, db 0-dim).  loss_method: None = the forward's (the state
    carries it); naming another one than the forward ran is an error."""
    if loss_method is None:
        loss_method = st.loss_method
    elif loss_method != st.loss_method:
        raise ValueError(f"ge2e_backward: the forward ran loss_method={st.loss_method!r}, not {loss_method!r}")
    kind = loss_id(loss_method)
    N, M, D = st.N, st.M, st.D
    dev = st.ws.device
    s = stream_of(st.ws)
    Np = (N + 3) // 4 * 4
    dE = torch.empty((N, M, D), dtype=torch.float32, device=dev)
    dwdb = torch.empty((2,), dtype=torch.float32, device=dev)
    dchat = torch.empty((Np, D), dtype=torch.float32, device=dev)
    beta = torch.empty((N,), dtype=torch.float32, device=dev)
    g = None if gloss is None else gloss.contiguous()
    call_as("sv_ge2e_bwd", kind, N, M, D, ptr(w.contiguous()), ptr(b.contiguous()), ptr(g), ptr(dE), ptr(dwdb),
            ptr(dchat), ptr(beta), ptr(st.ws), s)
    if st.D0 != D:
        dE = dE[..., :st.D0].contiguous()
    return dE, dwdb[0], dwdb[1]


def ge2e_train(E, w, b, dwdb_out=None, loss_method="softmax"):
    """Fused GE2E forward + closed-form backward for one GPU holding all N speakers (the training
    step's gloss = 1): returns (loss 0-dim, per [N,M], dE [N,M,D], dwdb [2]) from three launches
    (include/sv_ge2e.h, sv_ge2e_train); dwdb_out (2 contiguous fp32 on the device): written in
    place of a new dwdb tensor.  Shapes outside sv_ge2e_train_ok take the split path.
    loss_method: 'softmax' or 'contrast' (ge2e_forward)."""
    require_device(E, w, b)
    Ep, D0 = _pad_d(E)
    N, M, D = Ep.shape
    if M < 2:
        raise ValueError("GE2E expects embeddings [N, M, D] with M >= 2 (leave-one-out centroids)")
    kind = _loss_kind(loss_method, N)
    if not lib().sv_ge2e_train_ok(N, M, D):
        loss, per, st = ge2e_forward(E, w, b, loss_method)
        dE, dw, db = ge2e_backward(st, w, b)
        return loss, per, dE, torch.stack([dw, db])
    dev = E.device
    ws = _ws(lib().sv_ge2e_workspace_size(N, M, D, N), dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    per = torch.empty((N, M), dtype=torch.float32, device=dev)
    dE = torch.empty((N, M, D), dtype=torch.float32, device=dev)
    dwdb = torch.empty((2,), dtype=torch.float32, device=dev) if dwdb_out is None else dwdb_out
    if dwdb.numel() != 2 or dwdb.dtype != torch.float32 or not dwdb.is_contiguous() or dwdb.device != dev:
        raise ValueError("ge2e_train: dwdb_out must be 2 contiguous fp32 values on the embeddings' device")
    call_as("sv_ge2e_train", kind, ptr(Ep), N, M, D, ptr(w.contiguous()), ptr(b.contiguous()), ptr(loss), ptr(per),
            ptr(dE), ptr(dwdb), ptr(ws), stream_of(Ep))
    if D0 != D:
        dE = dE[..., :D0].contiguous()
    return loss, per, dE, dwdb


class GE2EFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, E, w, b, *loss_method):
        # apply(E, w, b) or apply(E, w, b, loss_method): the backward returns one gradient per input
        loss, per, st = ge2e_forward(E, w, b, *loss_method)
        ctx.n_extra = len(loss_method)
        ctx.st = st
        ctx.save_for_backward(w, b)
        ctx.mark_non_differentiable(per)
        return loss, per

    @staticmethod
    def backward(ctx, gloss, _gper):
        w, b = ctx.saved_tensors
        dE, dw, db = ge2e_backward(ctx.st, w, b, gloss.reshape(()).to(torch.float32))
        ctx.st = None
        return (dE, dw.reshape(w.shape), db.reshape(b.shape)) + (None,) * ctx.n_extra


# ----------------------------------------------------------------------------- clip + SGD
def clip_sgd_step_(flat_params, flat_grads, max_norm, lr, write_grad=False, norm_out=None, status=None):
    """In place: flat_params -= lr * min(1, max_norm/(|g|+1e-6)) * flat_grads.  With ``status``
    (a PersistStatus) the update is skipped on the device when its status word is set."""
    require_device(flat_params, flat_grads)
    ws = _ws(lib().sv_clip_sgd_workspace(), flat_params.device)
    call("sv_clip_sgd_step", ptr(flat_params), ptr(flat_grads), flat_params.numel(), float(max_norm), float(lr),
         int(write_grad), ptr(norm_out), status.ptr() if status is not None else None, ptr(ws),
         stream_of(flat_params))


def clip_sgd_step2_(p0, g0, max_norm0, p1, g1, max_norm1, lr, write_grad=False, norm_out=None, status=None,
                    report=None):
    """clip_sgd_step_ over two flat parameter groups (the network's and the loss's {w, b},
    train_speech_embedder.py:63-65) in one pair of launches; bit-identical to two calls.
    report: a tensor x for ``status.report(x)`` done inside the update launch
    (sv_clip_sgd_step2_report: the training step's status report without a launch of its own)."""
    require_device(p0, g0, p1, g1)
    ws = _ws(2 * lib().sv_clip_sgd_workspace(), p0.device)
    args = (ptr(p0), ptr(g0), p0.numel(), float(max_norm0), ptr(p1), ptr(g1), p1.numel(), float(max_norm1), float(lr),
            int(write_grad), ptr(norm_out), status.ptr() if status is not None else None, ptr(ws))
    if report is not None:
        if status is None:
            raise ValueError("clip_sgd_step2_: report needs the status block")
        require_device(report)
        slot, seq = status.next_slot()
        call("sv_clip_sgd_step2_report", *args, ptr(report), report.numel(), slot, seq, stream_of(p0))
    else:
        call("sv_clip_sgd_step2", *args, stream_of(p0))


def gemm_f32(A, B, a_kcontig=True, b_kcontig=True, bias=None, products="mfma_f32"):
    """C = op(A) op(B) through sv_gemm_f32 (test hook).  With a_kcontig A is [M,K] else [K,M];
    with b_kcontig B is [N,K] else [K,N]."""
    require_device(A, B, bias)
    M = A.shape[0] if a_kcontig else A.shape[1]
    K = A.shape[1] if a_kcontig else A.shape[0]
    N = B.shape[0] if b_kcontig else B.shape[1]
    C = torch.empty((M, N), dtype=torch.float32, device=A.device)
    ws = _ws(lib().sv_gemm_f32_workspace(M, N, K), A.device)
    call("sv_gemm_f32", int(a_kcontig), int(b_kcontig), M, N, K, ptr(A), A.shape[1], ptr(B), B.shape[1], ptr(C), N,
         ptr(bias), None, 0.0, ptr(ws), _products(products), stream_of(A))
    return C


def gemm_f32_nt_into(A, lda, B, ldb, C, ldc, M, N, K):
    """C[m * ldc + n] = sum_k A[m * lda + k] B[n * ldb + k] through sv_gemm_f32 (exact fp32 MFMA products):
    A, B and C are 1-D fp32 device views that start at the operands, so that the callers' packed
    buffers (diarization.py: one matrix per file at its own offset and leading dimension) need no
    copies.  K, lda and ldb multiples of 4, A and B on 16-byte boundaries (the kernel's own checks)."""
    require_device(A, B, C)
    if A.numel() < (M - 1) * lda + K or B.numel() < (N - 1) * ldb + K or C.numel() < (M - 1) * ldc + N:
        raise ValueError("gemm_f32_nt_into: an operand view is shorter than its matrix")
    ws = _ws(lib().sv_gemm_f32_workspace(M, N, K), A.device)
    call("sv_gemm_f32", 1, 1, M, N, K, ptr(A), lda, ptr(B), ldb, ptr(C), ldc, None, None, 0.0, ptr(ws), 0, stream_of(A))
