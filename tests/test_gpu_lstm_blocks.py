"""The fp32 LSTM and projection kernels on their own, block by block, against fp64.

Every fp32 entry point of the hot path -- the K2 / K3 step kernels, one layer, the stack under
both schedules, the projection head and the small movers -- is called directly (C ABI, or ops for
the stack) at the smallest shapes that reach each tile edge, and every output, saved state
included, is compared element-wise with a plain fp64 restatement of the same operation.

Tolerances are calibrated, not hard-coded: for a quantity q with fp64 reference ``ref64`` and the
same formula evaluated in fp32 on the CPU ``ref32`` (oracle.lstm_np with dtype=np.float32, or
numpy fp32),

    d_ref = max|ref32 - ref64| / max|ref64|
    assert  max|gpu - ref64| / max|ref64|  <=  8 * max(d_ref, 1e-6)

The factor 8 covers another summation order (MFMA, split-K, the persistent path's per-layer order)
and another exp; the floor 1e-6 (8 fp32 ulps) keeps a quantity fp32 happens to reproduce exactly
from demanding a bit match.  Exact checks (zero padding, sentinels, bit-equal movers,
db_ih == db_hh, determinism) take no tolerance.  Each check prints a MEASURED line.
"""
import functools

import numpy as np
import pytest
import torch

import recipe
from oracle import lstm_np

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR, FLOOR = 8.0, 1e-6
SENTINEL = 1234.5


def _lib():
    from pytorch_speaker_verification_amd import _lib
    return _lib


def _call(name, *args):
    _lib().call(name, *args)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _randn(gen, *shape):
    return torch.randn(shape, generator=gen).numpy()


def _ws(nbytes):
    return torch.empty(max(1, (int(nbytes) + 3) // 4), dtype=torch.float32, device=DEV)


def check(name, gpu, ref64, ref32, factor=FACTOR):
    """The calibrated comparison of the module docstring; returns (d_gpu, d_ref)."""
    gpu, ref64, ref32 = (np.asarray(a, np.float64) for a in (gpu, ref64, ref32))
    assert gpu.shape == ref64.shape == ref32.shape, (name, gpu.shape, ref64.shape, ref32.shape)
    scale = np.abs(ref64).max()
    assert np.isfinite(ref64).all(), name
    if scale == 0:  # an identically zero quantity (K3 with no incoming gradient): sums of exact zeros
        print(f"\nMEASURED {name} gpu {np.abs(gpu).max():.3e} ref32 {np.abs(ref32).max():.3e} (reference is zero)")
        assert (ref32 == 0).all() and (gpu == 0).all(), name
        return 0.0, 0.0
    d_ref = np.abs(ref32 - ref64).max() / scale
    finite = bool(np.isfinite(gpu).all())
    d_gpu = np.abs(gpu - ref64).max() / scale if finite else float("inf")
    print(f"\nMEASURED {name} gpu {d_gpu:.3e} ref32 {d_ref:.3e}")
    assert finite, f"{name}: non-finite values"
    assert d_gpu <= factor * max(d_ref, FLOOR), (name, d_gpu, d_ref)
    return d_gpu, d_ref


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


# ------------------------------------------------------------------------- 1. K2 / K3 alone
STEP_SHAPES = [(1, 4), (7, 36), (64, 32), (65, 96)]


def _k2_ref(dt, pre, h_prev, c_prev, w_hh):
    """One forward step from the pre-activation x-projection: (activated gates, c_t, h_t)."""
    pre, w_hh = pre.astype(dt), w_hh.astype(dt)
    H = w_hh.shape[1]
    z = pre if h_prev is None else pre + h_prev.astype(dt) @ w_hh.T
    i, f, g, o = _sig(z[:, :H]), _sig(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), _sig(z[:, 3 * H:])
    c = i * g if c_prev is None else f * c_prev.astype(dt) + i * g
    return np.concatenate([i, f, g, o], axis=1), c, o * np.tanh(c)


def _run_k2(name, pre, h_prev, c_prev, w_hh):
    B, H = pre.shape[0], w_hh.shape[1]
    # one extra row of sentinel behind each output: the row tails must be masked
    gates = torch.full((B + 1, 4 * H), SENTINEL, device=DEV)
    gates[:B] = _dev(pre)
    c_t = torch.full((B + 1, H), SENTINEL, device=DEV)
    h_t = torch.full((B + 1, H), SENTINEL, device=DEV)
    hp, cp, w = _dev(h_prev), _dev(c_prev), _dev(w_hh)
    _call("sv_lstm_step_fwd", _ptr(hp), _ptr(w), _ptr(gates), _ptr(cp), _ptr(c_t), _ptr(h_t), B, H, _stream())
    torch.cuda.synchronize()
    r64, r32 = _k2_ref(np.float64, pre, h_prev, c_prev, w_hh), _k2_ref(np.float32, pre, h_prev, c_prev, w_hh)
    for q, out, a, b in zip(("gates", "c_t", "h_t"), (gates, c_t, h_t), r64, r32):
        assert (_np(out[B]) == SENTINEL).all(), f"{name}.{q}: the row behind the last one was written"
        check(f"{name}.{q}", _np(out[:B]), a, b)


@pytest.mark.parametrize("first", [True, False], ids=["t0", "t>0"])
@pytest.mark.parametrize("B,H", STEP_SHAPES)
def test_k2_step_fwd(B, H, first):
    """sv_lstm_step_fwd (K2) against fp64: activated gates, c_t, h_t at t = 0 (h_prev = c_prev =
    NULL) and t > 0, at a single partial tile, partial row / unit / k tiles, the exact tile and a
    second row block of one row; the row behind the last keeps its sentinel."""
    g = torch.Generator().manual_seed(100 * B + H + int(first))
    pre, w_hh = _randn(g, B, 4 * H), _randn(g, 4 * H, H)
    h_prev, c_prev = (None, None) if first else (_randn(g, B, H), _randn(g, B, H))
    _run_k2(f"k2.B{B}H{H}.{'t0' if first else 'tn'}", pre, h_prev, c_prev, w_hh)


def test_k2_step_fwd_saturated():
    """Pre-activations up to |z| ~ 40: sigmoid / tanh must neither overflow nor lose the fp64 value."""
    B, H = 65, 96
    g = torch.Generator().manual_seed(7)
    pre = 10.0 * _randn(g, B, 4 * H)
    assert 35.0 < np.abs(pre).max() < 60.0
    _run_k2("k2.saturated", pre, None, _randn(g, B, H), _randn(g, 4 * H, H))


def _k3_ref(dt, dg_next, w_hh, dh_up, dcf_next, acts, c_t, c_prev):
    """One backward step, the formulas of lstm_np.lstm_layer_backward: (dG_t, dc_t f_t)."""
    acts, c_t = acts.astype(dt), c_t.astype(dt)
    H = c_t.shape[1]
    i, f, g, o = (acts[:, k * H:(k + 1) * H] for k in range(4))
    dh = np.zeros_like(c_t)
    if dg_next is not None:
        dh = dh + dg_next.astype(dt) @ w_hh.astype(dt)
    if dh_up is not None:
        dh = dh + dh_up.astype(dt)
    tc = np.tanh(c_t)
    dc = dh * o * (1 - tc * tc)
    if dcf_next is not None:
        dc = dc + dcf_next.astype(dt)
    cp = np.zeros_like(c_t) if c_prev is None else c_prev.astype(dt)
    dG = np.concatenate([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)],
                        axis=1)
    return dG, dc * f


# which of (dg_next, dh_up, dcf_next, c_prev) are passed: all, none (T = 1), each one NULL alone
K3_FORMS = [(1, 1, 1, 1), (0, 0, 0, 0), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)]


@pytest.mark.parametrize("form", K3_FORMS, ids=["".join(map(str, f)) for f in K3_FORMS])
@pytest.mark.parametrize("B,H", STEP_SHAPES)
def test_k3_step_bwd(B, H, form):
    """sv_lstm_step_bwd (K3) against fp64: dg_t and dcf_t with each nullable argument (dg_next,
    dh_up, dcf_next, c_prev) in its NULL and non-NULL form, all four NULL included; the row behind
    the last keeps its sentinel."""
    g = torch.Generator().manual_seed(1000 * B + 10 * H + sum(b << k for k, b in enumerate(form)))
    w_hh = _randn(g, 4 * H, H)
    z = _randn(g, B, 4 * H)  # the saved activations of N(0,1) pre-activations
    acts = np.concatenate([_sig(z[:, :2 * H]), np.tanh(z[:, 2 * H:3 * H]), _sig(z[:, 3 * H:])], axis=1)
    acts = acts.astype(np.float32)
    c_t = _randn(g, B, H)
    dg_next, dh_up, dcf_next, c_prev = (a if on else None for on, a in
                                        zip(form, (_randn(g, B, 4 * H), _randn(g, B, H), _randn(g, B, H),
                                                   _randn(g, B, H))))
    dg = torch.full((B + 1, 4 * H), SENTINEL, device=DEV)
    dcf = torch.full((B + 1, H), SENTINEL, device=DEV)
    ins = [_dev(a) for a in (dg_next, w_hh.T, dh_up, dcf_next, acts, c_t, c_prev)]
    _call("sv_lstm_step_bwd", *[_ptr(t) for t in ins], _ptr(dg), _ptr(dcf), B, H, _stream())
    torch.cuda.synchronize()
    r64 = _k3_ref(np.float64, dg_next, w_hh, dh_up, dcf_next, acts, c_t, c_prev)
    r32 = _k3_ref(np.float32, dg_next, w_hh, dh_up, dcf_next, acts, c_t, c_prev)
    name = f"k3.B{B}H{H}.{''.join(map(str, form))}"
    for q, out, a, b in zip(("dg_t", "dcf_t"), (dg, dcf), r64, r32):
        assert (_np(out[B]) == SENTINEL).all(), f"{name}.{q}: the row behind the last one was written"
        check(f"{name}.{q}", _np(out[:B]), a, b)
    if not form[3]:  # no c_{t-1}: the forget gate's gradient is exactly zero
        assert (_np(dg[:B, H:2 * H]) == 0).all()


# ------------------------------------------------------------------------- 2. one layer
LAYER_SHAPES = [(1, 5, 4, 36), (3, 8, 40, 64), (4, 65, 36, 96)]


@functools.lru_cache(maxsize=None)
def _layer_case(T, B, F, H):
    """Inputs, the GPU forward's outputs (every buffer pre-filled with NaN, so what the library
    must zero it has to zero itself) and the oracle's forward in fp64 and fp32."""
    sd = recipe.make_weights(T + 10 * B + F + H, F, H, 1, 4, scale=3.0)
    w = [sd[f"LSTM_stack.{n}_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    x = recipe.make_frames(B + H, B, T, F)  # [B,T,F]
    x_tm = np.ascontiguousarray(x.transpose(1, 0, 2))
    Bp = (B + 3) // 4 * 4
    nan = float("nan")
    gates = torch.full((T, B, 4 * H), nan, device=DEV)
    c_tm = torch.full((T, B, H), nan, device=DEV)
    h_tm = torch.full((T + 1, B, H), nan, device=DEV)
    hT = torch.full((H, (T + 1) * Bp), nan, device=DEV)
    wd = [_dev(a) for a in w]
    xd = _dev(x_tm)
    _call("sv_lstm_layer_fwd", _ptr(xd), T, B, F, H, *[_ptr(t) for t in wd], _ptr(gates), _ptr(c_tm), _ptr(h_tm),
          _ptr(hT), _stream())
    torch.cuda.synchronize()
    ref = {dt: lstm_np.lstm_layer_forward(x, *w, dtype=dt) for dt in (np.float64, np.float32)}
    return dict(w=w, wd=wd, x=x, x_tm=x_tm, Bp=Bp, gates=gates, c_tm=c_tm, h_tm=h_tm, hT=hT, ref=ref)


def _tm(a):
    """[B,T,*] (the oracle's batch-first layout) -> time-major [T,B,*]."""
    return np.ascontiguousarray(np.asarray(a).transpose(1, 0, 2))


@pytest.mark.parametrize("T,B,F,H", LAYER_SHAPES)
def test_layer_fwd(T, B, F, H):
    """sv_lstm_layer_fwd against lstm_np: the activated gates, c_tm, h_tm (slot 0 exactly zero) and
    hT (block t+1 = h_t^T bit for bit, block 0 and every padding column exactly zero) at
    Bp != B (the memset branch), Bp == B (no memset) and two row blocks."""
    c = _layer_case(T, B, F, H)
    (hs64, (_, _, cs64, acts64)), (hs32, (_, _, cs32, acts32)) = c["ref"][np.float64], c["ref"][np.float32]
    name = f"layer_fwd.T{T}B{B}F{F}H{H}"
    check(f"{name}.gates", _np(c["gates"]), _tm(acts64), _tm(acts32))
    check(f"{name}.c_tm", _np(c["c_tm"]), _tm(cs64), _tm(cs32))
    h_tm = _np(c["h_tm"])
    assert (h_tm[0] == 0).all()
    check(f"{name}.h_tm", h_tm[1:], _tm(hs64), _tm(hs32))
    Bp = c["Bp"]
    hT = _np(c["hT"]).reshape(H, T + 1, Bp)
    assert (hT[:, 0, :] == 0).all(), "hT block 0"
    assert (hT[:, :, B:] == 0).all(), "hT padding columns"
    assert np.array_equal(hT[:, 1:, :B], h_tm[1:].transpose(2, 0, 1)), "hT block t+1 != h_t^T"


def _layer_bwd_gpu(c, T, B, F, H, dh_up, full, with_dx=True, with_db_hh=True):
    Bp = c["Bp"]
    nan = float("nan")
    xT = np.zeros((F, T, Bp), np.float32)  # [F, T*Bp], column t*Bp + b = x_t[b], padding columns zero
    xT[:, :, :B] = c["x_tm"].transpose(2, 0, 1)
    out = dict(dgates=torch.full((T, B, 4 * H), nan, device=DEV), dgT=torch.full((4 * H, T * Bp), nan, device=DEV),
               dx=torch.full((T, B, F), nan, device=DEV) if with_dx else None,
               dw_ih=torch.full((4 * H, F), nan, device=DEV), dw_hh=torch.full((4 * H, H), nan, device=DEV),
               db_ih=torch.full((4 * H,), nan, device=DEV),
               db_hh=torch.full((4 * H,), nan, device=DEV) if with_db_hh else None)
    ws = _ws(_lib().lib().sv_lstm_layer_bwd_workspace(T, B, F, H))
    xTd, upd = _dev(xT), _dev(dh_up)
    _call("sv_lstm_layer_bwd", T, B, F, H, _ptr(xTd), T * Bp, _ptr(c["wd"][0]), _ptr(c["wd"][1]), _ptr(c["gates"]),
          _ptr(c["c_tm"]), _ptr(c["hT"]), _ptr(upd), int(full), *[_ptr(out[k]) for k in
                                                                 ("dgates", "dgT", "dx", "dw_ih", "dw_hh", "db_ih",
                                                                  "db_hh")], _ptr(ws), _stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("full", [1, 0], ids=["dh_up_full", "dh_up_last"])
@pytest.mark.parametrize("T,B,F,H", LAYER_SHAPES)
def test_layer_bwd(T, B, F, H, full):
    """sv_lstm_layer_bwd on the GPU forward's saved state against lstm_np: dgates, dgT (= dgates^T bit
    for bit, padding columns exactly zero), dx_tm, dw_ih, dw_hh, db_ih == db_hh, with a dense random
    dh_up [T,B,H] (dh_up_full = 1, a lower layer's view) and with [B,H] for the last step only; then
    the same call with dx_tm = NULL and db_hh = NULL: return 0, every other output bit-identical."""
    c = _layer_case(T, B, F, H)
    g = torch.Generator().manual_seed(T + B + F + H + full)
    dh_up = _randn(g, T, B, H) if full else _randn(g, B, H)
    dhs = np.zeros((B, T, H), np.float32)
    if full:
        dhs[:] = dh_up.transpose(1, 0, 2)
    else:
        dhs[:, -1] = dh_up
    out = _layer_bwd_gpu(c, T, B, F, H, dh_up, full)
    w_ih, w_hh = c["w"][0], c["w"][1]
    ref = {dt: lstm_np.lstm_layer_backward(dhs, w_ih, w_hh, c["ref"][dt][1], dtype=dt, return_dg=True)
           for dt in (np.float64, np.float32)}
    (dx64, dwih64, dwhh64, db64, dg64), (dx32, dwih32, dwhh32, db32, dg32) = ref[np.float64], ref[np.float32]
    name = f"layer_bwd.T{T}B{B}F{F}H{H}.full{full}"
    dgates = _np(out["dgates"])
    check(f"{name}.dgates", dgates, _tm(dg64), _tm(dg32))
    Bp = c["Bp"]
    dgT = _np(out["dgT"]).reshape(4 * H, T, Bp)
    assert (dgT[:, :, B:] == 0).all(), "dgT padding columns"
    assert np.array_equal(dgT[:, :, :B], dgates.transpose(2, 0, 1)), "dgT != dgates^T"
    check(f"{name}.dx_tm", _np(out["dx"]), _tm(dx64), _tm(dx32))
    check(f"{name}.dw_ih", _np(out["dw_ih"]), dwih64, dwih32)
    check(f"{name}.dw_hh", _np(out["dw_hh"]), dwhh64, dwhh32)
    check(f"{name}.db_ih", _np(out["db_ih"]), db64, db32)
    assert torch.equal(out["db_ih"], out["db_hh"]), "db_ih != db_hh"
    # NULL outputs (call raises on a nonzero return)
    part = _layer_bwd_gpu(c, T, B, F, H, dh_up, full, with_dx=False, with_db_hh=False)
    for k in ("dgates", "dgT", "dw_ih", "dw_hh", "db_ih"):
        assert torch.equal(part[k], out[k]), f"{k} changed with dx_tm = db_hh = NULL"


# ------------------------------------------------------------------------- 3. the stack
def _names(L):
    return [f"LSTM_stack.{n}_l{l}" for l in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + \
        ["projection.weight", "projection.bias"]


@functools.lru_cache(maxsize=None)
def _stack_ref(dims, B, T):
    """Inputs and the oracle's forward / backward (dense random demb) in fp64 and fp32, once per case."""
    F, H, L, P = dims
    sd = recipe.make_weights(B + T + H, *dims, scale=3.0)
    x = recipe.make_frames(B * T + F, B, T, F)
    demb = _randn(torch.Generator().manual_seed(B + 3 * T + P), B, P)
    ref = {}
    for dt in (np.float64, np.float32):
        emb, cache = lstm_np.embedder_forward(sd, x, L, dtype=dt)
        grads, dx = lstm_np.embedder_backward(sd, demb, cache, L, dtype=dt, return_dx=True)
        ref[dt] = dict(emb=emb, caches=cache[0], grads=grads, dx=dx)
    return sd, x, demb, ref


@functools.lru_cache(maxsize=None)
def _stack_gpu(dims, B, T, schedule, need_dx=False):
    """ops.embedder_forward / embedder_backward under `schedule`: emb, saved state, gradients (numpy)."""
    from pytorch_speaker_verification_amd import ops
    L = dims[2]
    sd, x, demb, _ = _stack_ref(dims, B, T)
    ps = [_dev(sd[k]) for k in _names(L)]
    layers = [tuple(ps[4 * l:4 * l + 4]) for l in range(L)]
    emb, st = ops.embedder_forward(_dev(x), layers, ps[4 * L], ps[4 * L + 1], schedule=schedule)
    out = ops.embedder_backward(st, _dev(demb), layers, ps[4 * L], schedule=schedule, need_dx=need_dx)
    grads, dx = out if need_dx else (out, None)
    torch.cuda.synchronize()
    ops.check_persistent_status(wait=True)  # raises if a persistent recurrence timed out
    return dict(emb=_np(emb), gates=[_np(t) for t in st.gates], c_tm=[_np(t) for t in st.c_tm],
                h_tm=[_np(t) for t in st.h_tm], grads={k: _np(t) for k, t in zip(_names(L), grads)},
                dx=None if dx is None else _np(dx))


def _check_stack(name, dims, B, T, schedule, need_dx=False):
    L = dims[2]
    _, _, _, ref = _stack_ref(dims, B, T)
    r64, r32 = ref[np.float64], ref[np.float32]
    got = _stack_gpu(dims, B, T, schedule, need_dx)
    check(f"{name}.emb", got["emb"], r64["emb"], r32["emb"])
    for l in range(L):
        (_, hs64, cs64, a64), (_, hs32, cs32, a32) = r64["caches"][l], r32["caches"][l]
        check(f"{name}.l{l}.gates", got["gates"][l], _tm(a64), _tm(a32))
        check(f"{name}.l{l}.c_tm", got["c_tm"][l], _tm(cs64), _tm(cs32))
        assert (got["h_tm"][l][0] == 0).all()
        check(f"{name}.l{l}.h_tm", got["h_tm"][l][1:], _tm(hs64), _tm(hs32))
    for k in _names(L):
        check(f"{name}.grad.{k}", got["grads"][k], r64["grads"][k], r32["grads"][k])
    for l in range(L):
        assert np.array_equal(got["grads"][f"LSTM_stack.bias_ih_l{l}"], got["grads"][f"LSTM_stack.bias_hh_l{l}"])
    if need_dx:
        check(f"{name}.dx", got["dx"], r64["dx"], r32["dx"])


PER_STEP_CASES = [((40, 72, 2, 20), 9, 37), ((8, 64, 3, 32), 4, 1)]


@pytest.mark.parametrize("need_dx", [False, True], ids=["stacked", "need_dx"])
@pytest.mark.parametrize("dims,B,T", PER_STEP_CASES, ids=["B9T37", "B4T1"])
def test_stack_per_step(dims, B, T, need_dx):
    """The per-step schedule through ops.embedder_forward / embedder_backward with a dense random demb
    against lstm_np: emb, every layer's saved gates / c_tm / h_tm, every parameter gradient, and with
    need_dx (the per-layer backward) the input gradient dx [B,T,F].  B = 9, T = 37: two pipeline
    chunks, ragged everything; B = 4, T = 1: three layers of a single step."""
    _check_stack(f"stack_per_step.B{B}T{T}{'.dx' if need_dx else ''}", dims, B, T, "per_step", need_dx)


PERSIST_CASES = [((40, 768, 3, 256), 9, 3), ((40, 768, 3, 256), 65, 2), ((8, 768, 2, 64), 12, 2)]


def _need_persist(B):
    lib = _lib()
    with torch.cuda.device(0):
        if not lib.lib().sv_lstm_f32_persist_ok(B, 768, lib.schedule_flags("persist")):
            pytest.skip("the fp32 persistent recurrences do not fit this device")


@pytest.mark.parametrize("dims,B,T", PERSIST_CASES, ids=["B9T3", "B65T2", "F8B12T2"])
def test_stack_persist(dims, B, T):
    """The fp32 persistent recurrences (H = 768) the same way: layer 0's in-recurrence projection
    (F = 40) at B = 9, a second row block of one row at B = 65, and F = 8, where layer 0 keeps its
    GEMM.  No hand-off wait may time out (check_persistent_status in _stack_gpu raises)."""
    _need_persist(B)
    _check_stack(f"stack_persist.B{B}T{T}F{dims[0]}", dims, B, T, "persist")


def test_stack_persist_vs_per_step():
    """include/sv_ge2e.h: the two fp32 schedules "agree to fp32 rounding" -- here with a number: on
    the same inputs (B = 65, T = 2, H = 768) their gradients differ by no more than the calibrated
    tolerance either is held to against fp64."""
    dims, B, T = PERSIST_CASES[1]
    _need_persist(B)
    _, _, _, ref = _stack_ref(dims, B, T)
    a, b = _stack_gpu(dims, B, T, "persist"), _stack_gpu(dims, B, T, "per_step")
    for k in _names(dims[2]):
        r64, r32 = (np.asarray(ref[dt]["grads"][k], np.float64) for dt in (np.float64, np.float32))
        scale = np.abs(r64).max()
        d_ref = np.abs(r32 - r64).max() / scale
        d = np.abs(a["grads"][k].astype(np.float64) - b["grads"][k]).max() / scale
        print(f"\nMEASURED persist_vs_per_step.B{B}T{T}.grad.{k} gpu {d:.3e} ref32 {d_ref:.3e}")
        assert d <= FACTOR * max(d_ref, FLOOR), (k, d, d_ref)


def _timing_events(n):
    """n timing events with their native event materialised (as bench.py creates its probes)."""
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
    for e in evs:
        e.record()
    return evs


INSTRUMENTED_CASES = [(PER_STEP_CASES[0], "per_step"), (PERSIST_CASES[0], "persist")]


@pytest.mark.parametrize("case,schedule", INSTRUMENTED_CASES, ids=["per_step.B9T37", "persist.B9T3"])
def test_stack_bwd_instrumented(case, schedule):
    """The stack backward's optional arguments -- timing probes, K3 stamps, grad_ready -- index the
    event, probe and stamp arrays per layer / chunk / step; no other test passes them.  Per-step
    (B = 9, T = 37: two chunks of PIPELINE_CHUNK = 32, the second ragged) and persistent (T = 3):
      * grad_ready: the projection (k = L) first -- with no event under per-step, behind the stack
        call with an event under persist -- then k = L-1 .. 0, each with an event; a clone of the
        group's gradients taken on another stream behind that event equals their final value;
      * every gradient is bit-identical to the uninstrumented call's (_stack_gpu; each schedule
        reproduced itself bit for bit when run twice on an MI355X);
      * every probe pair (2 L nch per-step, 2 L persist) measures a finite time >= 0;
      * per-step: every (l, t) stamp pair was written, start != -1 and end >= start; persist (the
        stamp tensor is passed there too, so the check means something): no stamp is touched."""
    from pytorch_speaker_verification_amd import ops
    (dims, B, T), L = case, case[0][2]
    persist = schedule == "persist"
    if persist:
        _need_persist(B)
    sd, x, demb, _ = _stack_ref(dims, B, T)
    ps = [_dev(sd[k]) for k in _names(L)]
    layers = [tuple(ps[4 * l:4 * l + 4]) for l in range(L)]
    nch = (T + ops.PIPELINE_CHUNK - 1) // ops.PIPELINE_CHUNK
    assert persist or nch == 2
    probe = _timing_events(2 * L if persist else 2 * L * nch)
    kstamp = torch.zeros(2 * L * T, dtype=torch.int64, device=DEV)
    kstamp[0::2] = -1
    grads = [torch.empty_like(t) for t in ps]
    main = torch.cuda.current_stream()
    calls, clones = [], {}

    def grad_ready(k, event):
        calls.append((k, event is not None))
        group = grads[4 * L:] if k == L else grads[4 * k:4 * k + 4]
        s = torch.cuda.Stream()
        if event is None:
            s.wait_stream(main)
        else:
            s.wait_event(event)
        with torch.cuda.stream(s):
            clones[k] = [g.clone() for g in group]

    emb, st = ops.embedder_forward(_dev(x), layers, ps[4 * L], ps[4 * L + 1], schedule=schedule)
    out = ops.embedder_backward(st, _dev(demb), layers, ps[4 * L], grads=grads, need_dx=False, grad_ready=grad_ready,
                                probe=probe, kstamp=kstamp, schedule=schedule)
    torch.cuda.synchronize()
    ops.check_persistent_status(wait=True)
    assert all(a is b for a, b in zip(out, grads))
    assert calls == [(L, persist)] + [(l, True) for l in range(L - 1, -1, -1)], calls
    for k, group in clones.items():
        final = grads[4 * L:] if k == L else grads[4 * k:4 * k + 4]
        for i, (c, g) in enumerate(zip(group, final)):
            assert torch.equal(c, g), f"group {k} tensor {i}: the clone behind its event is not the final gradient"
    plain = _stack_gpu(dims, B, T, schedule)
    assert np.array_equal(_np(emb), plain["emb"])
    for k, g in zip(_names(L), grads):
        assert np.array_equal(_np(g), plain["grads"][k]), f"{k} differs from the uninstrumented call"
    for i in range(len(probe) // 2):
        ms = probe[2 * i].elapsed_time(probe[2 * i + 1])
        assert np.isfinite(ms) and ms >= 0, (i, ms)
    ks = kstamp.cpu().view(L, T, 2)
    if persist:
        assert (ks[..., 0] == -1).all() and (ks[..., 1] == 0).all(), "the persistent schedule wrote a stamp"
    else:
        assert (ks[..., 0] != -1).all(), "an (l, t) stamp pair was not written"
        assert (ks[..., 1] >= ks[..., 0]).all()
        print(f"\nMEASURED stack_bwd_instrumented K3 span {float((ks[..., 1] - ks[..., 0]).float().mean()) / 100:.1f} us")


# ------------------------------------------------------------------------- 4. projection head
def _proj_ref(dt, h, w, b, demb):
    h, w, demb = h.astype(dt), w.astype(dt), demb.astype(dt)
    y = h @ w.T
    if b is not None:
        y = y + b.astype(dt)
    n = np.sqrt((y * y).sum(axis=1, keepdims=True))
    emb = y / n
    dy = (demb - emb * (demb * emb).sum(axis=1, keepdims=True)) / n
    return dict(y=y, ynorm=n[:, 0], emb=emb, dw_p=dy.T @ h, db_p=dy.sum(axis=0), dh_last=dy @ w)


def _proj_inputs(B, H, P, bias=True):
    g = torch.Generator().manual_seed(B * 31 + H * 7 + P)
    h, w, demb = _randn(g, B, H), _randn(g, P, H), _randn(g, B, P)
    return h, w, (_randn(g, P) if bias else None), demb


def _proj_gpu(B, H, P, h, w, b, demb):
    """(forward outputs, backward outputs); each direction raises RuntimeError on a nonzero return."""
    hd, wd, bd, dd = _dev(h), _dev(w), _dev(b), _dev(demb)
    ws = _ws(_lib().lib().sv_proj_norm_workspace(B, H, P))
    y, emb, ynorm = (torch.full(s, SENTINEL, device=DEV) for s in ((B + 1, P), (B + 1, P), (B + 1,)))
    _call("sv_proj_norm_fwd", _ptr(hd), B, H, P, _ptr(wd), _ptr(bd), _ptr(y), _ptr(emb), _ptr(ynorm), _ptr(ws),
          _stream())
    torch.cuda.synchronize()
    fwd = dict(y=y, emb=emb, ynorm=ynorm)

    def bwd():
        dw, db, dh = (torch.full(s, SENTINEL, device=DEV) for s in ((P + 1, H), (P + 1,), (B + 1, H)))
        _call("sv_proj_norm_bwd", _ptr(dd), _ptr(emb), _ptr(ynorm), _ptr(hd), B, H, P, _ptr(wd), _ptr(dw), _ptr(db),
              _ptr(dh), _ptr(ws), _stream())
        torch.cuda.synchronize()
        return dict(dw_p=dw, db_p=db, dh_last=dh)
    return fwd, bwd


def _check_proj(name, outs, rows, r64, r32):
    for k, t in outs.items():
        n = rows[k]
        assert (_np(t[n:]) == SENTINEL).all(), f"{name}.{k}: written behind its last row"
        check(f"{name}.{k}", _np(t[:n]), r64[k], r32[k])


PROJ_SHAPES = [(9, 96, 24, True), (5, 64, 6, True), (128, 64, 6, True), (64, 768, 256, True), (300, 768, 256, True),
               (9, 96, 24, False), (64, 768, 256, False)]


@pytest.mark.parametrize("B,H,P,bias", PROJ_SHAPES, ids=[f"B{s[0]}H{s[1]}P{s[2]}{'' if s[3] else '.nobias'}"
                                                           for s in PROJ_SHAPES])
def test_proj_norm(B, H, P, bias):
    """sv_proj_norm_fwd / _bwd against fp64: y = h W^T + b, ynorm = |y|, emb = y / ynorm, and with
    dy = (demb - emb <demb, emb>) / ynorm: dw_p = dy^T h, db_p = sum dy, dh_last = dy W.

    Forward branch by shape (proj_norm_fused / plan_gemm in sv_gemm_f32.hip: the fused form needs
    P <= 256, P % 4 == 0, no exact 256-row tiling, and a split-K plan of 2..8 slabs, which the
    `fine` plan gives from K = H >= 256 on):
      (64, 768, 256), (300, 768, 256)        fused split-K (6 slabs of K = 128) + row norm
                                             (slab_rownorm_kernel)
      (9, 96, 24), (5, 64, 6), (128, 64, 6)  GEMM (one 64 x 64 tile, no split) + rownorm_fwd_kernel
    Backward branch (sv_proj_norm_bwd in sv_misc.hip):
      P % 4 == 0: (9, 96, 24), (64, 768, 256), (300, 768, 256)   proj_bwd_tiles_kernel
      P % 4 != 0, B <= 128: (5, 64, 6), (128, 64, 6)             proj_bwd_small_kernel (128 = its
                                                                 upper row edge)
      neither (SV_EALIGN): see test_proj_norm_out_of_range.
    b_p = NULL once on each forward branch."""
    h, w, b, demb = _proj_inputs(B, H, P, bias)
    r64, r32 = _proj_ref(np.float64, h, w, b, demb), _proj_ref(np.float32, h, w, b, demb)
    fwd, bwd = _proj_gpu(B, H, P, h, w, b, demb)
    name = f"proj.B{B}H{H}P{P}{'' if bias else '.nobias'}"
    _check_proj(name, fwd, dict(y=B, emb=B, ynorm=B), r64, r32)
    _check_proj(name, bwd(), dict(dw_p=P, db_p=P, dh_last=B), r64, r32)


def test_proj_norm_out_of_range():
    """(130, 64, 6): B > 128 with P % 4 != 0 fits neither backward kernel, and sv_proj_norm_bwd
    returns SV_EALIGN for what fits neither (measured: the forward, GEMM + rownorm_fwd_kernel, is
    within tolerance; the backward returns SV_EALIGN).  The contract either way: a negative SV_E*
    return (call raises) or results within tolerance -- never return 0 with wrong values.

    A three-GEMM fallback once stood behind the two kernels; it could never return 0 either: it was
    reached only when proj_tiles_ok failed, i.e. P % 4 != 0 or H % 4 != 0 (its first GEMM's M = P /
    N = H alignment check) or a misaligned dy / h_last (that GEMM's pointer check) or a misaligned
    w_p alone (the last GEMM's pointer check) -- SV_EALIGN every time."""
    B, H, P = 130, 64, 6
    h, w, b, demb = _proj_inputs(B, H, P)
    r64, r32 = _proj_ref(np.float64, h, w, b, demb), _proj_ref(np.float32, h, w, b, demb)
    errors = tuple(_lib().ERRORS.values())
    try:
        fwd, bwd = _proj_gpu(B, H, P, h, w, b, demb)
    except RuntimeError as e:
        assert any(m in str(e) for m in errors), e
        print(f"\nMEASURED proj.B{B}H{H}P{P} forward rejected: {e}")
        return
    _check_proj(f"proj.B{B}H{H}P{P}", fwd, dict(y=B, emb=B, ynorm=B), r64, r32)
    try:
        out = bwd()
    except RuntimeError as e:
        assert any(m in str(e) for m in errors), e
        print(f"\nMEASURED proj.B{B}H{H}P{P} backward rejected: {e}")
        return
    _check_proj(f"proj.B{B}H{H}P{P}", out, dict(dw_p=P, db_p=P, dh_last=B), r64, r32)


# ------------------------------------------------------------------------- 5. the small movers
@pytest.mark.parametrize("B,T,F", [(1, 1, 4), (7, 5, 40), (33, 3, 8)])
def test_frames_to_time_major(B, T, F):
    x = torch.randn((B, T, F), generator=torch.Generator().manual_seed(B + T + F)).to(DEV)
    y = torch.full((T * B + 1, F), SENTINEL, device=DEV)
    _call("sv_frames_to_time_major", _ptr(x), _ptr(y), B, T, F, _stream())
    torch.cuda.synchronize()
    assert torch.equal(y[:T * B].view(T, B, F), x.permute(1, 0, 2))
    assert (y[T * B] == SENTINEL).all()


@pytest.mark.parametrize("R,C,ld_src,ld_dst", [(3, 5, 5, 3), (33, 31, 36, 40), (64, 64, 64, 64), (100, 40, 40, 104)])
def test_transpose(R, C, ld_src, ld_dst):
    """dst[c*ld_dst + r] = src[r*ld_src + c], bit for bit; dst's padding columns keep their sentinel."""
    src = torch.randn((R, ld_src), generator=torch.Generator().manual_seed(R + C)).to(DEV)
    dst = torch.full((C + 1, ld_dst), SENTINEL, device=DEV)
    _call("sv_transpose", _ptr(src), ld_src, R, C, _ptr(dst), ld_dst, _stream())
    torch.cuda.synchronize()
    assert torch.equal(dst[:C, :R], src[:, :C].T)
    assert (dst[:C, R:] == SENTINEL).all() and (dst[C] == SENTINEL).all()


@pytest.mark.parametrize("R,C", [(1, 1), (33, 255), (1025, 257), (5000, 24)])
def test_colsum(R, C):
    """sv_colsum against the fp64 column sums at one and several partial row chunks and a second
    column block (colsum_rows: chunks of 32 / 32 / 32 / 32 rows -> 1 / 2 / 33 / 157 chunks); a
    second call is bit-identical (the header's deterministic reduction)."""
    lib = _lib().lib()
    X = _randn(torch.Generator().manual_seed(R + C), R, C)
    Xd = _dev(X)
    nbytes = lib.sv_colsum_workspace(R, C)
    assert nbytes >= C * 4 and nbytes % (C * 4) == 0
    outs = []
    for _ in range(2):
        out = torch.full((C + 1,), SENTINEL, device=DEV)
        ws = _ws(nbytes)
        _call("sv_colsum", _ptr(Xd), R, C, _ptr(out), _ptr(ws), _stream())
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "sv_colsum is not deterministic"
    assert outs[0][C].item() == SENTINEL
    check(f"colsum.R{R}C{C}", _np(outs[0][:C]), X.astype(np.float64).sum(axis=0), X.sum(axis=0, dtype=np.float32))
