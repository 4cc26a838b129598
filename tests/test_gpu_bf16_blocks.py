"""The bf16 LSTM kernels against fp64, step by step, each step on the operands it read itself.

The bf16 forward saves everything a step consumes (h_bf, c_tm, the activated gates, hT) and the
backward leaves dgT, so oracle/bf16_stepwise.py recomputes every (layer, t) step in fp64 from the
GPU's own saved inputs to that step: no bf16 rounding flip propagates, and the comparison is at
fp32 level plus one bf16 rounding of known size (the rules, with the project's FACTOR = 8 and FLOOR
= 1e-6, are in that module's docstring; tests/test_bf16_stepwise_verifier.py shows on the CPU that
they accept a correct path and reject five seeded defects).

Rounding points (read in the kernels; all match include/sv_ge2e.h's bf16 variant):
  * K1 as its own launch (sv_gemm_bf16_bf: sv_lstm_layer_fwd_bf16, the per-step stack, every
    persistent layer but the fused one): XP = bf16(x q(W_ih)^T + b_ih + b_hh), fp32 accumulation,
    one rounding.  The test makes the same call (same M, N, K, leading dimensions, operand
    pointers; a fresh 256-byte-aligned output as the library's) and hands that XP to the verifier;
    XP itself must equal q(xp64) except on tie-near elements.  With T <= 4 the per-step stack's
    chunk (ops.PIPELINE_CHUNK = 32 steps) is the whole sequence, so its K1 has M = T B as well.
  * K1 fused into the persistent layer 0 (H = 768, F = 40; lstm_persist2_fwd_bf16_kernel XF = 5
    and the sv_persist3.hip forms): the MFMA over the zero-padded k range, then the two biases,
    rounded to bf16 (add_round_bf16x) BEFORE the h part is added.
  * the layer wavefront (sv_wave.hip, every layer): the x part is accumulated first, b_ih + b_hh
    added and the sum rounded to bf16 (round_bf2) in the accumulator, and the h part's MFMAs then
    add onto the rounded value -- "x and h parts in one accumulator" is a matter of summation
    order, not of a missing rounding.
  So every form computes q(XP) + h q(W_hh)^T; where XP cannot be read back the verifier assumes
  XP = q(xp64) and gives the cells with a tie-near x-projection element the loose bound.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bf16_cases
from oracle import bf16_stepwise as sw

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SENT = 1232.0   # exactly representable in bf16
NAN = float("nan")


def _lib():
    from pytorch_speaker_verification_amd import _lib
    return _lib


def _call(name, *args):
    _lib().call(name, *args)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=F32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).to(dtype).contiguous()


def _guarded(rows, cols, dtype, fill=NAN):
    """[rows + 1, cols] (cols = 0: a vector), the last row a sentinel the kernels must not touch."""
    t = torch.full((rows + 1, cols) if cols else (rows + 1,), fill, dtype=dtype, device=DEV)
    t[rows] = SENT
    return t


def _untouched(name, t):
    assert bool((t[-1] == SENT).all()), f"{name}: the row behind the buffer was written"


def _k1(inp, w_ih_bf, b_ih, b_hh):
    """The library's K1 call on its own: bf16(inp q(W_ih)^T + b_ih + b_hh) [T,B,4H]."""
    T, B, F = inp.shape
    G = w_ih_bf.shape[0]
    out = torch.full((T, B, G), NAN, dtype=BF, device=DEV)
    _call("sv_gemm_bf16_bf", T * B, G, F, _ptr(inp), F, _ptr(w_ih_bf), F, _ptr(out), G, _ptr(b_ih), _ptr(b_hh),
          _stream())
    return out


def _summary(rep):
    print(f"\nMEASURED {rep.name} worst of-bound {rep.worst:.3f} at {rep.worst_at}; tie-near share {rep.tie_share:.2e}")


# ------------------------------------------------------------------------- a. one layer
@functools.lru_cache(maxsize=None)
def _layer_fwd(B, F, H, T):
    sd, x, _ = bf16_cases.inputs(B, F, H, 1, T, bf16_cases.P_SMALL)
    (w,), _, _ = bf16_cases.layer_weights(sd, 1)
    Bp = (B + 7) // 8 * 8
    x_bf = _dev(x.transpose(1, 0, 2), BF)                       # [T,B,F]
    wd = dict(w_ih=_dev(w[0]), w_hh=_dev(w[1]), b_ih=_dev(w[2]), b_hh=_dev(w[3]))
    wd["w_ih_bf"], wd["w_hh_bf"] = wd["w_ih"].to(BF), wd["w_hh"].to(BF)
    gates, c_tm = _guarded(T * B, 4 * H, BF), _guarded(T * B, H, F32)
    h_tm, h_bf = _guarded((T + 1) * B, H, F32), _guarded((T + 1) * B, H, BF)
    hT = _guarded(H, (T + 1) * Bp, BF)
    _call("sv_lstm_layer_fwd_bf16", _ptr(x_bf), T, B, F, H, _ptr(wd["w_ih_bf"]), _ptr(wd["w_hh_bf"]), _ptr(wd["b_ih"]),
          _ptr(wd["b_hh"]), _ptr(gates), _ptr(c_tm), _ptr(h_tm), _ptr(h_bf), _ptr(hT), _stream())
    xp = _k1(x_bf, wd["w_ih_bf"], wd["b_ih"], wd["b_hh"])
    torch.cuda.synchronize()
    for k, t in dict(gates=gates, c_tm=c_tm, h_tm=h_tm, h_bf=h_bf, hT=hT).items():
        _untouched(f"layer_fwd.{k}", t)
    xT = torch.zeros((F, T, Bp), dtype=BF, device=DEV)
    xT[:, :, :B] = x_bf.permute(2, 0, 1)
    st = dict(B=B, T=T, Bp=Bp, x_bf=x_bf.cpu(), xT0=xT.reshape(F, T * Bp).cpu(),
              gates=[gates[:-1].view(T, B, 4 * H).cpu()], c_tm=[c_tm[:-1].view(T, B, H).cpu()],
              h_tm=[h_tm[:-1].view(T + 1, B, H).cpu()], h_bf=[h_bf[:-1].view(T + 1, B, H).cpu()],
              hT=[hT[:-1].cpu()])
    return dict(w=w, wd=wd, st=st, xp=xp.cpu(), dev=dict(gates=gates, c_tm=c_tm, hT=hT, xT=xT))


@pytest.mark.parametrize("B,F,H,T", bf16_cases.LAYER_CASES)
def test_layer_fwd_bf16(B, F, H, T):
    """sv_lstm_layer_fwd_bf16 (K1 + lstm_step_fwd_bf16_kernel per step) at every tile edge: each
    step's gates, c_tm, h_tm, h_bf from its own operands, the exact hT / padding / RNE checks, the
    K1 output against q(xp64), and a sentinel row behind every output buffer."""
    c = _layer_fwd(B, F, H, T)
    rep = sw.Report(f"layer_fwd.B{B}F{F}H{H}T{T}")
    sw.verify_forward(rep, [c["w"]], c["st"], xp_gpu=[c["xp"]])
    _summary(rep)


def _layer_bwd(c, B, F, H, T, dh_up, full, with_dx, with_db_hh):
    """sv_lstm_layer_bwd_bf16 on the forward's device buffers; returns the guarded outputs."""
    Bp = (B + 7) // 8 * 8
    wd, d = c["wd"], c["dev"]
    wihT, whhT = wd["w_ih"].T.contiguous().to(BF), wd["w_hh"].T.contiguous().to(BF)
    out = dict(dg=_guarded(T * B, 4 * H, BF), dgT=_guarded(4 * H, T * Bp, BF),
               dx=_guarded(T * B, F, F32) if with_dx else None, dw_ih=_guarded(4 * H, F, F32),
               dw_hh=_guarded(4 * H, H, F32), db_ih=_guarded(4 * H, 0, F32),
               db_hh=_guarded(4 * H, 0, F32) if with_db_hh else None)
    nbytes = _lib().lib().sv_lstm_layer_bwd_bf16_workspace(T, B, F, H)
    ws = torch.empty((nbytes + 3) // 4, dtype=F32, device=DEV)
    _call("sv_lstm_layer_bwd_bf16", T, B, F, H, _ptr(d["xT"]), T * Bp, _ptr(wihT), _ptr(whhT), _ptr(d["gates"]),
          _ptr(d["c_tm"]), _ptr(d["hT"]), _ptr(dh_up), int(full),
          *[_ptr(out[k]) for k in ("dg", "dgT", "dx", "dw_ih", "dw_hh", "db_ih", "db_hh")], _ptr(ws), _stream())
    torch.cuda.synchronize()
    for k, t in out.items():
        if t is not None:
            _untouched(f"layer_bwd.{k}", t)
    return out


@pytest.mark.parametrize("full", [1, 0], ids=["dh_up_full", "dh_up_last"])
@pytest.mark.parametrize("B,F,H,T", bf16_cases.LAYER_CASES)
def test_layer_bwd_bf16(B, F, H, T, full):
    """sv_lstm_layer_bwd_bf16 (lstm_step_bwd_bf16_kernel per step + the dW / db / dx launches) on the
    GPU forward's saved state, with a dense dh_up [T,B,H] and with [B,H] for the last step: each
    step's dG from the GPU's own dG_{t+1}, dg == dgT^T, zero dgT padding (the memset the kernel
    relies on when Bp != B; the buffers are pre-filled with NaN), dW_hh, dW_ih, db, dx from the bf16
    operands the launches read, db_ih == db_hh; then dx_tm = db_hh = NULL: every other output
    bit-identical."""
    c = _layer_fwd(B, F, H, T)
    g = torch.Generator().manual_seed(B + F + H + T + full)
    dh_up = torch.randn((T, B, H) if full else (B, H), generator=g)
    out = _layer_bwd(c, B, F, H, T, dh_up.to(DEV), full, True, True)
    top = torch.zeros(T, B, H)
    if full:
        top[:] = dh_up
    else:
        top[T - 1] = dh_up
    st = dict(c["st"], dg=[out["dg"][:-1].view(T, B, 4 * H).cpu()], dgT=[out["dgT"][:-1].cpu()])
    grads = {(0, k): out[f"d{k}"][:-1].cpu() for k in ("w_ih", "w_hh", "b_ih", "b_hh")}
    rep = sw.Report(f"layer_bwd.B{B}F{F}H{H}T{T}.full{full}")
    sw.verify_backward(rep, [c["w"]], st, (top.double(), top), grads=grads,
                       dx={0: out["dx"][:-1].view(T, B, F).cpu()})
    _summary(rep)
    part = _layer_bwd(c, B, F, H, T, dh_up.to(DEV), full, False, False)
    for k in ("dg", "dgT", "dw_ih", "dw_hh", "db_ih"):
        assert torch.equal(part[k].view(torch.int16 if part[k].dtype == BF else torch.int32),
                           out[k].view(torch.int16 if out[k].dtype == BF else torch.int32)), \
            f"{k} changed with dx_tm = db_hh = NULL"


# ------------------------------------------------------------------------- b / c. the stack
def _names(L):
    return [f"LSTM_stack.{n}_l{l}" for l in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + \
        ["projection.weight", "projection.bias"]


def _full_h_bf(st, l, L, T, B, H, Bp):
    """Layer l's h_bf [T+1,B,H]: the tensor the next layer's input is a view of; the top layer's is
    not kept by ops, so it is read back from its transposed copy hT (whose own check is then void)."""
    if l < L - 1:
        view = st.x_tm[l + 1]
        return view._base.view(T + 1, B, H) if view._base is not None else torch.cat([torch.zeros_like(view[:1]), view])
    return st.hT[l].view(H, T + 1, Bp)[:, :, :B].permute(1, 2, 0).contiguous()


def _run_stack(B, F, H, L, T, P, schedule, need_dx=False):
    """ops.embedder_forward_bf16 / embedder_backward_bf16 under `schedule` with a caller-owned sync
    block; the saved state in the verifier's layout, on `device`."""
    from pytorch_speaker_verification_amd import ops
    from pytorch_speaker_verification_amd._lib import PersistStatus
    sd, x, demb = bf16_cases.inputs(B, F, H, L, T, P)
    ps = [_dev(sd[k]) for k in _names(L)]
    layers = [tuple(ps[4 * l:4 * l + 4]) for l in range(L)]
    status = PersistStatus(torch.device(DEV, 0))
    emb, st = ops.embedder_forward_bf16(_dev(x), layers, ps[4 * L], ps[4 * L + 1], status=status, schedule=schedule)
    torch.cuda.synchronize()
    assert int(status.block[0]) == 0, "a persistent forward recurrence timed out"
    out = ops.embedder_backward_bf16(st, _dev(demb), layers, ps[4 * L], status=status, schedule=schedule,
                                     need_dx=need_dx)
    torch.cuda.synchronize()
    assert int(status.block[0]) == 0, "a persistent backward recurrence timed out"
    grads, dx = out if need_dx else (out, None)
    Bp = (B + 7) // 8 * 8
    state = dict(B=B, T=T, Bp=Bp, x_bf=st.x_tm[0], xT0=st.xT0, gates=st.gates, c_tm=st.c_tm, h_tm=st.h_tm,
                 h_bf=[_full_h_bf(st, l, L, T, B, H, Bp) for l in range(L)], hT=st.hT,
                 dgT=None if need_dx else st.dgT)
    return dict(st=st, state=state, layers=layers, grads=grads, dx=dx, ps=ps)


def _grad_dict(grads, L):
    return {(l, k): grads[4 * l + i] for l in range(L) for i, k in enumerate(("w_ih", "w_hh", "b_ih", "b_hh"))}


def _on(state, device):
    """The state's tensors on `device` (lists per layer stay lists)."""
    mv = lambda t: t if t is None or not torch.is_tensor(t) else t.to(device)  # noqa: E731
    return {k: [mv(t) for t in v] if isinstance(v, list) else mv(v) for k, v in state.items()}


def _dh_top(run, case, device):
    """(fp64, fp32) upstream dh of the top layer: the projection's backward of demb from the GPU's
    own h_last (fp32 slot T of the top layer), zero for t < T - 1."""
    B, F, H, L, T, P = case
    sd, _, demb = bf16_cases.inputs(*case)
    h_last = run["st"].h_tm[L - 1][T].to(device)
    top = []
    for dt in (sw.F64, sw.F32):
        a = torch.zeros(T, B, H, dtype=dt, device=device)
        a[T - 1] = sw.proj_backward(h_last, sd["projection.weight"], sd["projection.bias"], demb, dt)
        top.append(a)
    return top


def _check_stack(name, case, schedule, need_dx, fused, device, slots):
    """One stack case: forward and backward verified step by step.  fused: the layers whose
    x-projection cannot be read back (tie-near rule); every other layer's K1 is repeated here."""
    B, F, H, L, T, P = case
    run = _run_stack(*case, schedule, need_dx)
    sd, _, _ = bf16_cases.inputs(*case)
    ws, _, _ = bf16_cases.layer_weights(sd, L)
    st, layers = run["st"], run["layers"]
    xp = [None if l in fused else _k1(st.x_tm[l].contiguous(), layers[l][0].to(BF), layers[l][2], layers[l][3])
          for l in range(L)]
    torch.cuda.synchronize()
    state = _on(run["state"], device)
    rep = sw.Report(name)
    sw.verify_forward(rep, ws, state, xp_gpu=[None if t is None else t.to(device) for t in xp], h_tm_slots=slots)
    top = _dh_top(run, case, device)
    if not need_dx:
        sw.verify_backward(rep, ws, state, top, grads=_grad_dict([g.to(device) for g in run["grads"]], L))
        _summary(rep)
        return rep
    # need_dx: ops runs sv_lstm_layer_bwd_bf16 layer by layer through ONE dg / dgT buffer, so only
    # layer 0's dG survives.  The same calls are made here with a buffer per layer (the recurrences
    # are deterministic: same inputs, same dG), verified step by step, and ops' own gradients and dx
    # are then held to the fp64 products of those operands.
    Bp = state["Bp"]
    dh_up, full = _ops_dh_last(run, case), 0
    dgs, dgTs, mine, dxs = [None] * L, [None] * L, {}, {}
    for l in range(L - 1, -1, -1):
        Fl = F if l == 0 else H
        w_ih, w_hh = layers[l][0], layers[l][1]
        wihT, whhT = w_ih.T.contiguous().to(BF), w_hh.T.contiguous().to(BF)
        o = dict(dg=_guarded(T * B, 4 * H, BF), dgT=_guarded(4 * H, T * Bp, BF), dx=_guarded(T * B, Fl, F32),
                 dw_ih=_guarded(4 * H, Fl, F32), dw_hh=_guarded(4 * H, H, F32), db_ih=_guarded(4 * H, 0, F32),
                 db_hh=_guarded(4 * H, 0, F32))
        nbytes = _lib().lib().sv_lstm_layer_bwd_bf16_workspace(T, B, Fl, H)
        wsp = torch.empty((nbytes + 3) // 4, dtype=F32, device=DEV)
        xT, ld = (_ptr(st.xT0), T * Bp) if l == 0 else (_ptr(st.hT[l - 1]) + 2 * Bp, (T + 1) * Bp)
        _call("sv_lstm_layer_bwd_bf16", T, B, Fl, H, xT, ld, _ptr(wihT), _ptr(whhT), _ptr(st.gates[l]),
              _ptr(st.c_tm[l]), _ptr(st.hT[l]), _ptr(dh_up), full,
              *[_ptr(o[k]) for k in ("dg", "dgT", "dx", "dw_ih", "dw_hh", "db_ih", "db_hh")], _ptr(wsp), _stream())
        torch.cuda.synchronize()
        for k, t in o.items():
            _untouched(f"{name}.l{l}.{k}", t)
        dgs[l], dgTs[l] = o["dg"][:-1].view(T, B, 4 * H), o["dgT"][:-1]
        dxs[l] = o["dx"][:-1].view(T, B, Fl)
        for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
            mine[(l, k)] = o[f"d{k}"][:-1]
        dh_up, full = dxs[l].contiguous(), 1
    state = dict(state, dg=[t.to(device) for t in dgs], dgT=[t.to(device) for t in dgTs])
    sw.verify_backward(rep, ws, state, top, grads={k: v.to(device) for k, v in mine.items()},
                       dx={l: t.to(device) for l, t in dxs.items()})
    ops_rep = sw.Report(name + ".ops")
    sw.verify_backward(ops_rep, ws, state, top, grads=_grad_dict([g.to(device) for g in run["grads"]], L),
                       dx={0: run["dx"].permute(1, 0, 2).contiguous().to(device)})
    rep.worst = max(rep.worst, ops_rep.worst)
    _summary(rep)
    return rep


def _ops_dh_last(run, case):
    """dh_last [B,H] on the GPU as ops forms it (sv_proj_norm_bwd), for the repeated per-layer calls."""
    from pytorch_speaker_verification_amd import ops
    B, F, H, L, T, P = case
    _, _, demb = bf16_cases.inputs(*case)
    _, dh_last = ops._proj_norm_bwd(run["st"], _dev(demb), run["layers"], run["ps"][4 * L], None, _stream())
    return dh_last


@pytest.mark.parametrize("need_dx", [False, True], ids=["stacked", "need_dx"])
@pytest.mark.parametrize("schedule", ["per_step", "persist"])
@pytest.mark.parametrize("B,F,H,L,T", bf16_cases.STACK_CASES)
def test_stack_bf16(B, F, H, L, T, schedule, need_dx):
    """The bf16 stack through ops under the per-step schedule (K1 per chunk + step kernels, layer
    pipelined) and the persistent one (K1 + lstm_persist_fwd_bf16_kernel / the W-stationary backward
    at H = 64, 96), stacked backward and need_dx (the per-layer backward), L = 2 and 3, B = 35
    (ragged, Bp = 40), 64 (one row block, Bp == B) and 65.  Every layer's K1 is a separate
    sv_gemm_bf16_bf call of M = T B rows (T <= 4 is one chunk), repeated here on the same operands.
    The persistent forward guarantees only slot T of the fp32 h_tm; h_bf is checked at every slot."""
    lib = _lib().lib()
    if schedule == "persist":
        assert lib.sv_persist_fwd_ok(B, H) and lib.sv_persist_bwd_ok(B, H)
    slots = "all" if schedule == "per_step" else "last"
    name = f"stack.{schedule}.B{B}F{F}H{H}L{L}T{T}{'.dx' if need_dx else ''}"
    _check_stack(name, (B, F, H, L, T, bf16_cases.P_SMALL), schedule, need_dx, fused=(), device="cpu", slots=slots)


@pytest.mark.parametrize("B,T,schedule", bf16_cases.H768_CASES)
def test_stack_bf16_h768(B, T, schedule):
    """F = 40, H = 768, L = 3, one B per kernel family (dispatch read in sv_persist_plan.h:
    persist_plan, used by sv_persist_fwd_bf16, sv_persist_bwd_bf16 and sv_persist_bm; sv_wave.hip:
    sv_wave_fwd_fits; on 256 CUs):
      auto, B = 33, 80        the layer wavefront forward and backward (sv_wave_ok: 3 x 24 x
                              ceil(B / 32) <= 256 workgroups, i.e. B <= 96); B = 33 is a second 32-row
                              block of one row.  Every layer's x-projection is fused (tie-near rule).
      per_layer, B = 84, 160  lstm_persist2_fwd_bf16_kernel / lstm_persist2_bwd_bf16_kernel with the
                              32-row tile (persist_plan: 24 x ceil(B / 32) <= 256, every B <= 320; B =
                              84 has a ragged last block and Bp = 88, 160 is five full blocks)
      per_layer, B = 288      the 16-row wide forward (fwd16: B % 16 == 0, 256 < B <= 320), the
                              32-row backward
      per_layer, B = 340      the wide sv_persist3.hip pair (wide: 320 < B <= 672; 340 = 10 x 32
                              + 20, not a multiple of its 32-row tile, Bp = 344)
    The 64-row tile of the W-stationary kernels is not reachable at H = 768 on a 256-CU device:
    the 32-unit tile needs 64 rows only for B > 320, where the wide pair takes over up to B = 672, and
    beyond B = 640 the 64-row grid (24 x 11) no longer fits; its H = 768 instantiations are gone, and
    it runs at H = 64 / 96 in
    test_stack_bf16.  Under per_layer layer 0's projection is fused into its recurrence
    (sv_persist_fwd_fusex_ok), layers 1 and 2 take the K1 GEMM, repeated here.  The fp64 reference
    is stock torch fp64 on the device.  Only slot T of the fp32 h_tm is guaranteed."""
    lib = _lib().lib()
    F, H, L = 40, 768, 3
    if schedule == "auto":
        assert lib.sv_wave_ok(L, T, B, F, H), "the layer wavefront does not fit: another kernel would run"
        fused = (0, 1, 2)
    else:
        assert lib.sv_persist_fwd_ok(B, H) and lib.sv_persist_bwd_ok(B, H)
        fused = (0,)
    _check_stack(f"h768.{schedule}.B{B}T{T}", (B, F, H, L, T, bf16_cases.P_768), schedule, False, fused=fused,
                 device=DEV, slots="last")


# ------------------------------------------------------------------------- d. a stack of one layer
def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


# the smallest (B, F, H) case with B % 8 != 0 (Bp padding: hT and dgT zeroed), and the next one, whose
# T = 3 also runs a K1 of several steps and the backward's dcf ping-pong
@pytest.mark.parametrize("B,F,H,T", sorted(c for c in bf16_cases.LAYER_CASES if c[0] % 8)[:2])
def test_stack_of_one_layer_is_the_layer_bf16(B, F, H, T):
    """The single-layer entry points and the per-step stack run one set of host pieces (the BFwd /
    BBwd sequences of sv_bf16.hip): under per_step, sv_lstm_stack_fwd_bf16 with L = 1 gives gates, c,
    h, h_bf and hT bit-identical to sv_lstm_layer_fwd_bf16, and sv_lstm_stack_bwd_bf16 with L = 1
    (its wt filled by sv_lstm_weights_bf16, SV_SCHED_WT_READY) gives dg, dgT, dW_ih, dW_hh and db
    bit-identical to sv_lstm_layer_bwd_bf16 without dx_tm, both from the same forward buffers."""
    from pytorch_speaker_verification_amd import ops
    lib_ = _lib()
    c = _layer_fwd(B, F, H, T)
    wd, d, st = c["wd"], c["dev"], c["st"]
    Bp, dev, sched = st["Bp"], torch.device(DEV, 0), lib_.schedule_flags("per_step")
    one = lambda t: ops._parr([t])  # noqa: E731
    x_bf = st["x_bf"].to(DEV)
    o = dict(gates=_guarded(T * B, 4 * H, BF), c_tm=_guarded(T * B, H, F32), h_tm=_guarded((T + 1) * B, H, F32),
             h_bf=_guarded((T + 1) * B, H, BF), hT=_guarded(H, (T + 1) * Bp, BF))
    nch = (T + ops.PIPELINE_CHUNK - 1) // ops.PIPELINE_CHUNK
    sp, ep, _ = ops._side(dev, "fwd", 1, nch + 1)
    _call("sv_lstm_stack_fwd_bf16", 1, T, B, F, H, _ptr(x_bf), one(wd["w_ih_bf"]), one(wd["w_hh_bf"]),
          one(wd["b_ih"]), one(wd["b_hh"]), one(o["gates"]), one(o["c_tm"]), one(o["h_tm"]), one(o["h_bf"]),
          one(o["hT"]), ops.PIPELINE_CHUNK, _stream(), sp, ep, None, None, sched)
    torch.cuda.synchronize()
    for k, t in o.items():
        _untouched(f"stack_of_one.{k}", t)
        assert torch.equal(_bits(t[:-1].cpu()).reshape(-1), _bits(st[k][0]).reshape(-1)), f"forward {k} differs"

    dh_last = torch.randn((B, H), generator=torch.Generator().manual_seed(B + F + H + T)).to(DEV)
    ref = _layer_bwd(c, B, F, H, T, dh_last, 0, False, True)
    wt = ops._ws(lib_.lib().sv_lstm_wt_bf16_size(1, F, H), dev)
    w_bf = [torch.empty_like(wd["w_ih_bf"]), torch.empty_like(wd["w_hh_bf"])]
    _call("sv_lstm_weights_bf16", 1, F, H, one(wd["w_ih"]), one(wd["w_hh"]), one(w_bf[0]), one(w_bf[1]), _ptr(wt),
          _stream())
    g = dict(dg=_guarded(T * B, 4 * H, BF), dgT=_guarded(4 * H, T * Bp, BF), dw_ih=_guarded(4 * H, F, F32),
             dw_hh=_guarded(4 * H, H, F32), db_ih=_guarded(4 * H, 0, F32), db_hh=_guarded(4 * H, 0, F32))
    ws = ops._ws(lib_.lib().sv_lstm_stack_bwd_bf16_workspace(1, T, B, F, H), dev)
    sp, ep, _ = ops._side(dev, "bwd", 1, nch + 2)
    _call("sv_lstm_stack_bwd_bf16", 1, T, B, F, H, one(d["xT"]), (ctypes.c_long * 1)(T * Bp), one(wd["w_ih"]),
          one(wd["w_hh"]), one(d["gates"]), one(d["c_tm"]), one(d["hT"]), _ptr(dh_last), one(g["dg"]), one(g["dgT"]),
          one(None), one(g["dw_ih"]), one(g["dw_hh"]), one(g["db_ih"]), one(g["db_hh"]), _ptr(ws), _ptr(wt),
          ops.PIPELINE_CHUNK, _stream(), sp, ep, None, None, sched | lib_.SV_SCHED_WT_READY)
    torch.cuda.synchronize()
    for k, t in g.items():
        _untouched(f"stack_of_one.{k}", t)
        assert torch.equal(_bits(t), _bits(ref[k])), f"backward {k} differs"
