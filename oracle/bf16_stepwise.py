"""STEP-WISE VERIFIER (test infrastructure only) of the bf16 LSTM path: every (layer, t) step of
a bf16 forward and backward recomputed in fp64 from the operands that very step read on the GPU
(teacher-forced), so no bf16 rounding flip ever propagates and what is left is fp32 summation
noise plus one bf16 rounding of known size.

State (``st``): a dict in the layouts of include/sv_ge2e.h, time-major, Bp = B rounded up to 8
(oracle.lstm_bf16.gpu_state builds one on the CPU; tests/test_gpu_bf16_blocks.py fills one from the
GPU's buffers).  Per layer lists ``gates`` [T,B,4H] (bf16 activations), ``c_tm`` [T,B,H], ``h_tm``
[T+1,B,H] (fp32), ``h_bf`` [T+1,B,H], ``hT`` [H,(T+1)Bp], ``dgT`` [4H,T*Bp], optionally ``dg``
[T,B,4H]; ``x_bf`` [T,B,F], ``xT0`` [F,T*Bp].  Any float dtype; everything is widened to fp64.

  forward step (l, t)   z = XP_t + h_bf[l][t] q(W_hh)^T, the cell from z and the GPU's c_tm[l][t-1];
                        layer l > 0 reads the GPU's h_bf[l-1][t+1]; XP = bf16(x q(W_ih)^T + b_ih + b_hh)
  backward step (l, t)  dh = dh_up[t] + dG_gpu[t+1] q(W_hh); dc carried in fp64 (no bf16 rounding in
                        that chain); activations, c_t, c_{t-1} the GPU's; for l < L-1 dh_up = the
                        GPU's dG of layer l+1 times q(W_ih[l+1]) in fp64 (the dx GEMM)
  weight gradients      dW_hh = dgT hT[:, :T Bp]^T, dW_ih = dgT xT^T, db = row sums of dgT, dx = dG q(W_ih):
                        fp64 products of exactly the bf16 operands the launch read

Comparison rules (the constants are the project's, tests/test_gpu_lstm_blocks.py; none is new):
  fp32 outputs   max|gpu - ref64| <= FACTOR * max(d_ref32, FLOOR) * max|ref64|, ref32 = the same
                 step formula in fp32 on the CPU, d_ref32 = max|ref32 - ref64| / max|ref64|
  bf16 outputs   per element |gpu - ref64| <= |q(ref64) - ref64| + 2 * noise, noise = that fp32
                 bound: the stored value is the RNE rounding of a value within noise of the truth
                 (crossing a rounding tie at distance d <= noise costs exactly 2 d)
  exact          h_bf == RNE(h_tm), hT blocks and zero padding, dgT zero padding, dg == dgT^T
Where the GPU's x-projection cannot be read (K1 fused into the recurrence) XP = q(xp64) is assumed
and the cells with a tie-near x-projection element -- xp64 within TIE_WINDOW * (|x| |q(W_ih)|^T +
|b_ih| + |b_hh|) of a bf16 rounding tie, 8 fp32 ulps of the absolute sum -- get the loose bound of a
1-ulp flip of XP pushed through the activation slopes (sigmoid <= 1/4, tanh <= 1).  The tie-near
share is computed from the reference alone and must stay <= TIE_CAP.

Every check prints a MEASURED line and a failed one raises Mismatch (an AssertionError).
"""
from __future__ import annotations

import torch

FACTOR, FLOOR = 8.0, 1e-6   # tests/test_gpu_lstm_blocks.py
TIE_WINDOW = 2.0 ** -21
TIE_CAP = 0.02
F64, F32 = torch.float64, torch.float32


class Mismatch(AssertionError):
    pass


# bf16 keeps 7 of fp64's 52 fraction bits.  Integer arithmetic on the fp64 bit patterns: exact on
# any device (torch.ldexp goes through pow(2, e), which a GPU's fast powf need not return exactly).
_DROP = 45
_MASK = (1 << _DROP) - 1


def q64(v):
    """RNE to bf16 of an fp64 tensor, in fp64 (one rounding; normal range)."""
    bits = v.contiguous().view(torch.int64)
    lsb = (bits >> _DROP) & 1
    return ((bits + ((1 << (_DROP - 1)) - 1) + lsb) & ~_MASK).view(F64)


def ulp_bf16(v):
    """The bf16 spacing at |v| (fp64; v = 0: the spacing of the smallest normal binade)."""
    e = ((v.contiguous().view(torch.int64) >> 52) & 0x7FF).clamp_min(8)
    return ((e - 7) << 52).view(F64)


def tie_distance(v):
    """Distance of fp64 v to the nearest bf16 rounding tie."""
    a = v.abs().contiguous()
    lo = (a.view(torch.int64) & ~_MASK).view(F64)   # |v| truncated to bf16
    return (a - (lo + 0.5 * ulp_bf16(a))).abs()


def _qw(w, dev):
    """q(W) of an fp32 master weight, fp64."""
    return torch.as_tensor(w, dtype=F32).to(torch.bfloat16).to(F64).to(dev)


def _d(a, dev):
    return torch.as_tensor(a).to(dev).to(F64)


def _c32(a):
    """fp32 on the CPU: where ref32, "the same formula in fp32 on the CPU", is evaluated."""
    return a.to(F32).cpu()


class Report:
    """Collects the MEASURED lines of one case and the worst ratio of a deviation to its bound."""

    def __init__(self, name, verbose=True):
        self.name, self.verbose = name, verbose
        self.worst = 0.0          # worst deviation / bound over the tolerance checks
        self.worst_at = ""
        self.tie_share = 0.0      # largest tie-near share of an x-projection
        self.lines = []

    def _say(self, line):
        self.lines.append(line)
        if self.verbose:
            print("\nMEASURED " + line)

    def _ratio(self, what, ratio):
        if ratio > self.worst:
            self.worst, self.worst_at = ratio, what

    @staticmethod
    def _shapes(what, gpu, ref64, ref32):
        if not (gpu.shape == ref64.shape == ref32.shape):
            raise Mismatch(f"{what}: shapes {tuple(gpu.shape)} {tuple(ref64.shape)} {tuple(ref32.shape)}")
        if not bool(torch.isfinite(gpu).all()) or not bool(torch.isfinite(ref64).all()):
            raise Mismatch(f"{what}: non-finite values")

    def noise(self, ref64, ref32):
        """(fp32 bound as an absolute number, d_ref32, scale) of a quantity."""
        scale = float(ref64.abs().max())
        d_ref = float((ref32.to(ref64.device).to(F64) - ref64).abs().max()) / scale if scale else 0.0
        return FACTOR * max(d_ref, FLOOR) * scale, d_ref, scale

    def fp32(self, what, gpu, ref64, ref32, loose=None):
        """The calibrated fp32 rule; `loose` [same shape]: an additional per-element allowance."""
        what = f"{self.name}.{what}"
        gpu = gpu.to(F64)
        self._shapes(what, gpu, ref64, ref32)
        bound, d_ref, scale = self.noise(ref64, ref32)
        if scale == 0:
            self._say(f"{what} reference is zero, gpu {float(gpu.abs().max()):.3e}")
            if bool((gpu != 0).any()):
                raise Mismatch(f"{what}: nonzero where the reference is exactly zero")
            return
        err = (gpu - ref64).abs()
        allowed = bound if loose is None else bound + loose
        ratio = float((err / allowed).max())
        self._say(f"{what} gpu {float(err.max()) / scale:.3e} ref32 {d_ref:.3e} of-bound {ratio:.3f}")
        self._ratio(what, ratio)
        if ratio > 1.0:
            raise Mismatch(f"{what}: {ratio:.3f} of its fp32 bound ({float(err.max()) / scale:.3e} vs ref32 {d_ref:.3e})")

    def bf16(self, what, gpu, ref64, ref32, loose=None):
        """A stored bf16 output: per element |gpu - ref64| <= |q(ref64) - ref64| + 2 noise (+ loose)."""
        what = f"{self.name}.{what}"
        gpu = gpu.to(F64)
        self._shapes(what, gpu, ref64, ref32)
        noise, d_ref, scale = self.noise(ref64, ref32)
        qr = q64(ref64)
        err = (gpu - ref64).abs()
        allowed = (qr - ref64).abs() + 2.0 * noise
        if loose is not None:
            # the stored value is then the rounding of another value, up to loose + noise from the
            # truth: that distance plus half a bf16 spacing there
            other = loose + noise + 0.5 * ulp_bf16(ref64.abs() + loose + noise)
            allowed = torch.where(loose > 0, torch.maximum(allowed, other), allowed)
        # the ratio is taken on what exceeds the rounding itself, against the 2 * noise allowance
        over = (err - (qr - ref64).abs()).clamp_min(0.0)
        ratio = float((over / (allowed - (qr - ref64).abs())).max())
        share = float((gpu != qr).to(F64).mean())
        self._say(f"{what} not-q(ref64) share {share:.2e} ref32 {d_ref:.3e} of-bound {ratio:.3f}")
        self._ratio(what, ratio)
        if bool((err > allowed).any()):
            n = int((err > allowed).sum())
            raise Mismatch(f"{what}: {n} elements beyond the rounding of a value within fp32 noise "
                           f"(worst {ratio:.3f} of the allowance)")

    def exact(self, what, ok):
        if not bool(ok):
            raise Mismatch(f"{self.name}.{what}")


def _cell(z, c_prev, H):
    i, f = torch.sigmoid(z[..., :H]), torch.sigmoid(z[..., H:2 * H])
    g, o = torch.tanh(z[..., 2 * H:3 * H]), torch.sigmoid(z[..., 3 * H:])
    c = f * c_prev + i * g
    return torch.cat([i, f, g, o], dim=-1), c, o * torch.tanh(c)


def x_projection(rep, what, inp, w_ih, b_ih, b_hh, xp_gpu=None):
    """xp64 = inp q(W_ih)^T + b_ih + b_hh [T,B,4H], its tie-near mask (from the reference alone;
    share asserted <= TIE_CAP) and, if the GPU's stored projection is given, its check: equal to
    q(xp64), the neighbouring bf16 value allowed on tie-near elements only."""
    dev = inp.device
    qw = _qw(w_ih, dev)
    bias = _d(b_ih, dev) + _d(b_hh, dev)
    xp = inp @ qw.T + bias
    absum = inp.abs() @ qw.abs().T + _d(b_ih, dev).abs() + _d(b_hh, dev).abs()
    window = TIE_WINDOW * absum
    near = tie_distance(xp) <= window
    share = float(near.to(F64).mean())
    rep.tie_share = max(rep.tie_share, share)
    rep._say(f"{rep.name}.{what} tie-near share {share:.2e}")
    if share > TIE_CAP:
        raise Mismatch(f"{rep.name}.{what}: tie-near share {share:.3f} > {TIE_CAP}")
    if xp_gpu is not None:
        xg, qx = xp_gpu.to(F64), q64(xp)
        diff = (xg - qx).abs()
        flips = float((diff != 0).to(F64).mean())
        rep._say(f"{rep.name}.{what} != q(xp64) share {flips:.2e}")
        rep.exact(f"{what}: differs from q(xp64) off the tie-near elements", (diff[~near] == 0).all())
        # the neighbouring value, stated so that it also holds where |xp64| is itself below the
        # window (a cancelled sum, whose bf16 spacing is far finer than fp32 noise of the addends):
        # the rounding of some value within the window of xp64
        reach = window + 0.5 * ulp_bf16(xp.abs() + window)
        rep.exact(f"{what}: beyond the neighbouring bf16 value on a tie-near element",
                  ((xg - xp).abs()[near] <= reach[near]).all())
    return xp, near, window


def verify_forward(rep, weights, st, xp_gpu=None, h_tm_slots="all"):
    """Every forward step of every layer.  weights: [(w_ih, w_hh, b_ih, b_hh)] fp32 masters.
    xp_gpu: per layer the GPU's stored x-projection [T,B,4H] (the test's own K1 call), or None for
    a layer whose projection is fused into the recurrence.  h_tm_slots: "all", or "last" where the
    schedule guarantees only slot T of the fp32 h_tm."""
    dev = st["x_bf"].device
    T, B, Bp = st["T"], st["B"], st["Bp"]
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(weights):
        H = w_hh.shape[1]
        inp = _d(st["x_bf"] if l == 0 else st["h_bf"][l - 1][1:], dev)
        given = None if xp_gpu is None else xp_gpu[l]
        xp, near, window = x_projection(rep, f"l{l}.xp", inp, w_ih, b_ih, b_hh, given)
        XP = _d(given, dev) if given is not None else q64(xp)
        h_bf, h_tm, c_tm = _d(st["h_bf"][l], dev), _d(st["h_tm"][l], dev), _d(st["c_tm"][l], dev)
        c_prev = torch.cat([torch.zeros_like(c_tm[:1]), c_tm[:-1]])
        qwhh = _qw(w_hh, dev)
        a64, c64, h64 = _cell(XP + h_bf[:T] @ qwhh.T, c_prev, H)
        a32, c32, h32 = _cell(_c32(XP) + _c32(h_bf[:T]) @ _c32(qwhh).T, _c32(c_prev), H)
        la = lc = lh = None
        if given is None:  # a 1-ulp flip of XP on the tie-near elements, through the slopes
            flip = torch.where(near, ulp_bf16(xp.abs() + window) + window, torch.zeros_like(xp))
            fi, ff, fg, fo = (flip[..., k * H:(k + 1) * H] for k in range(4))
            la = torch.cat([fi / 4, ff / 4, fg, fo / 4], dim=-1)
            lc = ff / 4 * c_prev.abs() + fi / 4 + fg
            lh = fo / 4 + lc
        rep.bf16(f"l{l}.gates", _d(st["gates"][l], dev), a64, a32, la)
        rep.fp32(f"l{l}.c_tm", c_tm, c64, c32, lc)
        rep.exact(f"l{l}: h_tm / h_bf slot 0 not zero", (h_tm[0] == 0).all() and (h_bf[0] == 0).all())
        rep.bf16(f"l{l}.h_bf", h_bf[1:], h64, h32, lh)
        lo = 0 if h_tm_slots == "all" else T - 1
        rep.fp32(f"l{l}.h_tm", h_tm[1 + lo:], h64[lo:], h32[lo:], None if lh is None else lh[lo:])
        rne = st["h_tm"][l].to(dev).to(F32).to(torch.bfloat16).to(F64)
        rep.exact(f"l{l}: h_bf != RNE(h_tm)", (rne[1 + lo:] == h_bf[1 + lo:]).all())
        if st.get("hT") and st["hT"][l] is not None:
            hT = _d(st["hT"][l], dev).reshape(H, T + 1, Bp)
            rep.exact(f"l{l}: hT block 0 not zero", (hT[:, 0] == 0).all())
            rep.exact(f"l{l}: hT padding columns not zero", (hT[:, :, B:] == 0).all())
            rep.exact(f"l{l}: hT block t+1 != h_bf[t+1]^T", (hT[:, 1:, :B] == h_bf[1:].permute(2, 0, 1)).all())


def proj_backward(h_last, w_p, b_p, demb, dt=F64):
    """dh_last [B,H] of emb = y / |y|, y = h_last W_p^T + b_p, in dtype dt."""
    dev = h_last.device
    h, w, d = h_last.to(dt), torch.as_tensor(w_p).to(dev).to(dt), torch.as_tensor(demb).to(dev).to(dt)
    y = h @ w.T + torch.as_tensor(b_p).to(dev).to(dt)
    n = (y * y).sum(dim=1, keepdim=True).sqrt()
    e = y / n
    return ((d - e * (d * e).sum(dim=1, keepdim=True)) / n) @ w


def dg_of(st, l):
    """The GPU's dG of layer l as [T,B,4H] fp64, read back from dgT."""
    T, B, Bp = st["T"], st["B"], st["Bp"]
    dgT = st["dgT"][l]
    return dgT.to(F64).reshape(dgT.shape[0], T, Bp)[:, :, :B].permute(1, 2, 0).contiguous()


def _bwd_chain(dt, dh, acts, c_tm, c_prev, H):
    dh, acts, c_tm, c_prev = (a.to(dt) for a in (dh, acts, c_tm, c_prev))
    i, f, g, o = (acts[..., k * H:(k + 1) * H] for k in range(4))
    tc = torch.tanh(c_tm)
    T = dh.shape[0]
    dG = torch.empty_like(acts)
    dcn = torch.zeros_like(c_tm[0])
    for t in range(T - 1, -1, -1):
        dc = dcn + dh[t] * o[t] * (1 - tc[t] * tc[t])
        dG[t] = torch.cat([dc * g[t] * i[t] * (1 - i[t]), dc * c_prev[t] * f[t] * (1 - f[t]),
                           dc * i[t] * (1 - g[t] * g[t]), dh[t] * tc[t] * o[t] * (1 - o[t])], dim=-1)
        dcn = dc * f[t]
    return dG


def verify_backward(rep, weights, st, dh_top, grads=None, dx=None, layers=None, db_pairs=True):
    """Every backward step of the layers in ``layers`` (default all), top down.  dh_top: (fp64,
    fp32) pair of the top verified layer's upstream dh [T,B,H] (zeros where none arrives).
    grads: {(l, "w_ih" | "w_hh" | "b_ih" | "b_hh"): tensor} of the GPU's weight gradients to check
    (a missing key is skipped); dx: {l: [T,B,F_l]} of the GPU's input gradients."""
    dev = st["x_bf"].device
    T, B, Bp = st["T"], st["B"], st["Bp"]
    L = len(weights)
    layers = list(range(L - 1, -1, -1)) if layers is None else layers
    grads, dx = grads or {}, dx or {}
    for l in layers:
        w_ih, w_hh = weights[l][0], weights[l][1]
        H = w_hh.shape[1]
        dgT = _d(st["dgT"][l], dev)
        dG = dg_of(st, l).to(dev)
        rep.exact(f"l{l}: dgT padding columns not zero", (dgT.reshape(4 * H, T, Bp)[:, :, B:] == 0).all())
        if st.get("dg") and st["dg"][l] is not None:
            rep.exact(f"l{l}: dg != dgT^T", (_d(st["dg"][l], dev) == dG).all())
        if l == layers[0]:
            up64, up32 = dh_top[0].to(dev).to(F64), _c32(dh_top[1])
        else:  # the dx GEMM of the layer above, from the GPU's own dG
            above, qwa = dg_of(st, l + 1).to(dev), _qw(weights[l + 1][0], dev)
            up64, up32 = above @ qwa, _c32(above) @ _c32(qwa)
        qwhh = _qw(w_hh, dev)
        rec = torch.cat([dG[1:] @ qwhh, torch.zeros_like(up64[:1])])
        rec32 = torch.cat([_c32(dG[1:]) @ _c32(qwhh), torch.zeros_like(up32[:1])])
        acts, c_tm = _d(st["gates"][l], dev), _d(st["c_tm"][l], dev)
        c_prev = torch.cat([torch.zeros_like(c_tm[:1]), c_tm[:-1]])
        r64 = _bwd_chain(F64, up64 + rec, acts, c_tm, c_prev, H)
        r32 = _bwd_chain(F32, up32 + rec32, acts.cpu(), c_tm.cpu(), c_prev.cpu(), H)
        rep.bf16(f"l{l}.dG", dG, r64, r32)
        # weight gradients from exactly the operands the launch read
        hprev = _d(st["hT"][l], dev)[:, :T * Bp]
        xin = _d(st["xT0"], dev) if l == 0 else _d(st["hT"][l - 1], dev)[:, Bp:(T + 1) * Bp]
        refs = {"w_hh": (dgT @ hprev.T, _c32(dgT) @ _c32(hprev).T),
                "w_ih": (dgT @ xin.T, _c32(dgT) @ _c32(xin).T),
                "b_ih": (dgT.sum(dim=1), _c32(dgT).sum(dim=1))}
        refs["b_hh"] = refs["b_ih"]
        for k, (a, b) in refs.items():
            if (l, k) in grads:
                rep.fp32(f"l{l}.d{k}", grads[(l, k)].to(dev), a, b)
        if db_pairs and (l, "b_ih") in grads and (l, "b_hh") in grads:
            rep.exact(f"l{l}: db_ih != db_hh", torch.equal(grads[(l, "b_ih")], grads[(l, "b_hh")]))
        if l in dx:
            qwih = _qw(w_ih, dev)
            rep.fp32(f"l{l}.dx", dx[l].to(dev), dG @ qwih, _c32(dG) @ _c32(qwih))
