"""The inputs, case table, comparison and bounds of the GE2E edge tests, shared by
tests/test_ge2e_cases.py (CPU: the oracle off the unit sphere, the conditioning cap, the metric's
self-checks) and tests/test_gpu_ge2e_edges.py (the HIP kernels of csrc/sv_ge2e.hip).

Inputs are OFF the unit sphere: every other GE2E input of the suite has |E_r| = 1, where a wrong or
missing 1/|e| factor cannot be seen.  The reference is the fp64 numpy oracle (oracle/ge2e_np.py);
the fp32 torch port (oracle/torch_port.py, CPU autograd) sets the scale of the bounds.

Bounds.  PORT_MAX[stat] is the largest error the fp32 port shows against the fp64 oracle over
every input of the table below (the fused, split and sharded cases alike), measured on the
CPU with one thread and rounded UP to two digits; BOUNDS[stat] = K * PORT_MAX[stat] with K = 4.  K
is there because the kernels sum in another order than torch; no kernel measurement enters.
tests/test_ge2e_cases.py asserts per case that the port stays within BOUNDS / K, so the table
cannot drift away from the constants (a case that breaks the cap gets other inputs, never a wider
bound).  The port's measured maxima (this table, noise 1.5):
    per_abs 3.71e-05 (257,2,16)   dE_row 2.36e-05 (3,17,64)   loss_abs 9.73e-06 (255,2,256)
    dw 2.55e-07 (7,16,36)         db 5.13e-08 (129,2,252)
per_abs is that large for fp32 because U_r = (sum_i E_ji - E_r) / (M - 1) cancels when a row of
norm 20 shares a speaker with one of norm 0.05 (M = 2 is the worst); the reference, the port and
the kernels all form U that way, so it is the inputs' conditioning and not any one's defect.
"""
import functools
import math

import numpy as np

from oracle import ge2e_np

# ---------------------------------------------------------------------------------- the table
# (N, M, D, w, b), and the path of csrc/sv_ge2e.hip each must reach
FUSED_CASES = [
    (5, 2, 4, 10.0, -5.0),       # smallest: rows_kernel<2>, one live lane per row
    (7, 16, 36, 10.0, -5.0),     # M = GF_MMAX (prep: 4 passes of RW rows; 16-wave finalize), 27 dead d lanes
    (6, 13, 100, 3.7, -1.2),     # M % 4 != 0, M > GF_COLU, D % 64 != 0
    (128, 3, 8, 10.0, -5.0),     # the tile boundary of rows_kernel<2> (N == GF_TILE)
    (129, 2, 252, 10.0, -5.0),   # rows_kernel<4> (N > GF_TILE, D != 256), ragged second tile, M = 2
    (255, 3, 8, 10.0, -5.0),     # rows_kernel<4>, Np = 256 != N
    (129, 11, 256, 10.0, -5.0),  # rows4r<false>, M > GF_COLU
    (130, 3, 256, 10.0, -5.0),   # rows4r<false>, Np = 132
    (255, 2, 256, 10.0, -5.0),   # rows4r<false>, the last chunk one short
    (4, 5, 64, 1.0, -14.0),      # every S < 0 and sum_k e^S about the 1e-6 inside the log
    (4, 5, 64, -2.0, 0.5),       # negative w
]
# outside sv_ge2e_train_ok: ops.ge2e_train dispatches these to the split kernels
SPLIT_CASES = [
    (3, 17, 64, 10.0, -5.0),     # M > GF_MMAX_FIN: ge2e_finalize_serial_kernel
    (257, 2, 16, 10.0, -5.0),    # N > GF_NMAX
    (4, 3, 260, 10.0, -5.0),     # D > GF_DMAX
    (5, 4, 38, 10.0, -5.0),      # D % 4 != 0: ops._pad_d (see PADDED_FUSED below)
]
# sv_ge2e_train_ok is 0 for (5, 4, 38) itself, but ops.ge2e_train zero-pads D to 40 before it asks,
# so this one case then runs the FUSED kernels on the padded rows; ops.ge2e_forward / ge2e_backward
# run it through the split kernels with the same padding.  Both are checked.
PADDED_FUSED = {(5, 4, 38, 10.0, -5.0)}
GLOSS_CASE, GLOSS = (6, 13, 100, 3.7, -1.2), 0.37   # the split backward with an upstream gradient != 1

# ((N, M, D), [speakers per shard, ...]) at w = 10, b = -5
SHARD_W, SHARD_B = 10.0, -5.0
SHARDED_CASES = [
    ((132, 3, 256), (44, 44, 44)),   # rows4r<true> (C^ formed in-kernel: Np == N) below 256
    ((132, 3, 256), (50, 40, 42)),   # ... with unequal shards
    ((130, 3, 256), (65, 65)),       # Np != N: centroid kernel, rows4r<false> with s0 > 0, zeroed padding rows
    ((7, 16, 36), (3, 4)),           # N % 4 != 0, cols_partial with dead lanes, M = 16 finalize
    ((255, 3, 8), (100, 155)),       # rows_kernel<4>, Np != N
]
# the same shard lists on the split shard kernels (HipShardKernels)
SPLIT_SHARDED_CASES = [((130, 3, 256), (65, 65)), ((7, 16, 36), (3, 4))]

# get_cossim / calc_loss with external centroids: (N, M, D, Nc), E and C both off the sphere
HELPER_CASES = [(5, 3, 64, 3), (5, 3, 64, 9)]

# ---------------------------------------------------------------------------------- the bounds
K = 4
PORT_MAX = {"per_abs": 3.8e-5, "dE_row": 2.4e-5, "loss_abs": 9.8e-6, "dw": 2.6e-7, "db": 5.2e-8}
BOUNDS = {k: K * v for k, v in PORT_MAX.items()}

# seeds moved where a first draw broke the conditioning cap (none so far)
SEED_SHIFT = {}


def all_inputs():
    """(N, M, D, w, b) of every input of the table, each once, in table order."""
    out = list(FUSED_CASES) + list(SPLIT_CASES)
    out += [shape + (SHARD_W, SHARD_B) for shape, _ in SHARDED_CASES]
    return list(dict.fromkeys(out))


def case_id(case):
    return "-".join(f"{v:g}" for v in case)


# ---------------------------------------------------------------------------------- the inputs
def make_offsphere(seed, n, m, d, noise=1.5, lo=0.05, hi=20.0):
    """Clustered embeddings [n, m, d] float32 (a speaker direction plus `noise` x per-utterance
    noise, PCG64, normalised) with every row then scaled by exp(U(log lo, log hi)).  noise = 1.5,
    not recipe.make_embeddings' 0.7: at 0.7 and small N the softmax saturates and dE becomes a
    cancellation that fp32 cannot resolve (the fp32 port itself then errs by 1e-4 per row)."""
    rng = np.random.default_rng(seed)
    spk = rng.standard_normal((n, 1, d))
    e = spk + noise * rng.standard_normal((n, m, d))
    e = e / np.linalg.norm(e, axis=2, keepdims=True)
    e = e * np.exp(rng.uniform(math.log(lo), math.log(hi), (n, m, 1)))
    return e.astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(N, M, D):
    """The off-sphere E of a shape (one per shape: the cases at (4, 5, 64) differ in (w, b) only).
    Read-only, shared among the tests."""
    E = make_offsphere(7000 + 31 * N + 17 * M + D + SEED_SHIFT.get((N, M, D), 0), N, M, D)
    E.setflags(write=False)
    return E


@functools.lru_cache(maxsize=None)
def oracle(N, M, D, w, b, gloss=1.0):
    """The fp64 oracle's dict(loss, per, dE, dw, db) of a case, computed once (read-only)."""
    E = inputs(N, M, D)
    loss, per, _ = ge2e_np.ge2e_forward(E, w, b)
    dE, dw, db = ge2e_np.ge2e_backward(E, w, b, gloss)
    per.setflags(write=False)
    dE.setflags(write=False)
    return dict(loss=float(loss), per=per, dE=dE, dw=float(dw), db=float(db))


@functools.lru_cache(maxsize=None)
def helper_inputs(N, M, D, Nc):
    """(E [N,M,D], Eenr [Nc,M,D]) float32, both off the sphere: the external centroids are
    get_centroids(Eenr), another draw's (enrollment) speakers, so they are off the sphere too."""
    E = make_offsphere(9000 + 13 * N + Nc, N, M, D)
    Eenr = make_offsphere(9500 + 13 * N + Nc, Nc, M, D)
    E.setflags(write=False)
    Eenr.setflags(write=False)
    return E, Eenr


# ---------------------------------------------------------------------------------- the metric
def dE_row(got, ref):
    """max over rows r of max_d |got_r - ref_r| / max_d |ref_r| (rows = everything but the last
    axis): every row on its own scale, which off the sphere differ by about 1000x."""
    got = np.asarray(got, np.float64).reshape(-1, np.shape(ref)[-1])
    ref = np.asarray(ref, np.float64).reshape(got.shape)
    return float((np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())


def compare(got, ref):
    """The five statistics of dict(loss, per, dE, dw, db) `got` against the oracle's `ref`."""
    n_rows = ref["per"].size
    return {
        "per_abs": float(np.abs(np.asarray(got["per"], np.float64) - ref["per"]).max()),
        "dE_row": dE_row(got["dE"], ref["dE"]),
        "loss_abs": abs(float(got["loss"]) - ref["loss"]) / math.sqrt(n_rows),
        "dw": abs(float(got["dw"]) - ref["dw"]) / max(1.0, abs(ref["dw"])),
        "db": abs(float(got["db"]) - ref["db"]) / n_rows,
    }


def over(stats, bounds=None, scale=1.0):
    """The statistics that exceed scale * bound, as {name: (value, limit)} (empty = within)."""
    bounds = BOUNDS if bounds is None else bounds
    return {k: (v, scale * bounds[k]) for k, v in stats.items() if not v <= scale * bounds[k]}


def fmt(stats):
    return " ".join(f"{k} {v:.2e}" for k, v in stats.items())


# ---------------------------------------------------------------------------------- references
def port_f32(N, M, D, w, b):
    """dict(loss, per, dE, dw, db) of the fp32 torch port with autograd on the CPU (one thread,
    so the sums have one order wherever this runs)."""
    import torch

    from oracle import torch_port
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        E = torch.tensor(inputs(N, M, D), requires_grad=True)
        wt = torch.tensor(w, dtype=torch.float32, requires_grad=True)
        bt = torch.tensor(b, dtype=torch.float32, requires_grad=True)
        per = torch_port.ge2e_per(E, wt, bt)
        loss = per.sum()
        loss.backward()
    finally:
        torch.set_num_threads(old)
    return dict(loss=float(loss.detach()), per=per.detach().numpy(), dE=E.grad.numpy(), dw=float(wt.grad), db=float(bt.grad))


def cossim_torch(E, C):
    """get_cossim (utils.py:72-115) as plain torch for external centroids C [Nc, D], Nc != N
    allowed: cosine of every E_ji with every C_k, the entries k = j < Nc replaced by the cosine
    with E's own leave-one-out centroid, + 1e-6.  Differentiable; the dtype is the inputs'."""
    import torch
    import torch.nn.functional as F
    N, M, _ = E.shape
    Nc = C.shape[0]
    U = (E.sum(dim=1, keepdim=True) - E) / (M - 1)
    cos = F.cosine_similarity(E[:, :, None, :], C[None, None, :, :], dim=3)
    same = F.cosine_similarity(E, U, dim=2)
    n = min(N, Nc)
    eye = torch.zeros(N, 1, Nc, dtype=torch.bool)
    eye[torch.arange(n), 0, torch.arange(n)] = True
    pad = same.new_zeros(N, M, Nc) + same[:, :, None]
    return torch.where(eye, pad, cos) + 1e-6


def calc_loss_torch(S):
    """calc_loss (utils.py:126-132) as plain torch: (loss, per [N, M])."""
    import torch
    idx = list(range(S.shape[0]))
    per = (torch.exp(S).sum(dim=2) + 1e-6).log() - S[idx, :, idx]
    return per.sum(), per


# ---------------------------------------------------------------------------------- sharding
def shard_slices(shards):
    """[(s0, N_local)] of a list of speakers per shard."""
    out, s0 = [], 0
    for nl in shards:
        out.append((s0, nl))
        s0 += nl
    return out


def run_shards_numpy(E, w, b, shards):
    """The sharded protocol on NumpyShardKernels with hand-made exchanges (concatenated sums, a
    plain sum of the reduce buffers).  Returns (dict(loss, per, dE, dw, db), [each shard's red],
    [each shard's state: raw, off, ... of its rows])."""
    k = ge2e_np.NumpyShardKernels()
    N = E.shape[0]
    sl = shard_slices(shards)
    assert sl[-1][0] + sl[-1][1] == N
    parts = [E[s0:s0 + nl] for s0, nl in sl]
    ssum_all = np.concatenate([k.speaker_sums(p).numpy() for p in parts])
    fwd = [k.fwd_rows(p, s0, N, ssum_all, w, b) for p, (s0, _) in zip(parts, sl)]
    bwd = [k.bwd_rows(f[2], w, b, None) for f in fwd]
    reds = [r_[0].numpy() for r_ in bwd]
    red = np.sum(reds, axis=0)
    got = dict(loss=sum(float(f[0]) for f in fwd), per=np.concatenate([f[1].numpy() for f in fwd]),
               dE=np.concatenate([k.finalize(f[2], red).numpy() for f in fwd]),
               dw=sum(float(r_[1][0]) for r_ in bwd), db=sum(float(r_[1][1]) for r_ in bwd))
    return got, reds, [f[2] for f in fwd]
