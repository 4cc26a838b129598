"""Spectral diarization of d-vector sequences: from the aligned d-vectors of a recording
(dvector.embed_files) to one speaker label per d-vector, after Wang et al., "Speaker Diarization
with LSTM" (arXiv 1710.10468), on ragged batches of files and on the GPU throughout.

  matrix_tables      row offsets, leading dimensions and matrix offsets of a batch of files
  affinity, crop_blur, threshold_sym, diffuse, row_norm, refine
                     the refinement chain: A = X X^T, cropped diagonal and Gaussian blur, row-wise
                     p-percentile threshold, symmetrisation, diffusion Y Y^T, row-max normalisation
                     in its symmetric form S = D^-1/2 Z D^-1/2
  top_eigenpairs     the 16 largest eigenpairs of every S by block subspace iteration with
                     Rayleigh-Ritz steps: S is read once per iteration, no O(n^3) eigh
  n_speakers         the eigengap rule
  spectral_embedding, kmeans
                     row-normalised leading eigenvectors; Lloyd's algorithm, one workgroup per file
  cluster, diarize   the whole chain on a list of d-vector sequences / of (waveform, ranges) files
  segments, write_rttm, read_rttm
                     labels to wall-clock time: the samples every aligned d-vector owns
                     (dvector.aligned_spans) carry its label; RTTM out and in
  raster, count, assignment, der, evaluate
                     scoring: segment tables to per-frame speaker bit masks (sv_seg_raster), the
                     masks to the integers of the diarization error rate for all files of a batch in
                     one pass (sv_der_count), the optimal speaker mapping on the host

The kernels are sv_diar_* and sv_seg_raster / sv_der_count (include/sv_ge2e.h has their contracts,
csrc/sv_diar.hip and csrc/sv_der.hip their plans); the two n^3 products run on sv_gemm_f32.  What
stays in torch is plumbing: the batched 16 x 16 fp64 eigh of the subspace iteration, the row
normalisation of the embedding and the eigengap on the host.  There is no CPU path.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import call, lib, ptr, require_device, stream_of
from .hparam import hparam as hp

M = 16            # SV_DIAR_M: eigenpairs of the subspace iteration, columns of the embedding
MAX_N = 8192      # SV_DIAR_MAX_N
MAX_R = 8         # SV_DIAR_MAX_R
DROP = 2.0 ** -40  # directions of a Gram matrix below DROP x its largest eigenvalue are dropped
# the eigengap's denominators are floored at LAM_FLOOR x lam_1: an eigenvalue that is zero up to
# rounding (a matrix of low rank) compares as that floor instead of as its noise
LAM_FLOOR = 1e-6


class Tables:
    """The tables of a batch of F files with ns[f] rows each: row_off int32 [F + 1], ld int32 [F]
    (ns rounded up to a multiple of 4), mat_off int64 [F] (element offsets of the packed matrices) as
    numpy arrays, n_max, elems (the size of a packed matrix buffer), and, once on a device, the
    device copies d_row_off and d_mat_off."""

    def __init__(self, ns):
        ns = np.asarray(ns, dtype=np.int64).reshape(-1)
        if ns.size < 1 or ns.min() < 2:
            raise ValueError("matrix_tables: need at least one file, every file with n >= 2 rows")
        if ns.max() > MAX_N:
            raise ValueError(f"matrix_tables: a file has {int(ns.max())} rows, above the kernels' limit {MAX_N}")
        if ns.size > 65535:
            raise ValueError("matrix_tables: more than 65 535 files in one batch")
        if ns.sum() >= 2 ** 31:
            raise ValueError("matrix_tables: row offsets need 32 bits")
        self.ns = ns
        self.F = int(ns.size)
        self.row_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
        ld = (ns + 3) // 4 * 4
        self.ld = ld.astype(np.int32)
        off = np.concatenate([[0], np.cumsum(ns * ld)])
        self.mat_off = off[:-1].astype(np.int64)
        self.elems = int(off[-1])
        self.n_max = int(ns.max())
        self.rows = int(self.row_off[-1])
        self.device = None

    def to(self, device):
        if self.device != torch.device(device):
            self.device = torch.device(device)
            self.d_row_off = torch.from_numpy(self.row_off).to(self.device)
            self.d_mat_off = torch.from_numpy(self.mat_off).to(self.device)
        return self

    def args(self):
        return ptr(self.d_row_off), ptr(self.d_mat_off), self.F, self.n_max


def matrix_tables(ns, device=None):
    """Tables of a batch of files with ns[f] >= 2 rows (on `device` if given)."""
    tb = Tables(ns)
    return tb if device is None else tb.to(device)


def _device_of(t, tb):
    require_device(t)
    return tb.to(t.device)


def _packed(t, tb, name):
    _device_of(t, tb)
    if t.dim() != 1 or t.numel() != tb.elems:
        raise ValueError(f"{name} must be a packed matrix buffer of {tb.elems} elements (got {tuple(t.shape)})")


def pack_matrices(mats, tb, device):
    """The n_f x n_f matrices `mats` (anything np.asarray takes) as one packed fp32 buffer on device."""
    buf = np.zeros(tb.elems, dtype=np.float32)
    for f, m in enumerate(mats):
        n, ld, o = int(tb.ns[f]), int(tb.ld[f]), int(tb.mat_off[f])
        buf[o:o + n * ld].reshape(n, ld)[:, :n] = np.asarray(m, dtype=np.float32).reshape(n, n)
    tb.to(device)
    return torch.from_numpy(buf).to(device)


def unpack_matrices(buf, tb, pads=False):
    """The files' matrices of a packed buffer as numpy arrays [n, n] ([n, ld] with pads=True)."""
    h = buf.detach().cpu().numpy()
    out = []
    for f in range(tb.F):
        n, ld, o = int(tb.ns[f]), int(tb.ld[f]), int(tb.mat_off[f])
        m = h[o:o + n * ld].reshape(n, ld)
        out.append(m.copy() if pads else m[:, :n].copy())
    return out


def gaussian_taps(sigma):
    """The r + 1 fp32 taps g(d) = exp(-d^2 / 2 sigma^2), r = ceil(3 sigma); sigma = 0 gives [1], W = I."""
    sigma = float(sigma)
    if sigma < 0:
        raise ValueError("sigma must be >= 0")
    if sigma == 0:
        return np.ones(1, dtype=np.float32)
    r = int(np.ceil(3.0 * sigma))
    if r > MAX_R:
        raise ValueError(f"sigma = {sigma} needs {r} taps a side, above the kernel's limit {MAX_R}")
    d = np.arange(r + 1, dtype=np.float64)
    return np.exp(-d * d / (2.0 * sigma * sigma)).astype(np.float32)


def threshold_rank(n, p):
    """q = floor(p (n - 1)): the ascending rank (0-based) of a row's threshold."""
    if not 0.0 <= p <= 1.0:
        raise ValueError("p must be in [0, 1]")
    return int(np.floor(np.float64(p) * (int(n) - 1)))


# ----------------------------------------------------------------------------- refinement
def _gemm_per_file(src, src_off, src_ld, dst, tb):
    """dst_f = src_f src_f^T for every file (sv_gemm_f32): src_f is the [n_f, src_ld[f]] k-contiguous matrix
    at element src_off[f] of the flat buffer src, K = src_ld[f]."""
    from .ops import gemm_f32_nt_into
    for f, (o_src, ld_src) in enumerate(zip(src_off, src_ld)):
        n, ld, o = int(tb.ns[f]), int(tb.ld[f]), int(tb.mat_off[f])
        a = src[o_src:]
        gemm_f32_nt_into(a, ld_src, a, ld_src, dst[o:], ld, n, n, ld_src)


def affinity(x, tb):
    """Packed A_f = X_f X_f^T (sv_gemm_f32 per file): x [sum n, D] fp32 on the device, rows as they are."""
    tb = _device_of(x, tb)
    if x.dim() != 2 or x.shape[0] != tb.rows:
        raise ValueError(f"affinity: x must be [{tb.rows}, D] (got {tuple(x.shape)})")
    D = x.shape[1]
    if D % 4:
        pad = torch.zeros((x.shape[0], (D + 3) // 4 * 4), dtype=torch.float32, device=x.device)
        pad[:, :D] = x
        x, D = pad, pad.shape[1]
    with torch.cuda.device(x.device):
        A = torch.zeros(tb.elems, dtype=torch.float32, device=x.device)
        _gemm_per_file(x.reshape(-1), [int(r) * D for r in tb.row_off[:-1]], [D] * tb.F, A, tb)
    return A


def crop_blur(A, tb, sigma=1.0):
    """Packed B = W A' W^T (sv_diar_crop_blur): A' is A with every diagonal element replaced by the
    largest other element of its row, W the row-normalised Gaussian band of gaussian_taps(sigma).
    A is overwritten."""
    _packed(A, tb, "A")
    taps = gaussian_taps(sigma)
    with torch.cuda.device(A.device):
        B = torch.empty_like(A)
        call("sv_diar_crop_blur", ptr(A), ptr(B), *tb.args(), taps.ctypes.data, taps.size - 1, stream_of(A))
    return B


def threshold_sym(B, tb, p=0.95, mult=0.01):
    """(tau [sum n], packed Y): tau_i the element of ascending rank floor(p (n - 1)) of row i of B
    (sv_diar_row_select, exact), Y_ij = max(T_ij, T_ji) with T_ij = B_ij if B_ij >= tau_i else
    mult * B_ij (sv_diar_thresh_sym)."""
    _packed(B, tb, "B")
    q = torch.from_numpy(np.asarray([threshold_rank(n, p) for n in tb.ns], dtype=np.int32)).to(B.device)
    with torch.cuda.device(B.device):
        tau = torch.empty(tb.rows, dtype=torch.float32, device=B.device)
        Y = torch.empty_like(B)
        call("sv_diar_row_select", ptr(B), *tb.args(), ptr(q), ptr(tau), stream_of(B))
        call("sv_diar_thresh_sym", ptr(B), ptr(tau), float(np.float32(mult)), ptr(Y), *tb.args(), stream_of(B))
    return tau, Y


def diffuse(Y, tb, out=None):
    """Packed Z_f = Y_f Y_f^T (sv_gemm_f32 per file, K = ld_f: the pad columns are zero)."""
    _packed(Y, tb, "Y")
    with torch.cuda.device(Y.device):
        Z = torch.zeros_like(Y) if out is None else out.zero_()
        _gemm_per_file(Y, [int(o) for o in tb.mat_off], [int(v) for v in tb.ld], Z, tb)
    return Z


def row_norm(Z, tb, inplace=False):
    """(packed S, d [sum n]): d_i = max_j Z_ij and S_ij = Z_ij r_i r_j with r_i = 1 / sqrt(d_i), or 0 where
    d_i <= 0 (sv_diar_row_norm): D^-1/2 Z D^-1/2, similar to the paper's D^-1 Z and symmetric."""
    _packed(Z, tb, "Z")
    with torch.cuda.device(Z.device):
        S = Z if inplace else torch.empty_like(Z)
        d = torch.empty(tb.rows, dtype=torch.float32, device=Z.device)
        r = torch.empty(tb.rows, dtype=torch.float64, device=Z.device)
        call("sv_diar_row_norm", ptr(Z), ptr(S), ptr(d), ptr(r), *tb.args(), stream_of(Z))
    return S, d


def refine(x, row_off, sigma=1.0, p=0.95, mult=0.01):
    """(packed S, tables) of the unit rows x [sum n, D] of the files row_off [F + 1] (a host sequence):
    the whole refinement chain.  Two packed buffers are alive at any time."""
    tb = matrix_tables(np.diff(np.asarray(row_off, dtype=np.int64)), x.device if torch.is_tensor(x) else None)
    A = affinity(x, tb)
    B = crop_blur(A, tb, sigma)
    _, Y = threshold_sym(B, tb, p, mult)
    del A
    Z = diffuse(Y, tb, out=B)
    S, _ = row_norm(Z, tb, inplace=True)
    return S, tb


# ----------------------------------------------------------------------------- eigenpairs
def _workspace(tb, dev):
    return torch.empty(max(1, int(lib().sv_diar_workspace(tb.F, tb.n_max)) // 8), dtype=torch.float64, device=dev)


def spmm(S, W, T, tb):
    """P = S (W T) per file (sv_diar_spmm): W [sum n, 16] fp32, T [F, 16, 16] fp64."""
    P = torch.empty_like(W)
    call("sv_diar_spmm", ptr(S), ptr(W), ptr(T), ptr(P), *tb.args(), stream_of(S))
    return P


def gram(X, Y, tb, ws=None):
    """G [F, 16, 16] fp64 = X_f^T Y_f (sv_diar_gram; deterministic)."""
    ws = _workspace(tb, X.device) if ws is None else ws
    G = torch.empty((tb.F, M, M), dtype=torch.float64, device=X.device)
    call("sv_diar_gram", ptr(X), ptr(Y), ptr(G), ptr(ws), ptr(tb.d_row_off), tb.F, tb.n_max, stream_of(X))
    return G


def rmul(X, T, tb, P=None, lam=None, ws=None):
    """Y = X T per file (sv_diar_rmul); with P and lam [F, 16] also res2 [F, 16], the squared column
    norms of P T - Y diag(lam).  Returns Y or (Y, res2)."""
    Y = torch.empty_like(X)
    if P is None:
        call("sv_diar_rmul", ptr(X), ptr(T), ptr(Y), None, None, None, None, ptr(tb.d_row_off), tb.F, tb.n_max,
             stream_of(X))
        return Y
    ws = _workspace(tb, X.device) if ws is None else ws
    res2 = torch.empty((tb.F, M), dtype=torch.float64, device=X.device)
    call("sv_diar_rmul", ptr(X), ptr(T), ptr(Y), ptr(P), ptr(lam), ptr(res2), ptr(ws), ptr(tb.d_row_off), tb.F,
         tb.n_max, stream_of(X))
    return Y, res2


def start_block(tb, dev):
    """Q0 [sum n, 16] fp32: Q0_ij = cos(pi (i + 1/2) j / n) within every file."""
    n = torch.from_numpy(np.repeat(tb.ns, tb.ns)).to(dev).double()
    i = torch.arange(tb.rows, device=dev).double() - torch.from_numpy(np.repeat(tb.row_off[:-1], tb.ns)).to(dev).double()
    j = torch.arange(M, device=dev).double()
    return torch.cos(torch.pi * (i[:, None] + 0.5) * j[None, :] / n[:, None]).float().contiguous()


def _eigh_desc(G):
    w, v = torch.linalg.eigh(G)
    return w.flip(-1), v.flip(-1)


def _orthonormaliser(G):
    """T = V diag(mu^-1/2) of G = V diag(mu) V^T, columns by descending mu; a direction with
    mu < DROP x mu_max (or mu <= 0) is dropped: its column of T is zero."""
    mu, V = _eigh_desc(0.5 * (G + G.transpose(-1, -2)))
    keep = (mu > 0) & (mu >= DROP * mu[:, :1])
    scale = torch.where(keep, mu.clamp_min(torch.finfo(torch.float64).tiny).rsqrt(), torch.zeros_like(mu))
    return (V * scale[:, None, :]).contiguous()


@torch.no_grad()
def top_eigenpairs(S, tb, tol=1e-4, max_iter=200, check=4, k_max=8, strict=True):
    """The 16 largest eigenpairs of every file's symmetric positive semi-definite S (a packed buffer
    with tables tb) by block subspace iteration: W <- S (W T), T the 16 x 16 matrix that orthonormalises
    W (from the fp64 Gram matrix; directions below 2^-40 of the largest are dropped, so a matrix of
    rank < 16 is handled), and after every `check` iterations a Rayleigh-Ritz step, whose product is
    the next iteration.  A file has converged when the residuals |S u_j - lam_j u_j| of its leading
    min(k_max + 1, 16) Ritz pairs are <= tol lam_1; the loop ends when all have, or after max_iter
    iterations, and reads back one float per file per Rayleigh-Ritz step.

    Returns (lam [F, 16] fp64 descending, U [sum n, 16] fp32 Ritz vectors, res [F, 16] fp64 residual
    norms, iters [F] int64 numpy -- the iteration at which the file was first seen converged --
    converged [F] bool numpy).  A file with n < 16 gets torch.linalg.eigh of its S instead (zeros past
    n).  RuntimeError for a file that did not converge, unless strict=False."""
    _packed(S, tb, "S")
    if check < 1 or max_iter < 1:
        raise ValueError("top_eigenpairs: check and max_iter must be >= 1")
    dev = S.device
    lead = min(int(k_max) + 1, M)
    small = [f for f in range(tb.F) if tb.ns[f] < M]
    big = torch.from_numpy(tb.ns >= M).to(dev)
    with torch.cuda.device(dev):
        ws = _workspace(tb, dev)
        eye = torch.eye(M, dtype=torch.float64, device=dev).expand(tb.F, M, M).contiguous()
        W = start_block(tb, dev)
        T = _orthonormaliser(gram(W, W, tb, ws))
        iters = np.zeros(tb.F, dtype=np.int64)
        done = np.asarray(tb.ns < M)
        it = 0
        while True:
            for _ in range(check):
                W = spmm(S, W, T, tb)
                T = _orthonormaliser(gram(W, W, tb, ws))
                it += 1
            Q = rmul(W, T, tb)
            P = spmm(S, Q, eye, tb)
            H = gram(Q, P, tb, ws)
            lam, V = _eigh_desc(0.5 * (H + H.transpose(-1, -2)))
            V, lam = V.contiguous(), lam.contiguous()
            U, res2 = rmul(Q, V, tb, P=P, lam=lam, ws=ws)
            res = res2.clamp_min(0).sqrt()
            worst = (res[:, :lead].max(dim=1).values / (tol * lam[:, 0].clamp_min(torch.finfo(torch.float64).tiny)))
            ok = (torch.where(big, worst, torch.zeros_like(worst)).float().cpu().numpy() <= 1.0)
            W = P  # the Rayleigh-Ritz product is the next iteration
            T = _orthonormaliser(gram(W, W, tb, ws))
            it += 1
            iters[ok & ~done] = it
            done |= ok
            if done.all() or it >= max_iter:
                break
        iters[~done] = it
        for f in small:  # tiny files: a full eigh of the n x n matrix
            n, ld, o, r0 = int(tb.ns[f]), int(tb.ld[f]), int(tb.mat_off[f]), int(tb.row_off[f])
            Sf = S[o:o + n * ld].view(n, ld)[:, :n].double()
            w, v = _eigh_desc(0.5 * (Sf + Sf.T))
            lam[f].zero_()
            lam[f, :n] = w
            U[r0:r0 + n].zero_()
            U[r0:r0 + n, :n] = v.float()
            res[f].zero_()
            iters[f] = 0
    if strict and not done.all():
        bad = np.flatnonzero(~done).tolist()
        raise RuntimeError(f"top_eigenpairs: files {bad} did not converge to tol = {tol} in {max_iter} iterations "
                           "(strict=False returns them flagged)")
    return lam, U, res, iters, done


def n_speakers(lam, n, k_min=1, k_max=8):
    """The eigengap rule on the host in fp64: the k in [k_min, min(k_max, n - 1)] with the largest
    lam_k / max(lam_{k+1}, LAM_FLOOR lam_1) (1-based; the first of equal maxima).  lam: one file's
    descending eigenvalues (at least k_max + 1 of them)."""
    lam = np.asarray(lam, dtype=np.float64).reshape(-1)
    hi = min(int(k_max), int(n) - 1, lam.size - 1)
    if hi < k_min:
        return max(1, min(int(k_min), int(n)))
    floor = max(LAM_FLOOR * max(lam[0], 0.0), np.finfo(np.float64).tiny)
    ks = np.arange(k_min, hi + 1)
    ratio = lam[ks - 1] / np.maximum(lam[ks], floor)
    return int(ks[int(np.argmax(ratio))])


_eigengap = n_speakers  # (cluster's keyword of the same name shadows the function)


def spectral_embedding(U, tb, k):
    """E [sum n, 16] fp32: the first k[f] columns of every file's rows of U, each row L2-normalised
    (a zero row stays zero), the other columns zero."""
    k = torch.from_numpy(np.repeat(np.asarray(k, dtype=np.int64), tb.ns)).to(U.device)
    E = torch.where(torch.arange(M, device=U.device)[None, :] < k[:, None], U, torch.zeros_like(U))
    nrm = E.double().norm(dim=1, keepdim=True)
    return (E.double() / torch.where(nrm > 0, nrm, torch.ones_like(nrm))).float().contiguous()


def kmeans(E, row_off, k, max_iter=100):
    """(labels int32 [sum n], iters int32 [F]) on the device (sv_diar_kmeans): Lloyd's algorithm on the
    rows of E [sum n, 16] fp32 per file (row_off: a host sequence or a Tables), k an int or one per file;
    farthest-first start from row 0, at most max_iter assignment passes.  Labels are centre indices;
    relabel() renumbers them by first appearance."""
    require_device(E)
    if E.dim() != 2 or E.shape[1] != M:
        raise ValueError(f"kmeans: E must be [sum n, {M}] (got {tuple(E.shape)})")
    off = row_off.row_off if isinstance(row_off, Tables) else np.asarray(row_off, dtype=np.int32)
    F = off.size - 1
    if F < 1 or int(off[-1]) != E.shape[0]:
        raise ValueError("kmeans: row_off does not match E")
    ks = np.broadcast_to(np.asarray(k, dtype=np.int32), (F,)).copy()
    if ks.min() < 1 or ks.max() > M:
        raise ValueError(f"kmeans: k must be in [1, {M}]")
    dev = E.device
    with torch.cuda.device(dev):
        d_off, d_k = torch.from_numpy(off.astype(np.int32)).to(dev), torch.from_numpy(ks).to(dev)
        labels = torch.zeros(E.shape[0], dtype=torch.int32, device=dev)
        iters = torch.zeros(F, dtype=torch.int32, device=dev)
        call("sv_diar_kmeans", ptr(E), ptr(d_off), ptr(d_k), F, int(max_iter), ptr(labels), ptr(iters), stream_of(E))
    return labels, iters


def relabel(lab):
    """Labels renumbered by first appearance (host)."""
    lab = np.asarray(lab)
    _, first, inv = np.unique(lab, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv].astype(np.int64)


# ----------------------------------------------------------------------------- the whole chain
def _batches(costs, budget):
    groups, cur, tot = [], [], 0
    for i, c in enumerate(costs):
        if cur and tot + c > budget:
            groups.append(cur)
            cur, tot = [], 0
        cur.append(i)
        tot += c
    if cur:
        groups.append(cur)
    return groups


@torch.no_grad()
def cluster(dvectors, n_speakers=None, sigma=1.0, p=0.95, mult=0.01, k_min=1, k_max=8, tol=1e-4, max_iter=200,
            check=4, kmeans_iter=100, strict=True, max_elems=2 ** 26, device=None):
    """Speaker labels for every file of `dvectors`, a list of [n_i, proj] numpy arrays or device tensors
    (what dvector.embed_files returns): rows are normalised, then refine -> top_eigenpairs -> the
    eigengap (or n_speakers: an int for all files or one entry per file, None entries meaning the
    eigengap) -> spectral_embedding -> kmeans.  Files are grouped into batches whose packed n x n
    matrices hold at most max_elems elements (a larger file alone).

    Returns (labels, info): labels[i] an int64 numpy array [n_i], numbered by first appearance (a file
    with one row gets [0], an empty file an empty array); info = {"k": [..], "lam": [F, 16] numpy,
    "iters": [..], "converged": [..]} per input file.  Host tensors raise "GPU only"."""
    global_k, count = n_speakers, _eigengap
    nfiles = len(dvectors)
    per_file = list(global_k) if isinstance(global_k, (list, tuple, np.ndarray)) else [global_k] * nfiles
    if len(per_file) != nfiles:
        raise ValueError("cluster: n_speakers must be an int or one entry per file")
    xs = []
    for d in dvectors:
        if torch.is_tensor(d):
            if not d.is_cuda:
                raise RuntimeError("pytorch_speaker_verification_amd ops run on the GPU only "
                                   f"(got a {d.device} tensor); move the d-vectors with .to('cuda')")
            device = d.device if device is None else device
        xs.append(d)
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("pytorch_speaker_verification_amd ops run on the GPU only (HIP kernels, no CPU "
                               "fallback) and no GPU is visible")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    ns = [int(x.shape[0]) for x in xs]
    labels = [np.zeros(min(n, 1) * n, dtype=np.int64) for n in ns]
    info = {"k": [min(n, 1) for n in ns], "lam": np.zeros((nfiles, M)), "iters": [0] * nfiles,
            "converged": [True] * nfiles}
    live = [i for i, n in enumerate(ns) if n >= 2]
    for n in ns:
        if n > MAX_N:
            raise ValueError(f"cluster: a file has {n} d-vectors, above the kernels' limit {MAX_N}")
    for group in _batches([ns[i] * ((ns[i] + 3) // 4 * 4) for i in live], int(max_elems)):
        ids = [live[g] for g in group]
        with torch.cuda.device(device):
            x = torch.cat([torch.as_tensor(xs[i]).to(device=device, dtype=torch.float64) for i in ids])
            x = (x / x.norm(dim=1, keepdim=True).clamp_min(1e-300)).float().contiguous()
            tb = matrix_tables([ns[i] for i in ids], device)
            S, _ = refine(x, tb.row_off, sigma, p, mult)
            lam, U, _, iters, conv = top_eigenpairs(S, tb, tol, max_iter, check, k_max, strict)
            del S
            lam_h = lam.cpu().numpy()
            ks = [count(lam_h[j], ns[i], k_min, k_max) if per_file[i] is None else max(1, min(int(per_file[i]), ns[i], M))
                  for j, i in enumerate(ids)]
            lab, _ = kmeans(spectral_embedding(U, tb, ks), tb, ks, kmeans_iter)
            lab = lab.cpu().numpy()
        for j, i in enumerate(ids):
            labels[i] = relabel(lab[tb.row_off[j]:tb.row_off[j + 1]])
            info["k"][i], info["lam"][i], info["iters"][i], info["converged"][i] = ks[j], lam_h[j], int(iters[j]), bool(conv[j])
    return labels, info


def diarize(net, files, precision="bf16", path=None, max_samples=2 ** 27, times=False, **kw):
    """dvector.embed_files followed by cluster, the d-vectors staying on the device in between:
    `files` is a list of (waveform, voiced ranges) as embed_files takes them; **kw goes to cluster.
    Returns cluster's (labels, info): one label per aligned d-vector of every file.  times=True
    returns (labels, info, segments): per file the (start_s, end_s, label) list of segments() on the
    file's dvector.aligned_spans -- their union is exactly the ranges embed_files kept."""
    from .dvector import aligned_spans, embed_files
    labels, info = cluster(embed_files(net, files, precision=precision, path=path, max_samples=max_samples,
                                       on_device=True), **kw)
    if not times:
        return labels, info
    return labels, info, segments(labels, [aligned_spans(ranges) for _, ranges in files])


# ----------------------------------------------------------------------------- labels to wall-clock time
def segments(labels, spans, sr=None):
    """Per file the list of (start_s, end_s, label): every row (start_sample, end_sample, aligned_index)
    of `spans` (dvector.aligned_spans) carries the label of its aligned d-vector; neighbouring spans
    with one label and end == next start merge; times are sample / sr as Python floats."""
    from .dvector import _sr
    sr = _sr(sr)
    if len(labels) != len(spans):
        raise ValueError("segments: one label array and one span table per file")
    out = []
    for lab, sp in zip(labels, spans):
        sp = np.asarray(sp, dtype=np.int64).reshape(-1, 3)
        if sp.shape[0] and int(sp[:, 2].max()) >= len(lab):
            raise ValueError(f"segments: spans name aligned d-vector {int(sp[:, 2].max())}, the file has {len(lab)} labels")
        cur = []
        for s, e, i in sp.tolist():
            v = int(lab[i])
            if cur and cur[-1][2] == v and cur[-1][1] == s:
                cur[-1][1] = e
            else:
                cur.append([s, e, v])
        out.append([(s / sr, e / sr, v) for s, e, v in cur])
    return out


def write_rttm(path, file_ids, segments):
    """One `SPEAKER <file> 1 <tbeg> <tdur> <NA> <NA> <name> <NA> <NA>` line per segment (start_s, end_s,
    speaker) of every file, files in order.  Times carry nine decimals, so read_rttm gives back the
    sample positions (round(t * sr)) at any audio rate.  A file without segments gets a `;;` comment
    line only: RTTM has no record for it."""
    if len(file_ids) != len(segments):
        raise ValueError("write_rttm: one id per file")
    with open(path, "w") as f:
        for fid, segs in zip(file_ids, segments):
            fid = str(fid)
            if not fid or any(c.isspace() for c in fid):
                raise ValueError(f"write_rttm: file id {fid!r} is empty or holds white space")
            if not segs:
                f.write(f";; {fid} has no segments\n")
            for s, e, spk in segs:
                spk = str(spk)
                if not spk or any(c.isspace() for c in spk):
                    raise ValueError(f"write_rttm: speaker name {spk!r} is empty or holds white space")
                f.write(f"SPEAKER {fid} 1 {float(s):.9f} {float(e) - float(s):.9f} <NA> <NA> {spk} <NA> <NA>\n")


def read_rttm(path, file_ids=None):
    """{file_id: [(start_s, end_s, speaker), ...]} of the SPEAKER lines of an RTTM file, in the file's
    order (end = tbeg + tdur; speaker names are strings); every other line is skipped.  Ids in
    `file_ids` get an entry even without a line."""
    out = {str(fid): [] for fid in (file_ids or [])}
    with open(path) as f:
        for line in f:
            p = line.split()
            if len(p) < 8 or p[0] != "SPEAKER":
                continue
            t, d = float(p[3]), float(p[4])
            out.setdefault(p[1], []).append((t, t + d, p[7]))
    return out


# ----------------------------------------------------------------------------- scoring: DER on a frame grid
MAX_SPK = 32          # speakers per file and side: the bits of a frame's mask
RASTER_PIECE = 2048   # split_rows: table rows longer than this many frames are cut (one wave per row)
DER_OUT = 4 + MAX_SPK * MAX_SPK
_MAX_FILES = 65535


def split_rows(start, end, bits, file, step, piece=RASTER_PIECE):
    """The segment table (start, end, bits, file) with every row longer than piece * step samples cut
    into pieces of that length (the last one shorter): the same frames are covered, since every frame
    centre of [s, e) lies in exactly one piece, and sv_seg_raster's one wave per row is an even load."""
    start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    bits, file = np.asarray(bits, dtype=np.uint32), np.asarray(file, dtype=np.int64)
    span = int(piece) * int(step)
    n = np.maximum(1, -(-(end - start) // span))
    if n.size == 0 or n.max() == 1:
        return start, end, bits, file
    row = np.repeat(np.arange(n.size), n)
    k = np.arange(row.size) - np.repeat(np.cumsum(n) - n, n)
    s = start[row] + k * span
    return s, np.minimum(end[row], s + span), bits[row], file[row]


def _scoring_device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("pytorch_speaker_verification_amd ops run on the GPU only (HIP kernels, no CPU "
                               "fallback) and no GPU is visible")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"pytorch_speaker_verification_amd ops run on the GPU only (got device {device})")
    return device


def _int32_tensor(a, dev, name):
    a = np.asarray(a)
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError(f"{name} needs 32 bits")
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.int64).astype(np.int32))).to(dev)


def raster(seg_start, seg_end, seg_bits, seg_file, frame_off, step, mask=None, split=True, device=None, d_frame_off=None):
    """Per-frame masks of a segment table (sv_seg_raster): mask[frame_off[f] + i] |= seg_bits[k] for
    every frame i of file f = seg_file[k] whose centre i * step + step // 2 lies in [seg_start[k],
    seg_end[k]) (samples), clamped to the file's own frames.  frame_off: host int [F + 1].  Returns the
    int32 device tensor [frame_off[-1]] (the bits of a uint32); `mask` gives a tensor to OR into instead
    (at least that long; words past frame_off[-1] are not touched).  split=False passes the rows as
    they are, without split_rows.  d_frame_off: the int32 device copy of frame_off, where the caller
    holds one (der uploads it once per batch)."""
    frame_off = np.asarray(frame_off, dtype=np.int64).reshape(-1)
    F, n_total = frame_off.size - 1, int(frame_off[-1])
    if F < 1 or frame_off[0] != 0 or np.any(np.diff(frame_off) < 0) or n_total >= 2 ** 31:
        raise ValueError("raster: frame_off must be ascending from 0, [F + 1] with F >= 1, below 2^31 frames")
    if step < 1:
        raise ValueError("raster: step must be >= 1")
    dev = mask.device if mask is not None else _scoring_device(device)
    if mask is None:
        mask = torch.zeros(n_total, dtype=torch.int32, device=dev)
    elif not mask.is_cuda or mask.dtype != torch.int32 or not mask.is_contiguous() or mask.numel() < n_total:
        raise ValueError(f"raster: mask must be a contiguous int32 device tensor of at least {n_total} words")
    rows = (np.asarray(seg_start, dtype=np.int64), np.asarray(seg_end, dtype=np.int64),
            np.asarray(seg_bits, dtype=np.uint32), np.asarray(seg_file, dtype=np.int64))
    if len({r.size for r in rows}) != 1:
        raise ValueError("raster: the four segment tables must have one length")
    if split:
        rows = split_rows(*rows, step)
    n_seg = int(rows[0].size)
    if n_seg == 0 or n_total == 0:
        return mask
    with torch.cuda.device(dev):
        d_s, d_e = _int32_tensor(rows[0], dev, "a segment start"), _int32_tensor(rows[1], dev, "a segment end")
        d_b = torch.from_numpy(np.ascontiguousarray(rows[2]).view(np.int32)).to(dev)
        d_f = _int32_tensor(np.clip(rows[3], -1, F), dev, "a file index")
        d_off = torch.from_numpy(frame_off.astype(np.int32)).to(dev) if d_frame_off is None else d_frame_off
        call("sv_seg_raster", ptr(d_s), ptr(d_e), ptr(d_b), ptr(d_f), n_seg, ptr(d_off), F, int(step), n_total,
             ptr(mask), torch.cuda.current_stream(dev).cuda_stream)
    return mask


def count(ref, hyp, noscore, frame_off, uem=None, skip_overlap=False, d_frame_off=None):
    """The integers of the DER per file (sv_der_count): uint64 numpy [F, 4 + 32 * 32] -- total, miss, fa,
    both, then C[i][j] row-major -- over the scored frames of the int32 device masks ref, hyp, noscore
    (and uem: frames with uem == 0 are not scored; None scores every frame) of raster().  d_frame_off
    as in raster()."""
    frame_off = np.asarray(frame_off, dtype=np.int64).reshape(-1)
    F, n_total = frame_off.size - 1, int(frame_off[-1])
    if F < 1 or F > _MAX_FILES or frame_off[0] != 0 or np.any(np.diff(frame_off) < 0) or n_total >= 2 ** 31:
        raise ValueError(f"count: frame_off must be ascending from 0, [F + 1] with 1 <= F <= {_MAX_FILES}, below 2^31 frames")
    for name, t in (("ref", ref), ("hyp", hyp), ("noscore", noscore), ("uem", uem)):
        if t is None and name == "uem":
            continue
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("pytorch_speaker_verification_amd ops run on the GPU only "
                               f"({name} is not a device tensor); build the masks with raster()")
        if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < n_total or t.device != ref.device:
            raise ValueError(f"count: {name} must be a contiguous int32 tensor of at least {n_total} frames on ref's device")
    dev = ref.device
    with torch.cuda.device(dev):
        out = torch.empty((F, DER_OUT), dtype=torch.int64, device=dev)
        d_off = torch.from_numpy(frame_off.astype(np.int32)).to(dev) if d_frame_off is None else d_frame_off
        call("sv_der_count", ptr(ref), ptr(hyp), ptr(noscore), ptr(uem), ptr(d_off), F, int(np.diff(frame_off).max()),
             n_total, int(bool(skip_overlap)), ptr(out), torch.cuda.current_stream(dev).cuda_stream)
        return out.cpu().numpy().view(np.uint64)


def assignment(C):
    """The one-to-one mapping of rows to columns of the integer matrix C [R, K] that maximises
    sum_r C[r][col[r]] (the Hungarian method with potentials, exact in Python integers; min(R, K)
    pairs): (col int64 [R], -1 for a row left out; the total)."""
    C = np.asarray(C, dtype=np.int64)
    if C.ndim != 2:
        raise ValueError("assignment: C must be a matrix")
    R, K = C.shape
    if R == 0 or K == 0:
        return np.full(R, -1, dtype=np.int64), 0
    if R > K:
        row_of, total = assignment(C.T)
        col = np.full(R, -1, dtype=np.int64)
        col[row_of] = np.arange(K)
        return col, total
    cost = (-C).tolist()
    inf = 1 << 62
    u, v, p, way = [0] * (R + 1), [0] * (K + 1), [0] * (K + 1), [0] * (K + 1)
    for i in range(1, R + 1):
        p[0], j0 = i, 0
        minv, used = [inf] * (K + 1), [False] * (K + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], inf, 0
            row = cost[i0 - 1]
            for j in range(1, K + 1):
                if not used[j]:
                    cur = row[j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(K + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col = np.full(R, -1, dtype=np.int64)
    for j in range(1, K + 1):
        if p[j]:
            col[p[j] - 1] = j - 1
    return col, int(sum(int(C[r, c]) for r, c in enumerate(col)))


def _positions(segs, n, sr, names, what):
    """(start, end, bits) int lists of one file's (start_s, end_s, speaker) list: positions
    int(round(t * sr)) clamped to [0, n]; speakers to bits by first appearance (names: filled in)."""
    s_, e_, b_ = [], [], []
    for t0, t1, spk in segs:
        if spk not in names:
            if len(names) >= MAX_SPK:
                raise ValueError(f"der: more than {MAX_SPK} {what} speakers in one file")
            names[spk] = len(names)
        s_.append(min(max(int(round(t0 * sr)), 0), n))
        e_.append(min(max(int(round(t1 * sr)), 0), n))
        b_.append(1 << names[spk])
    return s_, e_, b_


def der(reference, hypothesis, n_samples, collar=0.25, skip_overlap=False, step=None, uem=None, sr=None,
        max_frames=2 ** 27, device=None):
    """The diarization error rate of per-file hypotheses against per-file references, both lists of
    (start_s, end_s, speaker) per file, on a frame grid, for all files in one pass per batch on the GPU.

    Grid: `step` samples per frame (default int(hp.data.hop * sr): 10 ms); a file of n_samples[f]
    samples has ceil(n / step) frames; frame i has its centre at i * step + step // 2 and a segment
    covers it iff start <= centre < end, with positions int(round(t * sr)) clamped to [0, n].  Around
    every reference boundary t the frames of [t - c, t + c), c = round(collar * sr), are not scored;
    `uem` (per file None or a list of (start_s, end_s) regions) restricts scoring to its regions;
    skip_overlap leaves out frames with more than one reference speaker.  Over the scored frames, with
    Nr / Nh the number of active reference / hypothesis speakers: total = sum Nr, miss = sum max(0,
    Nr - Nh), fa = sum max(0, Nh - Nr); with the one-to-one speaker mapping that maximises the
    co-occurrence sum_r C[r][map(r)] (assignment(), on the host), correct is that sum and
    conf = sum min(Nr, Nh) - correct.  DER = (miss + fa + conf) / total in fp64.

    Four sv_seg_raster launches (reference, hypothesis, collars, UEM) and one sv_der_count per batch of
    files holding at most max_frames frames (a larger file alone).  Returns {"total", "miss", "fa",
    "conf": int64 [F]; "file_der": float64 [F], nan where total == 0; "mapping": per file {reference
    speaker: hypothesis speaker} for the mapped pairs that co-occur; "der": sum of errors / sum of total
    over the files}.  More than 32 speakers on either side of a file is a ValueError.

    This DER is quantised to `step`: a boundary moves to the next frame centre.  It is not claimed
    equal to NIST md-eval's continuous-time figure, against which it has not been compared."""
    from .dvector import _sr
    sr = _sr(sr)
    step = int(hp.data.hop * sr) if step is None else int(step)
    if step < 1:
        raise ValueError("der: step must be >= 1")
    nfiles = len(reference)
    if len(hypothesis) != nfiles or len(n_samples) != nfiles or (uem is not None and len(uem) != nfiles):
        raise ValueError("der: reference, hypothesis, n_samples (and uem) need one entry per file")
    ns = [int(n) for n in n_samples]
    if nfiles and (min(ns) < 0 or max(ns) >= 2 ** 31):
        raise ValueError("der: sample positions need 32 bits")
    c = int(round(collar * sr))
    if c < 0:
        raise ValueError("der: collar must be >= 0")
    frames = [-(-n // step) for n in ns]
    # tables first (host): a speaker count above 32 is an error before anything runs
    tabs = []
    for f in range(nfiles):
        rn, hn = {}, {}
        rs, re_, rb = _positions(reference[f], ns[f], sr, rn, "reference")
        hs, he, hb = _positions(hypothesis[f], ns[f], sr, hn, "hypothesis")
        cs = [min(max(t - c, 0), ns[f]) for t in rs + re_] if c else []
        ce = [min(max(t + c, 0), ns[f]) for t in rs + re_] if c else []
        us = ue = None
        if uem is not None:
            us, ue = [0], [ns[f]]  # None: the whole file
            if uem[f] is not None:
                us = [min(max(int(round(t0 * sr)), 0), ns[f]) for t0, _ in uem[f]]
                ue = [min(max(int(round(t1 * sr)), 0), ns[f]) for _, t1 in uem[f]]
        tabs.append(((rs, re_, rb), (hs, he, hb), (cs, ce, [1] * len(cs)), None if us is None else (us, ue, [1] * len(us)),
                     list(rn), list(hn)))
    out = np.zeros((nfiles, DER_OUT), dtype=np.uint64)
    dev = _scoring_device(device) if nfiles else None
    groups = [g[i:i + _MAX_FILES] for g in _batches(frames, min(int(max_frames), 2 ** 31 - 1))
              for i in range(0, len(g), _MAX_FILES)]
    for ids in groups:
        frame_off = np.concatenate([[0], np.cumsum([frames[i] for i in ids])])
        if frame_off[-1] >= 2 ** 31:
            raise ValueError("der: a file has 2^31 frames or more; raise step")
        if frame_off[-1] == 0:
            continue
        d_off = torch.from_numpy(frame_off.astype(np.int32)).to(dev)  # one upload per batch
        masks = []
        for which in range(4):
            if tabs[ids[0]][which] is None:
                masks.append(None)
                continue
            rows = [tabs[i][which] for i in ids]
            cols = [np.fromiter((v for r in rows for v in r[c]), dtype=np.int64) for c in range(3)]
            cols.append(np.repeat(np.arange(len(ids)), [len(r[0]) for r in rows]))
            masks.append(raster(*cols, frame_off, step, device=dev, d_frame_off=d_off))
        out[ids] = count(masks[0], masks[1], masks[2], frame_off, uem=masks[3], skip_overlap=skip_overlap,
                         d_frame_off=d_off)
    res = {k: np.zeros(nfiles, dtype=np.int64) for k in ("total", "miss", "fa", "conf")}
    res["file_der"] = np.full(nfiles, np.nan)
    res["mapping"] = []
    for f in range(nfiles):
        rn, hn = tabs[f][4], tabs[f][5]
        total, miss, fa, both = (int(v) for v in out[f, :4])
        C = out[f, 4:].astype(np.int64).reshape(MAX_SPK, MAX_SPK)[:len(rn), :len(hn)]
        col, correct = assignment(C)
        res["total"][f], res["miss"][f], res["fa"][f], res["conf"][f] = total, miss, fa, both - correct
        res["mapping"].append({rn[r]: hn[j] for r, j in enumerate(col.tolist()) if j >= 0 and C[r, j] > 0})
        if total:
            res["file_der"][f] = np.float64(miss + fa + both - correct) / np.float64(total)
    err, tot = int(res["miss"].sum() + res["fa"].sum() + res["conf"].sum()), int(res["total"].sum())
    res["der"] = float(np.float64(err) / np.float64(tot)) if tot else float("nan")
    return res


def evaluate(net, files, references, n_speakers=None, collar=0.25, skip_overlap=False, **kw):
    """diarize(times=True) followed by der: `files` as diarize takes them, `references` per file a list
    of (start_s, end_s, speaker).  n_speakers goes to cluster; "oracle" gives it each file's number of
    reference speakers (a file with d-vectors and an empty reference gets 0, which cluster raises to
    one speaker).  step, uem, sr, max_frames go to der, device to both, everything else in **kw
    to diarize.  Returns der's dict plus "info", "labels" and "segments" of the diarization."""
    if len(references) != len(files):
        raise ValueError("evaluate: one reference per file")
    der_kw = {k: kw.pop(k) for k in ("step", "uem", "sr", "max_frames") if k in kw}
    if "device" in kw:
        der_kw["device"] = kw["device"]
    if isinstance(n_speakers, str):
        if n_speakers != "oracle":
            raise ValueError(f"evaluate: n_speakers must be None, an int, one entry per file or 'oracle' (got {n_speakers!r})")
        n_speakers = [len({spk for _, _, spk in ref}) for ref in references]
    labels, info, segs = diarize(net, files, times=True, n_speakers=n_speakers, **kw)
    res = der(references, segs, [int(len(w)) for w, _ in files], collar=collar, skip_overlap=skip_overlap, **der_kw)
    res.update(info=info, labels=labels, segments=segs)
    return res
