"""The reference, inputs and bounds of the GE2E CONTRAST loss tests (arXiv 1710.10467 eq. 7), shared
by tests/test_contrast_cases.py (CPU) and tests/test_gpu_contrast.py (the HIP kernels of
csrc/sv_ge2e_contrast.h).  The case table is tests/ge2e_cases.py's, imported: those shapes are the
kernels' edges (the 128 / 256 tile borders, Np != N, M = 2 / 16 / 17, D % 64 != 0, D = 260, D = 38,
negative w, S ~ -14).  The inputs are the same make_offsphere draws with a seed-shift table of
their own (below).

Reference.  For E [N, M, D], N >= 2, with cos = get_cossim(E, get_centroids(E)) (ge2e_cases.cossim_torch:
leave-one-out diagonal, + 1e-6, x^ = x / max(|x|, 1e-8)) and S = w cos + b (no clamp on w):
    per[j,i] = 1 - sigma(S[j,i,j]) + max_{k != j} sigma(S[j,i,k]),   loss = sum per,
as fp64 torch autograd.  The maximum is taken where S is largest over k != j (sigma is monotone, so a
negative w selects the smallest cosine); torch.max(dim) returns the lowest index among equals and
autograd sends the gradient there.  contrast_loop restates eq. 7 with Python loops; the two agree at
(3, 2, 4) (tests/test_contrast_cases.py).

Gap condition.  An fp32 kernel rounds S at |S| <= 15 by about 1e-6, so where the two largest
off-diagonal S of a row are closer than that it may legitimately pick the other column.  Every case
must keep the reference's smallest such gap >= GAP_FLOOR = 1e-4; a case below the floor gets another
seed (SEED_SHIFT), never a lower floor.  With ge2e_cases' own seeds (129, 11, 256) has 8.8e-5 and
(255, 2, 256) 2.2e-5; shifts + 2 and + 1 lift them to 1.3e-4 and 1.2e-4.  Measured minima of the
table as it stands: 1.2e-4 at (129, 2, 252) up to 1.3e-1 at (5, 2, 4); test_gap_floor_and_live_rows
prints each case's.

Bounds.  The project's rule (ge2e_cases.py): PORT_MAX[stat] is the largest error, against the fp64
reference over the whole table, of the fp32 torch restatement on the CPU with one thread, rounded UP
to two digits; BOUNDS = K PORT_MAX with K = 4; the metric is ge2e_cases.compare.  Measured maxima
(this table, these seeds):
    per_abs 4.24e-06 (255,3,8)    dE_row 1.64e-05 (255,3,8)    loss_abs 2.20e-06 (257,2,16)
    dw 2.75e-07 (128,3,8)         db 9.10e-08 (5,2,4)
"""
import functools
import math

import numpy as np
import torch

import ge2e_cases as gc

FUSED_CASES, SPLIT_CASES, PADDED_FUSED = gc.FUSED_CASES, gc.SPLIT_CASES, gc.PADDED_FUSED
GLOSS_CASE, GLOSS = gc.GLOSS_CASE, gc.GLOSS
SHARD_W, SHARD_B = gc.SHARD_W, gc.SHARD_B
SHARDED_CASES, SPLIT_SHARDED_CASES = gc.SHARDED_CASES, gc.SPLIT_SHARDED_CASES
all_inputs, case_id, compare, over, fmt, shard_slices = (gc.all_inputs, gc.case_id, gc.compare, gc.over, gc.fmt,
                                                         gc.shard_slices)

GAP_FLOOR = 1e-4
# seeds moved where the first draw's top-two gap fell below GAP_FLOOR
SEED_SHIFT = {(129, 11, 256): 2, (255, 2, 256): 1, (129, 16, 256): 9}

# one shape beyond ge2e_cases' table: 2064 rows above GF_TILE speakers, where the contrast rows kernel
# runs 16 rows per workgroup on a 256-CU device (csrc/sv_ge2e.hip ct_rows_per_wg; the table's own
# shapes reach 4 and 8).  Its reference is contrast_per_mm's (the broadcast form would take 4 GB);
# first seed shift with a gap above the floor: 9 (7.1e-4).  It is part of the PORT_MAX table.
BIG_CASE = (129, 16, 256, 10.0, -5.0)

K = 4
PORT_MAX = {"per_abs": 4.3e-6, "dE_row": 1.7e-5, "loss_abs": 2.3e-6, "dw": 2.8e-7, "db": 9.2e-8}
BOUNDS = {k: K * v for k, v in PORT_MAX.items()}


@functools.lru_cache(maxsize=None)
def inputs(N, M, D):
    """The off-sphere E of a shape (read-only, shared): ge2e_cases' seed + SEED_SHIFT."""
    E = gc.make_offsphere(7000 + 31 * N + 17 * M + D + SEED_SHIFT.get((N, M, D), 0), N, M, D)
    E.setflags(write=False)
    return E


def _eye(N, M, K):
    eye = torch.zeros(N, M, K, dtype=torch.bool)
    eye[torch.arange(N), :, torch.arange(N)] = True
    return eye


def contrast_on_S(S):
    """(per [N,M], k* [N,M]) of the contrast loss on a given S [N,M,K], K >= N: differentiable, the
    dtype is S's.  The positive is column j, the maximum runs over every k != j."""
    N, M, Kc = S.shape
    eye = _eye(N, M, Kc)
    pos = S[eye].view(N, M)
    neg, idx = S.masked_fill(eye, -math.inf).max(dim=2)
    return 1 - torch.sigmoid(pos) + torch.sigmoid(neg), idx


def contrast_per(E, w, b):
    """(per, S, k*) of E [N,M,D] (torch, any float dtype): the reference formulas."""
    S = w * gc.cossim_torch(E, E.mean(dim=1)) + b
    per, idx = contrast_on_S(S)
    return per, S, idx


def contrast_per_mm(E, w, b):
    """contrast_per with the cosines as one matrix product (oracle.torch_port.ge2e_per's form) in place
    of cossim_torch's [N, M, N, D] broadcast: the same formulas, for shapes where the broadcast would
    take gigabytes.  Agrees with contrast_per to fp64 rounding (tests/test_contrast_cases.py)."""
    N, M, _ = E.shape
    U = (E.sum(dim=1, keepdim=True) - E) / (M - 1)
    C = E.mean(dim=1)
    En = E / E.norm(dim=2, keepdim=True).clamp_min(1e-8)
    Cn = C / C.norm(dim=1, keepdim=True).clamp_min(1e-8)
    Un = U / U.norm(dim=2, keepdim=True).clamp_min(1e-8)
    cos = torch.where(_eye(N, M, N), (En * Un).sum(-1)[:, :, None], torch.einsum("jid,kd->jik", En, Cn)) + 1e-6
    S = w * cos + b
    per, idx = contrast_on_S(S)
    return per, S, idx


def contrast_loop(E, w, b):
    """Eq. 7 spelled out with loops on numpy fp64 (no autograd): per [N,M]."""
    E = np.asarray(E, np.float64)
    N, M, _ = E.shape

    def cosine(x, y):
        return float(x @ y) / (max(np.linalg.norm(x), 1e-8) * max(np.linalg.norm(y), 1e-8))

    per = np.zeros((N, M))
    for j in range(N):
        for i in range(M):
            s = []
            for k in range(N):
                c = (E[j].sum(0) - E[j, i]) / (M - 1) if k == j else E[k].mean(0)
                s.append(w * (cosine(E[j, i], c) + 1e-6) + b)
            sig = [1.0 / (1.0 + math.exp(-v)) for v in s]
            per[j, i] = 1.0 - sig[j] + max(v for k, v in enumerate(sig) if k != j)
    return per


def top_two_gap(S):
    """The smallest gap between the two largest off-diagonal S of any row (inf with one negative)."""
    N, M, Kc = S.shape
    if Kc < 3:
        return math.inf
    top = S.detach().masked_fill(_eye(N, M, Kc), -math.inf).topk(2, dim=2).values
    return float((top[..., 0] - top[..., 1]).min())


def _run(N, M, D, w, b, gloss, dtype, per_fn=None):
    E = torch.tensor(inputs(N, M, D), dtype=dtype, requires_grad=True)
    wt = torch.tensor(w, dtype=dtype, requires_grad=True)
    bt = torch.tensor(b, dtype=dtype, requires_grad=True)
    per, S, idx = (per_fn or contrast_per)(E, wt, bt)
    loss = per.sum()
    (gloss * loss).backward()
    out = dict(loss=float(loss.detach()), per=per.detach().numpy(), dE=E.grad.numpy(), dw=float(wt.grad),
               db=float(bt.grad), kstar=idx.numpy(), gap=top_two_gap(S))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(N, M, D, w, b, gloss=1.0):
    """The fp64 reference's dict(loss, per, dE, dw, db, kstar, gap) of a case, computed once
    (read-only).  The gradients are those of gloss * loss."""
    return _run(N, M, D, w, b, gloss, torch.float64)


@functools.lru_cache(maxsize=None)
def reference_mm(N, M, D, w, b):
    """reference() through contrast_per_mm (BIG_CASE)."""
    return _run(N, M, D, w, b, 1.0, torch.float64, contrast_per_mm)


def port_f32(N, M, D, w, b, per_fn=None):
    """The same restatement in fp32 on the CPU with one thread (one summation order anywhere)."""
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _run(N, M, D, w, b, 1.0, torch.float32, per_fn)
    finally:
        torch.set_num_threads(old)
