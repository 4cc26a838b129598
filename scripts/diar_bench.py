#!/usr/bin/env python
"""Times spectral diarization (diarization.py, csrc/sv_diar.hip) against the torch form a user can
write today on the same GPU, per stage and for the whole cluster(), on synthetic d-vector sequences
(D = 256, --speakers planted speakers in runs of 20 rows, the recipe of tests/diar_ref.planted):

  n1024, n4096   one file of that many d-vectors (iteration_parts_ms: one sv_diar_spmm, sv_diar_gram,
                 the batched 16 x 16 eigh with the construction of T, and sv_diar_rmul, each alone)
  batch64        64 files of 400 .. 600 d-vectors

torch form, file by file in a Python loop: x @ x.T; the cropped diagonal by masked_fill and max, the
blur as one conv2d with the outer product of the taps over conv1d normalisers; torch.kthvalue for
the row thresholds; Y @ Y.T; the row-max normalisation; a full torch.linalg.eigh for 16 eigenpairs;
the eigengap on the host; a Lloyd loop of torch ops with the same start and stopping rule.

Device events around windows of calls (_timing.timed_events); the two legs of every stage alternate
(ours, torch, ours, torch) and each reports the smaller of its two medians.  Prints one JSON line and
writes it to --out.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_speaker_verification_amd import diarization as D  # noqa: E402
from _timing import timed_events  # noqa: E402

DIM, RUN = 256, 20


def planted(n, k, seed, dev):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    c = torch.randn((k, DIM), generator=g, dtype=torch.float64)
    c /= c.norm(dim=1, keepdim=True)
    lab = (torch.arange(n) // RUN) % k
    x = c[lab] + 0.5 * torch.randn((n, DIM), generator=g, dtype=torch.float64) / DIM ** 0.5
    return (x / x.norm(dim=1, keepdim=True)).float().to(dev).contiguous()


# ---- the torch form, one file at a time
def t_crop_blur(A, g1):
    n, r = A.shape[0], (g1.numel() - 1) // 2
    eye = torch.eye(n, dtype=torch.bool, device=A.device)
    A = torch.where(eye, A.masked_fill(eye, float("-inf")).max(dim=1).values[:, None], A)
    num = F.conv2d(A[None, None], (g1[:, None] * g1[None, :])[None, None], padding=r)[0, 0]
    c = F.conv1d(torch.ones((1, 1, n), device=A.device), g1[None, None], padding=r)[0, 0]
    return num / (c[:, None] * c[None, :])


def t_threshold_sym(B, p, mult):
    tau = torch.kthvalue(B, D.threshold_rank(B.shape[0], p) + 1, dim=1).values
    T = torch.where(B >= tau[:, None], B, mult * B)
    return torch.maximum(T, T.T)


def t_row_norm(Z):
    d = Z.max(dim=1).values
    r = torch.where(d > 0, d.clamp_min(1e-30).rsqrt(), torch.zeros_like(d))
    return Z * (r[:, None] * r[None, :])


def t_eig(S):
    w, v = torch.linalg.eigh(S)
    return w.flip(0)[:D.M], v.flip(1)[:, :D.M]


def t_kmeans(E, k, max_iter=100):
    cen = [E[0]]
    for _ in range(1, k):
        md = torch.cdist(E, torch.stack(cen)).square().min(dim=1).values
        cen.append(E[md.argmax()])
    C = torch.stack(cen)
    lab = torch.full((E.shape[0],), -1, device=E.device)
    for _ in range(max_iter):
        new = torch.cdist(E, C).argmin(dim=1)
        if torch.equal(new, lab):
            break
        lab = new
        one = F.one_hot(lab, k).to(E.dtype)
        cnt = one.sum(dim=0)
        C = torch.where(cnt[:, None] > 0, (one.T @ E) / cnt.clamp_min(1)[:, None], C)
    return lab


def t_cluster(xs, g1, p, mult):
    out = []
    for x in xs:
        S = t_row_norm((lambda Y: Y @ Y.T)(t_threshold_sym(t_crop_blur(x @ x.T, g1), p, mult)))
        lam, U = t_eig(S)
        k = D.n_speakers(lam.double().cpu().numpy(), x.shape[0])
        E = U[:, :k] / U[:, :k].norm(dim=1, keepdim=True).clamp_min(1e-30)
        out.append(t_kmeans(E, k).cpu().numpy())
    return out


def split(buf, tb):
    """The files' matrices of a packed buffer as contiguous [n, n] device tensors (the torch form's inputs)."""
    return [buf[int(o):int(o) + int(n) * int(ld)].view(int(n), int(ld))[:, :int(n)].contiguous()
            for n, ld, o in zip(tb.ns, tb.ld, tb.mat_off)]


def legs(ours, theirs, repeats, calls=1):
    a, b = [], []
    for _ in range(2):
        a.append(timed_events(ours, repeats, 1, calls)[0])
        b.append(timed_events(theirs, repeats, 1, calls)[0])
    a, b = min(a), min(b)
    return {"ours_ms": round(a, 4), "torch_ms": round(b, 4), "torch_over_ours": round(b / a, 2)}


def bench_case(ns, k, repeats, dev):
    xs = [planted(n, k, 1000 + i, dev) for i, n in enumerate(ns)]
    x = torch.cat(xs)
    tb = D.matrix_tables(ns, dev)
    sigma, p, mult = 1.0, 0.95, 0.01
    g = D.gaussian_taps(sigma)
    g1 = torch.from_numpy(np.concatenate([g[:0:-1], g])).to(dev)
    A = D.affinity(x, tb)
    B = D.crop_blur(A.clone(), tb, sigma)
    _, Y = D.threshold_sym(B, tb, p, mult)
    Z = D.diffuse(Y, tb)
    S, _ = D.row_norm(Z, tb)
    lam, U, _, iters, conv = D.top_eigenpairs(S, tb, strict=False)
    lam_h = lam.cpu().numpy()
    ks = [D.n_speakers(lam_h[f], n) for f, n in enumerate(ns)]
    E = D.spectral_embedding(U, tb, ks)
    As, Bs, Ys, Zs, Ss = (split(m, tb) for m in (A, B, Y, Z, S))
    Es = [E[int(a):int(b), :kk].contiguous() for a, b, kk in zip(tb.row_off[:-1], tb.row_off[1:], ks)]
    few = max(2, repeats // 2)
    res = {"ns": [int(n) for n in ns] if len(ns) <= 4 else f"{len(ns)} files, {min(ns)} .. {max(ns)} rows",
           "k_found": sorted(set(ks)), "eig_iters_max": int(iters.max()), "eig_converged": bool(conv.all())}
    res["affinity"] = legs(lambda: D.affinity(x, tb), lambda: [v @ v.T for v in xs], repeats)
    res["crop_blur"] = legs(lambda: D.crop_blur(A.clone(), tb, sigma), lambda: [t_crop_blur(a.clone(), g1) for a in As], repeats)
    res["threshold_sym"] = legs(lambda: D.threshold_sym(B, tb, p, mult), lambda: [t_threshold_sym(b, p, mult) for b in Bs],
                                repeats)
    res["diffuse"] = legs(lambda: D.diffuse(Y, tb), lambda: [y @ y.T for y in Ys], repeats)
    res["row_norm"] = legs(lambda: D.row_norm(Z, tb), lambda: [t_row_norm(z) for z in Zs], repeats)
    res["eigenpairs"] = legs(lambda: D.top_eigenpairs(S, tb, strict=False), lambda: [t_eig(s) for s in Ss], few)
    # the parts of one subspace iteration, alone (no torch counterpart: the torch form has no iteration)
    W = D.start_block(tb, dev)
    G = D.gram(W, W, tb)
    T = D._orthonormaliser(G)
    res["iteration_parts_ms"] = {
        "spmm": round(timed_events(lambda: D.spmm(S, W, T, tb), repeats, 1, 10)[0], 4),
        "gram": round(timed_events(lambda: D.gram(W, W, tb), repeats, 1, 10)[0], 4),
        "eigh16_and_T": round(timed_events(lambda: D._orthonormaliser(G), repeats, 1, 10)[0], 4),
        "rmul": round(timed_events(lambda: D.rmul(W, T, tb), repeats, 1, 10)[0], 4)}
    res["kmeans"] = legs(lambda: D.kmeans(E, tb, ks), lambda: [t_kmeans(e, kk) for e, kk in zip(Es, ks)], repeats)
    res["cluster"] = legs(lambda: D.cluster(xs, strict=False), lambda: t_cluster(xs, g1, p, mult), few)
    ours, _ = D.cluster(xs, strict=False)
    theirs = t_cluster(xs, g1, p, mult)
    res["labels_equal_torch"] = bool(all(np.array_equal(a, D.relabel(b)) for a, b in zip(ours, theirs)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--speakers", type=int, default=4)
    ap.add_argument("--cases", nargs="+", default=["n1024", "n4096", "batch64"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "diar_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("diar_bench.py needs a GPU: there is no CPU timing path")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    shapes = {"n1024": [1024], "n4096": [4096], "batch64": [int(v) for v in rng.integers(400, 601, 64)]}
    result = {"bench": "diar", "device": torch.cuda.get_device_name(0), "D": DIM, "speakers": args.speakers, "cases": {}}
    with torch.no_grad():
        for name in args.cases:
            result["cases"][name] = bench_case(shapes[name], args.speakers, args.repeats, dev)
            torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
