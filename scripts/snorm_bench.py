#!/usr/bin/env python
"""Times adaptive score normalisation (csrc/sv_snorm.hip, sv_trial_hist_norm of csrc/sv_trials.hip)
against what a user can write with torch on the same GPU; D = 256, unit rows of synthetic speakers
(trial_hist_bench.make_rows), a cohort of unit rows of other speakers, top_k = 300:

  stats      sv_cohort_topk_stats at N in --rows x Nc in --cohorts: device events around windows of
             launches (the _timing helper); *_tf is 5 passes x N Nc x 2 D flops over the time -- what
             the kernel executes, of which only one pass is the scores themselves.
             torch form: chunked x[i0:i1] @ c.T (a chunk's score block is at most --chunk-mb),
             torch.topk, mean and std(unbiased=False) of the k values; the two forms' largest
             difference in mean and std is reported, not asserted.
  passes     with --stamp-lib (a -DSV_SNORM_STAMP build: `make ab NAME=snormstamp
             FLAGS=-DSV_SNORM_STAMP`): wave 0's cycles in each of the 4 select passes and the sum
             pass, summed over the workgroups, as shares of their total and as shares of stats_ms
  hist       at U = --trials: sv_trial_hist over [-1, 1) and sv_trial_hist_norm over norm_range, both
             symmetric with 4096 bins, the rows normalised by their statistics against the
             first cohort; the torch form of trial_hist_bench on z (chunked GEMM, z and the slot rule in
             torch ops, torch.bincount)
Prints one JSON line and writes it to --out.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_speaker_verification_amd import _lib, verification  # noqa: E402
from pytorch_speaker_verification_amd._lib import call, ptr, stream_of  # noqa: E402
from _timing import timed_events  # noqa: E402
from trial_hist_bench import BINS, D, make_rows  # noqa: E402

TOP_K = 300


def make_cohort(nc, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(10 ** 6 + nc)
    c = torch.randn((nc, D), generator=g, device=dev)
    return (c / c.norm(dim=1, keepdim=True)).contiguous()


def torch_stats(x, c, chunk_rows):
    mean, std = [], []
    for i0 in range(0, x.shape[0], chunk_rows):
        top = torch.topk(x[i0:i0 + chunk_rows] @ c.T, TOP_K, dim=1).values
        mean.append(top.mean(dim=1))
        std.append(top.std(dim=1, unbiased=False))
    return torch.cat(mean), torch.cat(std)


def torch_hist_norm(a, lab, mu, inv, lo, inv_width, chunk_rows):
    """counts int64 [2, BINS + 2] of z over the pairs i < j, chunk by chunk, with torch ops only."""
    U = a.shape[0]
    counts = torch.zeros(2 * (BINS + 2), dtype=torch.int64, device=a.device)
    for i0 in range(0, U, chunk_rows):
        i1 = min(i0 + chunk_rows, U)
        s = a[i0:i1] @ a[i0:].T
        z = 0.5 * ((s - mu[i0:i1, None]) * inv[i0:i1, None] + (s - mu[None, i0:]) * inv[None, i0:])
        q = torch.floor((z - lo) * inv_width)
        slot = torch.where(q >= 0, torch.clamp(q, max=float(BINS)) + 1, torch.zeros_like(q)).to(torch.int64)
        slot += (lab[i0:i1, None] == lab[None, i0:]) * (BINS + 2)
        rows = torch.arange(i1 - i0, device=a.device)[:, None]
        cols = torch.arange(U - i0, device=a.device)[None, :]
        counts += torch.bincount(slot[cols > rows], minlength=2 * (BINS + 2))
    return counts.view(2, BINS + 2)


def stamp_lib(path):
    h = ctypes.CDLL(path)
    if not hasattr(h, "sv_snorm_stamp_read"):
        sys.exit(f"{path} is not a -DSV_SNORM_STAMP build")
    h.sv_cohort_topk_stats.restype, h.sv_cohort_topk_stats.argtypes = _lib.SIGNATURES["sv_cohort_topk_stats"]
    h.sv_snorm_stamp_read.restype, h.sv_snorm_stamp_read.argtypes = ctypes.c_int, [ctypes.c_void_p]
    return h


def stamped(h, x, c, out):
    """wave 0's cycles in the passes 0 .. 4 of one launch, summed over the workgroups."""
    cyc = (ctypes.c_ulonglong * 5)()
    for _ in range(2):  # (the first read clears what the warm-up left)
        rc = h.sv_cohort_topk_stats(ptr(x), D, x.shape[0], ptr(c), D, c.shape[0], D, TOP_K, ptr(out[0]), ptr(out[1]), 0,
                                    stream_of(x))
        if rc or h.sv_snorm_stamp_read(ctypes.addressof(cyc)):
            sys.exit("stamp build: the launch or the read failed")
    return [int(v) for v in cyc]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--cohorts", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--trials", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk-mb", type=int, default=512, help="largest score block of the torch forms")
    ap.add_argument("--stamp-lib", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "snorm_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("snorm_bench.py needs a GPU: there is no CPU timing path")
    dev = torch.device("cuda", 0)
    sh = stamp_lib(args.stamp_lib) if args.stamp_lib else None
    result = {"bench": "snorm", "device": torch.cuda.get_device_name(0), "D": D, "top_k": TOP_K, "bins": BINS,
              "chunk_mb": args.chunk_mb, "stats": {}, "hist": {}}
    for N in args.rows:
        x, _ = make_rows(N, dev)
        for nc in args.cohorts:
            c = make_cohort(nc, dev)
            out = torch.empty((2, N), dtype=torch.float32, device=dev)

            def fused():
                call("sv_cohort_topk_stats", ptr(x), D, N, ptr(c), D, nc, D, TOP_K, ptr(out[0]), ptr(out[1]), 0,
                     stream_of(x))

            flops = 5 * N * nc * 2 * D
            calls = max(1, min(200, int(0.1 / (flops / 50e12))))  # windows of about 0.1 s at every size
            t_f = timed_events(fused, args.repeats, 2, calls)
            chunk_rows = max(1, min(N, args.chunk_mb * 2 ** 20 // (4 * nc)))
            ref = torch_stats(x, c, chunk_rows)
            t_calls = max(1, min(50, int(0.1 / (N * nc * 2 * D / 5e12))))
            t_t = timed_events(lambda: torch_stats(x, c, chunk_rows), max(3, args.repeats // 2), 1, t_calls)
            row = {"stats_ms": round(t_f[0], 4), "stats_min_ms": round(t_f[1], 4), "stats_max_ms": round(t_f[2], 4),
                   "stats_tf": round(flops / t_f[0] / 1e9, 2), "calls_per_window": calls,
                   "torch_ms": round(t_t[0], 3), "torch_min_ms": round(t_t[1], 3), "torch_max_ms": round(t_t[2], 3),
                   "torch_chunk_rows": chunk_rows, "torch_over_stats": round(t_t[0] / t_f[0], 2),
                   "max_mean_diff": float((out[0] - ref[0]).abs().max()), "max_std_diff": float((out[1] - ref[1]).abs().max())}
            if sh:
                cyc = stamped(sh, x, c, out)
                tot = float(sum(cyc))
                row["stamp"] = {"pass_cycles": cyc, "pass_share": [round(v / tot, 4) for v in cyc],
                                "pass_ms": [round(v / tot * t_f[0], 4) for v in cyc]}
            result["stats"][f"{N}x{nc}"] = row
            del c, out, ref
        del x
        torch.cuda.empty_cache()

    U = args.trials
    a, lab = make_rows(U, dev)
    mu, inv = verification.as_norm(a, make_cohort(args.cohorts[0], dev), TOP_K)
    lo_n, hi_n = verification.norm_range((mu, inv))
    lo32, _, inv32 = verification.bin_params(BINS, -1.0, 1.0)
    lon32, hin32, invn32 = verification.bin_params(BINS, lo_n, hi_n)
    hist = torch.zeros(2 * (BINS + 2), dtype=torch.int64, device=dev)

    def plain():
        call("sv_trial_hist", ptr(a), D, ptr(lab), U, ptr(a), D, ptr(lab), U, D, 1, float(lo32), float(inv32), BINS,
             ptr(hist), 0, stream_of(a))

    def normed():
        call("sv_trial_hist_norm", ptr(a), D, ptr(lab), U, ptr(a), D, ptr(lab), U, D, 1, float(lon32), float(invn32),
             BINS, ptr(mu), ptr(inv), ptr(mu), ptr(inv), ptr(hist), 0, stream_of(a))

    pairs = U * (U - 1) // 2
    calls = max(1, min(200, int(0.1 / (U * U * D / 50e12))))
    t_p, t_n = [], []
    for _ in range(2):  # the two kernels alternate
        t_p.append(timed_events(plain, args.repeats, 2, calls))
        t_n.append(timed_events(normed, args.repeats, 2, calls))
    t_p, t_n = min(t_p), min(t_n)
    hist.zero_()
    normed()
    got = hist.view(2, BINS + 2).cpu().numpy().copy()
    chunk_rows = max(1, min(U, args.chunk_mb * 2 ** 20 // (4 * U)))
    ref = torch_hist_norm(a, lab, mu, inv, float(lon32), float(invn32), chunk_rows).cpu().numpy()
    t_t = timed_events(lambda: torch_hist_norm(a, lab, mu, inv, float(lon32), float(invn32), chunk_rows),
                       max(3, args.repeats // 2), 1, 1)
    diff = np.abs(ref - got)
    result["hist"] = {"U": U, "pairs": pairs, "cohort": args.cohorts[0], "range": [lo_n, hi_n],
                      "plain_ms": round(t_p[0], 4), "plain_min_ms": round(t_p[1], 4), "plain_max_ms": round(t_p[2], 4),
                      "norm_ms": round(t_n[0], 4), "norm_min_ms": round(t_n[1], 4), "norm_max_ms": round(t_n[2], 4),
                      "norm_over_plain": round(t_n[0] / t_p[0], 4),
                      "norm_tf": round(pairs * 2 * D / t_n[0] / 1e9, 2), "calls_per_window": calls,
                      "torch_ms": round(t_t[0], 3), "torch_min_ms": round(t_t[1], 3), "torch_max_ms": round(t_t[2], 3),
                      "torch_over_norm": round(t_t[0] / t_n[0], 2), "counts_ok": bool(got.sum() == pairs == ref.sum()),
                      "outside_range": int(got[:, 0].sum() + got[:, -1].sum()),
                      "scores_in_another_bin": int(diff.sum() // 2), "max_slot_diff": int(diff.max())}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
