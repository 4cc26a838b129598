#!/usr/bin/env python
"""Times the fused trial scorer (sv_trial_hist, csrc/sv_trials.hip) against what a user can write with
torch on the same GPU, symmetric mode, D = 256, 4096 bins on [-1, 1), unit rows of synthetic speakers
(25 utterances each), at U in --sizes (default 4096, 16384, 65536):

  fused_ms   one sv_trial_hist launch: device events around windows of launches (the _timing helper)
  torch_ms   the same pairs as chunked A[i0:i1] @ A[i0:].T (a chunk's score block is at most
             --chunk-mb) plus a per-chunk histogram: the slot rule of include/sv_ge2e.h written with
             torch ops on the block, the pairs i < j and the two classes by masks, torch.bincount
  *_tf       the implied rate: U (U - 1) / 2 pairs x 2 D flops over the time (the fused kernel also
             computes the lower halves of its diagonal tiles, the torch form the lower half of every
             chunk's first block; neither is counted)
  counts     both histograms summed to U (U - 1) / 2, and how far they differ: the two forms add the
             256 products of a score in different orders, so a score within rounding of an edge may
             land one bin over -- the differences are reported, not asserted
  epilogue   with --stamp-lib (a -DSV_TRIAL_STAMP build of the library: `make ab NAME=trialstamp
             FLAGS=-DSV_TRIAL_STAMP`): wave 0's cycles inside the k-loops and inside the LDS-atomic
             epilogues, summed over the workgroups, and the epilogue's share of the two
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

D, BINS, PER_SPEAKER = 256, 4096, 25


def make_rows(U, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(U)
    lab = torch.arange(U, device=dev, dtype=torch.int32) // PER_SPEAKER
    mean = torch.randn((int(lab.max()) + 1, D), generator=g, device=dev)
    x = mean[lab.long()] + 2.5 * torch.randn((U, D), generator=g, device=dev)
    return (x / x.norm(dim=1, keepdim=True)).contiguous(), lab


def torch_hist(a, lab, lo, inv_width, chunk_rows):
    """counts int64 [2, BINS + 2] of the pairs i < j, chunk by chunk, with torch ops only."""
    U = a.shape[0]
    counts = torch.zeros(2 * (BINS + 2), dtype=torch.int64, device=a.device)
    for i0 in range(0, U, chunk_rows):
        i1 = min(i0 + chunk_rows, U)
        s = a[i0:i1] @ a[i0:].T  # [C, U - i0]
        q = torch.floor((s - lo) * inv_width)
        slot = torch.where(q >= 0, torch.clamp(q, max=float(BINS)) + 1, torch.zeros_like(q)).to(torch.int64)
        slot += (lab[i0:i1, None] == lab[None, i0:]) * (BINS + 2)
        rows = torch.arange(i1 - i0, device=a.device)[:, None]
        cols = torch.arange(U - i0, device=a.device)[None, :]
        counts += torch.bincount(slot[cols > rows], minlength=2 * (BINS + 2))
    return counts.view(2, BINS + 2)


def stamped(path, a, lab, lo, inv_width):
    """(k-loop cycles, epilogue cycles) of wave 0 summed over the workgroups, from a stamp build."""
    h = ctypes.CDLL(path)
    res, args = _lib.SIGNATURES["sv_trial_hist"]
    h.sv_trial_hist.restype, h.sv_trial_hist.argtypes = res, args
    h.sv_trial_hist_size.restype, h.sv_trial_hist_size.argtypes = _lib.SIGNATURES["sv_trial_hist_size"]
    words = int(h.sv_trial_hist_size(BINS)) // 8
    if words != 2 * (BINS + 2) + 2:
        sys.exit(f"{path} is not a -DSV_TRIAL_STAMP build")
    hist = torch.zeros(words, dtype=torch.int64, device=a.device)
    U = a.shape[0]
    rc = h.sv_trial_hist(ptr(a), D, ptr(lab), U, ptr(a), D, ptr(lab), U, D, 1, lo, inv_width, BINS, ptr(hist), 0,
                         stream_of(a))
    if rc:
        sys.exit(f"stamp build: sv_trial_hist returned {rc}")
    torch.cuda.synchronize()
    return int(hist[-2]), int(hist[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk-mb", type=int, default=512, help="largest score block of the torch form")
    ap.add_argument("--stamp-lib", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "trial_hist_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("trial_hist_bench.py needs a GPU: there is no CPU timing path")
    dev = torch.device("cuda", 0)
    lo32, _, inv32 = verification.bin_params(BINS, -1.0, 1.0)
    lo, inv_width = float(lo32), float(inv32)
    result = {"bench": "trial_hist", "device": torch.cuda.get_device_name(0), "D": D, "bins": BINS,
              "chunk_mb": args.chunk_mb, "sizes": {}}
    for U in args.sizes:
        a, lab = make_rows(U, dev)
        pairs = U * (U - 1) // 2
        flops = pairs * 2 * D
        hist = torch.zeros(2 * (BINS + 2), dtype=torch.int64, device=dev)

        def fused():
            call("sv_trial_hist", ptr(a), D, ptr(lab), U, ptr(a), D, ptr(lab), U, D, 1, lo, inv_width, BINS, ptr(hist),
                 0, stream_of(a))

        fused()
        torch.cuda.synchronize()
        got = hist.view(2, BINS + 2).cpu().numpy().copy()
        calls = max(1, min(200, int(0.1 / (U * U * D / 50e12))))  # windows of about 0.1 s at every size
        t_f = timed_events(fused, args.repeats, 2, calls)
        row = {"pairs": pairs, "fused_ms": round(t_f[0], 4), "fused_min_ms": round(t_f[1], 4),
               "fused_max_ms": round(t_f[2], 4), "fused_tf": round(flops / t_f[0] / 1e9, 2), "calls_per_window": calls,
               "fused_counts_ok": bool(got.sum() == pairs)}
        chunk_rows = max(1, min(U, args.chunk_mb * 2 ** 20 // (4 * U)))
        ref = torch_hist(a, lab, lo, inv_width, chunk_rows).cpu().numpy()
        t_t = timed_events(lambda: torch_hist(a, lab, lo, inv_width, chunk_rows), max(3, args.repeats // 2), 1, 1)
        diff = np.abs(ref - got)
        row.update({"torch_ms": round(t_t[0], 3), "torch_min_ms": round(t_t[1], 3), "torch_max_ms": round(t_t[2], 3),
                    "torch_tf": round(flops / t_t[0] / 1e9, 2), "torch_chunk_rows": chunk_rows,
                    "torch_over_fused": round(t_t[0] / t_f[0], 2), "torch_counts_ok": bool(ref.sum() == pairs),
                    "classes_agree": bool((ref.sum(axis=1) == got.sum(axis=1)).all()),
                    "scores_in_another_bin": int(diff.sum() // 2), "max_slot_diff": int(diff.max())})
        if args.stamp_lib:
            ck, ce = stamped(args.stamp_lib, a, lab, lo, inv_width)
            row["stamp"] = {"kloop_cycles": ck, "epilogue_cycles": ce, "epilogue_share": round(ce / float(ck + ce), 4)}
        result["sizes"][str(U)] = row
        del a, lab
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
