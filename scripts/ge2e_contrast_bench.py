"""The fused GE2E step (ops.ge2e_train) with the contrast loss against the softmax loss of the same
build, at the c2 shape (64, 10, 256) and the c5 global shape (256, 10, 256).

The two run in alternating windows of `--calls` calls each (device events around a window, `--repeats`
windows per loss after a warm-up of both), so drift of the shared machine hits both alike.  Prints one
JSON line: per shape and loss the median / min / max microseconds per call, and the spread
(max - min) / median of each, with the loss and sum |dE| of what was timed.  `--lib` loads an A/B
build of the library.  Kernel times: rocprofv3 --kernel-trace --stats over this script.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_speaker_verification_amd import _lib, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--lib", default=None, help="an A/B build of the library to load instead of the shipped one")
    a = ap.parse_args()
    if a.lib:
        _lib.use_library(os.path.abspath(a.lib))
    if not torch.cuda.is_available():
        sys.exit("ge2e_contrast_bench: no GPU")
    dev = torch.device("cuda", 0)
    out = {}
    for N, M, D in ((64, 10, 256), (256, 10, 256)):
        g = torch.Generator().manual_seed(N)
        E = torch.nn.functional.normalize(torch.randn(N, M, D, generator=g), dim=2).to(dev)
        w, b = torch.tensor(10.0, device=dev), torch.tensor(-5.0, device=dev)
        dwdb = torch.empty(2, device=dev)
        fns = {m: (lambda m=m: ops.ge2e_train(E, w, b, dwdb_out=dwdb, loss_method=m)) for m in ("softmax", "contrast")}
        for f in fns.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        us = {m: [] for m in fns}
        for _ in range(a.repeats):
            for m, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    f()
                e1.record()
                e1.synchronize()
                us[m].append(e0.elapsed_time(e1) / a.calls * 1e3)
        res = {}
        for m, v in us.items():
            med = statistics.median(v)
            res[m] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                      "spread": round((max(v) - min(v)) / med, 3)}
        for m, f in fns.items():  # (what was timed: the loss and a checksum of dE)
            loss, _, dE, _ = f()
            res[m]["loss"], res[m]["dE_abs_sum"] = float(loss), float(dE.double().abs().sum())
        res["contrast_over_softmax"] = round(res["contrast"]["median_us"] / res["softmax"]["median_us"], 3)
        out[f"N{N}xM{M}xD{D}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
