#!/usr/bin/env python
"""Times the log-mel front end (features.logmel, one fused HIP launch per ragged batch) against the
same function composed from stock torch on the same device (torch.stft + matmul + log10).

Workloads (seeded):
  file  one file's worth: 40 segments of 0.4 - 4 s at 16 kHz (the shape dvector_create.py runs per file)
  hour  an hour's worth: one 3600 s segment, 360 001 frames (torch's best case: a single stft call)

Per workload, the median over --repeats timed windows of --calls calls each, after --warmup calls,
all in this one process:
  hip_host    features.logmel on host arrays: pack, one copy in, one launch (host clock around a
              device synchronise)
  hip_dev     features.logmel on device-resident segments (cat + offset copy + launch; device events)
  hip_kernel  sv_logmel alone on pre-packed device buffers (device events)
  torch_dev   per segment torch.stft(center, reflect) -> |.|^2 -> mel matmul -> log10, results
              concatenated, on device-resident segments (device events)
and the largest difference between the two results.  Prints one JSON line.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_speaker_verification_amd import features  # noqa: E402
from _timing import timed_events, timed_host  # noqa: E402

SR, NFFT, WIN, HOP, NMELS = 16000, 512, 400, 160, 40


def workload(name, rng):
    if name == "file":
        lengths = rng.integers(int(0.4 * SR), int(4.0 * SR), size=40)
    else:
        lengths = [3600 * SR]
    return [(0.1 * rng.standard_normal(int(n))).astype(np.float32) for n in lengths]


def torch_logmel(segs, window, melfb_t):
    outs = []
    for y in segs:
        S = torch.stft(y, NFFT, HOP, WIN, window, center=True, pad_mode="reflect", return_complex=True)
        P = S.real.square() + S.imag.square()  # [nb, T]
        outs.append(torch.log10(P.t() @ melfb_t + 1e-6))
    return torch.cat(outs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="file,hour")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="calls per timed window (0: 50 for file, 3 for hour)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("logmel_bench.py needs a GPU: there is no CPU timing path")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    wbasis, melfb = features.stft_tables(SR, NFFT, WIN, NMELS, dev)
    window = torch.hann_window(WIN, periodic=True, device=dev)
    melfb_t = melfb.t().contiguous()
    result = {"bench": "logmel", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "workloads": {}}
    for name in args.workloads.split(","):
        segs = workload(name, rng)
        calls = args.calls or (50 if name == "file" else 3)
        dsegs = [torch.from_numpy(s).to(dev) for s in segs]
        seg_off, frame_off = features.segment_offsets([len(s) for s in segs], NFFT, HOP)
        n_frames = int(frame_off[-1])
        y = torch.cat(dsegs)
        so, fo = torch.from_numpy(seg_off).to(dev), torch.from_numpy(frame_off).to(dev)
        out = torch.empty((n_frames, NMELS), device=dev)

        def kernel():
            features.logmel_into(y, so, fo, len(segs), n_frames, NFFT, WIN, HOP, NMELS, wbasis, melfb, out)

        got = features.logmel(segs)[0]
        ref = torch_logmel(dsegs, window, melfb_t)
        diff = float((got - ref).abs().max())
        r = {"segments": len(segs), "frames": n_frames, "calls_per_window": calls, "max_abs_hip_vs_torch": diff}
        for key, t in (("hip_host", timed_host(lambda: features.logmel(segs), args.repeats, args.warmup, calls)),
                       ("hip_dev", timed_events(lambda: features.logmel(dsegs), args.repeats, args.warmup, calls)),
                       ("hip_kernel", timed_events(kernel, args.repeats, args.warmup, calls)),
                       ("torch_dev", timed_events(lambda: torch_logmel(dsegs, window, melfb_t), args.repeats,
                                                  args.warmup, calls))):
            r[key + "_ms"] = {"median": round(t[0], 4), "min": round(t[1], 4), "max": round(t[2], 4)}
        # the fused kernel's arithmetic: frames x (2 nb columns) x win taps, 2 flops each, + the mel product
        flops = 2.0 * n_frames * (NFFT + 2) * WIN + 2.0 * n_frames * (NFFT // 2 + 1) * NMELS
        r["hip_kernel_tflops"] = round(flops / (r["hip_kernel_ms"]["median"] * 1e-3) / 1e12, 2)
        r["torch_over_hip_dev"] = round(r["torch_dev_ms"]["median"] / r["hip_dev_ms"]["median"], 2)
        result["workloads"][name] = r
        del dsegs, y, out, got, ref
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
