#!/usr/bin/env python
"""Times the energy-based splitting (features.split / frame_energy, one HIP launch per ragged batch)
against the same framed energy composed from stock torch on the same device.

Workloads (seeded):
  speaker  one speaker's worth: 10 utterances of 3 s at 16 kHz (940 frames of 2048 / 512)
  hour     one 3600 s waveform, 112 501 frames

Per workload, the median over --repeats timed windows of --calls calls each, after --warmup calls,
all in this one process:
  split_host  features.split on host arrays: pack, one copy in, one launch, one copy out, the
              numpy threshold and edges (host clock)
  hip_dev     features.frame_energy on device-resident waveforms (cat + offset copy + launch;
              device events)
  hip_kernel  sv_frame_energy alone on pre-packed device buffers (device events)
  torch_dev   per waveform reflect-pad -> unfold -> square -> mean, results concatenated, on
              device-resident waveforms (device events)
and the largest relative difference between the two results.  Prints one JSON line.  Needs a GPU.
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

SR, FRAME, HOP = 16000, 2048, 512


def workload(name, rng):
    lengths = [3 * SR] * 10 if name == "speaker" else [3600 * SR]
    return [(0.1 * rng.standard_normal(int(n))).astype(np.float32) for n in lengths]


def torch_energy(waves):
    outs = []
    for y in waves:
        p = torch.nn.functional.pad(y[None, None, :], (FRAME // 2, FRAME // 2), mode="reflect")[0, 0]
        outs.append(p.unfold(0, FRAME, HOP).square().mean(dim=1))
    return torch.cat(outs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="speaker,hour")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="calls per timed window (0: 50 for speaker, 3 for hour)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("split_bench.py needs a GPU: there is no CPU timing path")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    result = {"bench": "split", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "workloads": {}}
    for name in args.workloads.split(","):
        waves = workload(name, rng)
        calls = args.calls or (50 if name == "speaker" else 3)
        dwaves = [torch.from_numpy(w).to(dev) for w in waves]
        seg_off, frame_off = features.energy_offsets([len(w) for w in waves], FRAME, HOP)
        n_frames = int(frame_off[-1])
        y = torch.cat(dwaves)
        so, fo = torch.from_numpy(seg_off).to(dev), torch.from_numpy(frame_off).to(dev)
        mse = torch.empty(n_frames, device=dev)

        def kernel():
            features.frame_energy_into(y, so, fo, len(waves), n_frames, FRAME, HOP, mse)

        got = features.frame_energy(waves)[0]
        ref = torch_energy(dwaves)
        diff = float(((got - ref).abs() / ref).max())
        r = {"waveforms": len(waves), "frames": n_frames, "calls_per_window": calls, "max_rel_hip_vs_torch": diff}
        for key, t in (("split_host", timed_host(lambda: features.split(waves, top_db=30), args.repeats,
                                                 args.warmup, calls)),
                       ("hip_dev", timed_events(lambda: features.frame_energy(dwaves), args.repeats, args.warmup,
                                                calls)),
                       ("hip_kernel", timed_events(kernel, args.repeats, args.warmup, calls)),
                       ("torch_dev", timed_events(lambda: torch_energy(dwaves), args.repeats, args.warmup, calls))):
            r[key + "_ms"] = {"median": round(t[0], 4), "min": round(t[1], 4), "max": round(t[2], 4)}
        # every frame reads frame_length samples (from L2 after the first touch)
        r["hip_kernel_read_gbs"] = round(4.0 * n_frames * FRAME / (r["hip_kernel_ms"]["median"] * 1e-3) / 1e9, 1)
        r["torch_over_hip_dev"] = round(r["torch_dev_ms"]["median"] / r["hip_dev_ms"]["median"], 2)
        r["torch_over_hip_kernel"] = round(r["torch_dev_ms"]["median"] / r["hip_kernel_ms"]["median"], 2)
        result["workloads"][name] = r
        del dwaves, y, mse, got, ref
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
