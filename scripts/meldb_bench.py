#!/usr/bin/env python
"""Times the raw-waveform training feature (features.mel_db_fixed: trim -> fix_length -> mel
magnitude in dB, one sv_frame_energy launch and one sv_meldb call per batch) against the same
definition composed from stock torch on the same device.

Workloads (seeded; every utterance is 0.2 s of silence, 1.6 - 2.4 s of noise, 0.2 s of silence, so
the trim moves both ends and fix_length pads some utterances and cuts others to 29200 samples):
  batch  one training batch: 40 utterances (N = 4 speakers x M = 10), 7320 frames
  big    640 utterances, 117 120 frames

Per workload, the median over --repeats timed windows of --calls calls each, after --warmup calls,
all in this one process:
  fixed_host    features.mel_db_fixed on host arrays: pack, copy in, energy launch, energies back,
                numpy trim bounds, segment table in, sv_meldb (host clock around a device synchronise)
  fixed_dev     the same on device-resident waveforms (host clock: the call waits for the energies)
  meldb_call    sv_meldb alone on the uploaded buffer and segment table: zeroing of seg_max, the
                fused kernel, the clip kernel (device events)
  meldb_noclip  the same with top_db < 0: no clip kernel; meldb_call - meldb_noclip is the clip kernel
  logmel_kernel sv_logmel (power, log10) on the same samples packed as fixed-length segments: the
                same MFMA work without the magnitude's square roots and the maximum (device events)
  torch_dev     torch.stft(center, reflect) of the [n, 29200] batch -> abs -> mel matmul ->
                20 log10(clamp) -> per-utterance amax -> clip, on the already trimmed and fixed
                device batch (device events): torch's best case, no trim and no fix_length in it
and the largest difference between the HIP result and torch's.  Prints one JSON line.  Needs a GPU.
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

SR, NFFT, WIN, HOP, NMELS, LENGTH = 16000, 512, 400, 160, 40, 29200
AMIN, TOP_DB = 1e-5, 80.0


def workload(name, rng):
    n = 40 if name == "batch" else 640
    waves = []
    for _ in range(n):
        body = int(rng.integers(int(1.6 * SR), int(2.4 * SR)))
        y = np.zeros(body + 2 * int(0.2 * SR), dtype=np.float32)
        y[int(0.2 * SR):int(0.2 * SR) + body] = 0.1 * rng.standard_normal(body)
        waves.append(y)
    return waves


def torch_meldb(batch, window, melfb_t):
    S = torch.stft(batch, NFFT, HOP, WIN, window, center=True, pad_mode="reflect", return_complex=True)
    x = S.abs().transpose(1, 2) @ melfb_t  # [n, T, nmels]
    db = 20.0 * torch.log10(torch.clamp(x, min=AMIN))
    return torch.maximum(db, db.amax(dim=(1, 2), keepdim=True) - TOP_DB)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="batch,big")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="calls per timed window (0: 200 for batch, 20 for big)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("meldb_bench.py needs a GPU: there is no CPU timing path")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    wbasis, melfb = features.stft_tables(SR, NFFT, WIN, NMELS, dev)
    window = torch.hann_window(WIN, periodic=True, device=dev)
    melfb_t = melfb.t().contiguous()
    T = 1 + LENGTH // HOP
    result = {"bench": "meldb", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "workloads": {}}
    for name in args.workloads.split(","):
        waves = workload(name, rng)
        n = len(waves)
        calls = args.calls or (200 if name == "batch" else 20)
        dwaves = [torch.from_numpy(w).to(dev) for w in waves]
        got = features.mel_db_fixed(waves, length=LENGTH)
        # the trimmed, fixed batch for the kernel-only timings and for torch
        bounds = [features.trim(w, 60, WIN, HOP)[1] for w in waves]
        fixed = np.zeros((n, LENGTH), dtype=np.float32)
        for row, w, (a, b) in zip(fixed, waves, bounds):
            row[:min(b - a, LENGTH)] = w[a:b][:LENGTH]
        batch = torch.from_numpy(fixed).to(dev)
        seg_off = np.concatenate([[0], np.cumsum([len(w) for w in waves])])
        table = torch.from_numpy(features.fixed_segments(bounds, seg_off, LENGTH, HOP)).to(dev)
        y = torch.cat(dwaves)
        out = torch.empty((n * T, NMELS), device=dev)
        seg_max = torch.empty(n, device=dev)
        lm_so = torch.arange(n + 1, dtype=torch.int32, device=dev) * LENGTH

        def meldb(top_db):
            features.mel_db_into(y, table[:n], table[n:2 * n], table[2 * n:3 * n], table[3 * n:], n, n * T, NFFT, WIN,
                                 HOP, NMELS, wbasis, melfb, out, seg_max, AMIN, top_db)

        def logmel():
            features.logmel_into(batch.view(-1), lm_so, table[3 * n:], n, n * T, NFFT, WIN, HOP, NMELS, wbasis, melfb,
                                 out)

        ref = torch_meldb(batch, window, melfb_t)
        diff = float((got - ref).abs().max())
        padded = sum(1 for a, b in bounds if b - a < LENGTH)
        r = {"utterances": n, "frames": n * T, "padded": padded, "truncated": n - padded, "calls_per_window": calls,
             "max_abs_hip_vs_torch_db": diff}
        for key, t in (("fixed_host", timed_host(lambda: features.mel_db_fixed(waves, length=LENGTH), args.repeats,
                                                 args.warmup, calls)),
                       ("fixed_dev", timed_host(lambda: features.mel_db_fixed(dwaves, length=LENGTH), args.repeats,
                                                args.warmup, calls)),
                       ("meldb_call", timed_events(lambda: meldb(TOP_DB), args.repeats, args.warmup, calls)),
                       ("meldb_noclip", timed_events(lambda: meldb(-1.0), args.repeats, args.warmup, calls)),
                       ("logmel_kernel", timed_events(logmel, args.repeats, args.warmup, calls)),
                       ("torch_dev", timed_events(lambda: torch_meldb(batch, window, melfb_t), args.repeats,
                                                  args.warmup, calls))):
            r[key + "_ms"] = {"median": round(t[0], 4), "min": round(t[1], 4), "max": round(t[2], 4)}
        r["clip_kernel_ms"] = round(r["meldb_call_ms"]["median"] - r["meldb_noclip_ms"]["median"], 4)
        r["torch_over_meldb_call"] = round(r["torch_dev_ms"]["median"] / r["meldb_call_ms"]["median"], 2)
        result["workloads"][name] = r
        del dwaves, y, out, got, ref, batch
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
