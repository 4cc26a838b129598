#!/usr/bin/env python
"""Times the device-resident corpus (data_load.DeviceCorpus / ResidentBatches, sv_corpus_batch)
against the host loader it replaces, at N = 64 speakers x M = 10 utterances, 40 mels, 180 stored
frames, 200 synthetic speakers written to a temporary directory (page-cached), all in this one process:

  host_loader_ms      DataLoader(SpeakerDatasetTIMITPreprocessed, num_workers=0) + DevicePrefetcher,
                      no training: host clock per batch over whole epochs, a device synchronise at the end
  resident_batches_ms DataLoader(SpeakerDatasetResident) + ResidentBatches, likewise
  kernel              sv_corpus_batch / sv_corpus_batch_bf16 at B = 640, T = 160 (device events around
                      windows of --calls launches): microseconds, and GB/s over the bytes the launch
                      must move (the batch read once, x_tm and xT written once); beside them the
                      launches they replace at the same shape (sv_frames_to_time_major + sv_transpose;
                      sv_frames_to_bf16) on the materialised batch
  train_loop_ms       the body of train() on bf16 (prefetcher -> GE2ETrainer.step, the default
                      40 -> 768 x 3 -> 256 net) per iteration, for both datasets
  step_T160 / T161    GE2ETrainer.step(CorpusBatch) on bf16 at T = 160 and at the off-grid T = 161
                      (T * B % 256 != 0: the GEMMs' fallback tiles), device events per step
  step_ab             the speed condition: step(CorpusBatch) against step(x) with x already on the
                      device, c3 shape, interleaved x / batch / x, --steps steps each, device events per
                      step; the two x series give the run-to-run spread of the tensor step itself
Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_speaker_verification_amd import data_load  # noqa: E402
from pytorch_speaker_verification_amd._lib import call, ptr, stream_of  # noqa: E402
from pytorch_speaker_verification_amd.hparam import hparam as hp  # noqa: E402
from pytorch_speaker_verification_amd.speech_embedder_net import GE2ELoss, SpeechEmbedder  # noqa: E402
from pytorch_speaker_verification_amd.trainer import GE2ETrainer  # noqa: E402
from _timing import timed_events  # noqa: E402

N, M, NMELS, FRAMES, SPEAKERS = 64, 10, 40, 180, 200


def write_speakers(root, rng):
    for k in range(SPEAKERS):
        np.save(os.path.join(root, f"speaker{k}.npy"),
                rng.standard_normal((int(rng.integers(8, 14)), NMELS, FRAMES)).astype(np.float32))


def per_batch_ms(make_batches, epochs, use=None):
    """Host clock per batch over `epochs` passes of make_batches() (after one warm-up pass), a device
    synchronise at the end; use(batch): the work done with every batch (None: none)."""
    n = 0
    for e in range(epochs + 1):
        if e == 1:
            torch.cuda.synchronize()
            t0, n = time.perf_counter(), 0
        for batch in make_batches():
            if use is not None:
                use(batch)
            n += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def step_events(fns, steps, warmup):
    """Per-step device-event milliseconds of each fn, the fns called in turn `steps` times."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
          for _ in fns]
    for i in range(steps):
        for k, fn in enumerate(fns):
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    return [[a.elapsed_time(b) for a, b in row] for row in ev]


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5, help="timed passes over the 3 batches of the loaders")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--calls", type=int, default=20, help="kernel launches per timed window (at least 20)")
    ap.add_argument("--steps", type=int, default=30, help="steps per series of the interleaved step timings")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("corpus_bench.py needs a GPU: there is no CPU timing path")
    dev = torch.device("cuda", 0)
    B, T = N * M, data_load.TRAIN_FRAMES
    result = {"bench": "corpus", "device": torch.cuda.get_device_name(0), "N": N, "M": M, "nmels": NMELS,
              "frames": FRAMES, "speakers": SPEAKERS}
    with tempfile.TemporaryDirectory() as root:
        write_speakers(root, np.random.default_rng(0))
        hp.training, hp.data.train_path, hp.train.N, hp.train.M = True, root, N, M
        corpus = data_load.DeviceCorpus(root, device=dev)
        result["corpus_mb"] = round(corpus.data.numel() * 4 / 2 ** 20, 1)
        host_ds = data_load.SpeakerDatasetTIMITPreprocessed()
        res_ds = data_load.SpeakerDatasetResident(corpus)
        host_loader = DataLoader(host_ds, batch_size=N, shuffle=True, num_workers=0, drop_last=True, pin_memory=True)
        res_loader = DataLoader(res_ds, batch_size=N, shuffle=True, num_workers=0, drop_last=True)
        resident = data_load.ResidentBatches(res_loader, corpus)
        host_batches = lambda: data_load.DevicePrefetcher(host_loader, dev)  # noqa: E731
        result["host_loader_ms"] = round(per_batch_ms(host_batches, args.epochs), 3)
        result["resident_batches_ms"] = round(per_batch_ms(lambda: resident, args.epochs), 3)

        # ---- the kernel beside the launches it replaces
        batch = next(iter(resident))
        torch.cuda.synchronize()
        xb = batch.frames()
        s = stream_of(xb)
        kern = {}
        for name, dtype, esz in (("f32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
            Bp = B
            x_tm = torch.empty((T, B, NMELS), dtype=dtype, device=dev)
            xT = torch.empty((NMELS, T * Bp), dtype=dtype, device=dev)
            entry = "sv_corpus_batch" if name == "f32" else "sv_corpus_batch_bf16"

            def new():
                call(entry, ptr(corpus.data), corpus.n_utt, NMELS, FRAMES, ptr(batch.utt), ptr(batch.start), B, T,
                     ptr(x_tm), ptr(xT), Bp, s)

            if name == "f32":
                def old():
                    call("sv_frames_to_time_major", ptr(xb), ptr(x_tm), B, T, NMELS, s)
                    call("sv_transpose", ptr(x_tm), NMELS, T * B, NMELS, ptr(xT), T * B, s)
            else:
                def old():
                    call("sv_frames_to_bf16", ptr(xb), B, T, NMELS, ptr(x_tm), ptr(xT), Bp, s)

            moved = B * T * NMELS * (4 + 2 * esz)  # bytes: the batch read once, both outputs written once
            t_new = timed_events(new, args.repeats, 5, max(20, args.calls))
            t_old = timed_events(old, args.repeats, 5, max(20, args.calls))
            kern[name] = {"corpus_batch_us": round(t_new[0] * 1e3, 2), "corpus_batch_gbs": round(moved / t_new[0] / 1e6, 1),
                          "replaced_launches_us": round(t_old[0] * 1e3, 2), "bytes": moved}
        result["kernel"] = kern

        # ---- the train() loop's body on bf16, both datasets; then the single-step series
        torch.manual_seed(0)
        net = SpeechEmbedder().to(dev)
        net.precision = "bf16"
        tr = GE2ETrainer(net, GE2ELoss(dev), lr=0.01)
        step = lambda x: tr.step(x, N, M)  # noqa: E731
        result["train_loop_ms"] = {
            "host_loader": round(per_batch_ms(host_batches, args.epochs,
                                              lambda b: step(b.reshape(B, b.size(2), b.size(3)))), 3),
            "resident": round(per_batch_ms(lambda: resident, args.epochs, step), 3)}
        b161 = data_load.CorpusBatch(corpus, batch.utt, batch.start, 161)
        x_dev = xb.clone()
        t160, t161 = step_events([lambda: step(batch), lambda: step(b161)], args.steps, 3)
        result["step_T160_ms"], result["step_T161_ms"] = stats(t160), stats(t161)
        xa, cb, xa2 = step_events([lambda: step(x_dev), lambda: step(batch), lambda: step(x_dev)], args.steps, 3)
        tr.check()
        result["step_ab"] = {"tensor_ms": stats(xa), "corpus_batch_ms": stats(cb), "tensor_again_ms": stats(xa2),
                             "tensor_spread_ms": round(abs(statistics.median(xa) - statistics.median(xa2)), 4),
                             "corpus_minus_tensor_ms": round(statistics.median(cb) - statistics.median(xa + xa2), 4),
                             "steps": args.steps}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
