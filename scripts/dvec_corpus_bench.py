#!/usr/bin/env python
"""Times the corpus d-vector export (dvector.embed_files: one log-mel launch, one embedding pass and
one averaging launch per batch of files) against the per-file loops it replaces.

Workload (seeded): --files synthetic files of 3 s at 16 kHz, each with two voiced ranges that cover
about 70 % of it (15 windows of 24 frames per file on average), the full-size net (40 -> 768 x 3 ->
256, recipe weights), in bf16 and fp32.

Per precision, the median over --repeats passes over the whole corpus after --warmup passes, all in
this one process, host clock around the pass with a device synchronisation at its end (every path
ends with its d-vectors on the host):
  corpus        dvector.embed_files(net, files, precision)
  per_file      the loop of dvector.embed_segments(net, [wave[a:b] ...], precision) over the files
  per_file_graph  per file features.logmel -> windows_from_logmel -> GraphedEmbedder -> align_embeddings
and, from device events around the three steps of one corpus pass (bf16: the in-place path,
sv_dvector_embed_bf16_frames; fp32: the chunked gather + embed_windows), the shares of
features.logmel_ranges (the host's packing, the upload and the sv_logmel_ranges launch), the
embedding and sv_dvec_align, and sv_logmel_ranges alone on device-resident audio.  Also the largest
difference between the corpus result and the per-file loop's.  Prints one JSON line.  No assertion on time.
Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from pytorch_speaker_verification_amd import dvector, features, ops  # noqa: E402
from pytorch_speaker_verification_amd.hparam import hparam as hp  # noqa: E402
from _timing import timed_events, timed_host  # noqa: E402

SR = 16000


def corpus(n_files, rng):
    """Files of 3 s: noise-modulated tones, two voiced ranges covering ~70 % of each."""
    t = np.arange(3 * SR) / SR
    files = []
    for _ in range(n_files):
        f0 = rng.uniform(100.0, 400.0)
        y = (0.4 * np.sin(2 * np.pi * f0 * t) + 0.2 * np.sin(2 * np.pi * 7.3 * f0 * t) +
             0.02 * rng.standard_normal(t.size)).astype(np.float32)
        a0 = int(rng.integers(0, 4000))
        b0 = a0 + int(rng.integers(18000, 22000))
        a1 = b0 + int(rng.integers(1600, 4000))
        b1 = min(3 * SR, a1 + int(rng.integers(12000, 16000)))
        files.append((y, [(a0, b0), (a1, b1)]))
    return files


def make_net():
    import recipe
    from pytorch_speaker_verification_amd.speech_embedder_net import SpeechEmbedder
    dims = (hp.data.nmels, hp.model.hidden, hp.model.num_layer, hp.model.proj)
    sd = recipe.make_weights(19, *dims, scale=2.0)
    net = SpeechEmbedder()
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(torch.as_tensor(sd[k]))
    return net.cuda()


def timed_ms(fn, repeats, warmup):
    t = timed_host(fn, repeats, warmup)
    return {"median": round(t[0], 2), "min": round(t[1], 2), "max": round(t[2], 2)}


def stages(net, files, precision):
    """Device-event times (ms) of the three steps of one corpus pass, composed from the same pieces
    embed_files uses."""
    layers, wp, bp = net.LSTM_stack.layer_params(), net.projection.weight, net.projection.bias
    ranges = [(w, a, b) for w, (_, r) in enumerate(files) for a, b in r]
    seg_file = [w for w, (_, r) in enumerate(files) for _ in r]

    def tables(frame_off):
        return list(dvector.batch_tables(frame_off, seg_file, len(files))[:2])

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    out, _, (win_start, part_off) = features.logmel_ranges([w for w, _ in files], ranges, tables=tables)
    ev[1].record()
    S = int(win_start.shape[0])
    if precision == "bf16":
        emb = torch.cat([ops.embedder_forward_dvec_bf16_frames(out, win_start[i:i + dvector.DVEC_CHUNK], layers, wp, bp)
                         for i in range(0, S, dvector.DVEC_CHUNK)])
    else:
        steps = torch.arange(dvector.WIN, device=out.device)
        emb = torch.cat([dvector.embed_windows(net, out[win_start[i:i + 16384].long()[:, None] + steps[None, :]])
                         for i in range(0, S, 16384)])
    ev[2].record()
    aligned = ops.dvec_align(emb, part_off)
    ev[3].record()
    aligned.cpu()
    torch.cuda.synchronize()
    return {"windows": S, "frames": int(out.shape[0]), "aligned": int(aligned.shape[0]),
            "pack_upload_logmel_ranges_ms": round(ev[0].elapsed_time(ev[1]), 3),
            "embed_ms": round(ev[1].elapsed_time(ev[2]), 3), "align_ms": round(ev[2].elapsed_time(ev[3]), 3)}


def logmel_ranges_kernel(files, repeats):
    """sv_logmel_ranges alone on device-resident audio and tables (device events, median ms)."""
    sr, nfft, win, hop_n, nmels = features._config(None, None, None, None, None)
    ranges = [(w, a, b) for w, (_, r) in enumerate(files) for a, b in r]
    seg_start, seg_len, frame_off = features.range_tables([len(w) for w, _ in files], ranges, nfft, hop_n)
    y = torch.from_numpy(np.concatenate([w for w, _ in files])).cuda()
    t = [torch.from_numpy(v).cuda() for v in (seg_start, seg_len, frame_off)]
    wbasis, melfb = features.stft_tables(sr, nfft, win, nmels, y.device)
    out = torch.empty((int(frame_off[-1]), nmels), dtype=torch.float32, device=y.device)

    def kernel():
        features.logmel_ranges_into(y, t[0], t[1], t[2], len(ranges), out.shape[0], nfft, win, hop_n, nmels, wbasis,
                                    melfb, out)

    return round(timed_events(kernel, repeats, 2)[0], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--precisions", default="bf16,f32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dvec_corpus_bench.py needs a GPU: there is no CPU timing path")
    files = corpus(args.files, np.random.default_rng(0))
    segs = [[w[a:b] for a, b in r] for w, r in files]
    voiced = sum(b - a for _, r in files for a, b in r) / sum(len(w) for w, _ in files)
    net = make_net()
    result = {"bench": "dvec_corpus", "device": torch.cuda.get_device_name(0), "files": args.files,
              "voiced_fraction": round(voiced, 3), "repeats": args.repeats,
              "logmel_ranges_kernel_ms": logmel_ranges_kernel(files, max(args.repeats, 5)), "precisions": {}}
    for precision in args.precisions.split(","):
        ge = dvector.GraphedEmbedder(net, precision=precision)

        def per_file():
            return [dvector.embed_segments(net, s, precision=precision) for s in segs]

        def per_file_graph():
            res = []
            for s in segs:
                out, frame_off = features.logmel(s)
                res.append(dvector.align_embeddings(ge(dvector.windows_from_logmel(out, frame_off)).cpu().numpy()))
            return res

        def whole():
            return dvector.embed_files(net, files, precision=precision)

        got, ref = whole(), per_file()
        r = {"max_abs_corpus_vs_per_file": float(max(np.abs(g - p).max() for g, p in zip(got, ref)))}
        r["corpus_ms"] = timed_ms(whole, args.repeats, args.warmup)
        r["per_file_ms"] = timed_ms(per_file, args.repeats, args.warmup)
        r["per_file_graph_ms"] = timed_ms(per_file_graph, args.repeats, args.warmup)
        stages(net, files, precision)  # warm-up
        r["stages"] = stages(net, files, precision)
        r["per_file_over_corpus"] = round(r["per_file_ms"]["median"] / r["corpus_ms"]["median"], 2)
        r["per_file_graph_over_corpus"] = round(r["per_file_graph_ms"]["median"] / r["corpus_ms"]["median"], 2)
        result["precisions"][precision] = r
    print(json.dumps(result))


if __name__ == "__main__":
    main()
