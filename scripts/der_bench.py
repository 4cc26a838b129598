#!/usr/bin/env python
"""Times the two kernels of the diarization scoring (diarization.py, csrc/sv_der.hip) against the
torch form a user can write today on the same GPU, on synthetic recordings of 4 speakers with
turns of 1 .. 10 s at the 10 ms frame grid (step 160 at 16 kHz):

  rec10h     one 10-hour recording (3.6 M frames)
  files1024  1 024 files of 5 .. 10 minutes (about 46 M frames in one batch)

The reference is one speaker at a time with a tenth of the turns followed by a pause; the hypothesis
is the reference with every boundary moved by up to 0.2 s and the names permuted, so single-speaker
frames on both sides -- the input the torch form can count.

  raster   the reference, hypothesis and collar masks of the batch: ours, one torch.zeros and one
           sv_seg_raster launch per table on device tables that split_rows cut (the host work of
           building the tables is outside the window on both sides); torch, masks by slice assignment
           per segment, mask[lo:hi] |= bit, with lo and hi computed on the host beforehand
  count    ours, one sv_der_count launch; torch, per file total / miss / false alarm by bincount over
           the file index of the scored frames and the 32 x 32 pair counts by
           torch.bincount((file * 32 + ref_bit) * 32 + hyp_bit), bit indices from log2 of the masks
  der      diarization.der() as a user calls it, host work included (host clock; no torch leg)

Device events around windows of calls (_timing.timed_events); the two legs of every stage alternate
(ours, torch, ours, torch) and each reports the smaller of its two medians.  Both forms are checked
equal on the timed input before they are timed.  Prints one JSON line and writes it to --out.
Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_speaker_verification_amd import diarization as D  # noqa: E402
from pytorch_speaker_verification_amd._lib import call, ptr  # noqa: E402
from _timing import timed_events, timed_host  # noqa: E402

SR, STEP, SPEAKERS, COLLAR = 16000, 160, 4, 0.25


def recording(n_samples, rng):
    """(reference, hypothesis) of one file as (start_s, end_s, speaker) lists."""
    ref, t = [], 0
    while t < n_samples:
        m = int(rng.integers(SR, 10 * SR + 1))
        ref.append((t, min(t + m, n_samples), int(rng.integers(0, SPEAKERS))))
        t += m + (int(rng.integers(SR // 2, 3 * SR)) if rng.random() < 0.1 else 0)
    perm = rng.permutation(SPEAKERS)
    hyp = []
    for s, e, v in ref:
        s2 = min(max(s + int(rng.integers(-SR // 5, SR // 5 + 1)), hyp[-1][1] if hyp else 0), n_samples)
        e2 = min(max(e + int(rng.integers(-SR // 5, SR // 5 + 1)), s2), n_samples)
        hyp.append((s2, e2, int(perm[v])))
    as_s = lambda rows: [(s / SR, e / SR, v) for s, e, v in rows if e > s]  # noqa: E731
    return as_s(ref), as_s(hyp)


def tables(reference, hypothesis, n_samples):
    """The three segment tables of the batch in samples, as der() builds them: lists of (start, end, bits, file)."""
    c = int(round(COLLAR * SR))
    out = [[[], [], [], []] for _ in range(3)]
    for f, (ref, hyp, n) in enumerate(zip(reference, hypothesis, n_samples)):
        for which, segs in ((0, ref), (1, hyp)):
            for t0, t1, v in segs:
                out[which][0].append(int(round(t0 * SR)))
                out[which][1].append(int(round(t1 * SR)))
                out[which][2].append(1 << v)
                out[which][3].append(f)
        for t0, t1, _ in ref:
            for t in (int(round(t0 * SR)), int(round(t1 * SR))):
                out[2][0].append(max(t - c, 0))
                out[2][1].append(min(t + c, n))
                out[2][2].append(1)
                out[2][3].append(f)
    return [[np.asarray(col, dtype=np.int64) for col in tab] for tab in out]


def legs(ours, theirs, repeats, calls):
    a, b = [], []
    for _ in range(2):
        a.append(timed_events(ours, repeats, 1, calls)[0])
        b.append(timed_events(theirs, max(2, repeats // 2), 1, 1)[0])
    a, b = min(a), min(b)
    return {"ours_ms": round(a, 4), "torch_ms": round(b, 4), "torch_over_ours": round(b / a, 2)}


def bench_case(n_samples, repeats, dev, seed):
    rng = np.random.default_rng(seed)
    pairs = [recording(n, rng) for n in n_samples]
    reference, hypothesis = [p[0] for p in pairs], [p[1] for p in pairs]
    frames = [-(-n // STEP) for n in n_samples]
    frame_off = np.concatenate([[0], np.cumsum(frames)])
    F, n_total, stream = len(frames), int(frame_off[-1]), torch.cuda.current_stream(dev).cuda_stream
    d_off = torch.from_numpy(frame_off.astype(np.int32)).to(dev)
    tabs = tables(reference, hypothesis, n_samples)

    # ---- raster
    ours_tabs = []
    for tab in tabs:
        s, e, b, f = D.split_rows(*tab, STEP)
        ours_tabs.append([torch.from_numpy(v.astype(np.int32)).to(dev) for v in (s, e, b, f)])

    def ours_raster():
        masks = []
        for s, e, b, f in ours_tabs:
            m = torch.zeros(n_total, dtype=torch.int32, device=dev)
            call("sv_seg_raster", ptr(s), ptr(e), ptr(b), ptr(f), int(s.numel()), ptr(d_off), F, STEP, n_total, ptr(m), stream)
            masks.append(m)
        return masks

    h = STEP // 2
    torch_tabs = []
    for s, e, b, f in tabs:  # first and one-past-last covered frame of every segment, on the host
        lo = np.where(s <= h, 0, (s - h + STEP - 1) // STEP)
        hi = np.minimum(np.where(e <= h, 0, (e - h + STEP - 1) // STEP), np.asarray(frames)[f])
        torch_tabs.append(list(zip((frame_off[f] + lo).tolist(), (frame_off[f] + hi).tolist(), b.tolist())))

    def torch_raster():
        masks = []
        for rows in torch_tabs:
            m = torch.zeros(n_total, dtype=torch.int32, device=dev)
            for lo, hi, b in rows:
                if hi > lo:
                    m[lo:hi] |= b
            masks.append(m)
        return masks

    ref, hyp, ns = ours_raster()
    equal = all(bool(torch.equal(a, b)) for a, b in zip((ref, hyp, ns), torch_raster()))

    # ---- count
    out = torch.empty((F, D.DER_OUT), dtype=torch.int64, device=dev)
    fmax = int(max(frames))

    def ours_count():
        call("sv_der_count", ptr(ref), ptr(hyp), ptr(ns), None, ptr(d_off), F, fmax, n_total, 0, ptr(out), stream)
        return out

    fid = torch.repeat_interleave(torch.arange(F, device=dev), torch.from_numpy(np.asarray(frames)).to(dev))

    def torch_count():
        scored = ns == 0
        r, hy = (ref != 0) & scored, (hyp != 0) & scored
        total = torch.bincount(fid[r], minlength=F)
        miss = torch.bincount(fid[r & ~hy], minlength=F)
        fa = torch.bincount(fid[hy & ~r], minlength=F)
        both = r & hy
        rb = torch.log2(ref[both].float()).long()
        hb = torch.log2(hyp[both].float()).long()
        C = torch.bincount((fid[both] * 32 + rb) * 32 + hb, minlength=F * 1024).view(F, 1024)
        return torch.cat([total[:, None], miss[:, None], fa[:, None], C.sum(dim=1, keepdim=True), C], dim=1)

    equal_count = bool(torch.equal(ours_count(), torch_count()))
    res = {"files": F, "frames": n_total, "segments": [int(t[0].size) for t in tabs],
           "rows_after_split": [int(t[0].numel()) for t in ours_tabs],
           "masks_equal_torch": equal, "counts_equal_torch": equal_count}
    res["raster"] = legs(ours_raster, torch_raster, repeats, 10)
    res["count"] = legs(ours_count, torch_count, repeats, 20)
    host = timed_host(lambda: D.der(reference, hypothesis, n_samples, collar=COLLAR, device=dev), max(2, repeats // 2), 1)
    r = D.der(reference, hypothesis, n_samples, collar=COLLAR, device=dev)
    res["der_call_host_ms"] = round(host[0], 2)
    res["der"] = round(r["der"], 6)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=["rec10h", "files1024"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "der_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("der_bench.py needs a GPU: there is no CPU timing path")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    shapes = {"rec10h": [10 * 3600 * SR], "files1024": [int(v) for v in rng.integers(300 * SR, 600 * SR + 1, 1024)],
              "tiny": [int(v) for v in rng.integers(20 * SR, 40 * SR + 1, 8)]}
    result = {"bench": "der", "device": torch.cuda.get_device_name(0), "step": STEP, "speakers": SPEAKERS,
              "collar_s": COLLAR, "cases": {}}
    with torch.no_grad():
        for i, name in enumerate(args.cases):
            result["cases"][name] = bench_case(shapes[name], args.repeats, dev, 100 + i)
            torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
