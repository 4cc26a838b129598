"""Numpy oracle of the diarization scoring (diarization.raster / count / assignment / der), written
from the rules alone: loops over segments and frames, no cleverness.

Grid: `step` samples per frame, a file of n samples has ceil(n / step) frames, frame i has its
centre at c_i = i * step + step // 2, and a segment [s, e) in samples covers frame i iff
s <= c_i < e.  Files are packed one after another with frame_off [F + 1]."""
import itertools

import numpy as np

HOP, WIN = 12, 24


def n_frames(n_samples, step):
    return -(-int(n_samples) // int(step))


def raster(seg_start, seg_end, seg_bits, seg_file, frame_off, step):
    """uint32 [frame_off[-1]]: the OR of seg_bits[k] over the rows that cover each frame; a row with
    a file index outside [0, F) or e <= s writes nothing; frames are the file's own [0, n_frames)."""
    F = len(frame_off) - 1
    mask = np.zeros(int(frame_off[-1]), dtype=np.uint32)
    for s, e, b, f in zip(seg_start, seg_end, seg_bits, seg_file):
        if not 0 <= f < F or e <= s:
            continue
        for i in range(int(frame_off[f + 1] - frame_off[f])):
            if s <= i * step + step // 2 < e:
                mask[frame_off[f] + i] |= np.uint32(b)
    return mask


def popc(v):
    return bin(int(v)).count("1")


def count(ref, hyp, noscore, frame_off, uem=None, skip_overlap=False):
    """uint64 [F, 4 + 1024]: total, miss, fa, both, C[i][j] over every file's scored frames."""
    F = len(frame_off) - 1
    out = np.zeros((F, 4 + 32 * 32), dtype=np.uint64)
    for f in range(F):
        for t in range(int(frame_off[f]), int(frame_off[f + 1])):
            nr, nh = popc(ref[t]), popc(hyp[t])
            if noscore[t] != 0 or (uem is not None and uem[t] == 0) or (skip_overlap and nr > 1):
                continue
            out[f, 0] += np.uint64(nr)
            out[f, 1] += np.uint64(max(0, nr - nh))
            out[f, 2] += np.uint64(max(0, nh - nr))
            out[f, 3] += np.uint64(min(nr, nh))
            for i in range(32):
                if int(ref[t]) >> i & 1:
                    for j in range(32):
                        if int(hyp[t]) >> j & 1:
                            out[f, 4 + 32 * i + j] += np.uint64(1)
    return out


def best_total(C):
    """max over one-to-one mappings of rows to columns of sum C[r][map(r)], by brute force."""
    C = np.asarray(C, dtype=np.int64)
    R, K = C.shape
    if R == 0 or K == 0:
        return 0
    if R > K:
        C, R, K = C.T, K, R
    return max(sum(int(C[r, p[r]]) for r in range(R)) for p in itertools.permutations(range(K), R))


def _table(segs, n, sr):
    names, rows = {}, []
    for t0, t1, spk in segs:
        names.setdefault(spk, len(names))
        rows.append((min(max(int(round(t0 * sr)), 0), n), min(max(int(round(t1 * sr)), 0), n), 1 << names[spk]))
    return rows, list(names)


def der(reference, hypothesis, n_samples, collar=0.25, skip_overlap=False, step=160, uem=None, sr=16000):
    """File by file: {"total", "miss", "fa", "conf": int64 [F], "file_der": float64 [F] (nan where
    total == 0), "der": the corpus figure}.  At most 5 speakers a side (the brute-force mapping)."""
    F = len(reference)
    res = {k: np.zeros(F, dtype=np.int64) for k in ("total", "miss", "fa", "conf")}
    res["file_der"] = np.full(F, np.nan)
    c = int(round(collar * sr))
    for f in range(F):
        n = int(n_samples[f])
        off = [0, n_frames(n, step)]
        ref_rows, rn = _table(reference[f], n, sr)
        hyp_rows, hn = _table(hypothesis[f], n, sr)

        def mask(rows):
            return raster([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [0] * len(rows), off, step)

        bounds = [r[0] for r in ref_rows] + [r[1] for r in ref_rows]
        ns_rows = [(min(max(t - c, 0), n), min(max(t + c, 0), n), 1) for t in bounds]
        um = None
        if uem is not None:
            regions = [(0.0, n / sr)] if uem[f] is None else uem[f]
            um = mask([(min(max(int(round(a * sr)), 0), n), min(max(int(round(b * sr)), 0), n), 1) for a, b in regions])
            if uem[f] is None:
                um[:] = 1
        out = count(mask(ref_rows), mask(hyp_rows), mask(ns_rows), off, um, skip_overlap)[0]
        total, miss, fa, both = (int(v) for v in out[:4])
        C = out[4:].astype(np.int64).reshape(32, 32)[:len(rn), :len(hn)]
        conf = both - best_total(C)
        res["total"][f], res["miss"][f], res["fa"][f], res["conf"][f] = total, miss, fa, conf
        if total:
            res["file_der"][f] = np.float64(miss + fa + conf) / np.float64(total)
    err, tot = int(res["miss"].sum() + res["fa"].sum() + res["conf"].sum()), int(res["total"].sum())
    res["der"] = float(np.float64(err) / np.float64(tot)) if tot else float("nan")
    return res


def aligned_spans_loop(ranges, hop_n, partitions):
    """The literal per-window loop of dvector.aligned_spans: rows (start, end, aligned index).
    `partitions`: dvector.partitions (the reference's loop, which this does not restate)."""
    kept = [(int(a), int(b)) for a, b in ranges if 1 + (int(b) - int(a)) // hop_n > WIN]
    wins = []  # (range index, start sample, end sample)
    for r, (a, b) in enumerate(kept):
        T = 1 + (b - a) // hop_n
        js = [j for j in range(0, T, HOP) if j + WIN < T]
        for j in js:
            wins.append((r, a + j * hop_n, b if j == js[-1] else a + (j + HOP) * hop_n))
    if not wins:
        return np.zeros((0, 3), dtype=np.int64)
    idx = [None] * len(wins)
    for p, (w0, w1) in enumerate(partitions(len(wins))):
        for w in range(w0, w1):
            idx[w] = p
    rows = []
    for w, (r, s, e) in enumerate(wins):
        if rows and wins[w - 1][0] == r and idx[w - 1] == idx[w]:
            rows[-1][1] = e
        else:
            rows.append([s, e, idx[w]])
    return np.asarray(rows, dtype=np.int64)
