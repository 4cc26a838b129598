"""Segment-level d-vectors for diarisation (reference dvector_create.py:38-73).

The reference turns each VAD-concatenated segment's log-mel spectrogram [nmels, T] into
24-frame windows at a 12-frame hop (0.24 s / 0.12 s, :48-52), embeds all windows with the
SpeechEmbedder (:100) and averages consecutive window embeddings into ~0.4 s segments
(align_embeddings, :55-73).  embed_segments starts from a file's waveform segments
(features.logmel is the STFT / log-mel front end), the rest of the module from the log-mel frames.
The embedding is the short-sequence, large-batch forward of the same HIP LSTM kernels (T = 24).

The corpus export (dvector_create.py:84-122, the module-level loop that writes
train_sequence.npy / train_cluster_id.npy / test_*.npy for uis-rnn) is export_sequences over
embed_files: per batch of files one packed upload, one sv_logmel_ranges launch over the voiced
ranges of all files, one window table, the embedding (bf16: sv_dvector_embed_bf16_frames, which
reads its windows in place from the log-mel rows), one sv_dvec_align launch and one copy out.  Its
input is what VAD_segments.VAD_chunk and concat_segs compute after the per-frame VAD decision:
vad_frame_count / vad_times / voiced_ranges are that bookkeeping (frame_generator, vad_collector,
the 0.4 s chunking, concat_segs) on per-frame is_speech flags from any VAD.  Only the per-frame
decision itself (webrtcvad) and audio decoding stay outside.
"""
from __future__ import annotations

import collections
import os

import numpy as np
import torch

from .hparam import hparam as hp
from .ops import (check_persistent_status, dvec_align, embedder_forward, embedder_forward_bf16,
                  embedder_forward_dvec_bf16, embedder_forward_dvec_bf16_frames)

WIN, HOP = 24, 12  # frames: int(.24/.01), int(.12/.01)
# bf16: from this many windows on, one pass of per-timestep GEMM launches with the cell in their
# epilogue (sv_dvector_embed_bf16) instead of co-resident persistent batches (bf16_batch)
DVEC_MIN = 3072
DVEC_CHUNK = 16384


def window_frames(logmel, win=WIN, hop=HOP):
    """[nmels, T] -> [S, win, nmels]: windows starting every `hop` frames while j + win < T
    (the strict '<' of dvector_create.py:50 drops a window that would end exactly at T)."""
    logmel = np.asarray(logmel)
    starts = [j for j in range(0, logmel.shape[1], hop) if j + win < logmel.shape[1]]
    if not starts:
        return np.zeros((0, win, logmel.shape[0]), dtype=np.float32)
    return np.stack([logmel[:, j:j + win].T for j in starts]).astype(np.float32)


def window_index(frame_off, win=WIN, hop=HOP):
    """Row indices [S, win] into time-major log-mel frames [n_frames, nmels] (features.logmel) of
    every segment's windows (window_starts' rows, dvector_create.py:49), segments in order."""
    starts, _ = window_starts(frame_off, win, hop)
    return starts.astype(np.int64)[:, None] + np.arange(win, dtype=np.int64)[None, :]


def windows_from_logmel(out, frame_off, win=WIN, hop=HOP):
    """[n_frames, nmels] time-major log-mel frames of a ragged batch (features.logmel) -> the
    windows [S, win, nmels] of all its segments, on out's device: one gather with a host-built
    index table (window_index)."""
    idx = window_index(frame_off, win, hop)
    if idx.shape[0] == 0:
        return out.new_zeros((0, win, out.shape[1]))
    return out[torch.from_numpy(idx).to(out.device)]


def dvec_ok(F, H):
    """Dimensions sv_dvector_embed_bf16 takes (include/sv_ge2e.h): the x part one padded k-tile,
    whole 256-column tiles of the unit-interleaved 4H gate columns."""
    return 0 < F <= 64 and H % 64 == 0 and (4 * H) % 256 == 0


def bf16_batch(H, limit=16384):
    """Windows per call of the bf16 forward: the largest multiple of 32 (<= limit) whose whole
    recurrence grid is co-resident, so each call runs the persistent W-stationary kernels (c3's)
    instead of one launch per timestep (a 16384-window call does not fit: 0.14 of the bf16 peak)."""
    from ._lib import lib
    b = max(32, min(limit, 4096) // 32 * 32)
    while b > 32 and not lib().sv_persist_fwd_ok(b, H):
        b -= 32
    return b if lib().sv_persist_fwd_ok(b, H) else limit


def _check_path(precision, path):
    if precision not in ("f32", "bf16"):
        raise ValueError(f"precision must be 'f32' or 'bf16', got {precision!r}")
    if path not in (None, "persist", "dvec") or (path is not None and precision != "bf16"):
        raise ValueError(f"path must be None, 'persist' or 'dvec' (bf16 only), got {path!r}")


def _takes_dvec(precision, path, n_windows, F, H):
    """Whether a bf16 embedding of n_windows windows takes the per-timestep GEMM path: asked for by
    name, or chosen from DVEC_MIN windows on where the dimensions allow it."""
    return precision == "bf16" and dvec_ok(F, H) and (path == "dvec" or (path is None and n_windows >= DVEC_MIN))


@torch.no_grad()
def embed_windows(net, windows, batch=None, precision="f32", path=None, schedule="auto"):
    """Embeddings [S, proj] of windows [S, win, nmels] with the module's weights (GPU), `batch`
    windows per call (None: 16384 in fp32; bf16: bf16_batch(), the largest co-resident
    persistent batch).  precision "bf16": the c3 mixed-precision forward (bf16 GEMM operands,
    fp32 accumulation and state), no activations saved.  Raises PersistentRecurrenceError if a
    persistent recurrence of the call timed out (either precision).  path (bf16 only): "persist"
    (batches of the training forward's persistent recurrences), "dvec" (sv_dvector_embed_bf16, DVEC_CHUNK windows
    per call) or None: "dvec" from DVEC_MIN windows on when no batch is given.  schedule: the
    recurrence schedule of the stack ('auto', 'per_step', 'persist', ...; ops.embedder_forward)."""
    _check_path(precision, path)
    dev = next(net.parameters()).device
    layers = net.LSTM_stack.layer_params()
    x = torch.as_tensor(windows, dtype=torch.float32)
    F, H = x.shape[-1], layers[0][1].shape[1]
    if path == "dvec" and not dvec_ok(F, H):
        raise ValueError(f"the per-timestep GEMM path needs F <= 64, H % 64 == 0 and 4H % 256 == 0 (F={F}, H={H})")
    # (a caller's batch size is a request for the batched forward unless it names the path)
    if _takes_dvec(precision, path, x.shape[0], F, H) and (path == "dvec" or batch is None):
        out = [embedder_forward_dvec_bf16(x[i:i + (batch or DVEC_CHUNK)].to(dev).contiguous(), layers,
                                          net.projection.weight, net.projection.bias)
               for i in range(0, x.shape[0], batch or DVEC_CHUNK)]
        return torch.cat(out) if out else torch.zeros((0, net.projection.weight.shape[0]), device=dev)
    if batch is None:
        batch = bf16_batch(layers[0][1].shape[1]) if precision == "bf16" else 16384
    out = []
    for i in range(0, x.shape[0], batch):
        xb = x[i:i + batch].to(dev).contiguous()
        fwd = embedder_forward_bf16 if precision == "bf16" else embedder_forward
        emb, _ = fwd(xb, layers, net.projection.weight, net.projection.bias, save=False, schedule=schedule)
        out.append(emb)
    # a persistent recurrence that timed out (its grid not co-resident) must not return silently
    # wrong embeddings: wait for this call's status words and raise (both precisions: the fp32
    # forward takes its persistent recurrences too where a batch fills the device)
    check_persistent_status(wait=True)
    return torch.cat(out) if out else torch.zeros((0, net.projection.weight.shape[0]), device=dev)


class GraphedEmbedder:
    """Per-file d-vector calls (dvector_create.py:96-101: one file's windows per
    ``embedder_net(windows)`` call, tens to hundreds of windows) replayed from HIP graphs.  Such a
    call is bound by its ~20 kernel launches and their host work (~0.3 ms), not by the kernels;
    here the whole forward -- frame transpose, casts, input projections, the recurrences, the
    projection and norm -- is captured once per window-count bucket (S rounded up to `bucket`;
    padding rows are zeros, rows are independent, and only the first S are returned) and each
    call is one copy in, one graph launch, one copy out.  Same kernels and numerics as
    embed_windows(..., batch=S); the weights are read through their pointers at every replay
    (in-place updates are seen; a module whose parameters were re-allocated is re-captured).
    precision: "f32" or "bf16"; schedule as embed_windows.  Raises PersistentRecurrenceError like
    embed_windows."""

    def __init__(self, net, precision="bf16", bucket=32, max_windows=640, schedule="auto"):
        if precision not in ("f32", "bf16"):
            raise ValueError(f"precision must be 'f32' or 'bf16', got {precision!r}")
        self.net, self.precision, self.bucket, self.max_windows = net, precision, bucket, max_windows
        self.schedule = schedule
        self._graphs = {}

    def _key(self, S, T, F):
        ptrs = tuple(p.data_ptr() for p in self.net.parameters())
        return (-(-S // self.bucket) * self.bucket, T, F, ptrs)

    def _capture(self, Sp, T, F, dev):
        from ._lib import PersistStatus
        layers = self.net.LSTM_stack.layer_params()
        wp, bp = self.net.projection.weight, self.net.projection.bias
        status = PersistStatus(dev)  # caller-owned: nothing polled or allocated during the capture
        x = torch.zeros((Sp, T, F), dtype=torch.float32, device=dev)

        def fwd():
            if self.precision == "bf16":
                return embedder_forward_bf16(x, layers, wp, bp, save=False, status=status, schedule=self.schedule)[0]
            return embedder_forward(x, layers, wp, bp, save=False, status=status, schedule=self.schedule)[0]

        side = torch.cuda.Stream(dev)  # warm-up off the capture (allocator, lazy init)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            fwd()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            emb = fwd()
        return g, x, emb, status

    @torch.no_grad()
    def __call__(self, windows):
        dev = next(self.net.parameters()).device
        x = torch.as_tensor(windows, dtype=torch.float32)
        S, T, F = x.shape
        if S == 0:
            return torch.zeros((0, self.net.projection.weight.shape[0]), device=dev)
        if S > self.max_windows:  # a long file: the batched path
            return embed_windows(self.net, x, precision=self.precision, schedule=self.schedule)
        key = self._key(S, T, F)
        if key not in self._graphs:
            self._graphs = {k: v for k, v in self._graphs.items() if k[3] == key[3]}  # drop stale weights
            self._graphs[key] = self._capture(key[0], T, F, dev)
        g, xs, emb, status = self._graphs[key]
        xs[:S].copy_(x.to(dev, non_blocking=True))
        if S < xs.shape[0]:
            xs[S:].zero_()
        g.replay()
        out = emb[:S].clone()
        status.arm()
        status.poll(wait=True)
        return out


def partitions(n_windows, win_s=0.24, hop_s=0.12, seg_s=0.401):
    """[start, end) window ranges averaged into one segment (dvector_create.py:56-69): a window i
    joins segment j while it ends (i*hop + win) before j*seg; the loop's else appends the last."""
    parts, start, end, j = [], 0, 0, 1
    for i in range(n_windows):
        if i * hop_s + win_s < j * seg_s:
            end += 1
        else:
            parts.append((start, end))
            start, end, j = end, end + 1, j + 1
    parts.append((start, end))
    return parts


def align_embeddings(embeddings):
    """Average window embeddings over partitions() -> [n_segments, D] float64 (:55-73)."""
    e = np.asarray(embeddings)
    parts = partitions(len(e))
    out = np.zeros((len(parts), e.shape[1]))
    for i, (a, b) in enumerate(parts):
        out[i] = np.average(e[a:b], axis=0)
    return out


def embed_segments(net, segs, precision="f32", **kw):
    """Aligned d-vectors [n_aligned, proj] float64 of one file's concatenated VAD segments (a list
    of 1-D waveforms at hp.data.sr): dvector_create.py:97-101 -- get_STFTs, embedder_net(windows),
    align_embeddings -- as features.logmel -> windows_from_logmel -> embed_windows on the device
    tensor (no host round trip) -> align_embeddings.  No window at all (every segment too short for
    one) gives an empty [0, proj] array.  **kw goes to embed_windows."""
    from .features import logmel
    out, frame_off = logmel(segs)
    windows = windows_from_logmel(out, frame_off)
    proj = net.projection.weight.shape[0]
    if windows.shape[0] == 0:
        return np.zeros((0, proj))
    emb = embed_windows(net, windows, precision=precision, **kw)
    return align_embeddings(emb.cpu().numpy())


# ---- the reference's VAD bookkeeping on per-frame flags (VAD_segments.py, dvector_create.concat_segs) ----
def _sr(sr):
    return hp.data.sr if sr is None else sr


def vad_frame_count(n_samples, sr=None, frame_ms=20):
    """How many frames VAD_segments.frame_generator yields for 16-bit PCM of n_samples samples: with
    n = int(sr * (frame_ms / 1000.0) * 2) bytes per frame, frames run while offset + n < 2 * n_samples
    (strict: a frame that would end exactly at the last byte is not yielded)."""
    n = int(_sr(sr) * (frame_ms / 1000.0) * 2)
    return max(0, (2 * int(n_samples) - 1) // n)


def vad_times(is_speech, sr=None, frame_ms=20, padding_ms=200):
    """VAD_chunk's speech_times from per-frame VAD decisions (one boolean per frame of
    frame_generator, in order; any VAD may have made them): vad_collector's padded sliding window
    (trigger when more than 0.9 maxlen of the ring's frames are voiced, detrigger when more than
    0.9 maxlen are unvoiced, the leftover voiced span at the end of input) and then the chunking
    of every span into 0.4 s pieces.  The reference's float arithmetic is kept literally -- frame
    timestamps accumulate by repeated `+= duration`, spans and chunk ends are np.round(., 2), the
    loop is `while j + .4 < end` with its else -- so the times compare equal (==) to the reference's,
    which concat_segs relies on.  A list of (start, end) float pairs; no speech gives []."""
    sr = _sr(sr)
    n = int(sr * (frame_ms / 1000.0) * 2)
    duration = (float(n) / sr) / 2.0
    ring = collections.deque(maxlen=int(padding_ms / frame_ms))
    triggered, voiced, start = False, False, 0.0
    timestamp, end_of_last = 0.0, 0.0
    spans = []
    for speech in is_speech:
        speech = bool(speech)
        if not triggered:
            ring.append((timestamp, speech))
            if len([1 for _, s in ring if s]) > 0.9 * ring.maxlen:
                triggered, voiced = True, True
                start = ring[0][0]
                ring.clear()
        else:
            voiced = True
            ring.append((timestamp, speech))
            if len([1 for _, s in ring if not s]) > 0.9 * ring.maxlen:
                triggered, voiced = False, False
                spans.append((start, timestamp + duration))
                ring.clear()
        end_of_last = timestamp + duration
        timestamp += duration
    if voiced:
        spans.append((start, end_of_last))
    times = []
    for t0, t1 in spans:
        start, end = np.round(t0, decimals=2), np.round(t1, decimals=2)
        j = start
        while j + .4 < end:
            end_j = np.round(j + .4, decimals=2)
            times.append((float(j), float(end_j)))
            j = end_j
        else:
            times.append((float(j), float(end)))
    return times


def voiced_ranges(times, n_samples, sr=None):
    """dvector_create.concat_segs as sample ranges [(a, b)] of the waveform: chunk i of VAD_chunk is
    audio[int(t0 * sr):int(t1 * sr)], and consecutive chunks with times[i][1] == times[i + 1][0]
    are concatenated.  Such chunks are contiguous in the waveform (the next starts at the very
    int(t * sr) the last ended at), so every concatenated segment is one slice: (int(first t0 * sr),
    int(last t1 * sr)), both clamped to n_samples as the slice clamps them.

    Ranges with fewer than WIN + 1 log-mel frames (1 + (b - a) // hop <= WIN: shorter than 3840
    samples at the default configuration) are dropped.  They give no window in get_STFTs (its
    `j + 24 < T`), so nothing is lost, and every kept range is longer than the log-mel's minimum
    of nfft // 2 + 1 samples."""
    sr = _sr(sr)
    hop_n = int(hp.data.hop * sr)
    out = []
    i = 0
    while i < len(times):
        k = i
        while k + 1 < len(times) and times[k][1] == times[k + 1][0]:
            k += 1
        a, b = min(int(times[i][0] * sr), n_samples), min(int(times[k][1] * sr), n_samples)
        b = max(a, b)
        if 1 + (b - a) // hop_n > WIN:
            out.append((a, b))
        i = k + 1
    return out


def window_starts(frame_off, win=WIN, hop=HOP):
    """(starts, counts): the int32 first-row table [S] of every window of every segment -- per
    segment of T_s frames, j = 0, hop, ... while j + win < T_s (window_frames' rule), segments in
    order -- and the number of windows of each segment.  The one array form of the rule:
    window_index is built on it."""
    starts, counts = [], []
    for a, b in zip(frame_off[:-1], frame_off[1:]):
        s = np.arange(0, max(b - a - win, 0), hop, dtype=np.int64)  # j + win < T
        starts.append(a + s)
        counts.append(int(s.size))
    starts = np.concatenate(starts) if starts else np.zeros(0, dtype=np.int64)
    return starts.astype(np.int32), counts


# ---- the corpus export (dvector_create.py:84-122) ----
def batch_tables(frame_off, seg_file, n_files):
    """The two device tables of one embed_files batch, from the log-mel frame offsets of its ranges
    and the file index of every range: (win_start [S] int32, window_starts' table; part_off
    [n_parts + 1] int32, every file's partitions() as row offsets into the batch's S embeddings;
    the number of partitions of each file).  Every file must hold at least one window."""
    starts, counts = window_starts(frame_off)
    nwin = np.bincount(seg_file, weights=counts, minlength=n_files).astype(np.int64)
    parts = [partitions(int(n)) for n in nwin]
    base = np.concatenate([[0], np.cumsum(nwin)])
    part_off = np.concatenate([[base[f] + a for a, _ in p] for f, p in enumerate(parts)] + [[base[-1]]])
    return starts, part_off.astype(np.int32), [len(p) for p in parts]


def aligned_spans(ranges, sr=None):
    """Which samples every aligned d-vector of one file owns: int64 [n_spans, 3] rows (start_sample,
    end_sample, aligned_index), from the file's voiced ranges alone (what embed_files takes).

    The ranges embed_files keeps (1 + (b - a) // hop_n > WIN) have T = 1 + (b - a) // hop_n log-mel
    frames and windows at the frames j of window_starts; the windows of all kept ranges, in order,
    are numbered 0 .. n_win - 1 and partitions(n_win) gives each its aligned index.  The window at
    frame j of range (a, b) owns the samples [a + j hop_n, a + (j + HOP) hop_n), the last window of
    its range [a + j hop_n, b): a range's windows tile exactly [a, b).  Consecutive windows of one
    range with one aligned index merge into one span.  Rows are ascending and disjoint, their union
    is the kept ranges, and every aligned index 0 .. n_aligned - 1 (batch_tables' count) appears at
    least once -- more than once where a partition straddles two ranges.  A file without a window
    gives [0, 3]."""
    hop_n = int(hp.data.hop * _sr(sr))
    rg = np.asarray([(int(a), int(b)) for a, b in ranges], dtype=np.int64).reshape(-1, 2)
    rg = rg[1 + (rg[:, 1] - rg[:, 0]) // hop_n > WIN]
    if rg.shape[0] == 0:
        return np.zeros((0, 3), dtype=np.int64)
    a, b = rg[:, 0], rg[:, 1]
    frame_off = np.concatenate([[0], np.cumsum(1 + (b - a) // hop_n)])
    starts, counts = window_starts(frame_off)
    counts = np.asarray(counts, dtype=np.int64)
    rid = np.repeat(np.arange(rg.shape[0]), counts)           # the range of every window
    j = starts.astype(np.int64) - frame_off[rid]              # its first frame within the range
    s = a[rid] + j * hop_n
    e = a[rid] + (j + HOP) * hop_n
    last = np.cumsum(counts) - 1                              # (every kept range holds a window)
    e[last] = b
    parts = np.asarray(partitions(int(counts.sum())), dtype=np.int64)
    idx = np.repeat(np.arange(parts.shape[0]), parts[:, 1] - parts[:, 0])
    head = np.ones(s.size, dtype=bool)
    head[1:] = (rid[1:] != rid[:-1]) | (idx[1:] != idx[:-1])
    first = np.flatnonzero(head)
    tail = np.concatenate([first[1:], [s.size]]) - 1
    return np.stack([s[first], e[tail], idx[first]], axis=1)


def _batches(sizes, max_samples):
    """Consecutive index groups whose sizes add up to at most max_samples (a larger item alone)."""
    groups, cur, tot = [], [], 0
    for i, n in enumerate(sizes):
        if cur and tot + n > max_samples:
            groups.append(cur)
            cur, tot = [], 0
        cur.append(i)
        tot += n
    if cur:
        groups.append(cur)
    return groups


@torch.no_grad()
def embed_files(net, files, precision="bf16", path=None, max_samples=2 ** 27, on_device=False, **kw):
    """Aligned d-vectors of many files: `files` is a list of (waveform, ranges), a decoded mono
    waveform at hp.data.sr and its voiced sample ranges [(a, b)] (voiced_ranges); returns one
    float64 [n_aligned_i, proj] array per file, in order -- per file what
    embed_segments(net, [wave[a:b] for a, b in ranges]) gives.  A file with no range or no window
    gives np.zeros((0, proj)); ranges too short for a window are not framed at all.

    Files are grouped into batches of at most max_samples samples.  Per batch: one packed upload of
    the waveforms and all tables, one sv_logmel_ranges launch over all ranges of all files, one
    window_starts table, the embedding, one sv_dvec_align launch over every file's partitions()
    and one copy out.  The embedding, in bf16 with dvec_ok(F, H) and (path == "dvec" or, with
    path None, at least DVEC_MIN windows in the batch): sv_dvector_embed_bf16_frames in chunks of
    DVEC_CHUNK windows, which reads the windows in place -- no window tensor exists.  Otherwise
    (fp32, small bf16 batches, path == "persist"): the windows of one chunk at a time gathered on the
    device from the same table (windows_from_logmel's gather) and embed_windows(**kw) on them, so
    the window tensor stays bounded by the chunk (kw's `batch`, else embed_windows' default).
    on_device=True skips the copy out: a file with d-vectors then gets a float64 device tensor (a view
    of its batch's sv_dvec_align output) instead of an array, for consumers on the GPU
    (diarization.diarize).  Raises PersistentRecurrenceError like embed_windows."""
    from .features import _config, logmel_ranges
    _check_path(precision, path)
    _, _, _, hop_n, nmels = _config(None, None, None, None, None)
    layers = net.LSTM_stack.layer_params()
    wp, bp = net.projection.weight, net.projection.bias
    proj, H = wp.shape[0], layers[0][1].shape[1]
    if path == "dvec" and not dvec_ok(nmels, H):
        raise ValueError(f"the per-timestep GEMM path needs F <= 64, H % 64 == 0 and 4H % 256 == 0 (F={nmels}, H={H})")
    results = [np.zeros((0, proj)) for _ in files]
    # only ranges that hold a window are framed (the others give nothing: get_STFTs' j + 24 < T)
    kept = [[(int(a), int(b)) for a, b in ranges if 1 + (int(b) - int(a)) // hop_n > WIN] for _, ranges in files]
    live = [i for i, r in enumerate(kept) if r]
    for group in _batches([int(files[i][0].shape[0]) for i in live], max_samples):
        ids = [live[g] for g in group]
        ranges = [(w, a, b) for w, i in enumerate(ids) for a, b in kept[i]]
        seg_file = [w for w, i in enumerate(ids) for _ in kept[i]]
        n_parts = []

        def tables(frame_off):  # (every file of the batch has a range with a window)
            starts, part_off, n_parts[:] = batch_tables(frame_off, seg_file, len(ids))
            return [starts, part_off]

        out, _, (win_start, part_off) = logmel_ranges([files[i][0] for i in ids], ranges, tables=tables)
        S = int(win_start.shape[0])
        with torch.cuda.device(out.device):
            if _takes_dvec(precision, path, S, nmels, H):
                emb = [embedder_forward_dvec_bf16_frames(out, win_start[i:i + DVEC_CHUNK], layers, wp, bp)
                       for i in range(0, S, DVEC_CHUNK)]
                check_persistent_status(wait=True)
            else:
                chunk = kw.get("batch") or (bf16_batch(H) if precision == "bf16" else 16384)
                steps = torch.arange(WIN, device=out.device)
                emb = [embed_windows(net, out[win_start[i:i + chunk].long()[:, None] + steps[None, :]], precision=precision,
                                     path=path, **kw) for i in range(0, S, chunk)]
            emb = emb[0] if len(emb) == 1 else torch.cat(emb)
            aligned = dvec_align(emb, part_off)
            if not on_device:
                aligned = aligned.cpu().numpy()
        pos = 0
        for i, n in zip(ids, n_parts):
            results[i] = aligned[pos:pos + n]
            pos += n
    return results


def export_sequences(net, speakers, out_dir, **kw):
    """The module-level loop of dvector_create.py:84-122 on decoded audio: `speakers` is a list
    (one entry per folder) of lists of (waveform, ranges) files (ranges from voiced_ranges).  Writes
    train_sequence.npy, train_cluster_id.npy, test_sequence.npy and test_cluster_id.npy into
    out_dir and returns the four arrays (train sequence, train ids, test sequence, test ids):
    sequences float64 [n, proj], the files' aligned d-vectors concatenated in order; ids np.asarray
    of one label string per row.

    As in the reference, the label is the folder's index as str and counts every folder, also one
    without a usable file; a file without voiced audio (no ranges: the reference's `segs == []`) is
    skipped.  A file whose ranges hold no window, where the reference would crash in np.stack([]),
    is skipped too.  The train part is closed after the first folder with index
    i > (len(speakers) // 10) * 9 -- so it holds folders 0 .. (len // 10) * 9 + 1 -- and the rest is
    the test part.  Where the reference's np.concatenate([]) would raise -- a part without a single
    d-vector, or no folder at all past the train part -- ValueError names the part and nothing is
    written; so does a corpus too small for the train part ever to be closed (fewer than two
    folders), where the reference would write the test files alone.

    All folders go through one embed_files call (**kw); the split is applied afterwards."""
    total = len(speakers)
    train_speaker_num = (total // 10) * 9
    flat = [f for folder in speakers for f in folder]
    embedded = iter(embed_files(net, flat, **kw))
    parts = {"train": ([], []), "test": ([], [])}
    train_saved = False
    for i, folder in enumerate(speakers):
        seq, ids = parts["test" if train_saved else "train"]
        for _ in folder:
            aligned = next(embedded)
            if len(aligned) == 0:
                continue  # no voice activity detected (or no window in what was detected)
            seq.append(aligned)
            ids.extend([str(i)] * len(aligned))
        if not train_saved and i > train_speaker_num:
            train_saved = True
    if not train_saved:
        raise ValueError(f"the train part is never closed with {total} folder(s): nothing written")
    for name, (seq, _) in parts.items():
        if not seq:
            raise ValueError(f"the {name} part holds no d-vector: nothing written")
    os.makedirs(out_dir, exist_ok=True)
    arrays = []
    for name, (seq, ids) in parts.items():
        sequence, cluster_id = np.concatenate(seq, axis=0), np.asarray(ids)
        np.save(os.path.join(out_dir, f"{name}_sequence.npy"), sequence)
        np.save(os.path.join(out_dir, f"{name}_cluster_id.npy"), cluster_id)
        arrays += [sequence, cluster_id]
    return tuple(arrays)
