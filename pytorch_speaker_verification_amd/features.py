"""Offline preprocessing on the GPU: waveforms -> voiced intervals -> log-mel frames -> the
``speakerN.npy`` training tensors (reference data_preprocess.py:24-54 and
dvector_create.get_STFTs, :38-47).

The function is the reference's ``librosa.stft(center=True, pad_mode='reflect')`` -> ``|.|**2`` ->
``librosa.filters.mel`` (Slaney scale, area-normalised) -> ``log10(. + 1e-6)``, written out from its
definition (librosa is not a dependency).  ``logmel`` packs a ragged batch of segments into one
buffer and runs the fused HIP kernel ``sv_logmel`` once: frames x (Hann window folded into the real
DFT basis) on the exact fp32 MFMA, power, mel and log10 in its epilogue.  The output is time-major
``[n_frames, nmels]``, so a d-vector window is a row slice and a ``[nmels, T]`` training slice is a
transposed row slice.

``split`` / ``trim`` are ``librosa.effects.split`` / ``trim`` of librosa < 0.10 (the versions the
reference's positional calls work with; ``feature.rms`` pads with ``pad_mode='reflect'`` there),
written out from their definition: the framed energy of a ragged batch of waveforms is one launch
of the HIP kernel ``sv_frame_energy``; the dB threshold against each waveform's own maximum and the
edges are numpy on the host.  ``preprocess_speaker`` is the body of data_preprocess.py:30-49 on
decoded waveforms (one ``split``, one ``logmel``, one gather) and ``save_speakers`` its 90/10 writer.

``mel_db`` is the raw-waveform training feature, ``mel_db`` of ``utils.mfccs_and_spec``
(utils.py:150-158): the same STFT's magnitude -> mel -> ``librosa.amplitude_to_db`` (ref 1,
amin 1e-5, top_db 80 against each utterance's own maximum), time-major, from the HIP entry point
``sv_meldb``.  ``mel_db_fixed`` puts ``wav_process=True`` (utils.py:145-148) in front --
``librosa.effects.trim(frame_length=win, hop_length=hop)`` and ``librosa.util.fix_length`` -- as
index arithmetic on the one uploaded buffer: a batch of utterances to ``[n, T, nmels]`` in one
``sv_frame_energy`` launch and one ``sv_meldb`` call.

``logmel_ranges`` is ``logmel`` of ranges of one uploaded buffer (``sv_logmel_ranges``): the voiced
ranges of many files, which may touch, overlap or leave gaps, are framed in one launch without
re-packing the audio, each bit-identical to ``logmel`` of its slice.  It is the front of the corpus
d-vector export (``dvector.embed_files``).

Audio decoding, resampling and the per-frame VAD decision (webrtcvad) stay out of scope (the
bookkeeping around that decision is ``dvector.vad_times`` / ``voiced_ranges``): this module starts from mono
fp32 samples at ``hp.data.sr``.  So do the other two outputs of ``utils.mfccs_and_spec``:
``mag_db`` (the reference's dataset drops it) and ``calc_mfccs`` (a DCT over the time axis of the
already transposed array, with ``librosa.filters.dct``, which librosa removed).
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _lib
from .hparam import hparam as hp

_TABLES = {}  # (sr, nfft, win, nmels, device) -> (wbasis, melfb) on the device


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3.0)
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)), m * (200.0 / 3.0))


def mel_filterbank(sr, nfft, nmels):
    """librosa.filters.mel(sr, nfft, nmels) with its defaults (fmin 0, fmax sr/2, Slaney scale,
    area normalisation): [nmels, nfft//2 + 1] float32, built in float64 and rounded once."""
    nb = nfft // 2 + 1
    bins = np.linspace(0.0, sr / 2.0, nb)
    f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), nmels + 2))
    lower = (bins[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    upper = (f[2:, None] - bins[None, :]) / (f[2:] - f[1:-1])[:, None]
    w = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (f[2:] - f[:-2]))[:, None]
    return w.astype(np.float32)


def window_basis(nfft, win):
    """The periodic Hann window of length win, centred in nfft, folded into the real-DFT basis
    (include/sv_ge2e.h, sv_logmel): [win, ld] float32 with column 2k = w[j] cos(2 pi k (j + lpad) / nfft)
    and column 2k + 1 = w[j] sin(...), k = 0 .. nfft//2; ld = 2 (nfft//2 + 1) rounded up to 4."""
    nb = nfft // 2 + 1
    lpad = (nfft - win) // 2
    j = np.arange(win)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * j / win)
    # k (j + lpad) reduced mod nfft in integers: the angle is exact to one float64 rounding
    ang = (2.0 * np.pi / nfft) * ((np.arange(nb)[None, :] * (j + lpad)[:, None]) % nfft)
    ld = (2 * nb + 3) // 4 * 4
    out = np.zeros((win, ld), dtype=np.float64)
    out[:, 0:2 * nb:2] = w[:, None] * np.cos(ang)
    out[:, 1:2 * nb:2] = w[:, None] * np.sin(ang)
    return out.astype(np.float32)


def stft_tables(sr, nfft, win, nmels, device):
    """(wbasis [win, ld], melfb [nmels, nfft//2 + 1]) fp32 on `device`, built once per
    (configuration, device) and kept."""
    device = torch.device(device)
    key = (sr, nfft, win, nmels, device.type, device.index)
    t = _TABLES.get(key)
    if t is None:
        t = (torch.from_numpy(window_basis(nfft, win)).to(device), torch.from_numpy(mel_filterbank(sr, nfft, nmels)).to(device))
        _TABLES[key] = t
    return t


def _config(sr, nfft, window, hop, nmels):
    sr = hp.data.sr if sr is None else sr
    nfft = hp.data.nfft if nfft is None else nfft
    window = hp.data.window if window is None else window
    hop = hp.data.hop if hop is None else hop
    nmels = hp.data.nmels if nmels is None else nmels
    win, hop_n = int(window * sr), int(hop * sr)
    if nfft % 2 or not 2 <= nfft <= 1024 or not 1 <= win <= nfft or hop_n < 1 or not 1 <= nmels <= 128:
        raise ValueError(f"unsupported log-mel configuration: nfft={nfft} (even, <= 1024), win={win} (<= nfft), "
                         f"hop={hop_n} (>= 1), nmels={nmels} (<= 128)")
    return sr, nfft, win, hop_n, nmels


def _frame_table(seg_len, hop, min_len, n_samples, name, noun="segment", rows=128):
    """frame_off [n + 1] int32 of segments of `seg_len` samples (an int64 array): segment s holds
    1 + len_s // hop frames (librosa's center=True).  ValueError for a segment shorter than min_len
    samples (its reflect padding would need a second reflection) and for totals past 32-bit
    offsets: n_samples samples in the packed buffer or `rows` output scalars per frame.  `name` is
    the call and `noun` the kind of segment the messages speak of."""
    short = np.nonzero(seg_len < min_len)[0]
    if short.size:
        raise ValueError(f"{noun} {int(short[0])} has {int(seg_len[short[0]])} samples; {name}'s reflect padding "
                         f"needs at least {min_len}")
    frame_off = np.concatenate([[0], np.cumsum(1 + seg_len // hop)])
    if n_samples >= 2 ** 31 or frame_off[-1] * rows >= 2 ** 31:
        raise ValueError(f"too many samples for one {name} call (32-bit offsets): split the batch")
    return frame_off.astype(np.int32)


def segment_offsets(lengths, nfft, hop):
    """(seg_off, frame_off) of segments of `lengths` samples, as int32 arrays of len + 1: segment s
    holds 1 + len_s // hop frames (librosa's center=True).  ValueError for a segment shorter than
    nfft//2 + 1 samples (its reflect padding would need a second reflection)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    if lengths.size == 0:
        raise ValueError("logmel needs at least one segment")
    seg_off = np.concatenate([[0], np.cumsum(lengths)])
    return seg_off.astype(np.int32), _frame_table(lengths, hop, nfft // 2 + 1, seg_off[-1], "logmel")


def _as_list(waves):
    return list(waves) if isinstance(waves, (list, tuple)) else [waves]


def _waves(waves, noun="waveform"):
    """One waveform or a list of them, as a list of 1-D arrays or tensors."""
    segs = _as_list(waves)
    for s in segs:
        if getattr(s, "ndim", None) != 1:
            raise ValueError(f"each {noun} must be a 1-D array or tensor of samples")
    return segs


def _pack(segs, seg_off, frame_off):
    """(y, seg_off, frame_off, device) on the GPU, the one packing of every entry point here: host
    segments and both offset tables in one pinned buffer and one copy; device-resident segments
    concatenated there."""
    on_dev = [s for s in segs if torch.is_tensor(s) and s.is_cuda]
    dev = on_dev[0].device if on_dev else _lib.compute_device(torch.empty(0))
    n, n_seg = int(seg_off[-1]), len(segs)
    offs = np.concatenate([seg_off, frame_off])
    if on_dev:
        y = torch.cat([torch.as_tensor(s).to(dev, torch.float32) for s in segs]) if n_seg > 1 else \
            on_dev[0].to(torch.float32).contiguous()
        if y.data_ptr() % 16:  # a slice of a larger tensor: the entry points want 16-byte alignment
            y = y.clone()
        o = torch.from_numpy(offs).to(dev)
    else:
        # samples and both offset tables in one pinned buffer: one host-to-device copy
        npad = (n + 3) // 4 * 4
        host = torch.empty(npad + offs.size, dtype=torch.float32, pin_memory=True)
        hn = host.numpy()
        for s, a in zip(segs, seg_off[:-1]):
            hn[a:a + s.shape[0]] = s.numpy() if torch.is_tensor(s) else np.asarray(s)
        hn[n:npad] = 0.0
        hn[npad:].view(np.int32)[:] = offs
        buf = host.to(dev, non_blocking=True)
        y, o = buf[:n], buf[npad:].view(torch.int32)
    return y, o[:n_seg + 1], o[n_seg + 1:], dev


def _stft_launch(into, y, tabs, n_seg, shape, cfg, dev, *extra):
    """out [*shape, nmels] (math.prod(shape) frames) of one of the three STFT entry points: the
    (wbasis, melfb) tables, the output buffer and into(y, *tabs, n_seg, n_frames, configuration,
    tables, out, *extra) on dev."""
    sr, nfft, win, hop_n, nmels = cfg
    wbasis, melfb = stft_tables(sr, nfft, win, nmels, dev)
    out = torch.empty((*shape, nmels), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        into(y, *tabs, n_seg, math.prod(shape), nfft, win, hop_n, nmels, wbasis, melfb, out, *extra)
    return out


def logmel(waves, sr=None, nfft=None, window=None, hop=None, nmels=None):
    """Log-mel frames of one waveform segment or a list of them (1-D arrays or tensors, host or
    device, mono at `sr`): (out [n_frames, nmels] cuda float32, frame_off) with segment s in rows
    frame_off[s] : frame_off[s + 1].  sr, nfft, window (s), hop (s), nmels default to hp.data.
    One packed copy in and one kernel launch for the whole batch."""
    cfg = _config(sr, nfft, window, hop, nmels)
    segs = _waves(waves, "segment")
    seg_off, frame_off = segment_offsets([int(s.shape[0]) for s in segs], cfg[1], cfg[3])
    y, so, fo, dev = _pack(segs, seg_off, frame_off)
    out = _stft_launch(logmel_into, y, (so, fo), len(segs), (int(frame_off[-1]),), cfg, dev)
    return out, [int(v) for v in frame_off]


def logmel_into(y, seg_off, frame_off, n_seg, n_frames, nfft, win, hop, nmels, wbasis, melfb, out):
    """sv_logmel on device tensors (y fp32, offsets int32, out [>= n_frames, nmels] fp32 contiguous)."""
    _lib.call("sv_logmel", _lib.ptr(y), _lib.ptr(seg_off), _lib.ptr(frame_off), n_seg, n_frames, nfft, win, hop,
              nmels, _lib.ptr(wbasis), wbasis.stride(0), _lib.ptr(melfb), _lib.ptr(out), None, _lib.stream_of(out))


def range_tables(lengths, ranges, nfft, hop):
    """(seg_start, seg_len, frame_off) int32 arrays (n, n, n + 1) of sv_logmel_ranges for waveforms
    of `lengths` samples packed back to back and `ranges` = (wave_index, a, b) entries, range r
    being samples [a, b) of its waveform with 1 + (b - a) // hop frames.  ValueError for no range, a
    wave index or bounds outside the waveform, a range shorter than nfft//2 + 1 samples (its reflect
    padding would need a second reflection) and for totals past 32-bit offsets."""
    lengths = np.asarray(lengths, dtype=np.int64)
    r = np.asarray([(int(w), int(a), int(b)) for w, a, b in ranges], dtype=np.int64).reshape(-1, 3)
    if r.shape[0] == 0:
        raise ValueError("logmel_ranges needs at least one range")
    bad = np.nonzero((r[:, 0] < 0) | (r[:, 0] >= lengths.size))[0]
    if bad.size:
        raise ValueError(f"range {int(bad[0])} names waveform {int(r[bad[0], 0])} of {lengths.size}")
    n = lengths[r[:, 0]]
    bad = np.nonzero((r[:, 1] < 0) | (r[:, 2] > n) | (r[:, 1] > r[:, 2]))[0]
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"range {k} [{int(r[k, 1])}, {int(r[k, 2])}) lies outside its waveform of {int(n[k])} samples")
    seg_len = r[:, 2] - r[:, 1]
    seg_off = np.concatenate([[0], np.cumsum(lengths)])
    frame_off = _frame_table(seg_len, hop, nfft // 2 + 1, seg_off[-1], "logmel_ranges", "range")
    return (seg_off[r[:, 0]] + r[:, 1]).astype(np.int32), seg_len.astype(np.int32), frame_off


def logmel_ranges(y, ranges, sr=None, nfft=None, window=None, hop=None, nmels=None, tables=None):
    """Log-mel frames of ranges of one waveform `y` (or of a list of waveforms, packed once; 1-D
    arrays or tensors, host or device, mono at `sr`): `ranges` holds (wave_index, a, b) entries,
    range r being samples [a, b) of waveform wave_index.  Returns (out [n_frames, nmels] cuda float32,
    frame_off) with range r in rows frame_off[r] : frame_off[r + 1], each bit-identical to
    logmel(wave[a:b]).  Ranges may touch, overlap or leave gaps: the audio is uploaded once and never
    re-packed, one sv_logmel_ranges launch frames all of them.  ValueError (before any upload) for an
    empty list, a range out of bounds or shorter than nfft//2 + 1 samples, and for totals past 32-bit
    offsets.  `tables` (a callable frame_off -> list of int32 arrays) rides in the same upload; with
    it the result is (out, frame_off, [the arrays on the device]) -- dvector.embed_files sends its
    window and partition tables this way."""
    cfg = _config(sr, nfft, window, hop, nmels)
    waves = _waves(y)
    lengths = [int(s.shape[0]) for s in waves]
    seg_start, seg_len, frame_off = range_tables(lengths, ranges, cfg[1], cfg[3])
    frame_off_l = [int(v) for v in frame_off]
    extra = [np.ascontiguousarray(t, dtype=np.int32) for t in tables(frame_off_l)] if tables is not None else []
    n_seg, n_frames = len(seg_len), frame_off_l[-1]
    seg_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    y_dev, _, tab, dev = _pack(waves, seg_off, np.concatenate([seg_start, seg_len, frame_off] + extra))
    out = _stft_launch(logmel_ranges_into, y_dev, (tab[:n_seg], tab[n_seg:2 * n_seg], tab[2 * n_seg:3 * n_seg + 1]),
                       n_seg, (n_frames,), cfg, dev)
    if tables is None:
        return out, frame_off_l
    pos, on_dev = 3 * n_seg + 1, []
    for t in extra:
        on_dev.append(tab[pos:pos + t.size])
        pos += t.size
    return out, frame_off_l, on_dev


def logmel_ranges_into(y, seg_start, seg_len, frame_off, n_seg, n_frames, nfft, win, hop, nmels, wbasis, melfb, out):
    """sv_logmel_ranges on device tensors (y fp32; seg_start, seg_len [n_seg] and frame_off
    [n_seg + 1] int32; out [>= n_frames, nmels] fp32 contiguous)."""
    _lib.call("sv_logmel_ranges", _lib.ptr(y), _lib.ptr(seg_start), _lib.ptr(seg_len), _lib.ptr(frame_off), n_seg,
              n_frames, nfft, win, hop, nmels, _lib.ptr(wbasis), wbasis.stride(0), _lib.ptr(melfb), _lib.ptr(out), None,
              _lib.stream_of(out))


def preprocess_utterance(utter, intervals, tisv_frame=None):
    """The body of data_preprocess.py:38-47 for one utterance: for each [start, end) interval longer
    than (tisv_frame * hop + window) * sr samples, the first and the last tisv_frame frames of that
    part's log-mel, as [nmels, tisv_frame] float32 arrays (the reference's orientation).  All
    intervals go through one logmel call."""
    tisv_frame = hp.data.tisv_frame if tisv_frame is None else tisv_frame
    utter_min_len = (tisv_frame * hp.data.hop + hp.data.window) * hp.data.sr
    parts = [utter[a:b] for a, b in intervals if (b - a) > utter_min_len]
    if not parts:
        return []
    out, frame_off = logmel(parts)
    out = out.cpu().numpy()
    specs = []
    for a, b in zip(frame_off[:-1], frame_off[1:]):
        S = out[a:b].T  # [nmels, T]
        specs.append(np.ascontiguousarray(S[:, :tisv_frame], dtype=np.float32))
        specs.append(np.ascontiguousarray(S[:, -tisv_frame:], dtype=np.float32))
    return specs


def energy_offsets(lengths, frame_length, hop_length):
    """(seg_off, frame_off) int32 arrays of len + 1 for waveforms of `lengths` samples: waveform s
    holds 1 + len_s // hop_length energy frames.  ValueError for an odd frame_length, a hop below 1
    or a waveform shorter than frame_length // 2 + 1 samples (one reflection at each end)."""
    if frame_length < 2 or frame_length % 2 or frame_length > 2 ** 20 or hop_length < 1:
        raise ValueError(f"unsupported framing: frame_length={frame_length} (even, 2 .. 2**20), hop_length={hop_length} "
                         "(>= 1)")
    lengths = np.asarray(lengths, dtype=np.int64)
    if lengths.size == 0:
        raise ValueError("frame_energy needs at least one waveform")
    seg_off = np.concatenate([[0], np.cumsum(lengths)])
    # (rows=1: mse holds one scalar per frame)
    return seg_off.astype(np.int32), _frame_table(lengths, hop_length, frame_length // 2 + 1, seg_off[-1],
                                                  "frame_energy", "waveform", rows=1)


def frame_energy(waves, frame_length=2048, hop_length=512):
    """Mean square of every centred, reflect-padded frame (librosa.feature.rms ** 2) of one waveform
    or a list of them (1-D arrays or tensors, host or device): (mse [n_frames] cuda float32,
    frame_off) with waveform s in mse[frame_off[s] : frame_off[s + 1]].  One packed copy in and one
    kernel launch for the whole batch; a waveform's values do not depend on its neighbours."""
    segs = _waves(waves)
    seg_off, frame_off = energy_offsets([int(s.shape[0]) for s in segs], frame_length, hop_length)
    y, so, fo, dev = _pack(segs, seg_off, frame_off)
    n_frames = int(frame_off[-1])
    mse = torch.empty(n_frames, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        frame_energy_into(y, so, fo, len(segs), n_frames, frame_length, hop_length, mse)
    return mse, [int(v) for v in frame_off]


def frame_energy_into(y, seg_off, frame_off, n_seg, n_frames, frame_length, hop_length, mse):
    """sv_frame_energy on device tensors (y fp32, offsets int32, mse [>= n_frames] fp32)."""
    _lib.call("sv_frame_energy", _lib.ptr(y), _lib.ptr(seg_off), _lib.ptr(frame_off), n_seg, n_frames, frame_length,
              hop_length, _lib.ptr(mse), _lib.stream_of(mse))


def intervals_from_energy(mse, n, hop_length, top_db=60, amin=1e-10):
    """The host half of split: the frames of one waveform of n samples whose power is within top_db
    of the waveform's loudest frame (10 log10(max(amin, mse)), a strict comparison), as [k, 2] int64
    sample intervals [start, end) -- frame edges times hop_length, capped at n."""
    mse = np.asarray(mse, dtype=np.float64)
    db = 10.0 * np.log10(np.maximum(amin, mse)) - 10.0 * np.log10(max(amin, float(mse.max())))
    nonsilent = db > -top_db
    edges = np.flatnonzero(np.diff(nonsilent.astype(np.int8), prepend=0, append=0))
    return np.minimum(edges.astype(np.int64) * hop_length, n).reshape(-1, 2)


def split(waves, top_db=60, frame_length=2048, hop_length=512):
    """librosa.effects.split: the non-silent [start, end) sample intervals of one waveform ([k, 2]
    int64, k may be 0) or of each waveform of a list (a list of such arrays).  Every waveform is
    measured against its own loudest frame.  One launch and one device-to-host copy per call."""
    segs = _as_list(waves)  # (frame_energy checks them)
    mse, frame_off = frame_energy(segs, frame_length, hop_length)
    mse = mse.cpu().numpy()
    out = [intervals_from_energy(mse[a:b], int(s.shape[0]), hop_length, top_db)
           for s, a, b in zip(segs, frame_off[:-1], frame_off[1:])]
    return out if isinstance(waves, (list, tuple)) else out[0]


def _trim_bounds(intervals):
    """trim's (start, end) from split's intervals: the first one's start and the last one's end."""
    return (int(intervals[0, 0]), int(intervals[-1, 1])) if len(intervals) else (0, 0)


def trim(wave, top_db=60, frame_length=2048, hop_length=512):
    """librosa.effects.trim: (wave[start:end], (start, end)) from the first non-silent interval's
    start to the last one's end; (0, 0) if no frame is non-silent."""
    start, end = _trim_bounds(split(wave, top_db, frame_length, hop_length))
    return wave[start:end], (start, end)


def _check_db(amin, top_db):
    if not amin > 0:
        raise ValueError(f"amin must be positive (got {amin})")
    if top_db is not None and top_db < 0:
        raise ValueError(f"top_db must be non-negative or None (got {top_db})")
    return float(amin), -1.0 if top_db is None else float(top_db)  # (a negative top_db: sv_meldb skips the clip)


def mel_db(waves, sr=None, nfft=None, window=None, hop=None, nmels=None, amin=1e-5, top_db=80.0):
    """Mel magnitude in dB of one waveform segment or a list of them (1-D arrays or tensors, host or
    device, mono at `sr`): (out [n_frames, nmels] cuda float32, frame_off), a ragged batch packed
    exactly as logmel packs one.  out = amplitude_to_db(melfb @ |stft|).T of librosa < 0.10:
    20 log10(max(amin, .)), then nothing below the segment's own maximum - top_db (top_db=None: no
    clip).  One packed copy in and one sv_meldb call for the whole batch; a segment's values do not
    depend on its neighbours.  Decoding, resampling, mag_db and calc_mfccs are out of scope."""
    cfg = _config(sr, nfft, window, hop, nmels)
    amin, top_db = _check_db(amin, top_db)
    segs = _waves(waves, "segment")
    seg_off, frame_off = segment_offsets([int(s.shape[0]) for s in segs], cfg[1], cfg[3])
    n_seg, n_frames = len(segs), int(frame_off[-1])
    # the lengths ride behind frame_off in _pack's one copy: seg_valid = seg_len = the real lengths
    y, so, fo, dev = _pack(segs, seg_off, np.concatenate([frame_off, np.diff(seg_off)]).astype(np.int32))
    lengths = fo[n_seg + 1:]
    seg_max = torch.empty(n_seg, dtype=torch.float32, device=dev)
    out = _stft_launch(mel_db_into, y, (so[:n_seg], lengths, lengths, fo[:n_seg + 1]), n_seg, (n_frames,), cfg, dev,
                       seg_max, amin, top_db)
    return out, [int(v) for v in frame_off]


def mel_db_into(y, seg_start, seg_valid, seg_len, frame_off, n_seg, n_frames, nfft, win, hop, nmels, wbasis, melfb, out,
                seg_max, amin=1e-5, top_db=80.0):
    """sv_meldb on device tensors (y fp32; seg_start, seg_valid, seg_len [n_seg] and frame_off
    [n_seg + 1] int32; out [>= n_frames, nmels] and seg_max [>= n_seg] fp32 contiguous): segment s is
    seg_valid[s] samples of y from seg_start[s], then zeros up to seg_len[s].  top_db < 0 or None:
    no clip.  seg_max receives each segment's largest mel magnitude."""
    _lib.call("sv_meldb", _lib.ptr(y), _lib.ptr(seg_start), _lib.ptr(seg_valid), _lib.ptr(seg_len), _lib.ptr(frame_off),
              n_seg, n_frames, nfft, win, hop, nmels, _lib.ptr(wbasis), wbasis.stride(0), _lib.ptr(melfb), amin,
              -1.0 if top_db is None else top_db, _lib.ptr(out), _lib.ptr(seg_max), None, _lib.stream_of(out))


def fixed_length(length=None):
    """The reference's fixed utterance length in samples, int(sr * (tisv_frame * hop + window))
    (utils.py:142,147; 29200 at the defaults), unless `length` is given."""
    return int(hp.data.sr * (hp.data.tisv_frame * hp.data.hop + hp.data.window)) if length is None else int(length)


def fixed_segments(bounds, seg_off, length, hop):
    """The segment table of mel_db_fixed as one int32 array [4 n + 1]: seg_start, seg_valid, seg_len
    (n entries each) and frame_off (n + 1).  Waveform s sits at seg_off[s] of the packed buffer and
    was trimmed to [a, b) = bounds[s]: fix_length(wave[a:b], length) is b - a real samples from
    seg_off[s] + a, cut at `length` (truncation) or followed by zeros up to it (padding; an empty
    trim has 0 real samples)."""
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    n = len(bounds)
    start = np.asarray(seg_off, dtype=np.int64)[:n] + bounds[:, 0]
    valid = np.minimum(bounds[:, 1] - bounds[:, 0], length)
    seg_len = np.full(n, length, dtype=np.int64)
    # (no minimum here: mel_db_fixed checks `length` itself; the samples stay where _pack put them)
    frame_off = _frame_table(seg_len, hop, 0, 0, "mel_db_fixed")
    return np.concatenate([start, valid, seg_len, frame_off]).astype(np.int32)


def mel_db_fixed(waves, length=None, trim_top_db=60, amin=1e-5, top_db=80.0):
    """utils.mfccs_and_spec(f, wav_process=True)[1] for every decoded waveform of a list (or one
    waveform; 1-D arrays or tensors, host or device, mono at hp.data.sr): cuda float32
    [n, 1 + length // hop, nmels] with hp.data's configuration, from
    trim(wave, top_db=trim_top_db, frame_length=win, hop_length=hop) -> fix_length(., length) ->
    mel_db.  `length` defaults to the reference's int(sr * (tisv_frame * hop + window));
    trim_top_db=None skips the trim.

    One pack and upload, one sv_frame_energy launch at (win, hop), one copy of the energies back for
    the trim bounds (numpy, intervals_from_energy), one upload of the segment table and one sv_meldb
    call: trim, zero padding and truncation are that table's index arithmetic, the audio is never
    copied or re-packed on the device.  ValueError for a waveform shorter than win // 2 + 1 samples
    (the trim's reflection) or a length below nfft // 2 + 1 (the STFT's)."""
    cfg = _, nfft, win, hop_n, nmels = _config(None, None, None, None, None)
    amin, top_db = _check_db(amin, top_db)
    length = fixed_length(length)
    if length < nfft // 2 + 1:
        raise ValueError(f"length={length}; reflect padding of an nfft={nfft} STFT needs at least {nfft // 2 + 1}")
    segs = _waves(waves)
    lengths = [int(s.shape[0]) for s in segs]
    seg_off, efo = energy_offsets(lengths, win, hop_n)  # (ValueError for a waveform shorter than win // 2 + 1)
    y, so, fo, dev = _pack(segs, seg_off, efo)
    n = len(segs)
    with torch.cuda.device(dev):
        if trim_top_db is None:
            bounds = [(0, m) for m in lengths]
        else:
            mse = torch.empty(int(efo[-1]), dtype=torch.float32, device=dev)
            frame_energy_into(y, so, fo, n, int(efo[-1]), win, hop_n, mse)
            mse = mse.cpu().numpy()
            bounds = [_trim_bounds(intervals_from_energy(mse[a:b], m, hop_n, trim_top_db))
                      for m, a, b in zip(lengths, efo[:-1], efo[1:])]
        table = torch.from_numpy(fixed_segments(bounds, seg_off, length, hop_n)).pin_memory().to(dev, non_blocking=True)
        T = 1 + length // hop_n
        seg_max = torch.empty(n, dtype=torch.float32, device=dev)
        out = _stft_launch(mel_db_into, y, (table[:n], table[n:2 * n], table[2 * n:3 * n], table[3 * n:]), n, (n, T),
                           cfg, dev, seg_max, amin, top_db)
    return out


def preprocess_speaker(utterances, top_db=30, tisv_frame=None):
    """The body of data_preprocess.py:30-49 for one speaker's decoded utterances (1-D waveforms at
    hp.data.sr): float32 [K, nmels, tisv_frame], for every utterance in order and every non-silent
    interval of split(utter, top_db) in order that is longer than (tisv_frame * hop + window) * sr
    samples, the first and then the last tisv_frame frames of that part's log-mel
    (np.array(utterances_spec)).  No kept interval gives shape (0, nmels, tisv_frame), where the
    reference would save an array of shape (0,).  Utterances too short to hold such an interval
    are skipped before the split.

    One split call over all utterances, one logmel call over all kept parts, one gather on the
    device, one copy out.  Only what is kept is computed: of a part with more than
    2 tisv_frame + 3 frames, logmel sees a head that ends nfft / 2 samples after the last kept
    frame's centre and a tail that starts on a hop multiple at least nfft / 2 samples before the
    first kept frame's centre; each kept frame reads exactly the samples it reads in the whole part,
    so by sv_logmel's order guarantee the result is bit-identical to the whole part's."""
    tisv = hp.data.tisv_frame if tisv_frame is None else tisv_frame
    _, nfft, _, hop_n, nmels = _config(None, None, None, None, None)
    utter_min_len = (tisv * hp.data.hop + hp.data.window) * hp.data.sr
    # an utterance of at most utter_min_len samples has no interval longer than that: not split at all
    # (nor refused for being shorter than split's reflect padding)
    utterances = [u for u in utterances if getattr(u, "ndim", None) != 1 or u.shape[0] > utter_min_len]
    if not utterances:
        return np.zeros((0, nmels, tisv), dtype=np.float32)
    lead = -(-(nfft // 2) // hop_n)  # frames of a tail before its first frame free of the cut's reflection
    segs, picks = [], []  # segments for logmel; (segment, first frame) of every [tisv] slice
    for utter, intervals in zip(utterances, split(utterances, top_db=top_db)):
        for a, b in intervals:
            a, b = int(a), int(b)
            if not (b - a) > utter_min_len:
                continue
            part = utter[a:b]
            T = 1 + (b - a) // hop_n
            if T > 2 * tisv + 3:
                picks += [(len(segs), 0), (len(segs) + 1, lead)]
                segs += [part[:(tisv - 1) * hop_n + nfft // 2], part[(T - tisv - lead) * hop_n:]]
            else:
                picks += [(len(segs), 0), (len(segs), T - tisv)]
                segs.append(part)
    if not segs:
        return np.zeros((0, nmels, tisv), dtype=np.float32)
    out, frame_off = logmel(segs)
    rows = np.array([frame_off[s] + f for s, f in picks], dtype=np.int64)[:, None] + np.arange(tisv)[None, :]
    spec = out[torch.from_numpy(rows).to(out.device)].transpose(1, 2).contiguous()  # [K, nmels, tisv]
    return spec.cpu().numpy().astype(np.float32, copy=False)


def save_speakers(speakers, train_path, test_path, top_db=30):
    """data_preprocess.py:24-27, 51-54 on decoded audio: `speakers` is a sequence of utterance lists;
    the first (len // 10) * 9 go to train_path/speaker%d.npy, the rest to test_path/speaker%d.npy
    renumbered from 0, each as preprocess_speaker(utterances, top_db).  Makes both directories.
    Returns (train files, test files)."""
    os.makedirs(train_path, exist_ok=True)
    os.makedirs(test_path, exist_ok=True)
    train_speaker_num = (len(speakers) // 10) * 9
    written = ([], [])
    for i, utterances in enumerate(speakers):
        spec = preprocess_speaker(utterances, top_db=top_db)
        if i < train_speaker_num:
            path = os.path.join(train_path, "speaker%d.npy" % i)
        else:
            path = os.path.join(test_path, "speaker%d.npy" % (i - train_speaker_num))
        np.save(path, spec)
        written[i >= train_speaker_num].append(path)
    return written
