"""Log-mel front end on the GPU: waveform segments -> log-mel frames (reference
data_preprocess.py:38-47 and dvector_create.get_STFTs, :38-47).

The function is the reference's ``librosa.stft(center=True, pad_mode='reflect')`` -> ``|.|**2`` ->
``librosa.filters.mel`` (Slaney scale, area-normalised) -> ``log10(. + 1e-6)``, written out from its
definition (librosa is not a dependency).  ``logmel`` packs a ragged batch of segments into one
buffer and runs the fused HIP kernel ``sv_logmel`` once: frames x (Hann window folded into the real
DFT basis) on the exact fp32 MFMA, power, mel and log10 in its epilogue.  The output is time-major
``[n_frames, nmels]``, so a d-vector window is a row slice and a ``[nmels, T]`` training slice is a
transposed row slice.

Audio decoding, resampling, VAD (webrtcvad), ``librosa.effects.split`` / ``trim`` and the
magnitude-dB feature of ``utils.mfccs_and_spec`` stay out of scope: this module starts from mono
fp32 samples at ``hp.data.sr``.
"""
from __future__ import annotations

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


def segment_offsets(lengths, nfft, hop):
    """(seg_off, frame_off) of segments of `lengths` samples, as int32 arrays of len + 1: segment s
    holds 1 + len_s // hop frames (librosa's center=True).  ValueError for a segment shorter than
    nfft//2 + 1 samples (its reflect padding would need a second reflection)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    if lengths.size == 0:
        raise ValueError("logmel needs at least one segment")
    short = np.nonzero(lengths < nfft // 2 + 1)[0]
    if short.size:
        raise ValueError(f"segment {int(short[0])} has {int(lengths[short[0]])} samples; reflect padding of an "
                         f"nfft={nfft} STFT needs at least {nfft // 2 + 1}")
    seg_off = np.concatenate([[0], np.cumsum(lengths)])
    frame_off = np.concatenate([[0], np.cumsum(1 + lengths // hop)])
    if seg_off[-1] >= 2 ** 31 or frame_off[-1] * 128 >= 2 ** 31:
        raise ValueError("too many samples for one logmel call (32-bit offsets): split the batch")
    return seg_off.astype(np.int32), frame_off.astype(np.int32)


def _as_list(waves):
    if isinstance(waves, (list, tuple)):
        return list(waves)
    return [waves]


def logmel(waves, sr=None, nfft=None, window=None, hop=None, nmels=None):
    """Log-mel frames of one waveform segment or a list of them (1-D arrays or tensors, host or
    device, mono at `sr`): (out [n_frames, nmels] cuda float32, frame_off) with segment s in rows
    frame_off[s] : frame_off[s + 1].  sr, nfft, window (s), hop (s), nmels default to hp.data.
    One packed copy in and one kernel launch for the whole batch."""
    sr, nfft, win, hop_n, nmels = _config(sr, nfft, window, hop, nmels)
    segs = _as_list(waves)
    for s in segs:
        if getattr(s, "ndim", None) != 1:
            raise ValueError("each segment must be a 1-D array or tensor of samples")
    seg_off, frame_off = segment_offsets([int(s.shape[0]) for s in segs], nfft, hop_n)
    on_dev = [s for s in segs if torch.is_tensor(s) and s.is_cuda]
    if on_dev:
        dev = on_dev[0].device
    else:
        dev = _lib.compute_device(torch.empty(0))
    n, n_seg, n_frames = int(seg_off[-1]), len(segs), int(frame_off[-1])
    offs = np.concatenate([seg_off, frame_off])
    if on_dev:
        y = torch.cat([torch.as_tensor(s).to(dev, torch.float32) for s in segs]) if n_seg > 1 else \
            on_dev[0].to(torch.float32).contiguous()
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
    wbasis, melfb = stft_tables(sr, nfft, win, nmels, dev)
    out = torch.empty((n_frames, nmels), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        logmel_into(y, o[:n_seg + 1], o[n_seg + 1:], n_seg, n_frames, nfft, win, hop_n, nmels, wbasis, melfb, out)
    return out, [int(v) for v in frame_off]


def logmel_into(y, seg_off, frame_off, n_seg, n_frames, nfft, win, hop, nmels, wbasis, melfb, out):
    """sv_logmel on device tensors (y fp32, offsets int32, out [>= n_frames, nmels] fp32 contiguous)."""
    _lib.call("sv_logmel", _lib.ptr(y), _lib.ptr(seg_off), _lib.ptr(frame_off), n_seg, n_frames, nfft, win, hop,
              nmels, _lib.ptr(wbasis), wbasis.stride(0), _lib.ptr(melfb), _lib.ptr(out), None, _lib.stream_of(out))


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
