"""Reference log-mel front end for the tests: plain numpy, written from the definition
(librosa.stft(center=True, pad_mode='reflect') -> |.|^2 -> Slaney mel filterbank -> log10(. + 1e-6)).

It shares no code with pytorch_speaker_verification_amd.features (the tests compare the two).
`dtype=np.float64` is the reference; `dtype=np.float32` is the yardstick for the GPU kernel's bound:
the same definition evaluated in fp32 on the CPU (frames x basis by a numpy fp32 matmul, then fp32
power, mel and log10)."""
import math

import numpy as np

DEFAULTS = dict(sr=16000, nfft=512, window=0.025, hop=0.01, nmels=40)


def hz_to_mel(f):
    return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def mel_to_hz(m):
    return m * (200.0 / 3.0) if m < 15.0 else 1000.0 * math.exp((m - 15.0) * (math.log(6.4) / 27.0))


def mel_fb(sr, nfft, nmels):
    """[nmels, nfft//2 + 1] float64: triangles over nmels + 2 equally spaced mel points between 0
    and sr/2, each scaled by 2 / (its width in Hz)."""
    nb = nfft // 2 + 1
    m_lo, m_hi = hz_to_mel(0.0), hz_to_mel(sr / 2.0)
    f = [mel_to_hz(m_lo + (m_hi - m_lo) * i / (nmels + 1)) for i in range(nmels + 2)]
    W = np.zeros((nmels, nb))
    for i in range(nmels):
        for k in range(nb):
            b = (sr / 2.0) * k / (nb - 1)
            up = (b - f[i]) / (f[i + 1] - f[i])
            down = (f[i + 2] - b) / (f[i + 2] - f[i + 1])
            W[i, k] = max(0.0, min(up, down)) * 2.0 / (f[i + 2] - f[i])
    return W


def hann(win):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)


def sizes(sr, nfft, window, hop):
    return int(window * sr), int(hop * sr), nfft // 2 + 1


def frames_of(y, nfft, win, hop):
    """[n_frames, win]: the samples under the window's non-zero taps of every frame of the
    reflect-padded signal (frame f covers padded samples [f hop, f hop + nfft), the window sits
    (nfft - win)//2 taps in)."""
    y = np.asarray(y)
    n = len(y)
    assert n >= nfft // 2 + 1
    lpad = (nfft - win) // 2
    nf = 1 + n // hop
    i = (np.arange(nf) * hop)[:, None] + (lpad + np.arange(win))[None, :] - nfft // 2
    i = np.where(i < 0, -i, i)
    i = np.where(i >= n, 2 * (n - 1) - i, i)
    return y[i]


def dft_basis(nfft, win):
    """(cos, sin) [win, nfft//2 + 1] float64 with the Hann window folded in."""
    lpad = (nfft - win) // 2
    k = np.arange(nfft // 2 + 1)
    t = np.arange(win) + lpad
    ang = 2.0 * np.pi * ((t[:, None] * k[None, :]) % nfft) / nfft
    w = hann(win)[:, None]
    return w * np.cos(ang), w * np.sin(ang)


def spectrum_ref(y, sr=16000, nfft=512, window=0.025, hop=0.01, dtype=np.float64):
    """(re, im) of the STFT, [n_frames, nfft//2 + 1] each, in `dtype`."""
    win, hp_, _ = sizes(sr, nfft, window, hop)
    fr = frames_of(np.asarray(y, dtype=np.float64), nfft, win, hp_).astype(dtype)
    c, s = dft_basis(nfft, win)
    return fr @ c.astype(dtype), fr @ s.astype(dtype)


def power_ref(y, sr=16000, nfft=512, window=0.025, hop=0.01, dtype=np.float64):
    """P [n_frames, nfft//2 + 1] in `dtype`."""
    re, im = spectrum_ref(y, sr, nfft, window, hop, dtype)
    return re * re + im * im


def logmel_ref(y, sr=16000, nfft=512, window=0.025, hop=0.01, nmels=40, dtype=np.float64):
    """log10(P W^T + 1e-6) [n_frames, nmels] (time-major) in `dtype`."""
    P = power_ref(y, sr, nfft, window, hop, dtype)
    W = mel_fb(sr, nfft, nmels).astype(dtype)
    out = np.log10(P @ W.T + dtype(1e-6))
    assert out.dtype == dtype
    return out


def frame_counts(lengths, hop_samples):
    return [1 + n // hop_samples for n in lengths]


def tones(n, seed=0, sr=16000):
    """Two amplitude-modulated tones (220 Hz, 1800 Hz) plus 0.01 white noise, float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    y = (0.5 * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) * np.sin(2 * np.pi * 220.0 * t + rng.uniform(0, 6.28))
         + 0.3 * (1.0 + 0.5 * np.sin(2 * np.pi * 5.0 * t + 1.0)) * np.sin(2 * np.pi * 1800.0 * t + rng.uniform(0, 6.28))
         + 0.01 * rng.standard_normal(n))
    return y.astype(np.float32)


def burst(n=8000, start=3000, length=2000, sr=16000):
    """Silence with a `length`-sample 440 Hz burst: most frames sit on the log10(1e-6) = -6 floor,
    the frames at the burst's edges just above it."""
    y = np.zeros(n, dtype=np.float32)
    t = np.arange(length) / sr
    y[start:start + length] = (0.4 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
    return y


def err_bound(y, factor=6.0, ref_fn=logmel_ref, **cfg):
    """(reference fp64 [n_frames, nmels], bound): bound = factor x the largest error the fp32 CPU
    evaluation of the same definition (ref_fn) makes against fp64 on this input."""
    ref = ref_fn(y, **cfg)
    f32 = ref_fn(y, dtype=np.float32, **cfg)
    return ref, factor * float(np.abs(f32.astype(np.float64) - ref).max())
