"""The fused log-mel kernel (sv_logmel, features.logmel) and the waveform-to-d-vector chain on the
GPU against the fp64 numpy reference (tests/logmel_ref.py).

The bound of every log-mel comparison is 6 x the largest error that an fp32 CPU evaluation of the
same definition (numpy fp32 matmuls, fp32 power / mel / log10) makes against fp64 on that input
(logmel_ref.err_bound); every output element is compared.

Measured on MI355X (max-abs error of the kernel / bound):
  tones 257 1.37e-6 / 8.19e-6      400 1.42e-6 / 8.47e-6      1234 6.16e-6 / 3.84e-5
  tones 1599 5.12e-6 / 3.21e-5     1600 6.04e-6 / 3.48e-5     10400 7.17e-6 / 4.18e-5
  tones 32000 1.24e-5 / 7.37e-5    burst 8000 2.38e-5 / 1.43e-4
  ragged (scaled segments) 8.5e-7 ... 6.0e-6 / 3.9e-6 ... 3.5e-5
  sr 8000 nfft 256: 6.9e-7 / 5.7e-6, 3.5e-6 / 2.1e-5     nfft 1024: 6.4e-6 / 3.3e-5, 1.7e-5 / 8.8e-5
  nfft 64, 128 mels: 1.8e-6 / 1.1e-5, 5.3e-6 / 3.2e-5    preprocess_utterance 1.05e-5 / 6.27e-5
  embed_segments fp32 8.6e-8 / 1e-6 (the floor; 6 x the fp32-CPU log-mel's effect is below it);
  bf16 vs fp32 1.12e-3 / 5e-3
"""
import numpy as np
import pytest
import torch

import logmel_ref as R
from pytorch_speaker_verification_amd import dvector, features

pytestmark = pytest.mark.gpu

RAGGED = [257, 400, 1234, 1600, 32000]
_cache = {}


def _signal(kind, n):
    return R.burst(n) if kind == "burst" else R.tones(n, seed=n)


def _ref(kind, n, **cfg):
    """(signal, fp64 reference, bound) of a case, computed once."""
    key = (kind, n, tuple(sorted(cfg.items())))
    if key not in _cache:
        y = R.tones(n, seed=n, sr=cfg.get("sr", 16000)) if kind == "tones" else R.burst(n)
        _cache[key] = (y,) + R.err_bound(y, **cfg)
    return _cache[key]


def _check(name, got, ref, bound):
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"\nMEASURED logmel[{name}] max-abs {err:.2e} bound {bound:.2e}")
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("kind,n", [("tones", 257), ("tones", 400), ("tones", 1234), ("tones", 1599), ("tones", 1600),
                                    ("tones", 10400), ("tones", 32000), ("burst", 8000)])
def test_single_segment_against_fp64(kind, n):
    y, ref, bound = _ref(kind, n)
    out, frame_off = features.logmel(y)
    assert frame_off == [0, 1 + n // 160] and out.is_cuda and out.shape == (1 + n // 160, 40)
    got = out.cpu().numpy()
    if kind == "burst":
        assert got.min() < -5.99  # frames of pure silence sit on the floor
    _check(f"{kind}{n}", got, ref, bound)


def test_ragged_batch_is_bit_identical_and_stays_in_bounds():
    """Five segments in one call, neighbours scaled 1e-3 / 1 / 1e-3 ... so a read across a segment
    boundary would show: bit-identical to the five single calls, rows exactly at frame_off, and a
    NaN guard row after n_frames left alone (through the entry point features.logmel uses)."""
    segs = [(_signal("tones", n) * (1e-3 if i % 2 == 0 else 1.0)).astype(np.float32) for i, n in enumerate(RAGGED)]
    out, frame_off = features.logmel(segs)
    assert frame_off == [0, 2, 5, 13, 24, 225] and out.shape == (225, 40)
    singles = [features.logmel(s)[0] for s in segs]
    for s, (a, b) in enumerate(zip(frame_off[:-1], frame_off[1:])):
        assert torch.equal(out[a:b], singles[s]), s
    for s, seg in enumerate(segs):
        ref, bound = R.err_bound(seg)
        _check(f"ragged{s}", out[frame_off[s]:frame_off[s + 1]].cpu().numpy(), ref, bound)
    # the same call into a buffer with a guard row
    dev = out.device
    seg_off, foff = features.segment_offsets(RAGGED, 512, 160)
    y = torch.from_numpy(np.concatenate(segs)).to(dev)
    wbasis, melfb = features.stft_tables(16000, 512, 400, 40, dev)
    guarded = torch.full((226, 40), float("nan"), device=dev)
    features.logmel_into(y, torch.from_numpy(seg_off).to(dev), torch.from_numpy(foff).to(dev), 5, 225, 512, 400, 160,
                         40, wbasis, melfb, guarded)
    assert torch.equal(guarded[:225], out)
    assert torch.isnan(guarded[225]).all()


@pytest.mark.parametrize("cfg,lengths", [
    (dict(sr=8000, nfft=256, window=0.025, hop=0.01, nmels=24), (129, 1000)),   # the issue's case: one mel tile
    (dict(sr=16000, nfft=1024, window=0.05, hop=0.01, nmels=80), (513, 2000)),  # two passes of bins, three mel tiles
    (dict(sr=16000, nfft=64, window=0.004, hop=0.002, nmels=128), (33, 700)),   # one tile of bins, four mel tiles
])
def test_non_default_configuration(cfg, lengths):
    """Sizes hard-coded to the defaults would show here; the three cases take every path the kernel
    selects by size (passes over the bins, mel tiles, a bin tile that is partly or wholly empty)."""
    hop = int(cfg["hop"] * cfg["sr"])
    refs = [_ref("tones", n, **cfg) for n in lengths]
    out, frame_off = features.logmel([r[0] for r in refs], **cfg)
    assert frame_off == [0, 1 + lengths[0] // hop, 2 + lengths[0] // hop + lengths[1] // hop]
    assert out.shape == (frame_off[-1], cfg["nmels"])
    for s, (_, ref, bound) in enumerate(refs):
        _check(f"sr{cfg['sr']}_nfft{cfg['nfft']}_{s}", out[frame_off[s]:frame_off[s + 1]].cpu().numpy(), ref, bound)


def test_device_resident_input_gives_the_same_bits():
    segs = [_signal("tones", n) for n in (1234, 10400)]
    host, foff = features.logmel(segs)
    devi, foff2 = features.logmel([torch.from_numpy(s).cuda() for s in segs])
    assert foff == foff2 and torch.equal(host, devi)
    one = features.logmel(torch.from_numpy(segs[0]).cuda())[0]
    assert torch.equal(one, host[:foff[1]])
    # a lone slice of a larger device tensor, 4 bytes off the allocation's alignment: packed (copied)
    # like every other input instead of being refused with SV_EALIGN
    x_host = _signal("tones", 1235)
    x_dev = torch.from_numpy(x_host).cuda()
    assert x_dev[1:1235].data_ptr() % 16 == 4
    assert torch.equal(features.logmel(x_dev[1:1235])[0], features.logmel(x_host[1:1235])[0])


def _small_net():
    import recipe
    from conftest import model_dims
    from pytorch_speaker_verification_amd.speech_embedder_net import SpeechEmbedder
    dims = (40, 64, 3, 32)
    sd = recipe.make_weights(31, *dims)
    with model_dims(*dims):
        net = SpeechEmbedder()
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(torch.as_tensor(sd[k]))
    return net.cuda()


def test_embed_segments_against_reference_chain():
    """Waveforms to aligned d-vectors: three segments of 0.5 s, 1.0 s and 0.27 s (28 frames: one
    window) against logmel_ref (fp64, cast to fp32) -> window_frames -> embed_windows ->
    align_embeddings.  Bound: 6 x what the fp32-CPU log-mel changes through the same embedder, not
    below 1e-6 (a few fp32 ulps of a unit-norm component).  bf16 within the project's bf16 d-vector
    bound (5e-3) of the fp32 result."""
    net = _small_net()
    segs = [R.tones(n, seed=n) for n in (8000, 16000, 4320)]

    def chain(dtype):
        w = np.concatenate([dvector.window_frames(R.logmel_ref(s, dtype=dtype).astype(np.float32).T) for s in segs])
        return w, dvector.align_embeddings(dvector.embed_windows(net, w).cpu().numpy())

    w64, e64 = chain(np.float64)
    _, e32 = chain(np.float32)
    assert w64.shape == (11, 24, 40)
    bound = max(1e-6, 6.0 * float(np.abs(e32 - e64).max()))
    got = dvector.embed_segments(net, segs)
    assert got.shape == (len(dvector.partitions(11)), 32) and got.dtype == np.float64
    err = float(np.abs(got - e64).max())
    print(f"\nMEASURED embed_segments f32 max-abs {err:.2e} bound {bound:.2e}")
    assert err <= bound, (err, bound)
    g16 = dvector.embed_segments(net, segs, precision="bf16")
    d16 = float(np.abs(g16 - got).max())
    print(f"\nMEASURED embed_segments bf16 vs f32 max-abs {d16:.2e}")
    assert g16.shape == got.shape and d16 <= 5e-3, d16
    # no window at all
    assert dvector.embed_segments(net, [segs[0][:3000]]).shape == (0, 32)


def test_preprocess_utterance_on_the_gpu():
    """A 3 s signal with one interval long enough (> 29200 samples) and one not: two [40, 180]
    arrays, the first and last 180 frames of the kept part's log-mel."""
    utter = R.tones(48000, seed=7)
    specs = features.preprocess_utterance(utter, [(1000, 33000), (35000, 47000)])
    assert len(specs) == 2 and all(s.shape == (40, 180) for s in specs)
    ref, bound = R.err_bound(utter[1000:33000])
    assert ref.shape[0] == 201
    _check("preprocess_first", np.ascontiguousarray(specs[0].T), ref[:180], bound)
    _check("preprocess_last", np.ascontiguousarray(specs[1].T), ref[-180:], bound)
