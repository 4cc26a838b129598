"""The mel-magnitude-in-dB feature (sv_meldb: features.mel_db, mel_db_into, mel_db_fixed) and the
raw-waveform dataset and training path built on it, on the GPU against the fp64 numpy reference
(tests/meldb_ref.py).

The bound of every dB comparison is 6 x the largest error that an fp32 CPU evaluation of the same
definition (numpy fp32 matmuls, fp32 magnitude / mel / log10 / maximum / clip) makes against fp64 on
that input (meldb_ref.err_bound, the yardstick of logmel_ref.err_bound); every output element is
compared, none is exempt.  The outputs span 80 dB (100 dB without a clip) and the bounds are 1e-4 to
2e-3 dB: a power / magnitude mix-up, a wrong clip level or a maximum leaked from a neighbour is off
by whole dB.  Values that the definition fixes exactly (the amin floor, maximum - top_db) are
compared exactly, or within 2 fp32 ulps of 100 where a log10f of another library is involved.
Trim bounds are compared exactly; each case first asserts that its fp64 margin to the trim
threshold is at least 0.01 dB, as test_gpu_split does.

Measured on MI355X (max-abs error of the kernel in dB / bound; the tests print `MEASURED ...`):
  tones 257 2.70e-5 / 1.62e-4      400 1.82e-5 / 1.09e-4      1599 8.90e-5 / 5.34e-4
  tones 1600 5.67e-5 / 3.40e-4     10400 7.24e-5 / 4.57e-4    burst 8000 3.43e-4 / 2.06e-3
  quiet (tones 1600 * 1e-3) 4.22e-5 / 2.39e-4
  ragged (scaled segments) 1.4e-5 ... 5.7e-5 / 8.8e-5 ... 3.4e-4; seg_max in dB 2.6e-8 ... 4.6e-6
  sr 8000 nfft 256: 1.1e-5 / 6.5e-5, 5.3e-5 / 3.2e-4     nfft 1024: 9.5e-5 / 4.0e-4, 1.6e-4 / 1.5e-3
  nfft 64, 128 mels: 2.0e-5 / 1.2e-4, 2.7e-4 / 1.6e-3
  top_db None / amin 1e-3 / top_db 20 on sr 8000: 3.2e-6 ... 5.3e-5 / 1.9e-5 ... 3.2e-4
  valid 1500 of 2000: 9.30e-5 / 5.81e-4      valid 1 of 400: 1.08e-5 / 4.58e-5
  mel_db_fixed 3600: burst 3.43e-4 / 2.06e-3, padded tones 9.46e-5 / 5.45e-4, two 1.34e-5 / 7.05e-5;
  29200: two 3.35e-4 / 2.01e-3
  training step on the dataset's batch against meldb_ref's features: loss 5.1e-7 relative (tol 1e-4),
  parameters 3.0e-8 (tol 2e-5), w and b 0 (tol 1e-5)
"""
import contextlib
import os
import random

import numpy as np
import pytest
import torch

import logmel_ref as R
import meldb_ref as M
import recipe
import split_ref as S
from conftest import golden, model_dims
from pytorch_speaker_verification_amd import data_load, features
from pytorch_speaker_verification_amd.hparam import hparam as hp

pytestmark = pytest.mark.gpu

RAGGED = [257, 400, 1234, 1600, 32000]
FLOOR_TOL = 2e-5  # 2 ulps of 100 in fp32 (7.6e-6 each): 20 * log10f(1e-5f) of two libraries' log10f
_cache = {}


def _ref(key, make, **kw):
    """(signal, fp64 reference, bound) of a case, computed once and left unchanged."""
    k = (key, tuple(sorted(kw.items())))
    if k not in _cache:
        y = make()
        ref, bound = M.err_bound(y, **kw)
        ref.setflags(write=False)
        _cache[k] = (y, ref, bound)
    return _cache[k]


def _check(name, got, ref, bound):
    if torch.is_tensor(got):
        got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"\nMEASURED meldb[{name}] max-abs {err:.2e} dB bound {bound:.2e} span {ref.max() - ref.min():.1f} dB")
    assert err <= bound, (name, err, bound)


def _into(y, starts, valids, lens, amin=1e-5, top_db=80.0, sr=16000, nfft=512, window=0.025, hop=0.01, nmels=40):
    """features.mel_db_into on a device copy of y with the given segment table, into buffers with a
    NaN guard row after n_frames and a guard entry after seg_max[n_seg]: (out, seg_max, frame_off)."""
    win, hop_n = int(window * sr), int(hop * sr)
    dev = torch.device("cuda", torch.cuda.current_device())
    n = len(starts)
    frame_off = np.concatenate([[0], np.cumsum([1 + L // hop_n for L in lens])])
    table = torch.tensor(np.concatenate([starts, valids, lens, frame_off]), dtype=torch.int32, device=dev)
    nf = int(frame_off[-1])
    out = torch.full((nf + 1, nmels), float("nan"), device=dev)
    seg_max = torch.full((n + 1,), float("nan"), device=dev)
    wbasis, melfb = features.stft_tables(sr, nfft, win, nmels, dev)
    features.mel_db_into(torch.as_tensor(y).to(dev), table[:n], table[n:2 * n], table[2 * n:3 * n], table[3 * n:], n,
                         nf, nfft, win, hop_n, nmels, wbasis, melfb, out, seg_max, amin, top_db)
    assert torch.isnan(out[nf]).all() and torch.isnan(seg_max[n])  # the guards are left alone
    return out[:nf], seg_max[:n], [int(v) for v in frame_off]


SINGLE = [("tones", 257), ("tones", 400), ("tones", 1599), ("tones", 1600), ("tones", 10400), ("burst", 8000),
          ("quiet", 1600)]


@pytest.mark.parametrize("kind,n", SINGLE)
def test_single_segment_against_fp64(kind, n):
    """tones: 2 frames (every tap reflected) up to 66 (two workgroups); burst: most elements on the
    clip level maximum - 80; quiet (tones * 1e-3): the amin floor active, the clip inactive."""
    make = {"tones": lambda: R.tones(n, seed=n), "burst": lambda: R.burst(n),
            "quiet": lambda: (R.tones(n, seed=n) * 1e-3).astype(np.float32)}[kind]
    y, ref, bound = _ref((kind, n), make)
    out, frame_off = features.mel_db(y)
    assert frame_off == [0, 1 + n // 160] and out.is_cuda and out.shape == (1 + n // 160, 40)
    got = out.cpu().numpy()
    if kind == "burst":
        assert (ref == ref.max() - 80.0).mean() > 0.8
        assert (got == got.min()).mean() > 0.8 and got.min() == got.max() - np.float32(80.0)  # exactly
    if kind == "quiet":
        assert ref.max() - 80.0 < -100.0 and (ref == ref.min()).mean() > 0.5 and ref.min() == 20.0 * np.log10(1e-5)
        assert abs(float(got.min()) + 100.0) <= FLOOR_TOL and (got == got.min()).mean() > 0.5
    _check(f"{kind}{n}", got, ref, bound)


def test_ragged_batch_is_bit_identical_and_keeps_every_segments_own_maximum():
    """Five segments in one call, scaled 1e-3 / 1 / 1e-3 ... so that loud and quiet segments share
    64-frame tiles: a maximum leaked from a loud neighbour would lift the quiet segment's clip level
    by tens of dB.  Bit-identical to the five single calls, seg_max equal to the singles', every
    segment within its bound of fp64, guards after n_frames and seg_max[n_seg] left alone."""
    segs = [(R.tones(n, seed=n) * (1e-3 if i % 2 == 0 else 1.0)).astype(np.float32) for i, n in enumerate(RAGGED)]
    out, frame_off = features.mel_db(segs)
    assert frame_off == [0, 2, 5, 13, 24, 225] and out.shape == (225, 40)
    singles = [features.mel_db(s)[0] for s in segs]
    for s, (a, b) in enumerate(zip(frame_off[:-1], frame_off[1:])):
        assert torch.equal(out[a:b], singles[s]), s
    seg_off = np.concatenate([[0], np.cumsum(RAGGED)])
    guarded, seg_max, foff = _into(np.concatenate(segs), seg_off[:-1], RAGGED, RAGGED)
    assert foff == frame_off and torch.equal(guarded, out)
    for s, seg in enumerate(segs):
        ref, bound = M.err_bound(seg)
        _check(f"ragged{s}", out[frame_off[s]:frame_off[s + 1]], ref, bound)
        one_out, one_max, _ = _into(seg, [0], [len(seg)], [len(seg)])
        assert torch.equal(one_out, singles[s]) and torch.equal(one_max, seg_max[s:s + 1]), s
        # seg_max is the raw maximum: its dB is the reference's largest element, within the same bound
        x = M.mel_mag_ref(seg)
        err = abs(20.0 * np.log10(max(float(seg_max[s]), 1e-5)) - 20.0 * np.log10(max(x.max(), 1e-5)))
        print(f"\nMEASURED meldb[ragged{s} seg_max] {float(seg_max[s]):.6e} fp64 {x.max():.6e} dB error {err:.2e}")
        assert err <= bound, (s, err, bound)
    assert float(seg_max[1]) > 500.0 * float(seg_max[0])  # loud next to quiet


CONFIGS = [
    (dict(sr=8000, nfft=256, window=0.025, hop=0.01, nmels=24), (129, 1000)),   # one pass, one mel tile
    (dict(sr=16000, nfft=1024, window=0.05, hop=0.01, nmels=80), (513, 2000)),  # two passes of bins, three mel tiles
    (dict(sr=16000, nfft=64, window=0.004, hop=0.002, nmels=128), (33, 700)),   # one tile of bins, four mel tiles
]


@pytest.mark.parametrize("cfg,lengths", CONFIGS)
def test_non_default_configuration(cfg, lengths):
    """The three configurations of test_gpu_logmel.test_non_default_configuration: every path the
    kernel selects by size (passes over the bins, 1 / 3 / 4 mel tiles, partly empty bin tiles)."""
    hop = int(cfg["hop"] * cfg["sr"])
    refs = [_ref(("tones", n), lambda n=n: R.tones(n, seed=n, sr=cfg["sr"]), **cfg) for n in lengths]
    out, frame_off = features.mel_db([r[0] for r in refs], **cfg)
    assert frame_off == [0, 1 + lengths[0] // hop, 2 + lengths[0] // hop + lengths[1] // hop]
    assert out.shape == (frame_off[-1], cfg["nmels"])
    for s, (_, ref, bound) in enumerate(refs):
        _check(f"sr{cfg['sr']}_nfft{cfg['nfft']}_{s}", out[frame_off[s]:frame_off[s + 1]], ref, bound)


def test_no_clip_and_another_amin():
    """top_db=None skips the clip kernel; amin = 1e-3 moves the floor to -60 dB (on the first of
    the non-default configurations, a quiet and a loud segment)."""
    cfg, lengths = CONFIGS[0]
    segs = [(R.tones(n, seed=n, sr=cfg["sr"]) * sc).astype(np.float32) for n, sc in zip(lengths, (1e-3, 1.0))]
    for kw in (dict(top_db=None), dict(amin=1e-3), dict(amin=1e-3, top_db=None), dict(top_db=20.0)):
        out, frame_off = features.mel_db(segs, **cfg, **kw)
        for s, seg in enumerate(segs):
            ref, bound = M.err_bound(seg, **cfg, **kw)
            _check(f"sr8000_{s}_{sorted(kw.items())}", out[frame_off[s]:frame_off[s + 1]], ref, bound)
    raw = features.mel_db(segs[0], **cfg, top_db=None)[0].cpu().numpy()
    assert raw.max() - raw.min() > 25.0  # nothing clipped the quiet segment at its own maximum - 20 ...
    assert features.mel_db(segs[0], **cfg, top_db=20.0)[0].min() == raw.max() - np.float32(20.0)  # ... until asked


def test_virtual_segments_read_the_buffer_in_place():
    """valid = L inside a longer buffer, at a start off every alignment, and two segments that
    overlap in y: bit-identical to mel_db of the slices."""
    y = R.tones(6000, seed=6)
    out, seg_max, foff = _into(y, [1001, 0, 1000], [2000, 2000, 2000], [2000, 2000, 2000])
    assert foff == [0, 13, 26, 39]
    for s, a in enumerate((1001, 0, 1000)):
        assert torch.equal(out[foff[s]:foff[s + 1]], features.mel_db(y[a:a + 2000])[0]), s


def test_virtual_segments_pad_with_zeros():
    """valid < L: against fp64 of the zero-padded slice; the last frame's end reflection lands in
    the zeros, and the frames wholly in the padding sit exactly on the clip level maximum - 80.
    valid = 1: one real sample.  valid = 0 at the buffer's last sample: all floor, seg_max 0."""
    y = R.tones(6000, seed=6)
    out, seg_max, foff = _into(y, [1003, 5, 5999, 1003], [1500, 1, 0, 0], [2000, 400, 400, 2000])
    assert foff == [0, 13, 16, 19, 32]
    got = out.cpu().numpy()
    z = np.concatenate([y[1003:2503], np.zeros(500, np.float32)])
    ref, bound = M.err_bound(z)
    _check("valid1500of2000", got[0:13], ref, bound)
    assert (ref[11:13] == ref.max() - 80.0).all()  # frames 11 and 12 see padding only (taps 1560 .. 2119)
    assert (got[11:13] == got[0:13].max() - np.float32(80.0)).all()
    z = np.zeros(400, np.float32)
    z[0] = y[5]
    ref, bound = M.err_bound(z)
    _check("valid1of400", got[13:16], ref, bound)
    for a, b in ((16, 19), (19, 32)):
        assert (got[a:b] == got[16, 0]).all() and abs(float(got[16, 0]) + 100.0) <= FLOOR_TOL
    assert seg_max.tolist()[2:] == [0.0, 0.0] and float(seg_max[0]) > 1.0


def test_sv_meldb_replays_from_a_graph():
    """No host synchronisation and no allocation in the entry point: its three launches (zeroing of
    seg_max, the fused kernel, the clip) are captured once and replayed on new samples in the same
    buffer; seg_max is zeroed again by every replay (a maximum kept from the louder first signal
    would lift the second one's clip level)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    loud, quiet = R.tones(4000, seed=1), (R.tones(4000, seed=2) * 1e-2).astype(np.float32)
    y = torch.from_numpy(loud).to(dev)
    table = torch.tensor([0, 1000, 4000, 2500, 4000, 2500, 0, 26, 42], dtype=torch.int32, device=dev)
    wbasis, melfb = features.stft_tables(16000, 512, 400, 40, dev)
    out = torch.empty((42, 40), device=dev)
    seg_max = torch.empty(2, device=dev)

    def call():
        features.mel_db_into(y, table[0:2], table[2:4], table[4:6], table[6:9], 2, 42, 512, 400, 160, 40, wbasis, melfb,
                             out, seg_max)

    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for sig in (quiet, loud):
        y.copy_(torch.from_numpy(sig))
        graph.replay()
        assert torch.equal(out[:26], features.mel_db(sig)[0])
        assert torch.equal(out[26:], features.mel_db(sig[1000:3500])[0])


def _padded_tones():
    return np.concatenate([np.zeros(1000, np.float32), R.tones(3000, seed=3000), np.zeros(1500, np.float32)])


FIXED = [("burst", lambda: R.burst(8000), (2880, 5280)), ("padded", _padded_tones, (960, 4320)),
         ("two", lambda: S.signal("two"), (0, 48000))]


def test_mel_db_fixed_against_reference():
    """trim -> fix_length -> mel_db at L = 3600 (23 frames): burst and the padded tones are trimmed
    and zero-padded, `two` is not trimmed and is truncated; and `two` at the reference's 29200 (183
    frames).  The batched call equals the single calls bit for bit."""
    waves = []
    for name, make, want in FIXED:
        y = make()
        assert S.margin(S.mse_ref(y, 400, 160), 60) >= 0.01  # (on the CPU, before anything is compared)
        assert S.trim_ref(y, 60, 400, 160) == want
        waves.append(y)
    assert features.fixed_length() == 29200
    out = features.mel_db_fixed(waves, length=3600)
    assert out.is_cuda and out.shape == (3, 23, 40) and out.dtype == torch.float32 and out.is_contiguous()
    for s, (name, _, (a, b)) in enumerate(FIXED):
        z = M.fix_length(waves[s][a:b], 3600)
        ref, bound = M.err_bound(z)
        np.testing.assert_array_equal(ref, M.fixed_ref(waves[s], 3600))
        _check(f"fixed3600_{name}", out[s], ref, bound)
        assert torch.equal(features.mel_db_fixed(waves[s], length=3600)[0], out[s]), name
    # device-resident waveforms: the same bits
    assert torch.equal(features.mel_db_fixed([torch.from_numpy(w).cuda() for w in waves], length=3600), out)
    # no trim: the leading silence stays
    ref, bound = M.err_bound(waves[1][:3600])
    _check("fixed3600_padded_notrim", features.mel_db_fixed(waves[1], length=3600, trim_top_db=None)[0], ref, bound)
    long = features.mel_db_fixed([waves[2]])
    assert long.shape == (1, 183, 40)
    ref, bound = M.err_bound(waves[2][:29200])
    _check("fixed29200_two", long[0], ref, bound)


@contextlib.contextmanager
def _small_hp(tmp_path=None):
    """tisv_frame 20 (3600 samples, 23 frames), model 40/64/3/32, N = M = 2, one epoch."""
    keys = [(hp.data, "tisv_frame", 20), (hp.train, "N", 2), (hp.train, "M", 2), (hp.train, "epochs", 1),
            (hp.train, "log_interval", 1), (hp.train, "log_file", None), (hp.train, "checkpoint_interval", 1),
            (hp.train, "restore", False), (hp, "training", True), (hp, "device", "cuda"),
            (hp.train, "checkpoint_dir", str(tmp_path) if tmp_path is not None else hp.train.checkpoint_dir)]
    old = [getattr(o, k) for o, k, _ in keys]
    for o, k, v in keys:
        setattr(o, k, v)
    try:
        with model_dims(40, 64, 3, 32):
            yield
    finally:
        for (o, k, _), v in zip(keys, old):
            setattr(o, k, v)


def _speakers():
    """4 speakers x 3 utterances: 800 zeros, tones(4000) of a seed of its own, 600 zeros (trimmed to
    (640, 5120), then cut to 3600)."""
    return [[np.concatenate([np.zeros(800, np.float32), R.tones(4000, seed=10 * s + u), np.zeros(600, np.float32)])
             for u in range(3)] for s in range(4)]


def _replay(seed, items, counts, m):
    """(speaker, utterances) of SpeakerDatasetWaveforms items under random.seed(seed)."""
    random.seed(seed)
    order = list(range(len(counts)))
    random.shuffle(order)
    picks = []
    for i in items:
        utts = list(range(counts[order[i]]))
        random.shuffle(utts)
        picks.append((order[i], utts[:m]))
    return picks


def test_dataset_item_is_mel_db_fixed_of_the_replayed_choice():
    speakers = _speakers()
    with _small_hp():
        picks = _replay(5, (1, 3), [3] * 4, 2)
        random.seed(5)
        ds = data_load.SpeakerDatasetWaveforms(speakers)
        assert ds.utterance_number == 2 and len(ds) == 4
        for i, (spk, utts) in zip((1, 3), picks):
            item = ds[i]
            assert item.is_cuda and item.shape == (2, 23, 40)
            assert torch.equal(item, features.mel_db_fixed([speakers[spk][u] for u in utts]))


def test_training_on_waveforms(tmp_path, capsys):
    """train(..., dataset=ds) for one epoch of two batches: finite losses and a checkpoint with the
    reference's keys; and one GE2ETrainer.step on the dataset's batch against a step on meldb_ref's
    features cast to fp32, within the model tests' tolerances for these dimensions
    (test_gpu_model.test_small_net_fused_trainer_matches_reference: loss 1e-4 relative, parameters
    2e-5, w and b 1e-5)."""
    from pytorch_speaker_verification_amd import train_speech_embedder as tse
    from pytorch_speaker_verification_amd.speech_embedder_net import GE2ELoss, SpeechEmbedder
    from pytorch_speaker_verification_amd.trainer import GE2ETrainer
    speakers = _speakers()
    with _small_hp(tmp_path):
        random.seed(11)
        torch.manual_seed(11)
        ds = data_load.SpeakerDatasetWaveforms(speakers)
        path = tse.train(str(tmp_path / "none.model"), dataset=ds)
        lines = [ln for ln in capsys.readouterr().out.splitlines() if "Loss:" in ln]
        losses = [float(ln.split("\tLoss:")[1].split("\t")[0]) for ln in lines]
        print(f"\nMEASURED train_on_waveforms losses {losses}")
        assert len(losses) == 2 and np.isfinite(losses).all()
        sd = torch.load(path, weights_only=True)
        assert list(sd.keys()) == list(golden("init_seed1234.npz").files)
        assert os.path.exists(tmp_path / "ckpt_epoch_1_batch_id_2.pth")
        assert all(torch.isfinite(v).all() for v in sd.values())

        # one step, on the dataset's features and on the reference's
        picks = _replay(23, (0, 2), [3] * 4, 2)
        random.seed(23)
        ds = data_load.SpeakerDatasetWaveforms(speakers)
        x_gpu = torch.cat([ds[0], ds[2]])
        for spk, utts in picks:
            for u in utts:
                assert S.margin(S.mse_ref(speakers[spk][u], 400, 160), 60) >= 0.01
        x_ref = np.stack([M.fixed_ref(speakers[spk][u], 3600).astype(np.float32) for spk, utts in picks for u in utts])
        assert x_gpu.shape == x_ref.shape == (4, 23, 40)
        w0 = recipe.make_weights(31, 40, 64, 3, 32)
        res = []
        for x in (x_gpu, torch.from_numpy(x_ref).cuda()):
            net = SpeechEmbedder()
            with torch.no_grad():
                for k, v in net.state_dict().items():
                    v.copy_(torch.as_tensor(w0[k]))
            net = net.cuda()
            ge2e = GE2ELoss("cuda")
            loss = float(GE2ETrainer(net, ge2e, lr=0.01).step(x, 2, 2))
            res.append((loss, {k: v.cpu().numpy() for k, v in net.state_dict().items()}, ge2e.w.item(), ge2e.b.item()))
    (la, pa, wa, ba), (lb, pb, wb, bb) = res
    perr = max(float(np.abs(pa[k] - pb[k]).max()) for k in pa)
    print(f"\nMEASURED train_on_waveforms step loss {la:.6f} ref {lb:.6f} rel {abs(la - lb) / abs(lb):.2e} "
          f"params max-abs {perr:.2e} w {abs(wa - wb):.2e} b {abs(ba - bb):.2e}")
    assert np.isfinite(la) and abs(la - lb) <= 1e-4 * abs(lb)
    assert perr <= 2e-5 and abs(wa - wb) <= 1e-5 and abs(ba - bb) <= 1e-5
