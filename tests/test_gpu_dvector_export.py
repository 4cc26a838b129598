"""The corpus d-vector export on the GPU: sv_logmel_ranges, sv_dvector_embed_bf16_frames and
sv_dvec_align against the entry points they extend (bit for bit), and dvector.embed_files /
export_sequences end to end on the small net of tests/test_gpu_logmel.py (40 -> 64 x 3 -> 32,
recipe weights) and the signals of tests/logmel_ref.py.

Bounds: the three kernels are compared with torch.equal / np.array_equal.  embed_files in fp32:
max(1e-6, 6 x what the fp32-CPU log-mel changes through the same embedder) against the fp64 chain
(the rule and floor of test_embed_segments_against_reference_chain) and 1e-5 against per-file
embed_segments (the project's fp32 cross-schedule bound, tests/test_dvector.py); bf16 on every path
5e-3 against the fp32 result (the project's bf16 d-vector bound).

Measured on MI355X (max-abs; files: three segments / one 25-frame range / 3 s):
  logmel_ranges, embed_frames B = 37 and 300, dvec_align P = 32, 256, 6: difference 0
  embed_files f32 vs the fp64 chain 8.57e-8 / 1.19e-7 / 7.26e-8 (bound 1e-6, the floor); vs per-file
  embed_segments 0 / 0 / 0 (bound 1e-5)
  embed_files bf16 vs f32, path dvec = persist = default: 1.12e-3 / 1.38e-3 / 1.04e-3 (bound 5e-3)
The whole file runs in under 3 s.
"""
import os

import numpy as np
import pytest
import torch

import logmel_ref as R
from pytorch_speaker_verification_amd import dvector, features, ops
from test_dvector_export import check_argument_codes
from test_gpu_logmel import _small_net

pytestmark = pytest.mark.gpu

_cache = {}


def _net():
    if "net" not in _cache:
        _cache["net"] = _small_net()
    return _cache["net"]


def _weights(net):
    return net.LSTM_stack.layer_params(), net.projection.weight, net.projection.bias


# ---- 4. sv_logmel_ranges
RANGES = [(1001, 5001),     # starts at an odd sample
          (5001, 9000),     # touches the one before
          (8000, 12000),    # overlaps it
          (20000, 20257),   # exactly nfft / 2 + 1 samples
          (12345, 16185),   # exactly 3840 samples: 25 frames
          (20000, 32000),   # 76 frames: crosses the 64-frame tile boundary together with its neighbours
          (44160, 48000)]   # ends at the buffer's last sample


def test_logmel_ranges_equals_logmel_of_the_slices():
    y = R.tones(48000, seed=3)
    out, frame_off = features.logmel_ranges(y, [(0, a, b) for a, b in RANGES])
    want_off = np.concatenate([[0], np.cumsum([1 + (b - a) // 160 for a, b in RANGES])]).tolist()
    assert frame_off == want_off == [0, 26, 51, 77, 79, 104, 180, 205]  # tile boundaries 64, 128 (inside a range), 192
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == (frame_off[-1], 40)
    for r, (a, b) in enumerate(RANGES):
        single = features.logmel(y[a:b])[0]
        assert torch.equal(out[frame_off[r]:frame_off[r + 1]], single), (r, a, b)
    # two of them alone: the same bits as in the batch
    two, off2 = features.logmel_ranges(y, [(0,) + RANGES[2], (0,) + RANGES[5]])
    assert torch.equal(two[:off2[1]], out[frame_off[2]:frame_off[3]])
    assert torch.equal(two[off2[1]:], out[frame_off[5]:frame_off[6]])
    # a device-resident buffer gives the same bits
    dev_out, _ = features.logmel_ranges(torch.from_numpy(y).cuda(), [(0, a, b) for a, b in RANGES])
    assert torch.equal(dev_out, out)


def test_logmel_ranges_of_two_waveforms():
    y0, y1 = R.tones(48000, seed=3), R.tones(10400, seed=10400)
    ranges = [(0, 1001, 5001), (1, 0, 10400), (1, 77, 5000), (0, 44160, 48000)]
    out, frame_off = features.logmel_ranges([y0, y1], ranges)
    for r, (w, a, b) in enumerate(ranges):
        single = features.logmel((y0, y1)[w][a:b])[0]
        assert torch.equal(out[frame_off[r]:frame_off[r + 1]], single), r
    # the tables that ride along arrive as they were sent
    _, _, (t0, t1) = features.logmel_ranges([y0, y1], ranges, tables=lambda fo: [np.arange(5), np.asarray(fo)])
    assert t0.dtype == torch.int32 and t0.tolist() == [0, 1, 2, 3, 4] and t1.tolist() == frame_off


def test_logmel_ranges_value_errors():
    y = R.tones(48000, seed=3)
    for ranges in ([], [(0, 0, 48001)], [(0, -1, 4000)], [(1, 0, 4000)], [(0, 100, 356)]):
        with pytest.raises(ValueError):
            features.logmel_ranges(y, ranges)
    with pytest.raises(ValueError, match="32-bit"):
        features.range_tables([2 ** 31], [(0, 0, 4000)], 512, 160)


# ---- 5. sv_dvector_embed_bf16_frames
@pytest.mark.parametrize("B,lengths", [(37, (42080, 34400, 5600)),        # 20 + 16 + 1 windows
                                       (300, (195680, 291680, 99680))])   # 100 + 150 + 50: two row tiles of 256
def test_embed_frames_equals_embed_of_materialised_windows(B, lengths):
    net = _net()
    layers, wp, bp = _weights(net)
    out, frame_off = features.logmel([R.tones(n, seed=n) for n in lengths])
    starts, counts = dvector.window_starts(frame_off)
    assert len(starts) == B and len(counts) == 3 and min(counts) >= 1
    assert np.array_equal(np.diff(starts)[:counts[0] - 1], np.full(counts[0] - 1, 12))  # windows overlap by half
    windows = dvector.windows_from_logmel(out, frame_off)
    assert windows.shape == (B, 24, 40)
    ref = ops.embedder_forward_dvec_bf16(windows, layers, wp, bp)
    got = ops.embedder_forward_dvec_bf16_frames(out, torch.from_numpy(starts).to(out.device), layers, wp, bp)
    assert got.shape == (B, 32) and torch.isfinite(got).all()
    print(f"\nMEASURED embed_frames[B={B}] max-abs difference {float((got - ref).abs().max()):.1e} (required 0)")
    assert torch.equal(got, ref)


def test_argument_checks_return_before_any_launch():
    check_argument_codes()


# ---- 6. sv_dvec_align
@pytest.mark.parametrize("P", [32, 256, 6])
def test_dvec_align_equals_align_embeddings(P):
    counts = [1, 2, 3, 4, 7, 40]
    rng = np.random.default_rng(100 + P)
    emb = rng.standard_normal((sum(counts), P)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    base = np.concatenate([[0], np.cumsum(counts)])
    want = np.concatenate([dvector.align_embeddings(emb[a:b]) for a, b in zip(base[:-1], base[1:])])
    part_off = np.asarray([base[f] + a for f, n in enumerate(counts) for a, _ in dvector.partitions(n)] + [base[-1]],
                          dtype=np.int32)
    got = ops.dvec_align(torch.from_numpy(emb).cuda(), torch.from_numpy(part_off).cuda())
    assert got.dtype == torch.float64 and got.shape == want.shape
    got = got.cpu().numpy()
    print(f"\nMEASURED dvec_align[P={P}] max-abs difference {float(np.abs(got - want).max()):.1e} (required 0)")
    assert np.array_equal(got, want)
    # an empty partition gives zeros
    z = ops.dvec_align(torch.from_numpy(emb).cuda(), torch.tensor([0, 3, 3, 5], dtype=torch.int32).cuda()).cpu().numpy()
    assert np.array_equal(z[1], np.zeros(P)) and np.array_equal(z[2], np.average(emb[3:5], axis=0).astype(np.float64))


# ---- 7. embed_files
def _files():
    """(files, the segments of each file): the three-segment file of
    test_embed_segments_against_reference_chain inside one waveform (two of its ranges touch), a
    file with one 25-frame range, a file with no range, a 3 s file."""
    if "files" not in _cache:
        s = [R.tones(n, seed=n) for n in (8000, 16000, 4320)]
        a = np.concatenate([np.zeros(501, np.float32), s[0], s[1], np.zeros(100, np.float32), s[2]])
        ra = [(501, 8501), (8501, 24501), (24601, 28921)]
        b, c, d = R.tones(6000, seed=6000), R.tones(5000, seed=5000), R.tones(48000, seed=7)
        files = [(a, ra), (b, [(101, 3941)]), (c, []), (d, [(0, 48000)])]
        _cache["files"] = files, [[w[x:y] for x, y in r] for w, r in files]
    return _cache["files"]


def _chains(net):
    """Per file the fp64 chain and the fp32-CPU one, computed once (as the existing test does)."""
    if "chains" not in _cache:
        def chain(segs, dtype):
            w = np.concatenate([dvector.window_frames(R.logmel_ref(s, dtype=dtype).astype(np.float32).T) for s in segs])
            return dvector.align_embeddings(dvector.embed_windows(net, w).cpu().numpy())
        _cache["chains"] = [(chain(s, np.float64), chain(s, np.float32)) if s else None for s in _files()[1]]
    return _cache["chains"]


def _f32(net):
    if "f32" not in _cache:
        _cache["f32"] = dvector.embed_files(net, _files()[0], precision="f32")
    return _cache["f32"]


def test_embed_files_f32_against_the_fp64_chain_and_embed_segments():
    net = _net()
    files, segs = _files()
    got = _f32(net)
    assert len(got) == 4 and all(g.dtype == np.float64 for g in got)
    assert got[2].shape == (0, 32)
    n_windows = [11, 1, 0, 24]
    for f, (g, n) in enumerate(zip(got, n_windows)):
        if n:
            assert g.shape == (len(dvector.partitions(n)), 32), f
    for f, ch in enumerate(_chains(net)):
        if ch is None:
            continue
        e64, e32 = ch
        bound = max(1e-6, 6.0 * float(np.abs(e32 - e64).max()))
        err = float(np.abs(got[f] - e64).max())
        per_file = dvector.embed_segments(net, segs[f])
        dev = float(np.abs(got[f] - per_file).max())
        print(f"\nMEASURED embed_files f32 file {f}: vs fp64 chain {err:.2e} bound {bound:.2e}; vs embed_segments {dev:.2e}")
        assert err <= bound, (f, err, bound)
        assert dev <= 1e-5, (f, dev)


@pytest.mark.parametrize("path", ["dvec", "persist", None])
def test_embed_files_bf16_paths(path):
    net = _net()
    ref = _f32(net)
    got = dvector.embed_files(net, _files()[0], precision="bf16", path=path)
    assert [g.shape for g in got] == [r.shape for r in ref] and got[2].shape == (0, 32)
    for f, (g, r) in enumerate(zip(got, ref)):
        if len(r):
            d = float(np.abs(g - r).max())
            print(f"\nMEASURED embed_files bf16 path={path} file {f}: vs f32 {d:.2e} bound 5e-3")
            assert g.dtype == np.float64 and d <= 5e-3, (path, f, d)


def test_embed_files_batches_give_the_same_bits():
    net = _net()
    files = _files()[0]
    one = dvector.embed_files(net, files, precision="f32", schedule="per_step")
    two = dvector.embed_files(net, files, precision="f32", schedule="per_step", max_samples=40000)  # [a, b], [d]
    assert dvector._batches([len(files[i][0]) for i in (0, 1, 3)], 40000) == [[0, 1], [2]]
    for f, (x, y) in enumerate(zip(one, two)):
        assert x.shape == y.shape and np.array_equal(x, y), f


def test_embed_files_argument_errors():
    net = _net()
    with pytest.raises(ValueError, match="precision"):
        dvector.embed_files(net, _files()[0], precision="fp16")
    with pytest.raises(ValueError, match="path"):
        dvector.embed_files(net, _files()[0], precision="f32", path="dvec")
    assert [g.shape for g in dvector.embed_files(net, [_files()[0][2]])] == [(0, 32)]  # nothing to upload at all


# ---- 8. export_sequences
def test_export_sequences_with_the_real_net(tmp_path):
    net = _net()
    speakers = []
    for i in range(12):
        folder = [(R.tones(16000, seed=100 + i), [(0, 16000)])]
        if i % 3 == 0:
            folder.append((R.tones(16000, seed=200 + i), [(160, 15000)]))
        speakers.append(folder)
    speakers[4].append((R.tones(16000, seed=300), []))  # no voice activity: skipped
    flat = [f for folder in speakers for f in folder]
    labels = [str(i) for i, folder in enumerate(speakers) for _ in folder]
    per_file = dvector.embed_files(net, flat)
    tr_s, tr_i, te_s, te_i = dvector.export_sequences(net, speakers, str(tmp_path))
    assert np.array_equal(np.concatenate([tr_s, te_s]), np.concatenate(per_file))
    want_ids = [lab for lab, e in zip(labels, per_file) for _ in range(len(e))]
    assert np.concatenate([tr_i, te_i]).tolist() == want_ids
    assert set(tr_i.tolist()) == {str(i) for i in range(11)} and set(te_i.tolist()) == {"11"}
    assert tr_s.dtype == np.float64 and tr_s.shape[1] == 32 and len(tr_s) == len(tr_i) and len(te_s) == len(te_i)
    for name, arr in (("train_sequence", tr_s), ("train_cluster_id", tr_i), ("test_sequence", te_s),
                      ("test_cluster_id", te_i)):
        assert np.array_equal(np.load(os.path.join(str(tmp_path), name + ".npy")), arr)
