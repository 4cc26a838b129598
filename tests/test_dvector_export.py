"""The host half of the corpus d-vector export (dvector.vad_frame_count / vad_times /
voiced_ranges / window_starts / export_sequences): the reference's VAD bookkeeping against
tests/golden/vad_chunk.npz, which tests/golden/make_dvector_golden.py recorded from the reference's
own VAD_segments.VAD_chunk on scripted per-frame decisions, and the export's split and labels with
a stub in place of the embedder.  No GPU."""
import os

import numpy as np
import pytest

from conftest import golden
from pytorch_speaker_verification_amd import dvector

SCRIPTS = ["none", "to_end", "short10", "short11", "touching", "between", "flips"]


def test_fixture_holds_the_cases():
    g = golden("vad_chunk.npz")
    assert sorted(g["names"].tolist()) == sorted(SCRIPTS)
    assert g["none_times"].shape == (0, 2)
    t = g["touching_times"]
    assert any(t[i, 1] == t[i + 1, 0] for i in range(len(t) - 1))
    assert int(g["flips_n"]) % 320 != 0 and g["short11_lens"][-1] < 6400


@pytest.mark.parametrize("name", SCRIPTS)
def test_vad_times_and_ranges_against_the_reference(name):
    g = golden("vad_chunk.npz")
    flags, n, ref_times, lens = g[name + "_flags"], int(g[name + "_n"]), g[name + "_times"], g[name + "_lens"]
    assert dvector.vad_frame_count(n, sr=16000) == len(flags)
    times = dvector.vad_times(flags, sr=16000)
    assert len(times) == len(ref_times)
    assert all(a == ra and b == rb for (a, b), (ra, rb) in zip(times, ref_times)), (times, ref_times)  # exactly
    if name == "none":
        assert times == [] and dvector.voiced_ranges(times, n, sr=16000) == []
        return
    # concat_segs joins chunk i + 1 to chunk i where the times meet: the joined lengths, in order
    joined = [int(lens[0])]
    for i in range(len(ref_times) - 1):
        if ref_times[i, 1] == ref_times[i + 1, 0]:
            joined[-1] += int(lens[i + 1])
        else:
            joined.append(int(lens[i + 1]))
    y = np.zeros(n, dtype=np.float32)
    ranges = dvector.voiced_ranges(times, n, sr=16000)
    assert min(joined) >= 3840  # (none of the fixture's segments is too short for a window)
    assert [len(y[a:b]) for a, b in ranges] == joined
    assert all(0 <= a < b <= n for a, b in ranges)


def test_voiced_ranges_drops_what_holds_no_window_and_clamps():
    # 25 frames (3840 samples) is the shortest range with a window; a slice past the end is clamped
    assert dvector.voiced_ranges([(0.0, 0.23)], 16000, sr=16000) == []
    assert dvector.voiced_ranges([(0.0, 0.24)], 16000, sr=16000) == [(0, 3840)]
    assert dvector.voiced_ranges([(0.1, 0.5), (0.5, 0.52), (0.6, 0.7), (0.7, 1.1)], 16000, sr=16000) == \
        [(1600, 8320), (9600, 16000)]
    assert dvector.voiced_ranges([(0.5, 0.9), (0.9, 1.3)], 17000, sr=16000) == [(8000, 17000)]
    assert dvector.voiced_ranges([(0.5, 0.9)], 10000, sr=16000) == []  # 2000 samples are left


def test_vad_frame_count_is_strict():
    # frame_generator: frames of n = 640 bytes while offset + n < 2 * n_samples
    for n_samples in (0, 1, 319, 320, 321, 640, 641, 16000, 112123):
        want, offset = 0, 0
        while offset + 640 < 2 * n_samples:
            want, offset = want + 1, offset + 640
        assert dvector.vad_frame_count(n_samples, sr=16000) == want, n_samples
    assert dvector.vad_frame_count(8000, sr=8000, frame_ms=10) == 99


@pytest.mark.parametrize("T", [24, 25, 36, 37, 200])
def test_window_starts_matches_window_index(T):
    frame_off = [0, T, T + 7, 2 * T + 7, 2 * T + 107]
    starts, counts = dvector.window_starts(frame_off)
    assert starts.dtype == np.int32
    # the literal loop of dvector_create.py:49-50 (window_index is built on window_starts now)
    want = [a + j for a, b in zip(frame_off[:-1], frame_off[1:]) for j in range(0, b - a, dvector.HOP)
            if j + dvector.WIN < b - a]
    assert np.array_equal(starts, np.asarray(want, dtype=np.int64))
    idx = dvector.window_index(frame_off)
    assert idx.dtype == np.int64 and np.array_equal(idx, np.asarray(want)[:, None] + np.arange(dvector.WIN)[None, :])
    for (a, b), c in zip(zip(frame_off[:-1], frame_off[1:]), counts):
        assert c == dvector.window_frames(np.zeros((40, b - a), dtype=np.float32)).shape[0]
    assert sum(counts) == len(starts)


def _stub(monkeypatch, proj=4):
    """embed_files replaced by a function of the file alone: a file (tag, n) gives n rows of tag."""
    calls = []

    def fake(net, files, **kw):
        calls.append((len(files), kw))
        return [np.full((n, proj), float(tag)) for tag, n in files]

    monkeypatch.setattr(dvector, "embed_files", fake)
    return calls


def test_export_sequences_split_labels_and_files(monkeypatch, tmp_path):
    calls = _stub(monkeypatch)
    # 12 folders: (12 // 10) * 9 = 9, the train part closes after folder 10; folder 11 is the test part
    speakers = [[(10 * i, 2), (10 * i + 1, 1)] for i in range(12)]
    speakers[3] = [(30, 0), (31, 3)]  # a file without voiced audio is skipped
    speakers[5] = []                  # a folder without a file still takes its label
    out = tmp_path / "seq"
    tr_s, tr_i, te_s, te_i = dvector.export_sequences(None, speakers, str(out), precision="f32")
    assert calls == [(22, {"precision": "f32"})]  # all folders in one embed_files call
    assert sorted(os.listdir(out)) == ["test_cluster_id.npy", "test_sequence.npy", "train_cluster_id.npy",
                                       "train_sequence.npy"]
    want_ids = [str(i) for i in range(11) if i != 5 for _ in range(3)]
    assert tr_i.tolist() == want_ids and "5" not in tr_i.tolist() and te_i.tolist() == ["11"] * 3
    assert tr_s.shape == (30, 4) and tr_s.dtype == np.float64 and te_s.shape == (3, 4) and te_s.dtype == np.float64
    assert tr_s[:, 0].tolist()[:12] == [0, 0, 1, 10, 10, 11, 20, 20, 21, 31, 31, 31]
    assert te_s[:, 0].tolist() == [110, 110, 111]
    for name, arr in (("train_sequence", tr_s), ("train_cluster_id", tr_i), ("test_sequence", te_s),
                      ("test_cluster_id", te_i)):
        saved = np.load(out / (name + ".npy"))
        assert saved.dtype == arr.dtype and np.array_equal(saved, arr)
    assert tr_i.dtype.kind == "U" and tr_i.shape == (30,)


def test_export_sequences_empty_part_writes_nothing(monkeypatch, tmp_path):
    _stub(monkeypatch)
    speakers = [[(i, 1)] for i in range(12)]
    speakers[11] = [(11, 0)]  # the only test folder has no voiced audio
    with pytest.raises(ValueError, match="test"):
        dvector.export_sequences(None, speakers, str(tmp_path / "a"))
    assert not (tmp_path / "a").exists()
    speakers = [[(i, 0)] for i in range(11)] + [[(11, 2)]]
    with pytest.raises(ValueError, match="train"):
        dvector.export_sequences(None, speakers, str(tmp_path / "b"))
    assert not (tmp_path / "b").exists()
    with pytest.raises(ValueError, match="train"):
        dvector.export_sequences(None, [[(0, 2)]], str(tmp_path / "c"))  # the train part is never closed
    assert not (tmp_path / "c").exists()
    # the smallest corpus the reference's loop splits: 3 folders, closed after folder 1
    tr_s, tr_i, te_s, te_i = dvector.export_sequences(None, [[(i, 1)] for i in range(3)], str(tmp_path / "d"))
    assert tr_i.tolist() == ["0", "1"] and te_i.tolist() == ["2"]


def check_argument_codes():
    """The three entry points' argument checks as return codes -- SV_EARG -1, SV_EALIGN -2,
    SV_ESHAPE -3 -- all host-side and before any launch (the pointers are never dereferenced)."""
    from pytorch_speaker_verification_amd import _lib
    h = _lib.lib()
    p = 4096  # a 256-byte aligned, non-null address

    def lm(y=p, start=p, length=p, fo=p, n_seg=1, n_frames=4, nfft=512, win=400, hop=160, nmels=40, wb=p, ld=516,
           mel=p, out=p):
        return h.sv_logmel_ranges(y, start, length, fo, n_seg, n_frames, nfft, win, hop, nmels, wb, ld, mel, out, None,
                                  None)

    assert lm(y=None) == -1 and lm(start=None) == -1 and lm(length=None) == -1 and lm(fo=None) == -1
    assert lm(out=None) == -1 and lm(n_seg=0) == -1 and lm(n_seg=5) == -1 and lm(ld=512) == -1
    assert lm(y=p + 4) == -2 and lm(out=p + 8) == -2 and lm(start=p + 2) == -2 and lm(length=p + 1) == -2
    assert lm(fo=p + 2) == -2 and lm(ld=518) == -2
    assert lm(nfft=511) == -3 and lm(nfft=2048) == -3 and lm(win=513) == -3 and lm(hop=0) == -3 and lm(nmels=129) == -3

    def dv(frames=p, n_rows=100, ws=p, B=37, T=24, F=40, H=64, work=p, emb=p):
        return h.sv_dvector_embed_bf16_frames(B, T, F, H, 3, frames, n_rows, ws, p, p, p, p, p, p, 32, emb, work, None)

    assert dv(frames=None) == -1 and dv(ws=None) == -1 and dv(n_rows=0) == -1 and dv(B=0) == -1 and dv(F=65) == -1
    assert dv(H=100) == -1 and dv(work=None) == -1 and dv(emb=None) == -1
    assert dv(frames=p + 4) == -2 and dv(ws=p + 2) == -2 and dv(work=p + 128) == -2

    def al(emb=p, S=10, P=32, po=p, n_parts=3, out=p):
        return h.sv_dvec_align(emb, S, P, po, n_parts, out, None)

    assert al(emb=None) == -1 and al(po=None) == -1 and al(out=None) == -1
    assert al(S=0) == -1 and al(P=0) == -1 and al(n_parts=0) == -1
    assert al(emb=p + 4) == -2 and al(out=p + 8) == -2 and al(po=p + 2) == -2


def test_argument_checks_return_before_any_launch():
    check_argument_codes()


def test_logmel_ranges_refuses_bad_ranges_on_the_host():
    """ValueError before any upload (no GPU is touched: this test has none)."""
    from pytorch_speaker_verification_amd import features
    y = np.zeros(48000, dtype=np.float32)
    for ranges in ([], [(0, 0, 48001)], [(0, -1, 4000)], [(0, 5000, 4000)], [(1, 0, 4000)], [(-1, 0, 4000)],
                   [(0, 100, 356)], [(0, 0, 4000), (0, 47800, 48000)]):
        with pytest.raises(ValueError):
            features.logmel_ranges(y, ranges)
    with pytest.raises(ValueError, match="1-D"):
        features.logmel_ranges(np.zeros((2, 4000), dtype=np.float32), [(0, 0, 4000)])
    with pytest.raises(ValueError, match="32-bit"):
        features.range_tables([2 ** 31], [(0, 0, 4000)], 512, 160)
    with pytest.raises(ValueError, match="32-bit"):
        features.range_tables([2 ** 30] * 3, [(0, 0, 4000)], 512, 160)
    start, length, frame_off = features.range_tables([1000, 5000], [(1, 3, 4003), (0, 0, 257)], 512, 160)
    assert start.tolist() == [1003, 0] and length.tolist() == [4000, 257] and frame_off.tolist() == [0, 26, 28]
    assert start.dtype == length.dtype == frame_off.dtype == np.int32
