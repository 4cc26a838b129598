"""Host-side checks of the energy-based splitting (no GPU): the fp64 reference helper
(tests/split_ref.py) against known answers, the host half of features.split / trim against the
helper, the argument checks of sv_frame_energy, and the bookkeeping of preprocess_speaker and
save_speakers on CPU stubs."""
import os

import numpy as np
import pytest
import torch

import logmel_ref as R
import split_ref as S
from pytorch_speaker_verification_amd import features


@pytest.mark.parametrize("name,fl,hop,top_db,want", S.KNOWN, ids=S.KNOWN_IDS)
def test_reference_known_answers(name, fl, hop, top_db, want):
    y = S.signal(name)
    got = S.split_ref(y, top_db, fl, hop)
    assert got.dtype == np.int64 and got.shape == (len(want), 2)
    assert got.tolist() == want


def test_reference_margins_and_frame_counts():
    """The plateau case pins the threshold to 0.026 dB from either side; `two` is 12 dB clear;
    `long` has 313 frames, all at least 10 dB from the threshold; without the amin floor the gaps
    of `quiet` would sit below -70 dB, under top_db = 60."""
    assert abs(S.margin(S.mse_of("plateaus"), 30) - 0.026) < 1e-3
    db = S.db_ref(S.mse_of("plateaus"))
    assert db[18] < -30 < db[42]  # the middles of the 0.997 q and 1.003 q plateaus
    assert 12.0 <= S.margin(S.mse_of("two"), 30) < 12.1
    assert len(S.mse_of("long")) == 313 and S.margin(S.mse_of("long"), 30) >= 10.0
    m = S.mse_of("quiet")
    raw = 10 * np.log10(m) - 10 * np.log10(m.max())
    assert raw.min() < -70 and S.db_ref(m).min() > -60
    assert len(S.mse_ref(np.zeros(1025), 2048, 512)) == 3
    assert len(S.mse_ref(np.zeros(1535), 2048, 512)) == 3 and len(S.mse_ref(np.zeros(1536), 2048, 512)) == 4


@pytest.mark.parametrize("name,fl,hop,top_db,want", S.KNOWN, ids=S.KNOWN_IDS)
def test_host_half_of_split_equals_reference(name, fl, hop, top_db, want):
    """features.intervals_from_energy on the helper's own mse rounded to fp32."""
    mse = S.mse_of(name, fl, hop).astype(np.float32)
    got = features.intervals_from_energy(mse, len(S.signal(name)), hop, top_db)
    assert got.dtype == np.int64 and got.shape == (len(want), 2)
    assert got.tolist() == want


def test_host_half_edge_patterns():
    """Edges at index 0 and F, single frames, and the strict comparison at exactly -top_db."""
    f = features.intervals_from_energy
    assert f(np.array([1, 1e-9, 1, 1, 1e-9, 1e-9, 1]), 3100, 512, 30).tolist() == [[0, 512], [1024, 2048], [3072, 3100]]
    assert f(np.array([1e-9, 1, 1e-9]), 1100, 512, 30).tolist() == [[512, 1024]]
    assert f(np.array([1.0, 1e-3, 1.0]), 1100, 512, 30).tolist() == [[0, 512], [1024, 1100]]  # -30 dB is not > -30
    assert f(np.array([1.0, 1.0001e-3, 1.0]), 1100, 512, 30).tolist() == [[0, 1100]]
    assert f(np.zeros(6), 3000, 512, 60).tolist() == [[0, 3000]]  # db = 0 everywhere: librosa's behaviour


@pytest.fixture
def cpu_energy(monkeypatch):
    """features.frame_energy replaced by the fp64 helper rounded to fp32 (a CPU tensor)."""
    calls = []

    def stub(waves, frame_length=2048, hop_length=512):
        calls.append(len(waves))
        ms = [S.mse_ref(np.asarray(w), frame_length, hop_length).astype(np.float32) for w in waves]
        return torch.from_numpy(np.concatenate(ms)), np.concatenate([[0], np.cumsum([len(m) for m in ms])]).tolist()

    monkeypatch.setattr(features, "frame_energy", stub)
    return calls


def test_split_single_and_list(cpu_energy):
    names = ["quiet", "burst", "zeros", "two"]
    got = features.split([S.signal(n) for n in names], top_db=30)
    assert cpu_energy == [4]  # one energy call for the whole list
    assert isinstance(got, list) and len(got) == 4
    for n, g in zip(names, got):
        assert g.tolist() == S.split_ref(S.signal(n), 30).tolist(), n
    one = features.split(S.signal("two"), top_db=30, frame_length=400, hop_length=160)
    assert isinstance(one, np.ndarray) and one.tolist() == [[4800, 38240], [40800, 46240]]


def test_trim(cpu_energy, monkeypatch):
    two = S.signal("two")
    y, (start, end) = features.trim(two, top_db=30, frame_length=400, hop_length=160)
    assert (start, end) == (4800, 46240) == S.trim_ref(two, 30, 400, 160)
    np.testing.assert_array_equal(y, two[4800:46240])
    # the loudest frame is at 0 dB, so some frame is non-silent for every top_db > 0: (0, 0) cannot
    # be reached through the energy; only the branch itself is exercised
    for name in ("zeros", "quiet", "plateaus"):
        assert len(features.split(S.signal(name), top_db=1e-9)) >= 1
    monkeypatch.setattr(features, "split", lambda *a, **k: np.zeros((0, 2), dtype=np.int64))
    y, idx = features.trim(two)
    assert idx == (0, 0) and len(y) == 0


def test_short_and_2d_inputs_raise_before_any_device(monkeypatch):
    from pytorch_speaker_verification_amd import _lib

    def no_device(t):
        raise AssertionError("a device was looked for")

    monkeypatch.setattr(_lib, "compute_device", no_device)
    with pytest.raises(ValueError):
        features.frame_energy(np.zeros(1024, np.float32))  # needs 1025
    with pytest.raises(ValueError):
        features.split([np.zeros(4000, np.float32), np.zeros(200, np.float32)], frame_length=400, hop_length=160)
    with pytest.raises(ValueError):
        features.split(np.zeros((2, 4000), np.float32))
    with pytest.raises(ValueError):
        features.trim(np.zeros(1000, np.float32))
    with pytest.raises(ValueError):
        features.preprocess_speaker([np.zeros((2, 40000), np.float32)])
    with pytest.raises(ValueError):
        features.frame_energy(np.zeros(4000, np.float32), frame_length=401)
    with pytest.raises(ValueError):
        features.frame_energy(np.zeros(4000, np.float32), hop_length=0)
    seg_off, frame_off = features.energy_offsets([1025, 1535, 1536, 8000], 2048, 512)
    assert seg_off.tolist() == [0, 1025, 2560, 4096, 12096] and frame_off.tolist() == [0, 3, 6, 10, 26]
    assert seg_off.dtype == frame_off.dtype == np.int32


def test_frame_energy_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU only"):
        features.split(np.zeros(4000, np.float32))


def test_sv_frame_energy_argument_checks_return_before_any_launch():
    """The limits of include/sv_ge2e.h as return codes (host-side checks; the pointers are never
    dereferenced): SV_EARG -1, SV_EALIGN -2, SV_ESHAPE -3."""
    from pytorch_speaker_verification_amd import _lib
    h = _lib.lib()
    p = 4096  # a 16-byte aligned, non-null address

    def rc(y=p, so=p, fo=p, n_seg=1, n_frames=4, fl=2048, hop=512, mse=p):
        return h.sv_frame_energy(y, so, fo, n_seg, n_frames, fl, hop, mse, None)

    assert rc(y=None) == -1 and rc(so=None) == -1 and rc(fo=None) == -1 and rc(mse=None) == -1
    assert rc(n_seg=0) == -1 and rc(n_seg=5) == -1
    assert rc(y=p + 4) == -2 and rc(mse=p + 8) == -2 and rc(so=p + 2) == -2 and rc(fo=p + 1) == -2
    assert rc(fl=2047) == -3 and rc(fl=0) == -3 and rc(hop=0) == -3 and rc(fl=2 ** 20 + 2) == -3


# ---- preprocess_speaker on CPU stubs

def _logmel_stub(calls):
    def stub(waves, **kw):
        calls.append([len(w) for w in waves])
        outs = [R.logmel_ref(np.asarray(w, dtype=np.float64)) for w in waves]
        return torch.from_numpy(np.concatenate(outs)), np.concatenate([[0], np.cumsum([len(o) for o in outs])]).tolist()
    return stub


def _fixed_split(table):
    """features.split replaced by a table of intervals per utterance (by position)."""
    def stub(waves, top_db=60, **kw):
        assert len(waves) == len(table)
        return [np.array(iv, dtype=np.int64).reshape(-1, 2) for iv in table]
    return stub


def test_preprocess_speaker_order_filter_and_head_tail(monkeypatch):
    """Utterances in order, intervals in order, first-180 before last-180; the strict '>' drops an
    interval of exactly utter_min_len samples; a part of T = 2 * 180 + 3 frames goes through whole
    and one of T = 2 * 180 + 4 as head and tail -- under the fp64 stub both equal the whole part's
    slices exactly."""
    calls = []
    monkeypatch.setattr(features, "logmel", _logmel_stub(calls))
    u0, u1 = R.tones(130000, seed=21), R.tones(60000, seed=22)
    n363, n364 = 362 * 160 + 7, 363 * 160  # 1 + n // 160 = 363, 364
    table = [[(100, 29300), (29400, 29400 + 29201), (58700, 58700 + n364)],  # 29200: dropped; 29201: kept
             [(1000, 1000 + n363), (59000, 59900)]]
    monkeypatch.setattr(features, "split", _fixed_split(table))
    got = features.preprocess_speaker([u0, u1])
    assert got.shape == (6, 40, 180) and got.dtype == np.float32
    head, lead = 179 * 160 + 256, 2
    assert calls == [[29201, head, n364 - (364 - 180 - lead) * 160, n363]]  # one logmel call; only what is kept
    parts = [u0[29400:29400 + 29201], u0[58700:58700 + n364], u1[1000:1000 + n363]]
    for i, part in enumerate(parts):
        full = R.logmel_ref(part.astype(np.float64)).astype(np.float32).T  # [40, T]
        np.testing.assert_array_equal(got[2 * i], full[:, :180])
        np.testing.assert_array_equal(got[2 * i + 1], full[:, -180:])


def test_preprocess_speaker_empty_result(monkeypatch):
    calls = []
    monkeypatch.setattr(features, "logmel", _logmel_stub(calls))
    monkeypatch.setattr(features, "split", _fixed_split([[(0, 29200)], []]))
    got = features.preprocess_speaker([R.tones(30000, seed=1), R.tones(30000, seed=2)])
    assert got.shape == (0, 40, 180) and got.dtype == np.float32 and calls == []
    assert features.preprocess_speaker([]).shape == (0, 40, 180)
    # utterances of at most utter_min_len samples cannot hold a kept interval: never split (a
    # 500-sample one would be refused by split's reflect padding), the others keep their order
    seen = []

    def split_stub(waves, top_db=60, **kw):
        seen.append([len(w) for w in waves])
        return [np.zeros((0, 2), dtype=np.int64) for _ in waves]

    monkeypatch.setattr(features, "split", split_stub)
    utts = [R.tones(n, seed=n) for n in (500, 29201, 29200, 40000)]
    assert features.preprocess_speaker(utts).shape == (0, 40, 180) and seen == [[29201, 40000]]
    assert features.preprocess_speaker(utts[:1]).shape == (0, 40, 180) and len(seen) == 1


def test_preprocess_speaker_with_reference_split(monkeypatch):
    """The whole chain on fp64 stubs: `long` keeps 3 of its 4 intervals, tones60000 is one interval
    of 376 frames (head / tail), `two` keeps [4096, 39424) only."""
    calls = []
    monkeypatch.setattr(features, "logmel", _logmel_stub(calls))
    monkeypatch.setattr(features, "split", lambda waves, top_db=60, **kw: [S.split_ref(w, top_db) for w in waves])
    utts = [S.signal("long"), R.tones(60000, seed=9), S.signal("two")]
    got = features.preprocess_speaker(utts)
    assert got.shape == (10, 40, 180) and len(calls) == 1
    kept = [(0, 2048, 41472), (0, 69120, 119296), (0, 120320, 160000), (1, 0, 60000), (2, 4096, 39424)]
    for i, (u, a, b) in enumerate(kept):
        full = R.logmel_ref(utts[u][a:b].astype(np.float64)).astype(np.float32).T
        np.testing.assert_array_equal(got[2 * i], full[:, :180])
        np.testing.assert_array_equal(got[2 * i + 1], full[:, -180:])


# ---- save_speakers

def test_save_speakers_split_numbering_and_loader(tmp_path, monkeypatch):
    """23 speakers -> speaker0..17.npy in the train directory, speaker0..4.npy (speakers 18..22) in
    the test directory; a written file loads through SpeakerDatasetTIMITPreprocessed."""
    from pytorch_speaker_verification_amd import data_load
    from pytorch_speaker_verification_amd.hparam import hparam as hp
    seen = []

    def stub(utterances, top_db=30, tisv_frame=None):
        seen.append(top_db)
        return np.full((6, 40, 180), float(utterances[0][0]), dtype=np.float32)

    monkeypatch.setattr(features, "preprocess_speaker", stub)
    train, test = str(tmp_path / "a" / "train"), str(tmp_path / "b" / "test")
    features.save_speakers([[np.full(8, i, np.float32)] for i in range(23)], train, test, top_db=25)
    assert seen == [25] * 23
    assert sorted(os.listdir(train)) == sorted(f"speaker{i}.npy" for i in range(18))
    assert sorted(os.listdir(test)) == sorted(f"speaker{i}.npy" for i in range(5))
    for i in range(18):
        assert (np.load(os.path.join(train, f"speaker{i}.npy")) == i).all()
    for i in range(5):
        assert (np.load(os.path.join(test, f"speaker{i}.npy")) == 18 + i).all()
    old = (hp.training, hp.data.train_path, hp.train.M)
    hp.training, hp.data.train_path, hp.train.M = True, train, 4
    try:
        ds = data_load.SpeakerDatasetTIMITPreprocessed(shuffle=False)
        assert len(ds) == 18
        item = ds[0]
        assert item.shape == (4, 160, 40) and item.dtype == torch.float32
    finally:
        hp.training, hp.data.train_path, hp.train.M = old
