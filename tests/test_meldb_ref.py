"""Host-side checks of the mel-magnitude-in-dB feature (no GPU): known answers of the fp64 reference
helper (tests/meldb_ref.py), the argument checks of sv_meldb, the segment table mel_db_fixed builds
from trim bounds, and the sampling of SpeakerDatasetWaveforms against a replay of random.shuffle."""
import random

import numpy as np
import pytest
import torch

import logmel_ref as R
import meldb_ref as M
from pytorch_speaker_verification_amd import data_load, features


def test_reference_unit_sine_at_a_bin_centre_has_magnitude_win_over_4():
    """Bin 32 of nfft 512 at 16 kHz is 1000 Hz, 25 whole cycles per 400-sample window: the Hann
    window's transform puts sum(w) / 2 = win / 4 on that bin and zeros on the negative image."""
    t = np.arange(4000) / 16000.0
    mag = M.mag_ref(np.sin(2 * np.pi * 1000.0 * t + 0.3))
    assert mag.shape == (26, 257)
    interior = mag[2:-2]  # frames that reflect nowhere
    assert np.abs(interior[:, 32] - 100.0).max() <= 1e-9
    assert (interior.argmax(axis=1) == 32).all()
    # and the dB of a mel sum is 20 log10 of it: power and magnitude differ by a factor 2 in dB
    x = M.mel_mag_ref(np.sin(2 * np.pi * 1000.0 * t + 0.3))
    db = M.db_of(x, top_db=None)
    assert abs(db.max() - 20.0 * np.log10(x.max())) <= 1e-12


def test_reference_zero_input_sits_on_the_amin_floor():
    ref = M.meldb_ref(np.zeros(3000))
    assert ref.shape == (19, 40)
    assert (ref == 20.0 * np.log10(1e-5)).all() and abs(ref[0, 0] + 100.0) <= 1e-12  # max - 80 < floor: no clip
    assert (M.meldb_ref(np.zeros(3000), amin=1e-3) == 20.0 * np.log10(1e-3)).all()


def test_reference_clip_level_is_the_maximum_minus_top_db():
    y = R.burst(8000)
    ref, raw = M.meldb_ref(y), M.meldb_ref(y, top_db=None)
    assert raw.min() == 20.0 * np.log10(1e-5) and raw.max() == ref.max()
    assert ref.min() == ref.max() - 80.0  # exactly
    clipped = raw < raw.max() - 80.0
    assert clipped.mean() > 0.8 and (ref[clipped] == ref.min()).all() and (ref[~clipped] == raw[~clipped]).all()
    assert M.meldb_ref(y, top_db=20.0).min() == ref.max() - 20.0
    # the fp32 yardstick is the same function
    ref32 = M.meldb_ref(y, dtype=np.float32)
    assert ref32.dtype == np.float32 and ref32.min() == ref32.max() - np.float32(80.0)


def test_reference_fixed_pads_and_truncates():
    y = np.concatenate([np.zeros(1000, np.float32), R.tones(3000, seed=1), np.zeros(1500, np.float32)])
    assert M.trim_bounds(y, 60) == (960, 4320)
    assert M.trim_bounds(R.burst(8000), 60) == (2880, 5280)
    padded = np.concatenate([y[960:4320], np.zeros(240, np.float32)])
    np.testing.assert_array_equal(M.fix_length(y[960:4320], 3600), padded)
    np.testing.assert_array_equal(M.fix_length(y[960:4320], 3000), y[960:3960])
    assert M.fixed_ref(y, 3600).shape == (23, 40)
    np.testing.assert_array_equal(M.fixed_ref(y, 3000), M.meldb_ref(y[960:3960]))
    np.testing.assert_array_equal(M.fixed_ref(y, 3000, trim_top_db=None), M.meldb_ref(y[:3000]))


def test_sv_meldb_argument_checks_return_before_any_launch():
    """The limits of include/sv_ge2e.h as return codes (host-side checks; the pointers are never
    dereferenced): SV_EARG -1, SV_EALIGN -2, SV_ESHAPE -3; the workspace query is 0."""
    from pytorch_speaker_verification_amd import _lib
    h = _lib.lib()
    assert h.sv_meldb_workspace(1000, 512, 400, 40) == 0
    p = 4096  # a 16-byte aligned, non-null address

    def rc(y=p, st=p, va=p, ln=p, fo=p, n_seg=1, n_frames=4, nfft=512, win=400, hop=160, nmels=40, wb=p, ld=516, fb=p,
           amin=1e-5, top_db=80.0, out=p, smax=p):
        return h.sv_meldb(y, st, va, ln, fo, n_seg, n_frames, nfft, win, hop, nmels, wb, ld, fb, amin, top_db, out,
                          smax, None, None)

    assert rc(y=None) == -1 and rc(n_seg=0) == -1 and rc(n_seg=5) == -1 and rc(ld=512) == -1
    assert rc(st=None) == -1 and rc(va=None) == -1 and rc(ln=None) == -1 and rc(smax=None) == -1
    assert rc(amin=0.0) == -1 and rc(amin=-1.0) == -1 and rc(amin=float("nan")) == -1
    assert rc(nfft=511) == -3 and rc(nfft=1026, ld=1028) == -3 and rc(win=513) == -3
    assert rc(hop=0) == -3 and rc(nmels=129) == -3 and rc(nmels=0) == -3
    assert rc(y=p + 4) == -2 and rc(out=p + 8) == -2 and rc(ld=518) == -2 and rc(st=p + 2) == -2
    assert rc(va=p + 1) == -2 and rc(ln=p + 2) == -2 and rc(smax=p + 2) == -2 and rc(fo=p + 2) == -2


def test_fixed_segment_table_pads_truncates_and_takes_an_empty_trim():
    """Three waveforms packed at 0, 8000, 13500: trimmed to 2400 samples (padded to 3600), to 3360
    (padded), to 5000 (truncated), and one whose trim is empty (valid = 0, start inside the buffer)."""
    seg_off = [0, 8000, 13500, 20000, 21000]
    t = features.fixed_segments([(2880, 5280), (960, 4320), (500, 5500), (0, 0)], seg_off, 3600, 160)
    assert t.dtype == np.int32 and t.shape == (17,)
    assert t[0:4].tolist() == [2880, 8960, 14000, 20000]   # seg_start
    assert t[4:8].tolist() == [2400, 3360, 3600, 0]        # seg_valid = min(count, L)
    assert t[8:12].tolist() == [3600] * 4                  # seg_len
    assert t[12:].tolist() == [0, 23, 46, 69, 92]          # frame_off: 1 + 3600 // 160 frames each
    # every segment's real samples lie inside its own waveform
    for s in range(4):
        assert seg_off[s] <= t[s] and t[s] + max(t[4 + s], 1) <= seg_off[s + 1]
    assert features.fixed_length() == 29200 and features.fixed_length(3600) == 3600
    assert features.fixed_segments([(0, 29200)], [0, 29200], 29200, 160)[3:].tolist() == [0, 183]


def test_mel_db_refuses_bad_arguments_on_the_host(monkeypatch):
    """Before it looks for a device."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError):
        features.mel_db([np.zeros(400, np.float32), np.zeros(256, np.float32)])  # shorter than nfft // 2 + 1
    with pytest.raises(ValueError):
        features.mel_db(np.zeros((2, 400), np.float32))
    with pytest.raises(ValueError):
        features.mel_db(np.zeros(400, np.float32), amin=0.0)
    with pytest.raises(ValueError):
        features.mel_db_fixed([np.zeros(4000, np.float32), np.zeros(200, np.float32)])  # shorter than win // 2 + 1
    with pytest.raises(ValueError):
        features.mel_db_fixed([np.zeros(4000, np.float32)], length=256)  # below nfft // 2 + 1
    with pytest.raises(RuntimeError, match="GPU only"):
        features.mel_db(np.zeros(400, np.float32))
    with pytest.raises(RuntimeError, match="GPU only"):
        features.mel_db_fixed([np.zeros(4000, np.float32)], length=3600)


def test_waveform_dataset_sampling_replays_random_shuffle(monkeypatch):
    """data_load.py:29-40 with the featuriser stubbed: one shuffle of the speaker order in __init__,
    one shuffle of the speaker's utterance order per item, the first M of it -- the same draws from
    `random` as the reference's, so the state of the generator afterwards is the replay's."""
    from pytorch_speaker_verification_amd.hparam import hparam as hp
    counts = [7, 5, 9, 6]
    speakers = [[np.full(3, 100 * s + u, dtype=np.float32) for u in range(k)] for s, k in enumerate(counts)]
    monkeypatch.setattr(features, "mel_db_fixed", lambda waves: [int(w[0]) for w in waves])

    random.seed(77)
    ds = data_load.SpeakerDatasetWaveforms(speakers, utterance_number=4)
    got = [ds[i] for i in (2, 0, 2, 3)]
    after = random.random()

    random.seed(77)
    order = list(range(4))
    random.shuffle(order)
    want = []
    for i in (2, 0, 2, 3):
        utts = list(range(counts[order[i]]))
        random.shuffle(utts)
        want.append([100 * order[i] + u for u in utts[:4]])
    assert got == want and after == random.random()
    assert len(ds) == 4 and ds.on_device
    assert [len(s) for s in speakers] == counts and int(speakers[0][0][0]) == 0  # the caller's lists are left alone
    # the default M follows hp.training
    old = hp.training
    try:
        hp.training = True
        assert data_load.SpeakerDatasetWaveforms(speakers).utterance_number == hp.train.M
        hp.training = False
        assert data_load.SpeakerDatasetWaveforms(speakers).utterance_number == hp.test.M
    finally:
        hp.training = old


def test_raw_wav_entry_points_still_refuse_and_the_shim_exports_the_new_class():
    import importlib.util
    import os
    from conftest import ROOT
    with pytest.raises(NotImplementedError, match="SpeakerDatasetWaveforms"):
        data_load.SpeakerDatasetTIMIT()
    spec = importlib.util.spec_from_file_location("_dropin_data_load", os.path.join(ROOT, "dropin", "data_load.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SpeakerDatasetWaveforms is data_load.SpeakerDatasetWaveforms
