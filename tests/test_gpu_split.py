"""The framed-energy kernel (sv_frame_energy, features.frame_energy) and what is built on it
(features.split, trim, preprocess_speaker) on the GPU against the fp64 numpy reference
(tests/split_ref.py).

The bound of every mse comparison is a priori: frame_length fp32 squares summed in any order plus
one multiply are within (frame_length + 2) * 2**-24 of the exact value, relative, per frame
(1.22e-4 at 2048) -- still below the 1 / frame_length = 4.9e-4 effect of one dropped or doubled
sample of average energy.  Intervals are compared exactly; each case first asserts that its fp64
margin to the threshold is at least 0.01 dB, ten times what the mse bound can move a frame.

Measured on MI355X (largest relative error of a frame / bound; the tests print `MEASURED ...`):
  tones 1025 5.46e-8 / 1.22e-4     1535 2.49e-8 / 1.22e-4     1536 1.21e-7 / 1.22e-4
  tones 2048 2.65e-8 / 1.22e-4     4095 8.38e-8 / 1.22e-4     4096 8.34e-8 / 1.22e-4
  burst 8000 7.03e-8 / 1.22e-4     long 160000 1.21e-7 / 1.22e-4
  two 400 / 160: 1.48e-7 / 2.40e-5     tones 700 at 64 / 32: 8.08e-8 / 3.93e-6
  preprocess_speaker (max-abs of a slice / logmel_ref.err_bound) 8.0e-6 ... 1.40e-5 / 5.6e-5 ... 8.4e-5;
  its head / tail slices bit-identical to the whole waveform's log-mel
"""
import numpy as np
import pytest
import torch

import logmel_ref as R
import split_ref as S
from pytorch_speaker_verification_amd import features

pytestmark = pytest.mark.gpu

BATCH = ["quiet", "burst", "zeros", "long", "two"]
_single = {}


def _single_energy(name):
    """(mse cuda, frame_off) of a named signal alone at 2048 / 512, computed once."""
    if name not in _single:
        _single[name] = features.frame_energy(S.signal(name))
    return _single[name]


def _check_mse(name, got, ref, frame_length):
    bound = (frame_length + 2) * 2.0 ** -24
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all()
    zero = ref == 0.0
    assert (got[zero] == 0.0).all()  # frames of exact silence are exactly 0
    rel = np.abs(got[~zero].astype(np.float64) - ref[~zero]) / ref[~zero]
    err = float(rel.max()) if rel.size else 0.0
    print(f"\nMEASURED mse[{name}] max-rel {err:.2e} bound {bound:.2e} frames {len(ref)}")
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("n", [1025, 1535, 1536, 2048, 4095, 4096])
def test_mse_of_short_waveforms_against_fp64(n):
    """1025 samples: 3 frames, every one reflecting on both sides; 1535 / 1536: 3 against 4 frames;
    up to 4096: the first frame that reflects nowhere."""
    y = R.tones(n, seed=n)
    mse, frame_off = features.frame_energy(y)
    assert frame_off == [0, 1 + n // 512] and mse.is_cuda and mse.shape == (1 + n // 512,)
    _check_mse(f"tones{n}", mse, S.mse_ref(y), 2048)


@pytest.mark.parametrize("name,fl,hop", [("burst", 2048, 512), ("long", 2048, 512), ("two", 400, 160)])
def test_mse_of_signals_against_fp64(name, fl, hop):
    mse, frame_off = features.frame_energy(S.signal(name), fl, hop)
    ref = S.mse_of(name, fl, hop)
    assert frame_off == [0, len(ref)]
    if name == "burst":
        assert (ref == 0.0).sum() >= 4  # the helper sees exact silence too
    _check_mse(f"{name}_{fl}_{hop}", mse, ref, fl)


def test_mse_of_a_small_frame_configuration():
    """frame_length 64 is one pass of a quarter of the lanes' partial sums; hop 32."""
    y = R.tones(700, seed=700)
    mse, frame_off = features.frame_energy(y, 64, 32)
    assert frame_off == [0, 22]
    _check_mse("tones700_64_32", mse, S.mse_ref(y, 64, 32), 64)


@pytest.mark.parametrize("name,fl,hop,top_db,want", S.KNOWN, ids=S.KNOWN_IDS)
def test_intervals_equal_reference_exactly(name, fl, hop, top_db, want):
    ref = S.mse_of(name, fl, hop)
    assert S.margin(ref, top_db) >= 0.01  # (on the CPU, before anything is compared)
    y = S.signal(name)
    got = features.split(y, top_db=top_db, frame_length=fl, hop_length=hop)
    assert got.dtype == np.int64 and got.ndim == 2
    assert got.tolist() == S.intervals_ref(ref, len(y), hop, top_db).tolist() == want


def test_ragged_batch_is_bit_identical_and_stays_in_bounds():
    """Five waveforms in one call: `quiet` and the zeros have loud neighbours, so a maximum taken
    across waveforms would change their intervals.  Intervals equal the single calls', the mse rows
    are bit-identical to the single calls', and a NaN guard element after n_frames is left alone
    (through the entry point features.frame_energy uses)."""
    waves = [S.signal(n) for n in BATCH]
    got = features.split(waves, top_db=30)
    assert isinstance(got, list) and len(got) == 5
    for name, g in zip(BATCH, got):
        assert g.tolist() == features.split(S.signal(name), top_db=30).tolist() == S.split_ref(S.signal(name), 30).tolist()
    mse, frame_off = features.frame_energy(waves)
    assert frame_off == [0, 94, 110, 116, 429, 523] and mse.shape == (523,)
    for s, name in enumerate(BATCH):
        assert torch.equal(mse[frame_off[s]:frame_off[s + 1]], _single_energy(name)[0]), name
    dev = mse.device
    seg_off, foff = features.energy_offsets([len(w) for w in waves], 2048, 512)
    y = torch.from_numpy(np.concatenate(waves)).to(dev)
    guarded = torch.full((524,), float("nan"), device=dev)
    features.frame_energy_into(y, torch.from_numpy(seg_off).to(dev), torch.from_numpy(foff).to(dev), 5, 523, 2048, 512,
                               guarded)
    assert torch.equal(guarded[:523], mse)
    assert torch.isnan(guarded[523])


def test_device_resident_input_gives_the_same_bits():
    waves = [S.signal("two"), S.signal("burst")]
    host, foff = features.frame_energy(waves)
    dwaves = [torch.from_numpy(w).cuda() for w in waves]
    devi, foff2 = features.frame_energy(dwaves)
    assert foff == foff2 and torch.equal(host, devi)
    assert torch.equal(features.frame_energy(dwaves[0])[0], _single_energy("two")[0])
    # a slice that starts off a 16-byte boundary
    assert torch.equal(features.frame_energy(dwaves[0][1:])[0], features.frame_energy(waves[0][1:])[0])
    assert features.split(dwaves, top_db=30)[0].tolist() == S.split_ref(waves[0], 30).tolist()


def test_trim_returns_the_slice():
    two = S.signal("two")
    y, (start, end) = features.trim(two, top_db=30, frame_length=400, hop_length=160)
    assert (start, end) == (4800, 46240)
    np.testing.assert_array_equal(y, two[4800:46240])


def test_preprocess_speaker_on_the_gpu():
    """`long` keeps 3 of its 4 intervals (39424, 50176 and 39680 samples; the 4096-sample one is
    dropped), tones60000 is one interval of 376 frames and takes the head / tail path, `two` keeps
    [4096, 39424) only: (10, 40, 180).  Every slice within logmel_ref.err_bound of the fp64 log-mel
    of split_ref's intervals; the head / tail result bit-identical to the whole waveform's log-mel."""
    tones = R.tones(60000, seed=9)
    utts = [S.signal("long"), tones, S.signal("two")]
    got = features.preprocess_speaker(utts)
    assert got.shape == (10, 40, 180) and got.dtype == np.float32 and np.isfinite(got).all()
    kept = []
    for u in utts:
        kept += [(u, int(a), int(b)) for a, b in S.split_ref(u, 30) if b - a > 29200]
    assert [(b - a) for _, a, b in kept] == [39424, 50176, 39680, 60000, 35328]
    for i, (u, a, b) in enumerate(kept):
        ref, bound = R.err_bound(u[a:b])
        for k, want in ((2 * i, ref[:180]), (2 * i + 1, ref[-180:])):
            err = float(np.abs(got[k].T.astype(np.float64) - want).max())
            print(f"\nMEASURED preprocess_speaker[{k}] max-abs {err:.2e} bound {bound:.2e}")
            assert err <= bound, (k, err, bound)
    full = features.logmel(tones)[0]
    assert full.shape == (376, 40)
    assert torch.equal(torch.from_numpy(got[6]), full[:180].t().cpu())
    assert torch.equal(torch.from_numpy(got[7]), full[-180:].t().cpu())
