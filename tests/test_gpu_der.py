"""Diarization in wall-clock time and its scoring on the GPU (diarization.raster / count / der /
evaluate, sv_seg_raster and sv_der_count) against tests/der_ref.py.  Every number is an integer (the
rates are one fp64 division of integers), so every comparison is equality."""
import numpy as np
import pytest
import torch

import der_ref as R
import diar_ref
from pytorch_speaker_verification_amd import diarization as D
from pytorch_speaker_verification_amd import dvector

pytestmark = pytest.mark.gpu

SR = 16000
# frames per file: around a wave (64), a workgroup's uint4 step (1024) and half a workgroup's chunk (4096),
# the long file second so that the others sit at odd offsets behind it; file 7 gets no row in the raster test
FRAMES = [63, 4097, 1, 1024, 2, 1025, 64, 1023, 65]
OFF = np.concatenate([[0], np.cumsum(FRAMES)])
_cache = {}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(_dev())


def _down(t):
    return t.cpu().numpy().view(np.uint32)


# ----------------------------------------------------------------------------- rasteriser
def _rows(step):
    h = step // 2

    def c(i):
        return i * step + h

    n = [nf * step for nf in FRAMES]  # samples per file
    F = len(FRAMES)
    rows = [
        (5, 5, 1, 0),                          # s == e
        (c(3), c(7), 1, 0),                    # s == c_3: frame 3 is in; e == c_7: frame 7 is out
        (c(60), n[0] + 1000 * step, 2, 0),     # an end past the file's last sample
        (-5 * step - 1, 10 ** 6, 4, 2),        # a start below 0, the one-frame file
        (0, 10 ** 6, 8, F),                    # seg_file == F: ignored
        (0, 10 ** 6, 8, -1),
        (c(100), c(600), 16, 3), (c(500), c(900), 32, 3), (c(500), c(900), 32, 3),  # overlapping bits; a row twice
        (c(1023), c(1023) + 1, 16, 3),         # the last frame alone
        (0, n[1], 1 << 31, 1),                 # a whole 4097-frame file, bit 31
        (c(2047), c(2049) + 1, 1, 1),          # across the host splitter's cut at frame 2048
        (c(1), c(1) + 1, 64, 4),
        (0, c(1024) + 1, 128, 5), (c(1024), c(1024), 3, 5), (c(1000) + 1, c(1001), 1, 5),  # (s, e] between two centres: nothing
        (c(63), n[6] + 5, 256, 6), (900, 100, 512, 6),  # e < s
        (c(64), c(64) + 1, 1 << 30, 8), (0, c(0), 1 << 29, 8),  # e == c_0: nothing
    ]
    return [np.array(v) for v in zip(*rows)]


@pytest.mark.parametrize("step", [1, 7, 160])
def test_raster(step):
    s, e, b, f = _rows(step)
    want = R.raster(s, e, b, f, OFF, step)
    assert want[OFF[7]:OFF[8]].max() == 0 and want[OFF[1]:OFF[2]].min() >= 1 << 31  # no row; the whole-file row
    for split in (False, True):
        buf = torch.zeros(int(OFF[-1]) + 1, dtype=torch.int32, device=_dev())
        buf[-1] = 0x5A5A5A5A
        got = _down(D.raster(s, e, b, f, OFF, step, mask=buf, split=split))
        assert got[-1] == 0x5A5A5A5A, split  # the word past the last file's last frame
        assert np.array_equal(got[:-1], want), (step, split, np.flatnonzero(got[:-1] != want)[:8])
    ps = D.split_rows(s, e, b, f, step)
    assert ps[0].size > s.size and np.all(ps[1] - ps[0] <= D.RASTER_PIECE * step)  # the long rows are cut
    again = _down(D.raster(s, e, b, f, OFF, step))
    assert again.size == OFF[-1] and np.array_equal(again, want)


# ----------------------------------------------------------------------------- counter
def _runs(rng, n, values, lo, hi):
    """n frames of runs of lo .. hi frames, every run one of `values`."""
    out = np.zeros(n, dtype=np.uint32)
    i = 0
    while i < n:
        m = int(rng.integers(lo, hi + 1))
        out[i:i + m] = values[int(rng.integers(0, len(values)))]
        i += m
    return out


def _patterns():
    if "patterns" in _cache:
        return _cache["patterns"]
    n = int(OFF[-1])
    rng = np.random.default_rng(3)
    zeros = np.zeros(n, dtype=np.uint32)
    t = np.arange(n)
    sets = [0, 1, 2, 4, 8, 3, 5, 6, 7, 16 | 32, 1 | 16 | 32, 1 << 31 | 1]  # up to three speakers at once
    cut = zeros.copy()  # a UEM that ends in the middle of a uint4 group of every file
    for a, b in zip(OFF[:-1], OFF[1:]):
        cut[a:a + (b - a) // 2 + 1] = 7
    pats = {
        "constant": (np.full(n, 1 << 2, dtype=np.uint32), np.full(n, 1 << 5, dtype=np.uint32), zeros, None),
        "alternating": (np.where(t % 2, 1, 2).astype(np.uint32), np.where(t % 3 == 0, 2, 1).astype(np.uint32), zeros, None),
        "random": (_runs(rng, n, sets, 1, 40), _runs(rng, n, sets, 1, 40), _runs(rng, n, [0, 0, 0, 1], 1, 30),
                   _runs(rng, n, [1, 1, 1, 0], 1, 200)),
        "random_short": (_runs(rng, n, sets, 1, 3), _runs(rng, n, sets, 1, 3), zeros, None),
        "long_turns": (_runs(rng, n, [1, 2, 4, 8, 0], 100, 1000), _runs(rng, n, [1, 2, 4, 8, 0], 100, 1000), zeros, None),
        "unscored": (_runs(rng, n, sets, 1, 40), _runs(rng, n, sets, 1, 40), np.full(n, 1 << 31, dtype=np.uint32), None),
        "zeros": (zeros, zeros, zeros, None),
        "bit31": (np.full(n, 1 << 31, dtype=np.uint32), _runs(rng, n, [1 << 31, 1 << 31 | 1 << 30], 1, 9), zeros, None),
        "uem_cut": (np.full(n, 3, dtype=np.uint32), np.full(n, 1 << 7, dtype=np.uint32), zeros, cut),
    }
    _cache["patterns"] = pats
    return pats


@pytest.mark.parametrize("name", ["constant", "alternating", "random", "random_short", "long_turns", "unscored", "zeros",
                                  "bit31", "uem_cut"])
def test_count(name):
    ref, hyp, ns, uem = _patterns()[name]
    d = [_up(ref), _up(hyp), _up(ns)]
    d_uem = None if uem is None else _up(uem)
    for skip in (False, True):
        want = R.count(ref, hyp, ns, OFF, uem, skip)
        got = D.count(*d, OFF, uem=d_uem, skip_overlap=skip)
        assert got.dtype == np.uint64 and got.shape == (len(FRAMES), 4 + 1024)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (name, skip, bad[:6], got[got != want][:6], want[got != want][:6])
        assert np.array_equal(D.count(*d, OFF, uem=d_uem, skip_overlap=skip), got)  # the same call twice
    if name == "constant":
        plain = D.count(*d, OFF)
        assert plain[1, 0] == 4097 and plain[1, 4 + 32 * 2 + 5] == 4097 and plain[:, 4:].sum() == OFF[-1]
    if name == "unscored" or name == "zeros":
        assert got.sum() == 0


def test_count_one_file_and_offsets_inside_a_group():
    """A single file, and files of 1 .. 9 frames: every alignment of a file inside the uint4 groups."""
    rng = np.random.default_rng(4)
    for frames in ([4097], [1], list(range(1, 10)) + [5, 3, 8]):
        off = np.concatenate([[0], np.cumsum(frames)])
        n = int(off[-1])
        ref, hyp = _runs(rng, n, [1, 2, 3, 0], 1, 5), _runs(rng, n, [1, 2, 6, 0], 1, 5)
        ns = _runs(rng, n, [0, 0, 1], 1, 4)
        assert np.array_equal(D.count(_up(ref), _up(hyp), _up(ns), off), R.count(ref, hyp, ns, off)), frames


# ----------------------------------------------------------------------------- der() end to end
def _turns(rng, n, speakers, lo, hi, p_gap, p_overlap):
    """Random (start_s, end_s, speaker) turns over a file of n samples, with gaps and overlaps, some
    positions before 0 and past the end."""
    segs, t = [], -int(rng.integers(0, 300))
    while t < n + 200:
        m = int(rng.integers(lo, hi))
        segs.append((t / SR, (t + m) / SR, speakers[int(rng.integers(0, len(speakers)))]))
        u = rng.random()
        t += m + int(rng.integers(1, hi)) if u < p_gap else m - int(rng.integers(1, lo)) if u < p_gap + p_overlap else m
    return segs


def _der_case():
    if "der" not in _cache:
        rng = np.random.default_rng(9)
        step = 160
        n_samples = [nf * step - int(rng.integers(0, step)) for nf in FRAMES]
        refs = [_turns(rng, n, ["A", "B", "C"], 800, 40000, 0.2, 0.3) for n in n_samples]
        hyps = [_turns(rng, n, [0, 1, 2, 3], 800, 30000, 0.2, 0.1) for n in n_samples]
        refs[2], hyps[4], refs[8], hyps[8] = [], [], [], []  # no reference; no hypothesis; neither
        uem = [None if f % 2 else [(0.01, n / SR / 2), (n / SR * 0.75, n / SR + 1.0)] for f, n in enumerate(n_samples)]
        _cache["der"] = (refs, hyps, n_samples, uem, {})
    return _cache["der"]


@pytest.mark.parametrize("kw", [dict(collar=0.25), dict(collar=0.0, skip_overlap=True), dict(collar=0.1, uem=True)],
                         ids=["collar", "skip_overlap", "uem"])
def test_der_end_to_end(kw):
    refs, hyps, n_samples, uem, _ = _der_case()
    kw = dict(kw)
    if kw.pop("uem", False):
        kw["uem"] = uem
    want = R.der(refs, hyps, n_samples, **kw)
    assert [R.n_frames(n, 160) for n in n_samples] == FRAMES
    for max_frames in (1500, 2 ** 27):  # several batches (the long file alone, the others in groups); one batch
        got = D.der(refs, hyps, n_samples, max_frames=max_frames, **kw)
        for k in ("total", "miss", "fa", "conf"):
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (k, max_frames, got[k], want[k])
        assert np.array_equal(got["file_der"], want["file_der"], equal_nan=True)
        assert got["der"] == want["der"] and np.isnan(got["file_der"][2]) and np.isnan(got["file_der"][8])
        assert got["mapping"][8] == {} and got["mapping"][4] == {} and set(got["mapping"][1]) <= {"A", "B", "C"}
    assert want["total"].sum() > 1000 and want["conf"].sum() > 0 and want["miss"].sum() > 0 and want["fa"].sum() > 0


def test_der_known_answer_and_step():
    ref = [[(0.0, 5.0, "A"), (5.0, 10.0, "B")]]
    hyp = [[(0.0, 6.0, "x"), (6.0, 10.0, "y")]]
    got = D.der(ref, hyp, [10 * SR], collar=0.0)
    assert (got["total"][0], got["miss"][0], got["fa"][0], got["conf"][0]) == (1000, 0, 0, 100) and got["der"] == 0.1
    assert got["mapping"] == [{"A": "x", "B": "y"}]
    got = D.der(ref, hyp, [10 * SR], collar=0.25)
    assert (got["total"][0], got["conf"][0]) == (900, 75) and got["der"] == 75 / 900
    # reference boundaries outside the file are clamped before the collars are built, and a row that is empty after
    # clamping still has its boundary (both worked out by hand in test_der_ref.test_oracle_known_answers)
    got = D.der([[(-1.0, 5.0, "A"), (5.0, 12.0, "B")]], hyp, [10 * SR], collar=0.25)
    assert (got["total"][0], got["miss"][0], got["fa"][0], got["conf"][0]) == (900, 0, 0, 75)
    got = D.der([[(0.0, 5.0, "A"), (5.0, 9.0, "B"), (11.0, 12.0, "C")]], hyp, [10 * SR], collar=0.25)
    assert (got["total"][0], got["miss"][0], got["fa"][0], got["conf"][0]) == (800, 0, 50, 75)
    fine = D.der(ref, hyp, [10 * SR], collar=0.0, step=1)  # one frame per sample
    assert (fine["total"][0], fine["conf"][0]) == (10 * SR, SR) and fine["der"] == 0.1


# ----------------------------------------------------------------------------- labels to score, no network
def _ranges_for(n_aligned):
    """Two voiced ranges (a one-window range first, so that aligned d-vector 0 straddles both) whose
    aligned_spans hold exactly n_aligned d-vectors."""
    for frames in range(200, 6000, 12):
        ranges = [(1000, 1000 + 30 * 160), (20000, 20000 + frames * 160 + 3)]
        spans = dvector.aligned_spans(ranges)
        if spans[-1, 2] + 1 == n_aligned:
            return ranges, spans
    raise AssertionError("no range length gives that many aligned d-vectors")


@pytest.mark.parametrize("k,run", [(2, 8), (4, 4)])
def test_planted_labels_to_score(k, run):
    x, lab = diar_ref.planted(64, k, run, 0)
    ranges, spans = _ranges_for(64)
    n = ranges[-1][1] + 4000
    reference = [[(s, e, f"spk{v}") for s, e, v in D.segments([lab], [spans])[0]]]
    labels, _ = D.cluster([x], n_speakers=k)
    assert np.array_equal(labels[0], diar_ref.relabel(lab))
    hyp = D.segments(labels, [spans])
    voiced = int((R.raster(spans[:, 0], spans[:, 1], [1] * len(spans), [0] * len(spans), [0, R.n_frames(n, 160)], 160) != 0).sum())
    got = D.der(reference, hyp, [n], collar=0.0)
    assert (got["total"][0], got["miss"][0], got["fa"][0], got["conf"][0]) == (voiced, 0, 0, 0) and got["der"] == 0.0
    assert got["mapping"][0] == {f"spk{v}": v for v in range(k)}
    swapped = [[(s, e, {0: 1, 1: 0}.get(v, v)) for s, e, v in hyp[0]]]
    sw = D.der(reference, swapped, [n], collar=0.0)
    assert all(np.array_equal(sw[key], got[key]) for key in ("total", "miss", "fa", "conf")) and sw["der"] == 0.0
    assert sw["mapping"][0]["spk0"] == 1 and sw["mapping"][0]["spk1"] == 0
    # speakers 0 and 1 under one hypothesis name: the smaller of the two is confused, frame for frame
    merged = [[(s, e, 0 if v == 1 else v) for s, e, v in hyp[0]]]
    per_spk = []
    for v in (0, 1):
        rows = [(int(round(s * SR)), int(round(e * SR))) for s, e, name in reference[0] if name == f"spk{v}"]
        per_spk.append(int((R.raster([r[0] for r in rows], [r[1] for r in rows], [1] * len(rows), [0] * len(rows),
                                     [0, R.n_frames(n, 160)], 160) != 0).sum()))
    mg = D.der(reference, merged, [n], collar=0.0)
    assert (mg["total"][0], mg["miss"][0], mg["fa"][0]) == (voiced, 0, 0) and mg["conf"][0] == min(per_spk) > 0


# ----------------------------------------------------------------------------- with a small random network
def _net():
    import recipe
    from conftest import model_dims
    from pytorch_speaker_verification_amd.speech_embedder_net import SpeechEmbedder
    dims = (40, 64, 2, 32)
    sd = recipe.make_weights(33, *dims)
    with model_dims(*dims):
        net = SpeechEmbedder()
    with torch.no_grad():
        for key, v in net.state_dict().items():
            v.copy_(torch.as_tensor(sd[key]))
    return net.cuda()


def test_diarize_times_and_evaluate(monkeypatch):
    import logmel_ref as L
    net = _net()
    files = [(L.tones(64000, seed=1), [(0, 20000), (20000, 23000), (30000, 64000)]),   # (the middle range is too short)
             (L.tones(5000, seed=2), []),
             (L.tones(56000, seed=3), [(500, 6000), (8000, 30000), (31000, 55999)]),
             (L.tones(48000, seed=4), [(0, 24000), (24000, 48000)])]
    two = D.diarize(net, files, precision="f32", n_speakers=2)
    assert isinstance(two, tuple) and len(two) == 2
    labels, info, segs = D.diarize(net, files, precision="f32", n_speakers=2, times=True)
    assert len(segs) == len(files) and segs[1] == []
    for f, (wave, ranges) in enumerate(files):
        assert np.array_equal(labels[f], two[0][f])
        kept = [(a, b) for a, b in ranges if 1 + (b - a) // 160 > dvector.WIN]
        cover = np.zeros(len(wave) + 1, dtype=np.int32)
        for s, e, v in segs[f]:
            cover[int(round(s * SR)):int(round(e * SR))] += 1
            assert isinstance(s, float) and 0 <= v < 2
        want = np.zeros(len(wave) + 1, dtype=np.int32)
        for a, b in kept:
            want[a:b] += 1
        assert np.array_equal(cover, want), f  # the segments' union is exactly the kept ranges, nothing twice
    res = D.evaluate(net, files, segs, precision="f32", n_speakers=2, collar=0.0)
    assert res["der"] == 0.0 and res["conf"].sum() == 0 and res["miss"].sum() == 0 and res["fa"].sum() == 0
    assert res["total"][1] == 0 and res["total"][0] > 0 and np.isnan(res["file_der"][1])
    for f, m in enumerate(res["mapping"]):
        assert m == {v: v for v in sorted({v for _, _, v in segs[f]})}
    assert all(np.array_equal(a, b) for a, b in zip(res["labels"], labels)) and res["segments"] == segs
    assert res["info"]["k"] == info["k"]
    seen = {}
    real = D.cluster

    def spy(dvectors, **kw):
        seen.update(kw)
        return real(dvectors, **kw)

    monkeypatch.setattr(D, "cluster", spy)
    references = [[(0.0, 1.0, "a"), (1.0, 2.0, "b"), (2.5, 3.5, "a")], [], [(0.0, 3.0, "z")],
                  [(0.0, 1.0, "p"), (1.0, 2.0, "q"), (2.0, 3.0, "r")]]
    res = D.evaluate(net, files, references, n_speakers="oracle", precision="f32")
    assert seen["n_speakers"] == [2, 0, 1, 3]
    assert res["info"]["k"] == [2, 0, 1, 3] and len(set(res["labels"][3].tolist())) == 3
    assert set(res["mapping"][2]) == {"z"}
    # a file with d-vectors and an empty reference: the oracle count is 0, which cluster raises to one speaker
    res = D.evaluate(net, files, [[], [], [], []], n_speakers="oracle", precision="f32")
    assert seen["n_speakers"] == [0, 0, 0, 0] and res["info"]["k"] == [1, 0, 1, 1]
    assert res["total"].sum() == 0 and res["fa"].sum() > 0 and np.isnan(res["der"])
