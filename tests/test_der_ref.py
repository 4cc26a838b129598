"""CPU: the host half of diarization in wall-clock time and of its scoring -- dvector.aligned_spans
against the literal per-window loop, segments, RTTM, the assignment solver against brute force, the
scoring oracle (der_ref.py) on answers worked out by hand, split_rows, and the header text, ctypes
rows and argument codes of sv_seg_raster / sv_der_count (returned before any launch)."""
import os

import numpy as np
import pytest

import der_ref as R

SR, HOP_N = 16000, 160


def _spans_case(ranges):
    from pytorch_speaker_verification_amd import dvector
    got = dvector.aligned_spans(ranges)
    want = R.aligned_spans_loop(ranges, HOP_N, dvector.partitions)
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (ranges, got, want)
    kept = [(a, b) for a, b in ranges if 1 + (b - a) // HOP_N > dvector.WIN]
    if not kept:
        assert got.shape == (0, 3)
        return got
    assert np.all(got[:, 0] < got[:, 1]) and np.all(got[1:, 0] >= got[:-1, 1])  # ascending, disjoint
    top = max(b for _, b in kept)
    cover, want_cover = np.zeros(top, dtype=np.int32), np.zeros(top, dtype=np.int32)
    for s, e, _ in got:
        cover[s:e] += 1
    for a, b in kept:
        want_cover[a:b] += 1
    assert np.array_equal(cover, want_cover)  # the union is exactly the kept ranges
    frame_off = np.concatenate([[0], np.cumsum([1 + (b - a) // HOP_N for a, b in kept])])
    n_aligned = dvector.batch_tables(frame_off, [0] * len(kept), 1)[2][0]
    assert sorted(set(got[:, 2].tolist())) == list(range(n_aligned))
    assert np.all(np.diff(got[:, 2]) >= 0)
    return got


def test_aligned_spans_against_the_window_loop():
    from pytorch_speaker_verification_amd.hparam import hparam as hp
    assert int(hp.data.hop * hp.data.sr) == HOP_N and hp.data.sr == SR
    one = _spans_case([(1000, 1000 + 3 * SR)])
    assert one[0, 0] == 1000 and one[-1, 1] == 1000 + 3 * SR
    # partitions(): windows 0, 1 are aligned d-vector 0 -- 24 frames of hop 160 from the range's start
    assert one[0].tolist() == [1000, 1000 + 24 * HOP_N, 0]
    _spans_case([(0, 3000), (5000, 60000)])                       # the first range is too short: dropped
    _spans_case([(0, 24 * HOP_N - 1), (5000, 5000 + 24 * HOP_N)])  # 24 frames: dropped; 25 frames: one window
    # a one-window range (31 frames), then a long one: aligned d-vector 0 averages windows 0 and 1,
    # one from each range, and so owns two spans with a gap between them
    st = _spans_case([(100, 100 + 30 * HOP_N), (10000, 90000)])
    zero = st[st[:, 2] == 0]
    assert zero.shape[0] == 2 and zero[0].tolist() == [100, 100 + 30 * HOP_N, 0] and zero[1, 0] == 10000
    # one window, then two windows (41 frames), then a long range: aligned d-vector 1 (windows 2, 3, 4) straddles
    st = _spans_case([(0, 30 * HOP_N), (10000, 10000 + 40 * HOP_N + 7), (30000, 90000)])
    assert (st[:, 2] == 1).sum() == 2 and (st[:, 2] == 0).sum() == 2
    _spans_case([(0, 30000), (30000, 64000)])                     # touching ranges stay two
    for d in (-1, 0, 1):                                           # an exact multiple of hop_n, and one off
        _spans_case([(0, 200 * HOP_N + d)])
        _spans_case([(777, 777 + 37 * HOP_N + d), (20000, 20000 + 100 * HOP_N + d)])
        _spans_case([(5, 5 + 36 * HOP_N + d)])                     # 37 frames is where the second window appears
    for empty in ([], [(0, 3000)], [(10, 10 + 24 * HOP_N - 1), (9000, 9100)]):
        assert _spans_case(empty).shape == (0, 3)
    from pytorch_speaker_verification_amd import dvector
    assert np.array_equal(dvector.aligned_spans([(0, 80000)], sr=SR), _spans_case([(0, 80000)]))
    half = dvector.aligned_spans([(0, 40000)], sr=SR // 2)  # hop_n = 80: the same frames, half the samples
    assert np.array_equal(half[:, :2] * 2, _spans_case([(0, 80000)])[:, :2])


def test_segments_merge_and_times():
    from pytorch_speaker_verification_amd import diarization as D
    spans = [np.array([[0, 3840, 0], [3840, 8000, 1], [8000, 9000, 2], [12000, 16000, 2], [16000, 20000, 3]]),
             np.zeros((0, 3), dtype=np.int64)]
    labels = [np.array([0, 0, 1, 1]), np.zeros(0, dtype=np.int64)]
    segs = D.segments(labels, spans)
    # 0, 1 merge (label 0, touching); 2 has label 1; the gap 9000 .. 12000 splits label 1; 3 merges into it
    assert segs == [[(0.0, 8000 / SR, 0), (8000 / SR, 9000 / SR, 1), (12000 / SR, 20000 / SR, 1)], []]
    assert all(isinstance(v, float) for s in segs[0] for v in s[:2]) and isinstance(segs[0][0][2], int)
    assert D.segments(labels, spans, sr=8000)[0][0] == (0.0, 1.0, 0)
    with pytest.raises(ValueError):
        D.segments([np.array([0, 0, 1])], spans[:1])  # the spans name a fourth d-vector


def test_rttm_round_trip(tmp_path):
    from pytorch_speaker_verification_amd import diarization as D
    rng = np.random.default_rng(5)
    files = []
    for f in range(3):
        cuts = np.sort(rng.choice(36000 * SR, size=40, replace=False))  # up to ten hours
        files.append([(int(a) / SR, int(b) / SR, int(rng.integers(0, 4))) for a, b in zip(cuts[0::2], cuts[1::2])])
    files.insert(1, [])
    ids = ["rec0", "empty", "rec-2", "rec_3"]
    path = str(tmp_path / "hyp.rttm")
    D.write_rttm(path, ids, files)
    text = open(path).read()
    assert text.count("SPEAKER rec0 1 ") == 20 and "<NA> <NA> 3 <NA> <NA>\n" in text
    with open(path, "a") as f:
        f.write(";; a comment\nSPKR-INFO rec0 1 <NA> <NA> <NA> unknown 3 <NA> <NA>\n\n")
    got = D.read_rttm(path)
    assert sorted(got) == ["rec-2", "rec0", "rec_3"]
    assert D.read_rttm(path, file_ids=ids)["empty"] == []
    for fid, want in zip(ids, files):
        have = got.get(fid, [])
        assert len(have) == len(want)
        for (s0, e0, n0), (s1, e1, n1) in zip(have, want):
            assert (round(s0 * SR), round(e0 * SR), n0) == (round(s1 * SR), round(e1 * SR), str(n1))
    with pytest.raises(ValueError):
        D.write_rttm(path, ["a b"], [[]])
    with pytest.raises(ValueError):
        D.write_rttm(path, ["a"], [[(0.0, 1.0, "two words")]])


def _check_assignment(C):
    from pytorch_speaker_verification_amd import diarization as D
    col, total = D.assignment(C)
    used = col[col >= 0]
    assert col.shape == (C.shape[0],) and len(set(used.tolist())) == used.size == min(C.shape)
    assert total == sum(int(C[r, c]) for r, c in enumerate(col) if c >= 0)
    return total


def test_assignment_reaches_the_brute_force_maximum():
    rng = np.random.default_rng(11)
    for R_ in range(1, 6):
        for K in range(1, 6):
            for trial in range(12):
                C = rng.integers(0, (3, 1000, 2 ** 40)[trial % 3], (R_, K))  # small ranges: many ties
                if trial % 4 == 1:
                    C[rng.integers(0, R_)] = 0  # an all-zero row
                if trial % 4 == 2:
                    C[:, rng.integers(0, K)] = 0
                assert _check_assignment(C) == R.best_total(C), C
    assert _check_assignment(np.zeros((3, 4), dtype=np.int64)) == 0
    assert _check_assignment(np.zeros((0, 4), dtype=np.int64)) == 0 and _check_assignment(np.zeros((2, 0), dtype=np.int64)) == 0
    assert _check_assignment(np.array([[5, 5], [5, 5]])) == 10
    assert _check_assignment(np.array([[1, 2], [3, 100]])) == 101      # not the greedy row-by-row answer's sum
    assert _check_assignment(np.array([[10, 9], [9, 0]])) == 18


def test_assignment_at_32_against_scipy():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(12)
    for shape in ((32, 32), (32, 17), (9, 32)):
        for hi in (4, 10 ** 6):
            C = rng.integers(0, hi, shape)
            r, c = opt.linear_sum_assignment(C, maximize=True)
            assert _check_assignment(C) == int(C[r, c].sum())


N10 = 10 * SR  # a 10 s file: 1000 frames of 160 samples, centres at 160 i + 80


def _der(ref, hyp, **kw):
    res = R.der([ref], [hyp], [N10], **kw)
    return tuple(int(res[k][0]) for k in ("total", "miss", "fa", "conf")), res


def test_oracle_known_answers():
    ref = [(0.0, 5.0, "A"), (5.0, 10.0, "B")]
    hyp = [(0.0, 6.0, "x"), (6.0, 10.0, "y")]
    # collar 0: A owns frames 0 .. 499, B 500 .. 999; x 0 .. 599, y 600 .. 999.  C[A][x] = 500, C[B][x] = 100,
    # C[B][y] = 400: A -> x, B -> y is correct on 900 frames, the 100 frames of [5, 6) s are confused
    got, res = _der(ref, hyp, collar=0.0)
    assert got == (1000, 0, 0, 100) and res["der"] == 0.1 and res["file_der"][0] == 0.1
    # collar 0.25 s = 4000 samples around the boundaries at 0, 80 000 (twice) and 160 000 samples, clamped to the
    # file: [0, 4000) holds the centres 80 .. 3920, frames 0 .. 24 (25); [76 000, 84 000) frames 475 .. 524 (50);
    # [156 000, 160 000) frames 975 .. 999 (25).  900 frames are scored: A 25 .. 474, B 525 .. 974.
    # C[A][x] = 450, C[B][x] = |525 .. 599| = 75, C[B][y] = |600 .. 974| = 375: correct 825, conf 75
    got, res = _der(ref, hyp, collar=0.25)
    assert got == (900, 0, 0, 75) and res["der"] == 75 / 900
    # reference boundaries outside the file, at -1 s and 12 s, are clamped to 0 and 160 000 samples before the
    # collars are built, so the collars are the ones above ([0, 4000) and [156 000, 160 000)) and nothing changes;
    # collars around the unclamped positions would end at -0.75 s and start at 11.75 s and leave the file's first and
    # last 25 frames scored: (950, 0, 0, 75)
    out = [(-1.0, 5.0, "A"), (5.0, 12.0, "B")]
    assert _der(out, hyp, collar=0.25)[0] == (900, 0, 0, 75) and _der(out, hyp, collar=0.0)[0] == (1000, 0, 0, 100)
    # a reference row that lies past the file, C on [11, 12) s, is empty after clamping, yet its boundaries are
    # reference boundaries at the file's end: the collar [156 000, 160 000) leaves frames 975 .. 999 unscored.  With B
    # ending at 9 s (collar [140 000, 148 000): frames 875 .. 924) the scored frames are A 25 .. 474 (450) and
    # B 525 .. 874 (350); y runs on over silence and is a false alarm on the scored frames 925 .. 974 (50; it would be
    # 75 without C's collar); C[B][x] = 75 as before
    late = [(0.0, 5.0, "A"), (5.0, 9.0, "B"), (11.0, 12.0, "C")]
    assert _der(late, hyp, collar=0.25)[0] == (800, 0, 50, 75)
    # reference overlap on [4, 6) s (frames 400 .. 599, Nr = 2) under one hypothesis speaker at a time:
    # total = 600 + 600, one of the two is missed on 200 frames, min(Nr, Nh) = 1 everywhere = 1000 = C[A][x] + C[B][y]
    ref2 = [(0.0, 6.0, "A"), (4.0, 10.0, "B")]
    hyp2 = [(0.0, 5.0, "x"), (5.0, 10.0, "y")]
    got, res = _der(ref2, hyp2, collar=0.0)
    assert got == (1200, 200, 0, 0) and res["der"] == 200 / 1200
    # skip_overlap drops those 200 frames: A 0 .. 399 under x, B 600 .. 999 under y
    got, res = _der(ref2, hyp2, collar=0.0, skip_overlap=True)
    assert got == (800, 0, 0, 0) and res["der"] == 0.0
    # a hypothesis speaker over reference silence: x on [0, 7) s, A on [0, 5) s -> 200 frames of false alarm
    got, res = _der([(0.0, 5.0, "A")], [(0.0, 7.0, "x")], collar=0.0)
    assert got == (500, 0, 200, 0) and res["der"] == 0.4
    # no hypothesis at all: everything is missed; no reference at all: total = 0 and the rate is nan
    assert _der(ref, [], collar=0.0)[0] == (1000, 1000, 0, 0)
    got, res = _der([], hyp, collar=0.0)
    assert got == (0, 0, 1000, 0) and np.isnan(res["file_der"][0]) and np.isnan(res["der"])
    # a UEM of [2, 8) s scores frames 200 .. 799: A 300, B 300, the confusion of [5, 6) s is inside
    got, _ = _der(ref, hyp, collar=0.0, uem=[[(2.0, 8.0)]])
    assert got == (600, 0, 0, 100)
    # the frame rule at a centre: a segment that starts exactly at c_3 = 560 holds frame 3, one that ends there does not
    off = [0, 10]
    assert R.raster([560], [1000], [1], [0], off, 160).tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0, 0]   # c_6 = 1040
    assert R.raster([0], [560], [4], [0], off, 160).tolist() == [4, 4, 4, 0, 0, 0, 0, 0, 0, 0]


def test_split_rows_covers_the_same_frames():
    from pytorch_speaker_verification_amd import diarization as D
    off = np.array([0, 700, 700, 1500])
    s, e = np.array([-50, 3, 900, 10, 40, 0]), np.array([5000, 3, 100, 11, 4000, 10 ** 6])
    b, f = np.array([1, 2, 4, 8, 1 << 31, 16], dtype=np.uint32), np.array([0, 0, 2, 2, 2, 3])
    for step, piece in ((7, 64), (1, 100), (7, 5)):
        ps, pe, pb, pf = D.split_rows(s, e, b, f, step, piece)
        assert ps.size > s.size and np.all((pe - ps <= piece * step) | (pe <= ps))
        assert np.array_equal(R.raster(ps, pe, pb, pf, off, step), R.raster(s, e, b, f, off, step))
    same = D.split_rows(s[:4], e[:4], b[:4], f[:4], 160, 2048)
    assert np.array_equal(same[0], s[:4]) and np.array_equal(same[1], e[:4])


def test_too_many_speakers_is_an_error_before_anything_runs():
    from pytorch_speaker_verification_amd import diarization as D
    many = [(i * 0.1, i * 0.1 + 0.1, f"s{i}") for i in range(33)]
    with pytest.raises(ValueError, match="more than 32 reference"):
        D.der([many], [[]], [N10])
    with pytest.raises(ValueError, match="more than 32 hypothesis"):
        D.der([[]], [many], [N10])
    with pytest.raises(ValueError):
        D.der([[]], [[]], [N10, N10])


def test_header_and_bindings():
    from pytorch_speaker_verification_amd import _lib
    h = _lib.lib()
    a, b, c, d, t, m = 4096, 8192, 16384, 32768, 1 << 20, 1 << 21

    def rs(s=a, e=b, bits=c, file=d, n_seg=5, off=t, F=3, step=160, n_total=100, mask=m):
        return h.sv_seg_raster(s, e, bits, file, n_seg, off, F, step, n_total, mask, None)

    assert rs(s=None) == -1 and rs(e=None) == -1 and rs(bits=None) == -1 and rs(file=None) == -1
    assert rs(off=None) == -1 and rs(mask=None) == -1 and rs(F=0) == -1 and rs(step=0) == -1 and rs(n_seg=-1) == -1
    assert rs(n_total=-1) == -1 and rs(mask=m + 2) == -2 and rs(s=a + 1) == -2
    assert rs(n_seg=0) == 0 and rs(n_total=0) == 0  # nothing to do: no launch

    def dc(ref=a, hyp=b, ns=c, uem=None, off=t, F=3, max_frames=50, n_total=100, out=m):
        return h.sv_der_count(ref, hyp, ns, uem, off, F, max_frames, n_total, 0, out, None)

    assert dc(ref=None) == -1 and dc(hyp=None) == -1 and dc(ns=None) == -1 and dc(off=None) == -1 and dc(out=None) == -1
    assert dc(F=0) == -1 and dc(max_frames=-1) == -1 and dc(n_total=-1) == -1
    assert dc(ref=a + 4) == -2 and dc(uem=d + 8) == -2 and dc(out=m + 4) == -2 and dc(off=t + 2) == -2
    assert dc(F=65536) == -3

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "sv_ge2e.h")).read()
    assert "#define SV_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12
    assert "diarization scoring on a frame grid (added under v12; additive)" in header
    for proto in ("int sv_seg_raster(const int* seg_start, const int* seg_end, const unsigned* seg_bits, const int* seg_file, int n_seg,",
                  "int sv_der_count(const unsigned* ref, const unsigned* hyp, const unsigned* noscore, const unsigned* uem,"):
        assert proto in header, proto
    for rule in ("c_i = i * step + step / 2", "s <= c_i < e", "miss = sum max(0, Nr - Nh)"):
        assert rule in header, rule
    for name, nargs in {"sv_seg_raster": 11, "sv_der_count": 11}.items():
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        start = header.index(f"int {name}(")
        assert header[start:header.index(";", start)].count(",") == nargs - 1, name
