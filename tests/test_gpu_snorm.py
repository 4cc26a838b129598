"""GPU: adaptive score normalisation -- the per-row top-K cohort statistics (sv_cohort_topk_stats,
csrc/sv_snorm.hip) and the histograms of the normalised score (sv_trial_hist_norm, csrc/sv_trials.hip)
against the numpy oracle (snorm_ref.py, verification_ref.py), and evaluate(cohort=...) above them."""
import itertools

import numpy as np
import pytest
import torch

import snorm_ref as S
import verification_ref as R
from test_gpu_verification import DELTA, DIMS, SHAPES, _dev, _label_kinds, toy  # noqa: F401 (toy: a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
# mean and std of exactly representable scores: fp64 sums of <= 65 535 fp32 values are good to 1e-11, the
# one rounding to fp32 is 2^-24 relative; the factor 4 leaves room for the kernel's sums shifted by tau
EXACT = 2.0 ** -22


def _V():
    from pytorch_speaker_verification_amd import verification
    return verification


def _stats(V, x, c, k, grid=0, sliced=False):
    m, s = V.cohort_stats(_dev(x, sliced), _dev(c, sliced), k, grid=grid)
    assert m.dtype == s.dtype == torch.float32 and m.shape == s.shape == (x.shape[0],) and m.is_cuda
    return m.cpu().numpy().astype(np.float64), s.cpu().numpy().astype(np.float64)


def _top_ks(nc):
    return sorted({k for k in (1, 2, nc // 2, nc - 1, nc) if 1 <= k <= nc})


@pytest.mark.parametrize("n", [1, 127, 129, 300])
def test_stats_of_exact_scores(n):
    """Case 1.  Dyadic rows: every score is exact in fp32 in any order, so the kernel's scores are the
    oracle's and mean and std are within 2^-22 max|s| of it -- for every Nc, D, top_k, grid and stride."""
    V = _V()
    rng = np.random.default_rng(100 + n)
    n_cases, worst = 0, 0.0
    for nc, D in itertools.product((1, 127, 129, 700), (4, 36, 256)):
        x, c = R.dyadic_rows(rng, n, D), R.dyadic_rows(rng, nc, D)
        s = R.scores(x, c)
        bound = EXACT * float(np.abs(s).max())
        for k in _top_ks(nc):
            want_m, want_s = S.topk_stats(s, k)
            for grid, sliced in ((0, False), (1, False), (3, False), (0, True)):
                m, sd = _stats(V, x, c, k, grid, sliced)
                err = max(float(np.abs(m - want_m).max()), float(np.abs(sd - want_s).max()))
                worst = max(worst, err / bound if bound else err)
                assert err <= bound, (nc, D, k, grid, sliced, err, bound)
                n_cases += 1
    print("worst error / bound:", worst)
    assert n_cases == 3 * 4 * (1 + 5 + 5 + 5)


def test_ties_across_cohort_tiles():
    """Case 2.  Five distinct cohort rows, each repeated 60 times round-robin over three cohort tiles: the
    top_k-th value is shared by rows in different tiles -- at top_k = 60 and 45 with nothing above it
    (n_gt = 0), at top_k = 90 and 61 with a full group above it (n_gt = 60)."""
    V = _V()
    rng = np.random.default_rng(21)
    D, n = 36, 130
    base = R.dyadic_rows(rng, 5, D)
    c = np.tile(base, (60, 1))  # row j is base[j % 5]: every tile holds all five
    x = R.dyadic_rows(rng, n, D)
    s = R.scores(x, c)
    distinct = np.array([np.unique(r).size == 5 for r in s])
    assert distinct.sum() > n // 2  # (a row may score two base rows alike: more ties, still checked)
    bound = EXACT * float(np.abs(s).max())
    seen = set()
    for k in (45, 60, 61, 90, 299, 300):
        srt = np.sort(s, axis=1)
        kth = srt[:, -k]
        n_gt, n_eq = (s > kth[:, None]).sum(axis=1), (s == kth[:, None]).sum(axis=1)
        assert np.all(n_eq[distinct] == 60)
        seen |= {(k, int(v)) for v in n_gt[distinct]}
        want_m, want_s = S.topk_stats(s, k)
        for grid in (0, 1):
            m, sd = _stats(V, x, c, k, grid)
            assert np.abs(m - want_m).max() <= bound and np.abs(sd - want_s).max() <= bound, (k, grid)
    assert {(45, 0), (60, 0), (61, 60), (90, 60), (300, 240)} <= seen


def test_cancellation_in_the_variance():
    """Case 3.  D = 4, rows of ones against cohort rows that sum to 3.5 + m 2^-10 with 100 distinct m < 128
    (and 400 rows that score at most 3): the top 100 scores are distinct, within 2^-3 of one another, at
    magnitude >= 3.5.  std is within 2^-22 max|s| of the oracle; a fp32 sum(s^2) - sum(s)^2 / K is not."""
    V = _V()
    rng = np.random.default_rng(33)
    n, k = 130, 100
    m = rng.permutation(128)[:k]
    top = np.full((k, 4), 0.875)
    split = rng.integers(0, m + 1)
    top[:, 0] += split * 2.0 ** -10
    top[:, 2] += (m - split) * 2.0 ** -10
    low = rng.integers(0, 7, size=(400, 4)) / 8.0
    c = np.concatenate([top, low])[rng.permutation(500)].astype(np.float32)
    x = np.ones((n, 4), dtype=np.float32)
    s = R.scores(x, c)
    topk = np.sort(s, axis=1)[:, -k:]
    assert np.all(np.diff(topk, axis=1) > 0) and np.all(topk[:, -1] - topk[:, 0] < 2.0 ** -3) and topk.min() >= 3.5
    assert np.sort(s, axis=1)[:, -k - 1].max() <= 3.0
    bound = EXACT * float(np.abs(s).max())
    want_m, want_s = S.topk_stats(s, k)
    f = np.float32
    s1, s2 = f(0), f(0)
    for v in topk[0].astype(f):
        s1, s2 = f(s1 + v), f(s2 + f(v * v))
    naive = np.sqrt(max(float(f(f(s2 - f(f(s1 * s1) / f(k))) / f(k))), 0.0))
    print("fp32 sum-of-squares std error:", abs(naive - want_s[0]), "bound:", bound)
    assert abs(naive - want_s[0]) > bound  # (the formulation this case exists to catch)
    for grid in (0, 1):
        mean, sd = _stats(V, x, c, k, grid)
        print("kernel std error:", float(np.abs(sd - want_s).max()))
        assert np.abs(mean - want_m).max() <= bound and np.abs(sd - want_s).max() <= bound


@pytest.fixture(scope="module")
def real():
    """Real-valued unit rows, D = 256: 300 trial rows, a cohort of 300 rows of other speakers, the fp64
    scores of the trial rows (and of the cohort rows) against the cohort.  Computed once, read-only."""
    x, lab = R.speaker_rows()
    c, _ = R.speaker_rows(seed=1)
    out = (x, lab, c, R.scores(x, c))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("k", [1, 20, 299, 300])
def test_stats_of_real_valued_unit_rows(real, k):
    """Case 4.  A fp32 dot product of unit rows is within DELTA of the fp64 one (test_gpu_verification.py),
    and order statistics, the mean and the population std of the top K are 1-Lipschitz in the largest
    score error: mean and std within DELTA of the oracle on the fp64 scores."""
    V = _V()
    x, _, c, s = real
    want_m, want_s = S.topk_stats(s, k)
    m, sd = _stats(V, x, c, k)
    print("mean err", float(np.abs(m - want_m).max()), "std err", float(np.abs(sd - want_s).max()))
    assert np.abs(m - want_m).max() <= DELTA and np.abs(sd - want_s).max() <= DELTA
    assert want_s.min() > 1e-3 or k == 1


def test_nan_reaches_its_own_row_only():
    """Case 5."""
    V = _V()
    rng = np.random.default_rng(5)
    x, c = R.dyadic_rows(rng, 131, 8), R.dyadic_rows(rng, 140, 8)
    s = R.scores(x, c)
    bound = EXACT * float(np.abs(s).max())
    xn = x.copy()
    xn[77, 3] = np.nan
    for k in (1, 7, 140):
        m, sd = _stats(V, xn, c, k)
        want_m, want_s = S.topk_stats(s, k)
        assert np.isnan(m[77]) and np.isnan(sd[77])
        rest = np.arange(131) != 77
        assert np.abs(m - want_m)[rest].max() <= bound and np.abs(sd - want_s)[rest].max() <= bound
    cn = c.copy()
    cn[133, 0] = np.nan  # in the second cohort tile
    for k in (1, 7, 140):
        m, sd = _stats(V, x, cn, k)
        assert np.isnan(m).all() and np.isnan(sd).all()


# ----------------------------------------------------------------------------- normalised histograms
def _dyadic_norm(rng, n):
    return (rng.integers(-8, 9, n) / 8.0).astype(np.float32), (2.0 ** rng.integers(-1, 3, n)).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}" if s[1] else f"sym{s[0]}")
def test_normalised_counts_are_exact_on_dyadic_inputs(shape):
    """Case 6.  Rows k / 8, mu multiples of 1/8, inv in {1/2, 1, 2, 4}: s is a multiple of 1/64 below D in
    size, so za, zb and z are exact in fp32 (|z| <= 4 (D + 1), a multiple of 2^-8); with [lo, hi) =
    [-8 P, 8 P), P the power of two >= D, and bins a power of two, so is the slot.  Counts equal the
    oracle slot for slot; with mu = 0 and inv = 1 they equal the un-normalised kernel's."""
    V = _V()
    na, nb = shape
    sym = nb is None
    rng = np.random.default_rng(40 + na + (nb or 0))
    n_cases = 0
    for D in (4, 36, 256):
        span = 8.0 * float(1 << int(np.ceil(np.log2(D))))
        a = R.dyadic_rows(rng, na, D)
        b = None if sym else R.dyadic_rows(rng, nb, D)
        s = R.scores(a, b)
        norm_a = _dyadic_norm(rng, na)
        norm_b = norm_a if sym else _dyadic_norm(rng, nb)
        z = S.normalise(s, *norm_a, *norm_b)
        assert np.array_equal(z, S.as_norm_fp64(s, *norm_a, *norm_b)) and np.abs(z).max() < span
        da, db = _dev(a), None if sym else _dev(b)
        dna = tuple(_dev(t) for t in norm_a)
        dnb = None if sym else tuple(_dev(t) for t in norm_b)
        unit_a = (torch.zeros(na, device=DEV), torch.ones(na, device=DEV))
        unit_b = None if sym else (torch.zeros(nb, device=DEV), torch.ones(nb, device=DEV))
        for kind, (la, lb) in _label_kinds(rng, na, na if sym else nb).items():
            live, target = R.pairs(la, None if sym else lb)
            dla, dlb = _dev(la), None if sym else _dev(lb)
            for bins, grid in itertools.product((1, 64, 8192), (0, 1, 3)):
                lo32, hi32, inv = V.bin_params(bins, -span, span)
                want = S.normalised_hist(s, live, target, norm_a, norm_b, lo32, inv, bins)
                h = V.trial_histograms(da, dla, db, dlb, bins=bins, lo=-span, hi=span, grid=grid, norm_a=dna, norm_b=dnb)
                assert np.array_equal(h.counts, want), (D, kind, bins, grid)
                assert int(h.counts.sum()) == int(live.sum())
                n_cases += 1
            plain = V.trial_histograms(da, dla, db, dlb, bins=64, lo=-span, hi=span)
            same = V.trial_histograms(da, dla, db, dlb, bins=64, lo=-span, hi=span, norm_a=unit_a, norm_b=unit_b)
            assert np.array_equal(plain.counts, same.counts), (D, kind)
    assert n_cases == 3 * 3 * 9


def test_normalised_counts_lie_between_the_fp64_counts(real):
    """Case 6, real values.  The 300 unit rows, symmetric, normalised by their own top-20 cohort statistics
    as the GPU computed them: at every edge e the kernel's count of z >= e lies between the fp64 counts of
    z >= e + slack and >= e - slack, slack = DELTA (max inv_a + max inv_b) / 2 -- the score's own error
    through z's slope (the five fp32 roundings of z, at most 6 2^-24 max|z|, fit into what DELTA leaves
    over of the dot product's 256 2^-24)."""
    V = _V()
    x, lab, c, _ = real
    dx, dl = _dev(x), _dev(lab)
    mu, inv = V.as_norm(dx, _dev(c), 20)
    assert np.array_equal(V.trial_histograms(dx, dl, bins=256).counts,
                          V.trial_histograms(dx, dl, bins=256, norm_a=(torch.zeros_like(mu), torch.ones_like(mu))).counts)
    lo, hi = V.norm_range((mu, inv))
    h = V.trial_histograms(dx, dl, bins=256, lo=lo, hi=hi, norm_a=(mu, inv))
    mu64, inv64 = mu.cpu().numpy().astype(np.float64), inv.cpu().numpy().astype(np.float64)
    live, target = R.pairs(lab)
    non, tar = R.split(S.as_norm_fp64(R.scores(x), mu64, inv64, mu64, inv64), live, target)
    assert h.n_nontarget == non.size == 41250 and h.n_target == tar.size == 3600
    assert h.counts[:, 0].sum() == 0 and h.counts[:, -1].sum() == 0  # norm_range holds every z
    slack = DELTA * float(inv64.max())
    assert 6 * 2.0 ** -24 * max(abs(lo), abs(hi)) <= (DELTA - 256 * 2.0 ** -24) * float(inv64.min())
    edges = h.edges()
    acc_non, acc_tar, _, _ = V._accepted(h)
    near = 0
    for got, ref in ((acc_non, non), (acc_tar, tar)):
        lo_cnt, hi_cnt = R.count_ge(ref, edges + slack), R.count_ge(ref, edges - slack)
        assert np.all(lo_cnt <= got) and np.all(got <= hi_cnt)
        near += int((hi_cnt - lo_cnt).sum())
    share = near / float(non.size + tar.size)
    print("range", (lo, hi), "slack", slack, "share of pairs within slack of an edge:", share)
    assert share <= 0.05  # (the sandwich leaves a miscount nowhere to hide)


def test_error_codes_in_the_documented_order():
    """Case 7.  Through _lib.call: SV_EARG before SV_EALIGN before SV_ESHAPE, nothing launched."""
    from pytorch_speaker_verification_amd._lib import call, ptr, stream_of
    x = torch.zeros((8, 16), device=DEV)
    c = torch.zeros((12, 16), device=DEV)
    out = torch.full((2, 8), 7.0, device=DEV)
    lab = torch.zeros(12, dtype=torch.int32, device=DEV)
    hist = torch.zeros(2 * 66, dtype=torch.int64, device=DEV)
    st = stream_of(x)

    def cs(X=ptr(x), ldx=16, N=8, C=ptr(c), ldc=16, Nc=12, D=16, top_k=3, mean=ptr(out[0]), std=ptr(out[1]), grid=0):
        call("sv_cohort_topk_stats", X, ldx, N, C, ldc, Nc, D, top_k, mean, std, grid, st)

    def tn(A=ptr(x), lda=16, Na=8, B=ptr(c), ldb=16, Nb=12, D=16, symmetric=0, n_bins=64, mu_a=ptr(out[0]),
           inv_a=ptr(out[1]), mu_b=ptr(c), inv_b=ptr(c[1]), h=ptr(hist), grid=0):
        call("sv_trial_hist_norm", A, lda, ptr(lab), Na, B, ldb, ptr(lab), Nb, D, symmetric, -1.0, 32.0, n_bins, mu_a,
             inv_a, mu_b, inv_b, h, grid, st)

    for fn, cases in ((cs, [("SV_EARG", dict(top_k=13)), ("SV_EARG", dict(top_k=0)), ("SV_EARG", dict(mean=None)),
                            ("SV_EARG", dict(grid=-1)), ("SV_EARG", dict(top_k=13, X=ptr(x) + 4)),
                            ("SV_EALIGN", dict(X=ptr(x) + 4)), ("SV_EALIGN", dict(D=14)), ("SV_EALIGN", dict(ldx=12)),
                            ("SV_EALIGN", dict(std=ptr(out[1]) + 2, Nc=70000, top_k=3)),
                            ("SV_ESHAPE", dict(Nc=65536)), ("SV_ESHAPE", dict(D=1028, ldx=1028, ldc=1028))]),
                      (tn, [("SV_EARG", dict(mu_b=None)), ("SV_EARG", dict(Na=0, A=ptr(x) + 4)),
                            ("SV_EARG", dict(symmetric=1, B=ptr(x), ldb=16, Nb=8)),  # mu_b is not mu_a
                            ("SV_EALIGN", dict(inv_a=ptr(out[1]) + 2, n_bins=9000)), ("SV_EALIGN", dict(D=14)),
                            ("SV_ESHAPE", dict(n_bins=8193)), ("SV_ESHAPE", dict(D=1028, lda=1028, ldb=1028))])):
        for code, kw in cases:
            with pytest.raises(RuntimeError, match=code):
                fn(**kw)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(hist.sum()) == 0  # nothing ran
    cs()
    tn(symmetric=1, B=ptr(x), ldb=16, Nb=8, mu_b=ptr(out[0]), inv_b=ptr(out[1]))
    torch.cuda.synchronize()
    # (zero rows: mean = std = 0; then mu = inv = 0 gives z = 0, slot 33 of the 28 target pairs)
    assert bool((out == 0.0).all()) and int(hist.view(2, 66)[1, 33]) == 28 == int(hist.sum())
    V = _V()
    with pytest.raises(ValueError, match="top_k = 13 outside"):
        V.cohort_stats(x, c, 13)
    with pytest.raises(ValueError, match="norm_a and norm_b together"):
        V.trial_histograms(x, lab[:8], c, lab, norm_a=(out[0], out[1]))


# ----------------------------------------------------------------------------- the public surface, toy dims
def _oracle_eer(d_a, lab_a, d_b, lab_b, cohort, k, floor=1e-5):
    """Sorted-scores EER of the oracle-normalised fp64 scores, and the two class sizes."""
    sym = d_b is None
    live, target = R.pairs(lab_a, None if sym else lab_b)
    norms = []
    for d in (d_a, d_a if sym else d_b):
        mu, sd = S.topk_stats(R.scores(d, cohort), k)
        norms += [mu, 1.0 / np.maximum(sd, floor)]
    non, tar = R.split(S.as_norm_fp64(R.scores(d_a, None if sym else d_b), *norms), live, target)
    return R.eer_sorted(non, tar)[0], non, tar


def test_evaluate_with_a_cohort_against_the_oracle(toy, tmp_path, capsys):
    """Case 8."""
    from conftest import model_dims
    from pytorch_speaker_verification_amd import data_load
    from pytorch_speaker_verification_amd import train_speech_embedder as tse
    from pytorch_speaker_verification_amd.hparam import hparam as hp
    V = _V()
    net, corpus = toy
    rng = np.random.default_rng(19)
    mean = rng.standard_normal((5, 1, 40, 1))
    cohort_corpus = data_load.DeviceCorpus(
        [(mean[k] + rng.standard_normal((3, 40, 180))).astype(np.float32) for k in range(5)], device=DEV)
    plain = V.evaluate(net, corpus)
    assert sorted(plain) == ["eer", "eer_hi", "eer_lo", "min_dcf", "n_nontarget", "n_target", "threshold"]
    d_dev = V.corpus_dvectors(net, corpus)
    models_dev = V.cohort_models(V.corpus_dvectors(net, cohort_corpus), cohort_corpus.speaker_off)
    assert models_dev.shape == (5, 32) and models_dev.dtype == torch.float32
    assert torch.allclose(models_dev.norm(dim=1), torch.ones(5, device=DEV), atol=1e-6)
    d, models = d_dev.cpu().numpy().astype(np.float64), models_dev.cpu().numpy().astype(np.float64)
    lab = np.repeat(np.arange(3, dtype=np.int32), 4)
    want, non, tar = _oracle_eer(d, lab, None, None, models, 3)
    for cohort in (cohort_corpus, models_dev):
        r = V.evaluate(net, corpus, cohort=cohort, top_k=3)
        print(r, "oracle eer", want)
        assert sorted(r) == sorted(list(plain) + ["n_cohort", "range", "score_norm", "top_k"])
        assert (r["score_norm"], r["top_k"], r["n_cohort"]) == ("as-norm", 3, 5)
        assert (r["n_target"], r["n_nontarget"]) == (plain["n_target"], plain["n_nontarget"]) == (tar.size, non.size)
        assert r["eer_lo"] <= want <= r["eer_hi"] and r["eer_lo"] <= r["eer"] <= r["eer_hi"]
        lo, hi = r["range"]
        assert lo <= min(non.min(), tar.min()) and max(non.max(), tar.max()) < hi
    # enrol on two utterances: the tests and the speaker models are both normalised
    mods = np.stack([d[4 * k:4 * k + 2].mean(axis=0) for k in range(3)])
    mods /= np.linalg.norm(mods, axis=1, keepdims=True)
    tests = np.concatenate([d[4 * k + 2:4 * k + 4] for k in range(3)])
    want2, non2, tar2 = _oracle_eer(tests, np.repeat(np.arange(3), 2), mods, np.arange(3), models, 5)
    r2 = V.evaluate(net, corpus, enroll=2, cohort=models_dev, top_k=5)
    assert (r2["n_target"], r2["n_nontarget"]) == (6, 12) and r2["eer_lo"] <= want2 <= r2["eer_hi"]
    with pytest.raises(ValueError, match="top_k = 300 outside"):
        V.evaluate(net, corpus, cohort=models_dev)
    assert V.evaluate(net, corpus) == plain  # the cohort-less dict, unchanged
    # test(protocol="corpus", cohort=...) returns that EER and says so
    ckpt = str(tmp_path / "toy.pth")
    torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, ckpt)
    ds = data_load.SpeakerDatasetResident(corpus, utter_num=4)
    old_device = hp.device
    try:
        hp.device = DEV
        with model_dims(*DIMS):
            capsys.readouterr()
            got = tse.test(ckpt, dataset=ds, protocol="corpus", cohort=models_dev, top_k=3)
            out = capsys.readouterr().out
            assert tse.test(ckpt, dataset=ds, protocol="corpus") == plain["eer"]
            with pytest.raises(ValueError, match="needs protocol='corpus'"):
                tse.test(ckpt, dataset=ds, cohort=models_dev)
    finally:
        hp.device = old_device
    assert got == r["eer"] and "AS-norm top 3 of 5" in out
    line = tse._corpus_line(net, corpus, "Epoch:1\t", models_dev, 3)
    assert line.startswith("Epoch:1\tcorpus EER:{0:.4f} [".format(r["eer"])) and line.endswith("\tAS-norm top 3 of 5\t\n")
    assert "AS-norm" not in tse._corpus_line(net, corpus)
