"""CPU: the AS-norm oracle (snorm_ref.py) against brute force on tiny cases -- ties, k = 1, k = Nc, the
key order of negatives and +-0 -- and the host-side half of the new entry points: argument codes in
the documented order, the header's contracts, norm_range."""
import math
import os

import numpy as np
import pytest

import snorm_ref as S


def _brute(row, k):
    """mean and population std of the k largest of a list, NaN largest, plain Python."""
    top = sorted(row, key=lambda v: (math.isnan(v), v))[len(row) - k:]
    m = math.fsum(top) / k
    return m, math.sqrt(math.fsum((v - m) ** 2 for v in top) / k)


CASES = {
    "distinct": [0.5, -0.25, 0.75, 0.125, -1.0, 0.0],
    "ties at the cut": [0.5, 0.5, 0.5, 0.25, 0.75, 0.5, -0.5],
    "all equal": [0.375] * 5,
    "negatives": [-0.5, -0.25, -2.0, -0.125, -0.125, -3.0],
    "zeros": [0.0, -0.0, 0.0, -0.0, -1.0],
    "across exponents": [1e-30, 3.0, -1e-30, 2.0 ** -10, 1.5, 1.0, -4.0, 2.0 ** -126],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_brute_force(name):
    row = CASES[name]
    for k in range(1, len(row) + 1):  # k = 1 and k = Nc included
        want_m, want_s = _brute(row, k)
        m, s = S.topk_stats(np.array([row, row[::-1]]), k)
        assert np.allclose(m, want_m, rtol=0, atol=1e-15) and np.allclose(s, want_s, rtol=0, atol=1e-15), (name, k)


def test_key_order_of_negatives_zeros_and_nan():
    vals = np.array([-np.inf, -3.0e38, -2.0, -1.0, -2.0 ** -126, -1e-45, -0.0, 0.0, 1e-45, 2.0 ** -126, 0.5, 1.0, 2.0,
                     3.0e38, np.inf], dtype=np.float32)
    keys = S.key32(vals)
    assert np.all(np.diff(keys.astype(np.int64)) > 0)  # strictly rising: -0 sorts just below +0
    assert keys[6] == 0x7FFFFFFF and keys[7] == 0x80000000
    nan = np.array([np.nan, -np.nan, np.float32(np.nan)], dtype=np.float32)
    assert np.all(S.key32(nan) == 0xFFFFFFFF) and np.all(S.key32(nan) > keys[-1])
    rng = np.random.default_rng(0)
    x = rng.standard_normal(1000).astype(np.float32)
    assert np.array_equal(np.argsort(S.key32(x), kind="stable"), np.argsort(x, kind="stable"))


def test_nan_rows():
    s = np.array([[0.5, np.nan, 0.25, 0.125], [0.5, 0.75, 0.25, 0.125]])
    m, sd = S.topk_stats(s, 2)
    assert np.isnan(m[0]) and np.isnan(sd[0]) and m[1] == 0.625 and sd[1] == 0.125


def test_normalise_is_the_literal_fp32_formula():
    rng = np.random.default_rng(1)
    s = (rng.integers(-64, 65, size=(5, 7)) / 64.0).astype(np.float32)
    mu_a, mu_b = rng.integers(-8, 9, 5) / 8.0, rng.integers(-8, 9, 7) / 8.0
    inv_a, inv_b = 2.0 ** rng.integers(-1, 3, 5), 2.0 ** rng.integers(-1, 3, 7)
    z = S.normalise(s, mu_a, inv_a, mu_b, inv_b)
    assert z.dtype == np.float32 and np.array_equal(z, S.as_norm_fp64(s, mu_a, inv_a, mu_b, inv_b))  # dyadic: exact
    assert np.array_equal(S.normalise(s, np.zeros(5), np.ones(5), np.zeros(7), np.ones(7)), s)
    # real values: one element by hand, rounding after every operation
    f = np.float32
    s1, ma, ia, mb, ib = f(0.3), f(0.11), f(7.3), f(-0.07), f(12.9)
    want = f(f(0.5) * f(f(f(s1 - ma) * ia) + f(f(s1 - mb) * ib)))
    assert S.normalise([[s1]], [ma], [ia], [mb], [ib])[0, 0] == want


def test_abi_argument_codes_and_header():
    """SV_EARG -1, SV_EALIGN -2, SV_ESHAPE -3 in the documented order, all host-side and before any
    launch (the pointers are never dereferenced)."""
    from pytorch_speaker_verification_amd import _lib
    h = _lib.lib()
    p, q = 4096, 8192

    def cs(X=p, ldx=256, N=100, C=q, ldc=256, Nc=500, D=256, top_k=300, mean=p, std=q, grid=0):
        return h.sv_cohort_topk_stats(X, ldx, N, C, ldc, Nc, D, top_k, mean, std, grid, None)

    assert cs(X=None) == -1 and cs(C=None) == -1 and cs(mean=None) == -1 and cs(std=None) == -1
    assert cs(N=0) == -1 and cs(Nc=0) == -1 and cs(D=0) == -1 and cs(top_k=0) == -1 and cs(grid=-1) == -1
    assert cs(top_k=501) == -1
    assert cs(X=p + 4) == -2 and cs(C=q + 8) == -2 and cs(mean=p + 2) == -2 and cs(std=q + 1) == -2
    assert cs(ldx=258) == -2 and cs(ldc=257) == -2 and cs(D=254) == -2 and cs(ldx=252) == -2 and cs(ldc=128) == -2
    assert cs(Nc=65536) == -3 and cs(D=1028, ldx=1028, ldc=1028) == -3
    assert cs(Nc=65536, X=p + 4) == -2 and cs(Nc=65536, top_k=0) == -1 and cs(Nc=65536, top_k=65537) == -1

    def tn(A=p, lda=256, lab_a=p, Na=100, B=q, ldb=256, lab_b=q, Nb=70, D=256, symmetric=0, n_bins=4096, mu_a=p,
           inv_a=q, mu_b=p + 512, inv_b=q + 512, hist=p, grid=0):
        return h.sv_trial_hist_norm(A, lda, lab_a, Na, B, ldb, lab_b, Nb, D, symmetric, -1.0, 2048.0, n_bins, mu_a,
                                    inv_a, mu_b, inv_b, hist, grid, None)

    assert tn(A=None) == -1 and tn(hist=None) == -1 and tn(Na=0) == -1 and tn(n_bins=0) == -1 and tn(grid=-1) == -1
    assert tn(mu_a=None) == -1 and tn(inv_a=None) == -1 and tn(mu_b=None) == -1 and tn(inv_b=None) == -1
    sym = dict(B=p, lab_b=p, Nb=100, symmetric=1, mu_b=p, inv_b=q)
    assert tn(symmetric=1) == -1 and tn(**{**sym, "mu_b": p + 512}) == -1 and tn(**{**sym, "inv_b": q + 512}) == -1
    assert tn(A=p + 4) == -2 and tn(D=254) == -2 and tn(mu_a=p + 2) == -2 and tn(inv_b=q + 513) == -2
    assert tn(n_bins=8193) == -3 and tn(D=1028, lda=1028, ldb=1028) == -3
    assert tn(n_bins=8193, mu_a=p + 2) == -2 and tn(n_bins=8193, inv_a=None) == -1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "sv_ge2e.h")).read()
    assert "int sv_cohort_topk_stats(const float* X, long ldx, int N, const float* C, long ldc, int Nc, int D" in header
    assert "int sv_trial_hist_norm(const float* A, long lda, const int* lab_a, int Na, const float* B, long ldb" in header
    for rule in ("za = (s - mu_a[i]) * inv_a[i];", "zb = (s - mu_b[j]) * inv_b[j];", "z = 0.5f * (za + zb);"):
        assert rule in header
    assert "#define SV_ABI_VERSION 12" in header
    assert len(_lib.SIGNATURES["sv_cohort_topk_stats"][1]) == 12 and len(_lib.SIGNATURES["sv_trial_hist_norm"][1]) == 20


def test_norm_range_contains_every_normalised_score():
    import torch
    from pytorch_speaker_verification_amd import verification as V
    rng = np.random.default_rng(2)
    mu_a, mu_b = rng.uniform(-0.2, 0.6, 40).astype(np.float32), rng.uniform(-0.2, 0.6, 9).astype(np.float32)
    inv_a, inv_b = rng.uniform(3, 60, 40).astype(np.float32), rng.uniform(3, 60, 9).astype(np.float32)
    na, nb = (torch.from_numpy(mu_a), torch.from_numpy(inv_a)), (torch.from_numpy(mu_b), torch.from_numpy(inv_b))
    for s_max in (1.0, 4.0):
        lo, hi = V.norm_range(na, nb, s_max=s_max)
        assert np.float32(lo) == lo and np.float32(hi) == hi
        for s in (-s_max, s_max, 0.3):
            z = S.normalise(np.full((40, 9), s, np.float32), mu_a, inv_a, mu_b, inv_b)
            assert lo <= z.min() and z.max() < hi
        z_lo = S.as_norm_fp64(np.full((40, 9), -s_max), mu_a, inv_a, mu_b, inv_b).min()
        z_hi = S.as_norm_fp64(np.full((40, 9), s_max), mu_a, inv_a, mu_b, inv_b).max()
        assert lo < z_lo and z_hi < hi and hi - lo <= (z_hi - z_lo) * (1 + 2.0 ** -18)  # (and no wider than needed)
    lo, hi = V.norm_range(na)  # one side for both
    z = S.normalise(np.full((40, 40), 1.0, np.float32), mu_a, inv_a, mu_a, inv_a)
    assert z.max() < hi and S.normalise(np.full((40, 40), -1.0, np.float32), mu_a, inv_a, mu_a, inv_a).min() >= lo


def test_no_cpu_path_and_argument_checks():
    import torch
    from pytorch_speaker_verification_amd import verification as V
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.cohort_stats(torch.zeros((4, 8)), torch.zeros((5, 8)), 2)
    with pytest.raises(ValueError, match="passes must be >= 1"):
        V._passes(None, None, None, None, 4096, 0)
    with pytest.raises(ValueError, match="lo and hi together"):
        V._passes(None, None, None, None, 4096, 1, lo=0.0)
