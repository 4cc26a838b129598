"""CPU: the diarization oracle (diar_ref.py) on the planted sequences, the identities the pipeline
rests on, and the host-side half of the sv_diar_* entry points: header text, ctypes signatures and
the argument codes, which are returned before any launch (the pointers are never dereferenced)."""
import os

import numpy as np
import pytest

import diar_ref as R


@pytest.mark.parametrize("case", R.PLANTED)
def test_oracle_recovers_the_planted_cases(case):
    n, k, run = case
    for seed in (0, 1, 2):
        x, lab = R.planted(n, k, run, seed)
        got, k_hat, lam, margin = R.cluster(x)
        assert margin >= 1.5, (case, seed, margin)  # the eigengap is not a close call
        assert k_hat == k and np.array_equal(got, R.relabel(lab)), (case, seed, k_hat)
        assert np.all(lam[:-1] >= lam[1:])


def test_symmetric_normalisation_is_similar_to_the_papers():
    """S = D^-1/2 Z D^-1/2 has the eigenvalues of R = D^-1 Z, and D^-1/2 u are R's eigenvectors."""
    for n, k, run in ((40, 2, 5), (257, 5, 8)):
        x, _ = R.planted(n, k, run, 0)
        B = R.crop_blur(R.affinity(x), R.taps(1.0))
        _, Y = R.threshold_sym(B, R.q_rank(n, 0.95))
        Z = Y @ Y.T
        S, d = R.row_norm(Z)
        assert np.array_equal(S, S.T)
        Rm = Z / d[:, None]
        ev_r = np.sort(np.linalg.eigvals(Rm).real)
        ev_s = np.linalg.eigvalsh(S)
        assert np.abs(ev_r - ev_s).max() <= 1e-11 * ev_s.max()
        lam, U = R.top_eig(S)
        v = U[:, 0] / np.sqrt(d)
        assert np.abs(Rm @ v - lam[0] * v).max() <= 1e-11 * np.abs(v).max() * lam[0]
        assert S.max() <= 1.0 + 1e-12 and np.linalg.eigvalsh(S).min() >= -1e-10


def test_threshold_rank_rule():
    from pytorch_speaker_verification_amd import diarization as D
    for n, want in ((2, 0), (3, 1), (21, 19)):
        assert R.q_rank(n, 0.95) == want and D.threshold_rank(n, 0.95) == want
    assert D.threshold_rank(21, 0.0) == 0 and D.threshold_rank(21, 1.0) == 20
    row = np.arange(21, dtype=np.float64)[None, ::-1].repeat(21, axis=0)
    assert np.array_equal(R.row_tau(row, 19), np.full(21, 19.0))


def test_tables_taps_and_eigengap():
    from pytorch_speaker_verification_amd import diarization as D
    tb = D.matrix_tables([2, 257, 5])
    assert tb.row_off.dtype == np.int32 and tb.row_off.tolist() == [0, 2, 259, 264]
    assert tb.ld.tolist() == [4, 260, 8] and tb.mat_off.dtype == np.int64
    assert tb.mat_off.tolist() == [0, 8, 8 + 257 * 260] and tb.elems == 8 + 257 * 260 + 40 and tb.n_max == 257
    with pytest.raises(ValueError):
        D.matrix_tables([1, 5])
    with pytest.raises(ValueError):
        D.matrix_tables([8193])
    for sigma in (0, 1.0, 2.5):
        assert np.array_equal(D.gaussian_taps(sigma), R.taps(sigma))
    assert D.gaussian_taps(0).tolist() == [1.0] and D.gaussian_taps(2.5).size == 9
    with pytest.raises(ValueError):
        D.gaussian_taps(3.0)  # r = 9
    lam = np.array([1.0, 0.9, 0.1, 0.09, 0.05] + [0.01] * 11)
    assert D.n_speakers(lam, 40) == R.n_speakers(lam, 40) == 2
    assert D.n_speakers(lam, 40, k_min=3) == R.n_speakers(lam, 40, k_min=3) == 5  # 0.05 / 0.01
    assert D.n_speakers(lam, 2) == 1 and D.n_speakers(lam, 1) == 1
    low_rank = np.array([1.0, 1.0, 3e-17, -2e-17] + [0.0] * 12)
    assert D.n_speakers(low_rank, 64) == R.n_speakers(low_rank, 64) == 2  # the floor, not the noise
    assert D.relabel([3, 3, 0, 3, 1, 0]).tolist() == R.relabel([3, 3, 0, 3, 1, 0]).tolist() == [0, 0, 1, 0, 2, 1]


def test_kmeans_oracle_rules():
    E = np.array([[0.0, 0], [0.1, 0], [5, 0], [5.2, 0], [0, 9]])
    lab, it, margin = R.kmeans(E, 3)
    assert lab.tolist() == [0, 0, 2, 2, 1] and it == 2 and margin > 1  # farthest-first: rows 0, 4, 3
    assert R.kmeans(E, 1)[0].tolist() == [0] * 5 and R.kmeans(E[:2], 2)[0].tolist() == [0, 1]
    # an empty cluster keeps its centre: the third centre is a second copy of row 0, and ties go to centre 0
    lab2, it2, _ = R.kmeans(np.array([[0.0, 0], [0, 0], [3, 0]]), 3)
    assert lab2.tolist() == [0, 0, 1] and it2 == 2


def test_abi_argument_codes_and_header():
    from pytorch_speaker_verification_amd import _lib
    h = _lib.lib()
    a, b, c, t = 4096, 8192, 16384, 1 << 20
    taps = (np.ones(9, dtype=np.float32))
    tp = taps.ctypes.data

    def cb(A=a, B=b, row_off=t, mat_off=t + 64, F=3, n_max=100, taps=tp, r=3):
        return h.sv_diar_crop_blur(A, B, row_off, mat_off, F, n_max, taps, r, None)

    assert cb(A=None) == -1 and cb(B=None) == -1 and cb(row_off=None) == -1 and cb(mat_off=None) == -1
    assert cb(taps=None) == -1 and cb(F=0) == -1 and cb(n_max=0) == -1 and cb(r=-1) == -1 and cb(B=a) == -1
    assert cb(A=a + 4) == -2 and cb(B=b + 8) == -2 and cb(row_off=t + 2) == -2 and cb(mat_off=t + 4) == -2
    assert cb(n_max=8193) == -3 and cb(F=65536) == -3 and cb(r=9) == -3
    assert cb(n_max=8193, A=a + 4) == -2 and cb(n_max=8193, A=None) == -1

    def rs(B=a, row_off=t, mat_off=t + 64, F=3, n_max=100, q=t + 128, tau=b):
        return h.sv_diar_row_select(B, row_off, mat_off, F, n_max, q, tau, None)

    assert rs(B=None) == -1 and rs(q=None) == -1 and rs(tau=None) == -1 and rs(F=0) == -1
    assert rs(B=a + 4) == -2 and rs(q=t + 2) == -2 and rs(n_max=8193) == -3

    def ts(B=a, tau=c, Y=b, row_off=t, mat_off=t + 64, F=3, n_max=100):
        return h.sv_diar_thresh_sym(B, tau, 0.01, Y, row_off, mat_off, F, n_max, None)

    assert ts(B=None) == -1 and ts(tau=None) == -1 and ts(Y=None) == -1 and ts(Y=a) == -1
    assert ts(Y=b + 4) == -2 and ts(n_max=8193) == -3

    def rn(Z=a, S=b, d=c, r=c + 4096, row_off=t, mat_off=t + 64, F=3, n_max=100):
        return h.sv_diar_row_norm(Z, S, d, r, row_off, mat_off, F, n_max, None)

    assert rn(Z=None) == -1 and rn(S=None) == -1 and rn(d=None) == -1 and rn(r=None) == -1
    assert rn(r=c + 4) == -2 and rn(n_max=8193) == -3

    def sp(S=a, W=b, T=c, P=c + 4096, row_off=t, mat_off=t + 64, F=3, n_max=100):
        return h.sv_diar_spmm(S, W, T, P, row_off, mat_off, F, n_max, None)

    assert sp(S=None) == -1 and sp(W=None) == -1 and sp(T=None) == -1 and sp(P=None) == -1 and sp(P=b) == -1
    assert sp(W=b + 8) == -2 and sp(T=c + 4) == -2 and sp(n_max=8193) == -3 and sp(F=65536) == -3

    def gr(X=a, Y=b, G=c, ws=c + 4096, row_off=t, F=3, n_max=100):
        return h.sv_diar_gram(X, Y, G, ws, row_off, F, n_max, None)

    assert gr(X=None) == -1 and gr(G=None) == -1 and gr(ws=None) == -1 and gr(n_max=0) == -1
    assert gr(G=c + 4) == -2 and gr(X=a + 2) == -2 and gr(n_max=8193) == -3

    def rm(X=a, T=c, Y=b, P=None, lam=None, res2=None, ws=None, row_off=t, F=3, n_max=100):
        return h.sv_diar_rmul(X, T, Y, P, lam, res2, ws, row_off, F, n_max, None)

    assert rm(X=None) == -1 and rm(T=None) == -1 and rm(Y=None) == -1 and rm(Y=a) == -1
    assert rm(P=c + 4096) == -1 and rm(P=c + 4096, lam=t + 256, res2=t + 512) == -1  # residuals need all three
    assert rm(Y=b + 4) == -2 and rm(n_max=8193) == -3

    def km(E=a, row_off=t, k=t + 64, F=3, max_iter=100, labels=b, iters=c):
        return h.sv_diar_kmeans(E, row_off, k, F, max_iter, labels, iters, None)

    assert km(E=None) == -1 and km(k=None) == -1 and km(labels=None) == -1 and km(iters=None) == -1
    assert km(F=0) == -1 and km(max_iter=0) == -1 and km(E=a + 4) == -2 and km(F=65536) == -3
    assert h.sv_diar_workspace(3, 8192) == 3 * 32 * 256 * 8 and h.sv_diar_workspace(3, 8193) == 0
    assert h.sv_diar_workspace(1, 64) == 256 * 8 and h.sv_diar_workspace(0, 64) == 0

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "sv_ge2e.h")).read()
    assert "#define SV_ABI_VERSION 12" in header and "#define SV_DIAR_M 16" in header
    assert "spectral diarization (added under v12; additive)" in header
    for proto in ("int sv_diar_crop_blur(float* A, float* B, const int* row_off, const long* mat_off, int F, int n_max,",
                  "int sv_diar_row_select(const float* B, const int* row_off, const long* mat_off, int F, int n_max",
                  "int sv_diar_thresh_sym(const float* B, const float* tau, float mult, float* Y,",
                  "int sv_diar_row_norm(const float* Z, float* S, float* d, double* r,",
                  "int sv_diar_spmm(const float* S, const float* W, const double* T, float* P,",
                  "int sv_diar_gram(const float* X, const float* Y, double* G, double* workspace,",
                  "int sv_diar_rmul(const float* X, const double* T, float* Y, const float* P, const double* lam",
                  "int sv_diar_kmeans(const float* E, const int* row_off, const int* k, int F, int max_iter"):
        assert proto in header, proto
    for rule in ("T_ij = B_ij >= tau_i ? B_ij : mult * B_ij", "S_ij = Z_ij (r_i r_j)", "ld_f = (n_f + 3) & ~3"):
        assert rule in header, rule
    want = {"sv_diar_crop_blur": 9, "sv_diar_row_select": 8, "sv_diar_thresh_sym": 9, "sv_diar_row_norm": 9,
            "sv_diar_spmm": 9, "sv_diar_workspace": 2, "sv_diar_gram": 8, "sv_diar_rmul": 11, "sv_diar_kmeans": 8}
    for name, nargs in want.items():
        assert len(_lib.SIGNATURES[name][1]) == nargs, name


def test_no_cpu_path():
    import torch
    from pytorch_speaker_verification_amd import diarization as D
    tb = D.matrix_tables([4, 6])
    with pytest.raises(RuntimeError, match="GPU only"):
        D.affinity(torch.zeros((10, 8)), tb)
    with pytest.raises(RuntimeError, match="GPU only"):
        D.crop_blur(torch.zeros(tb.elems), tb)
    with pytest.raises(RuntimeError, match="GPU only"):
        D.kmeans(torch.zeros((10, 16)), tb, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        D.cluster([torch.zeros((5, 8))])
