"""Spectral diarization on the GPU (diarization.py, sv_diar_*), every stage on its own fp32 input
against tests/diar_ref.py, so that a threshold flip cannot hide behind an upstream rounding.

Bounds:
  crop + blur   |B - oracle| <= ((2 r + 1)^2 + 8) 2^-24 max|A| per file: (2 r + 1)^2 positive-weighted
                terms of at most max|A| each, 8 for the two normalisers
  threshold     tau and Y bit for bit against the rule applied literally in np.float32
  row norm      d exact; |S - oracle| <= 4 2^-24 |S| elementwise
  eigenpairs    for the pairs j <= k_max of every file, with rho_j and r_j recomputed on the host in fp64:
                r_j <= 2 tol lam_1, |rho_j - lam_j(eigh)| <= r_j (+ n eps lam_1, eigh's own fp64 error), and |lam^_j - rho_j| <= LAM_BOUND lam_1 --
                LAM_BOUND is 4 x the worst value measured over these cases (the orthogonality of fp32
                Ritz vectors is not derivable in advance), and never above 1e-4
  k-means       the labels of the fp64 oracle on the same E, whose best and second-best distances differ
                by >= 1e-3 in every pass (asserted)
Measured on MI355X: see the MEASURED lines each test prints (DESIGN 3.15 keeps the record).
"""
import numpy as np
import pytest
import torch

import diar_ref as R
from pytorch_speaker_verification_amd import diarization as D

pytestmark = pytest.mark.gpu

NS = [2, 257, 3, 4, 5, 63, 64, 65, 129]  # n = 2 next to 257; n <= r; around the 32- and 64-wide tiles
TOL, K_MAX = 1e-4, 8
# |lam^ - rho| / lam_1: worst measured 1.61e-7 over the cases of test_eigenpairs (MI355X), times 4
LAM_BOUND = min(4 * 1.61e-7, 1e-4)
_cache = {}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _sym(n, rng, lo=-1.0, hi=1.0):
    a = rng.uniform(lo, hi, (n, n))
    return ((a + a.T) / 2).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- crop + blur
@pytest.mark.parametrize("sigma", [0, 1.0, 2.5])
def test_crop_blur(sigma):
    rng = np.random.default_rng(10)
    mats = [_sym(n, rng) for n in NS]
    tb = D.matrix_tables(NS)
    B = D.crop_blur(D.pack_matrices(mats, tb, _dev()), tb, sigma)
    got = D.unpack_matrices(B, tb, pads=True)
    g = R.taps(sigma)
    r = g.size - 1
    worst = 0.0
    for n, a, b in zip(NS, mats, got):
        assert np.all(b[:, n:] == 0), n  # the pad columns
        want = R.crop_blur(a.astype(np.float64), g)
        bound = ((2 * r + 1) ** 2 + 8) * 2.0 ** -24 * float(np.abs(a).max())
        err = float(np.abs(b[:, :n] - want).max())
        worst = max(worst, err / bound)
        assert err <= bound, (sigma, n, err, bound)
    print(f"\nMEASURED crop_blur sigma={sigma}: worst error / bound {worst:.3f}")
    if sigma == 0:  # W = I: the cropped matrix itself
        for a, b in zip(mats, got):
            assert np.array_equal(b[:, :a.shape[0]], R.crop(a).astype(np.float32))


# ----------------------------------------------------------------------------- threshold + symmetrise
def _check_threshold(mats, ns, p):
    tb = D.matrix_tables(ns)
    B = D.pack_matrices(mats, tb, _dev())
    tau, Y = D.threshold_sym(B, tb, p=p, mult=0.01)
    tau = tau.cpu().numpy()
    for f, (n, b, y) in enumerate(zip(ns, mats, D.unpack_matrices(Y, tb, pads=True))):
        want_tau, want_y = R.threshold_sym(b, R.q_rank(n, p), 0.01)
        assert want_y.dtype == np.float32
        assert np.array_equal(_bits(tau[tb.row_off[f]:tb.row_off[f + 1]]), _bits(want_tau)), (p, n)
        assert np.array_equal(_bits(y[:, :n]), _bits(want_y)), (p, n)
        assert np.all(y[:, n:] == 0), n


@pytest.mark.parametrize("p", [0.95, 0.0, 1.0])
def test_threshold_sym_bit_for_bit(p):
    rng = np.random.default_rng(11)
    _check_threshold([rng.uniform(-1, 1, (n, n)).astype(np.float32) for n in NS], NS, p)  # B need not be symmetric


def test_threshold_sym_heavy_ties():
    rng = np.random.default_rng(12)
    vals = np.array([-0.5, 0.25, 0.5, 0.75, 1.0], dtype=np.float32)
    ns = [65, 21, 4]
    mats = [vals[rng.integers(0, 5, (n, n))] for n in ns]
    for n, m in zip(ns, mats):  # tau sits on a tie in every row
        s = np.sort(m, axis=1)
        q = R.q_rank(n, 0.95)
        assert n < 21 or np.all((s[:, q] == s[:, q - 1]) | (s[:, q] == s[:, min(q + 1, n - 1)]))
    _check_threshold(mats, ns, 0.95)


# ----------------------------------------------------------------------------- row norm
def test_row_norm():
    rng = np.random.default_rng(13)
    mats = [_sym(n, rng, 0.0, 40.0) for n in NS]
    mats[1][7, :] = 0  # a zero row and column
    mats[1][:, 7] = 0
    mats[5][3, :] = -np.abs(mats[5][3, :])  # d <= 0 without being zero
    mats[5][:, 3] = mats[5][3, :]
    tb = D.matrix_tables(NS)
    S, d = D.row_norm(D.pack_matrices(mats, tb, _dev()), tb)
    d = d.cpu().numpy()
    worst = 0.0
    for f, (n, z, s) in enumerate(zip(NS, mats, D.unpack_matrices(S, tb, pads=True))):
        want, want_d = R.row_norm(z)
        assert np.array_equal(d[tb.row_off[f]:tb.row_off[f + 1]], want_d.astype(np.float32)), n
        assert np.all(np.isfinite(s)) and np.all(s[:, n:] == 0)
        err = np.abs(s[:, :n] - want)
        assert np.all(err <= 4 * 2.0 ** -24 * np.abs(want)), (n, float((err / np.maximum(np.abs(want), 1e-300)).max()))
        worst = max(worst, float((err[want != 0] / np.abs(want[want != 0])).max()) / 2.0 ** -24)
        assert np.array_equal(s[:, :n], s[:, :n].T)
    s1 = D.unpack_matrices(S, tb)[1]
    assert np.all(s1[7, :] == 0) and np.all(s1[:, 7] == 0)
    s5 = D.unpack_matrices(S, tb)[5]
    assert np.all(s5[3, :] == 0) and np.all(s5[:, 3] == 0)
    print(f"\nMEASURED row_norm: worst relative error {worst:.3f} x 2^-24 (bound 4)")


# ----------------------------------------------------------------------------- eigenpairs
def _eig_cases():
    """Exactly symmetric fp32 S: the oracle's refine of the planted cases, and a rank-2 matrix (two blocks
    of ones, 40 and 24 rows; its row maxima are 1, so it is its own normalisation)."""
    if "eig" not in _cache:
        mats = []
        for n, k, run in R.PLANTED:
            x, _ = R.planted(n, k, run, 0)
            S = R.refine(x)
            mats.append(((S + S.T) / 2).astype(np.float32))
        blocks = np.zeros((64, 64), dtype=np.float32)
        blocks[:40, :40] = 1
        blocks[40:, 40:] = 1
        mats.append(blocks)
        for m in mats:
            assert np.array_equal(m, m.T)
        lams = [R.top_eig(m.astype(np.float64))[0] for m in mats]
        for (n, k, run), lam in zip(R.PLANTED, lams):  # the precondition of everything that relies on k^
            assert R.gap_margin(lam, n) >= 1.5 and R.n_speakers(lam, n) == k
        _cache["eig"] = mats, lams
    return _cache["eig"]


def test_eigenpairs():
    mats, lams = _eig_cases()
    ns = [m.shape[0] for m in mats]
    tb = D.matrix_tables(ns)
    S = D.pack_matrices(mats, tb, _dev())
    lam, U, res, iters, conv = D.top_eigenpairs(S, tb, tol=TOL, max_iter=200, check=4, k_max=K_MAX)
    lam2, U2, _, iters2, _ = D.top_eigenpairs(S, tb, tol=TOL, max_iter=200, check=4, k_max=K_MAX)
    assert torch.equal(lam, lam2) and torch.equal(U, U2) and np.array_equal(iters, iters2)  # the same bits
    assert conv.all() and lam.shape == (len(ns), 16) and U.shape == (tb.rows, 16)
    print(f"\nMEASURED top_eigenpairs iterations per file: {iters.tolist()}")
    lam, U = lam.cpu().numpy(), U.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(U))
    worst_lam = worst_res = 0.0
    for f, (m, want) in enumerate(zip(mats, lams)):
        Sf = m.astype(np.float64)
        lam1 = lam[f, 0]
        for j in range(K_MAX):
            if lam[f, j] <= TOL * lam1:  # the rank-deficient tail: finite is all that is asked
                continue
            u = U[tb.row_off[f]:tb.row_off[f + 1], j]
            rho = float(u @ Sf @ u / (u @ u))
            r = float(np.linalg.norm(Sf @ u - rho * u) / np.linalg.norm(u))
            assert r <= 2 * TOL * lam1, (f, j, r)
            # (eigh's own error, n eps lam_1, matters where u is exact: the block matrix gives r = 0 to 1e-20)
            assert abs(rho - want[j]) <= r + m.shape[0] * np.finfo(np.float64).eps * lam1, (f, j, rho, want[j], r)
            worst_lam = max(worst_lam, abs(lam[f, j] - rho) / lam1)
            worst_res = max(worst_res, r / lam1)
    print(f"MEASURED worst |lam^ - rho| / lam_1 = {worst_lam:.3e} (bound {LAM_BOUND:.3e}); worst residual / lam_1 = "
          f"{worst_res:.3e} (bound {2 * TOL:.1e})")
    assert worst_lam <= LAM_BOUND
    assert abs(lam[-1, 0] - 40) <= 40 * LAM_BOUND and abs(lam[-1, 1] - 24) <= 40 * LAM_BOUND and np.all(lam[-1, 2:] <= 40 * TOL)


# ----------------------------------------------------------------------------- k-means
def _pad16(E):
    out = np.zeros((E.shape[0], 16), dtype=np.float32)
    out[:, :E.shape[1]] = E
    return out


def test_kmeans_planted():
    Es, ks = [], []
    for n, k, run in R.PLANTED:
        x, _ = R.planted(n, k, run, 0)
        Es.append(_pad16(R.embedding(R.top_eig(R.refine(x))[1], k)))
        ks.append(k)
    row_off = np.concatenate([[0], np.cumsum([e.shape[0] for e in Es])])
    lab, iters = D.kmeans(torch.from_numpy(np.concatenate(Es)).to(_dev()), row_off, ks)
    lab, iters = lab.cpu().numpy(), iters.cpu().numpy()
    for f, (E, k) in enumerate(zip(Es, ks)):
        want, it, margin = R.kmeans(E.astype(np.float64), k)
        assert margin >= 1e-3, (f, margin)  # no close call in any pass of the oracle
        assert np.array_equal(lab[row_off[f]:row_off[f + 1]], want) and iters[f] == it, (f, k)
        truth = R.relabel((np.arange(E.shape[0]) // R.PLANTED[f][2]) % k)
        assert np.array_equal(R.relabel(want), truth)


def test_kmeans_edge_cases():
    rng = np.random.default_rng(14)
    two = np.array([[1.0, 0], [0, 1.0]])
    empty = np.array([[0.0, 0], [0, 0], [3, 0]])  # k = 3: the third centre repeats row 0 and stays empty
    blobs = np.concatenate([c + 0.25 * rng.integers(-2, 3, (300, 2)) for c in ([0, 0], [8, 0], [0, 8])])  # > 256 rows
    slow = np.array([[0.0], [1], [2], [3], [4], [5], [12], [13]])  # several passes
    Es = [_pad16(e) for e in (two, empty, blobs, blobs[:5], slow, slow)]
    ks = [2, 3, 3, 1, 2, 2]
    row_off = np.concatenate([[0], np.cumsum([e.shape[0] for e in Es])])
    for max_iter in (100, 1):
        lab, iters = D.kmeans(torch.from_numpy(np.concatenate(Es)).to(_dev()), row_off, ks, max_iter=max_iter)
        lab, iters = lab.cpu().numpy(), iters.cpu().numpy()
        for f, (E, k) in enumerate(zip(Es, ks)):
            want, it, _ = R.kmeans(E.astype(np.float64), k, max_iter=max_iter)
            assert np.array_equal(lab[row_off[f]:row_off[f + 1]], want) and iters[f] == it, (f, max_iter)
    assert lab[row_off[1]:row_off[2]].tolist() == [0, 0, 1]


# ----------------------------------------------------------------------------- end to end
def test_cluster_end_to_end():
    files, truth, forced = [], [], []
    for n, k, run in R.PLANTED:
        x, lab = R.planted(n, k, run, 0)
        files.append(x)
        truth.append(R.relabel(lab))
        forced.append(None)
    for n, run in ((0, 1), (1, 1), (2, 1), (15, 3), (16, 4), (17, 4)):  # below n = 24 the eigengap is not used
        x, lab = R.planted(n, 2, run, 0)
        files.append(x)
        truth.append(R.relabel(lab))
        forced.append(2)
    order = [9, 0, 11, 5, 10, 1, 12, 2, 13, 3, 14, 4, 6, 7, 8]  # ragged: tiny files between the large ones
    files, truth, forced = [[v[i] for i in order] for v in (files, truth, forced)]
    dev_files = [torch.from_numpy(x).to(_dev()) if i % 2 else x for i, x in enumerate(files)]  # arrays and tensors
    labels, info = D.cluster(dev_files, n_speakers=forced)
    small, _ = D.cluster(dev_files, n_speakers=forced, max_elems=70000)  # several batches: the same labels
    for i, (x, t, k_in) in enumerate(zip(files, truth, forced)):
        want, k, lam, margin = R.cluster(x, n_spk=k_in)
        if k_in is None:
            assert margin >= 1.5, (i, margin)
        assert info["k"][i] == k and info["converged"][i], (i, info["k"][i], k)
        assert labels[i].dtype == np.int64 and np.array_equal(labels[i], want), i
        assert np.array_equal(labels[i], t), i
        assert np.array_equal(small[i], labels[i]), i
        if x.shape[0] >= 16:
            assert np.abs(info["lam"][i][:K_MAX + 1] - lam[:K_MAX + 1]).max() <= 1e-3 * lam[0], i
    print(f"\nMEASURED cluster iterations per file: {info['iters']}")


def test_diarize_two_waveforms():
    import logmel_ref as L
    from pytorch_speaker_verification_amd import dvector
    from test_gpu_logmel import _small_net
    net = _small_net()
    files = [(L.tones(48000, seed=7), [(0, 48000)]), (L.tones(64000, seed=8), [(0, 30000), (30000, 64000)]),
             (L.tones(5000, seed=9), [])]
    emb = dvector.embed_files(net, files, precision="f32")
    labels, info = D.diarize(net, files, precision="f32", n_speakers=2)
    assert [len(lab) for lab in labels] == [e.shape[0] for e in emb] and len(labels[2]) == 0
    for lab, e, k in zip(labels, emb, info["k"]):
        assert lab.dtype == np.int64 and (len(lab) == 0 or (lab[0] == 0 and lab.max() < max(k, 1)))
    on_dev = dvector.embed_files(net, files, precision="f32", on_device=True)
    assert on_dev[0].is_cuda and np.array_equal(on_dev[0].cpu().numpy(), emb[0])
