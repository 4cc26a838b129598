"""CPU side of the GE2E edge tests (tests/ge2e_cases.py, tests/test_gpu_ge2e_edges.py): everything
that can be settled without a GPU is settled here, before any GPU time is spent.

  * the fp64 numpy oracle (oracle/ge2e_np.py) OFF the unit sphere against fp64 autograd of the torch
    port -- the unit-norm goldens cannot see its norm handling (sE, pE, sU, pU, sC, pC);
  * the per-shard oracle (NumpyShardKernels) on the sharded cases, unequal shards included;
  * the conditioning cap: per case the fp32 port stays within BOUNDS / K, so the bounds of
    ge2e_cases.py are K times the port's error on exactly these inputs;
  * the metric sees what it is for: a missing 1/|e|, an error confined to the rows of largest norm,
    a dropped projection term;
  * get_cossim with external centroids, Nc != N: a plain-torch fp64 reference against the oracle.
"""
import numpy as np
import pytest
import torch

import ge2e_cases as gc
import recipe
from oracle import ge2e_np, torch_port

ALL = gc.all_inputs()
IDS = [gc.case_id(c) for c in ALL]


def _autograd64(E, w, b):
    Et = torch.tensor(np.asarray(E, np.float64), requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    per = torch_port.ge2e_per(Et, wt, bt)
    loss = per.sum()
    loss.backward()
    return dict(loss=float(loss.detach()), per=per.detach().numpy(), dE=Et.grad.numpy(), dw=float(wt.grad),
                db=float(bt.grad))


def test_table_reaches_what_it_says():
    """The shape conditions the case table relies on, restated from the dispatch of
    csrc/sv_ge2e.hip (GF_NMAX = GF_DMAX = 256, GF_MMAX = 16, GF_TILE = 128)."""
    def train_ok(N, M, D):
        return 0 < N <= 256 and 2 <= M <= 16 and 0 < D <= 256 and D % 4 == 0
    assert all(train_ok(N, M, D) for N, M, D, _, _ in gc.FUSED_CASES)
    assert not any(train_ok(N, M, D) for N, M, D, _, _ in gc.SPLIT_CASES)
    assert all(train_ok(*shape) and sum(shards) == shape[0] for shape, shards in gc.SHARDED_CASES)
    assert set(gc.SPLIT_SHARDED_CASES) <= set(gc.SHARDED_CASES)
    assert gc.GLOSS_CASE in gc.FUSED_CASES and gc.PADDED_FUSED <= set(gc.SPLIT_CASES)
    # off the sphere: the norms spread over more than 30x in every input with more than a few rows
    for N, M, D, _, _ in ALL:
        n = np.linalg.norm(gc.inputs(N, M, D), axis=2)
        assert n.min() >= 0.05 * 0.999 and n.max() <= 20.0 * 1.001
        assert N * M < 20 or n.max() / n.min() > 30.0


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_oracle_off_sphere_matches_fp64_autograd(case):
    """ge2e_np.ge2e_forward / ge2e_backward against fp64 autograd of torch_port.ge2e_loss on the
    off-sphere inputs: dE to 1e-9 of every row's own largest entry, loss, dw, db to 1e-10 relative
    (measured: at most 2e-13).  dw and db are sums of N*M*N terms dS (|dS| <= 1) that cancel -- db to
    about -sum_r 1e-6 / Z_r, 6e-5 at (128, 3, 8) -- so on top of 1e-10 of their value they get what
    fp64 itself can lose in such a sum on either side, 2^-52 per term."""
    N, M, D, w, b = case
    ref, o = _autograd64(gc.inputs(N, M, D), w, b), gc.oracle(*case)
    d_row = gc.dE_row(o["dE"], ref["dE"])
    rel = {k: abs(o[k] - ref[k]) / max(abs(ref[k]), 1e-300) for k in ("loss", "dw", "db")}
    print(f"\nMEASURED ge2e_oracle_offsphere.{gc.case_id(case)} dE_row {d_row:.2e} "
          + " ".join(f"{k} {v:.2e}" for k, v in rel.items()))
    assert d_row <= 1e-9
    assert rel["loss"] <= 1e-10
    fp64_sum = 2.0 ** -52 * N * M * N
    for k in ("dw", "db"):
        assert abs(o[k] - ref[k]) <= 1e-10 * abs(ref[k]) + fp64_sum, (k, rel)
    np.testing.assert_allclose(o["per"], ref["per"], rtol=0, atol=1e-10 * max(1.0, np.abs(ref["per"]).max()))


def test_oracle_gloss_scales_the_gradient():
    """The oracle's gloss argument (the GPU test's reference for an upstream gradient != 1) against
    fp64 autograd of gloss * loss."""
    N, M, D, w, b = gc.GLOSS_CASE
    Et = torch.tensor(np.asarray(gc.inputs(N, M, D), np.float64), requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    (gc.GLOSS * torch_port.ge2e_loss(Et, wt, bt)).backward()
    o = gc.oracle(N, M, D, w, b, gc.GLOSS)
    assert gc.dE_row(o["dE"], Et.grad.numpy()) <= 1e-9
    fp64_sum = 2.0 ** -52 * N * M * N   # as in test_oracle_off_sphere_matches_fp64_autograd
    assert abs(o["dw"] - float(wt.grad)) <= 1e-10 * abs(float(wt.grad)) + fp64_sum
    assert abs(o["db"] - float(bt.grad)) <= 1e-10 * abs(float(bt.grad)) + fp64_sum
    # and it is gloss times the gradient at gloss = 1
    o1 = gc.oracle(N, M, D, w, b)
    np.testing.assert_allclose(o["dE"], gc.GLOSS * o1["dE"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape,shards", gc.SHARDED_CASES, ids=[f"{s}-{h}" for s, h in gc.SHARDED_CASES])
def test_sharded_oracle_reproduces_the_whole(shape, shards):
    """NumpyShardKernels with the test's hand-made exchanges (what the GPU test holds each shard's
    `red` buffer to) against ge2e_forward / ge2e_backward on the whole batch, to 1e-10; the padding
    rows N..Np-1 of every shard's red are exactly zero."""
    N, M, D = shape
    E, ref = gc.inputs(N, M, D), gc.oracle(N, M, D, gc.SHARD_W, gc.SHARD_B)
    got, reds, _ = gc.run_shards_numpy(E, gc.SHARD_W, gc.SHARD_B, shards)
    assert gc.dE_row(got["dE"], ref["dE"]) <= 1e-10
    np.testing.assert_allclose(got["per"], ref["per"], rtol=0, atol=1e-10 * np.abs(ref["per"]).max())
    for k in ("loss", "dw", "db"):
        assert abs(got[k] - ref[k]) <= 1e-10 * max(1.0, abs(ref[k])), k
    Np = (N + 3) // 4 * 4
    for red in reds:
        assert red.shape == (Np * D + N,)
        assert not red[N * D:Np * D].any()


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_conditioning_cap(case):
    """A condition on the inputs, not a measurement of anything under test: the fp32 torch port
    (CPU autograd) is within BOUNDS / K of the fp64 oracle in every statistic, on every case."""
    stats = gc.compare(gc.port_f32(*case), gc.oracle(*case))
    print(f"\nMEASURED ge2e_port_f32.{gc.case_id(case)} {gc.fmt(stats)}")
    assert not gc.over(stats, scale=1.0 / gc.K)


def test_bounds_are_k_times_the_port():
    assert gc.K <= 8 and set(gc.BOUNDS) == {"per_abs", "dE_row", "loss_abs", "dw", "db"}
    assert all(gc.BOUNDS[k] == gc.K * gc.PORT_MAX[k] for k in gc.BOUNDS)


# ------------------------------------------------------------------- the metric's self-checks
def _backward_variant(E, w, b, keep_sE=True, keep_projE=True, keep_projU=True):
    """ge2e_np.ge2e_backward restated with three switches, each of which removes one piece of the
    norm handling: the final 1/max(|e|, eps) of the E side (sE), the projection term alpha E^ of
    the E side (pE), the projection term of the leave-one-out side (pU).  All on = the oracle."""
    E = np.asarray(E, np.float64)
    N, M, D = E.shape
    C, U = ge2e_np.get_centroids(E), ge2e_np.get_utterance_centroids(E)
    (Eh, En), (Ch, Cn), (Uh, Un) = ge2e_np._unit(E), ge2e_np._unit(C), ge2e_np._unit(U)
    cos = ge2e_np.get_cossim(E, C)
    S = w * cos + b
    P = np.exp(S) / (np.exp(S).sum(axis=2, keepdims=True) + ge2e_np.EPS_LOG)
    idx = np.arange(N)
    dS = P.copy()
    dS[idx, :, idx] -= 1.0
    dcos = w * dS
    raw = cos - ge2e_np.EPS_SIM
    off = dcos.copy()
    off[idx, :, idx] = 0.0
    dcd, rawd = dcos[idx, :, idx], raw[idx, :, idx]
    sE = 1.0 / np.maximum(En, ge2e_np.EPS_COS) if keep_sE else np.ones_like(En)
    pE = (En > ge2e_np.EPS_COS) * (1.0 if keep_projE else 0.0)
    pU = (Un > ge2e_np.EPS_COS) * (1.0 if keep_projU else 0.0)
    pC = (Cn > ge2e_np.EPS_COS) * 1.0
    alpha = (off * raw).sum(axis=2) + dcd * rawd
    dE = (np.einsum("jik,kd->jid", off, Ch) + dcd[..., None] * Uh - (alpha * pE)[..., None] * Eh) * sE[..., None]
    beta = np.einsum("jik,jik->k", off, raw)
    dC = (np.einsum("jik,jid->kd", off, Eh) - (beta * pC)[:, None] * Ch) / np.maximum(Cn, ge2e_np.EPS_COS)[:, None]
    dE += dC[:, None, :] / M
    dU = (dcd[..., None] * Eh - (dcd * rawd * pU)[..., None] * Uh) / np.maximum(Un, ge2e_np.EPS_COS)[..., None]
    dE += (dU.sum(axis=1, keepdims=True) - dU) / (M - 1)
    return dE


def _with_dE(ref, dE):
    return dict(ref, dE=dE)


def test_variant_with_every_switch_on_is_the_oracle():
    for case in (gc.FUSED_CASES[1], gc.FUSED_CASES[-1]):
        N, M, D, w, b = case
        assert gc.dE_row(_backward_variant(gc.inputs(N, M, D), w, b), gc.oracle(*case)["dE"]) <= 1e-13


def test_missing_inverse_norm_is_invisible_on_the_sphere():
    """(a), first half: on recipe.make_embeddings' unit-norm rows (every GE2E input the suite had)
    an oracle without the final 1/|e| passes even the new per-row metric."""
    for seed, n, m, d, w, b in [(3, 6, 4, 64, 10.0, -5.0), (5, 9, 3, 36, 3.7, -1.2)]:
        E = recipe.make_embeddings(seed, n, m, d, True)
        ref = ge2e_np.ge2e_backward(E, w, b)[0]
        assert gc.dE_row(_backward_variant(E, w, b, keep_sE=False), ref) <= gc.BOUNDS["dE_row"] / gc.K


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_metric_rejects_wrong_norm_handling(case):
    """(a), second half, and (c): off the sphere, `compare` rejects an oracle copy without the final
    1/|e|, one without the E-side projection term and one without the leave-one-out side's, on
    every case of the table."""
    N, M, D, w, b = case
    E, ref = gc.inputs(N, M, D), gc.oracle(*case)
    for switch in ("keep_sE", "keep_projE", "keep_projU"):
        wrong = _backward_variant(E, w, b, **{switch: False})
        assert "dE_row" in gc.over(gc.compare(_with_dE(ref, wrong), ref)), switch


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_metric_sees_an_error_in_the_rows_of_largest_norm(case):
    """(b): an error of 1e-3 relative confined to the quarter of the rows with the largest norm
    (whose gradients are the smallest: dE_r ~ 1/|E_r|).  The old statistic, max|.| over the tensor's
    largest entry <= 1e-4, accepts it wherever those rows' gradients are below a tenth of the
    largest -- on most of the table, asserted for the table as a whole -- and dE_row rejects it
    everywhere."""
    N, M, D, w, b = case
    E, ref = gc.inputs(N, M, D), gc.oracle(*case)
    norms = np.linalg.norm(E, axis=2)
    big = norms >= np.quantile(norms, 0.75)
    wrong = ref["dE"].copy()
    wrong[big] *= 1.0 + 1e-3
    assert "dE_row" in gc.over(gc.compare(_with_dE(ref, wrong), ref))
    assert gc.dE_row(wrong, ref["dE"]) == pytest.approx(1e-3, rel=1e-6)


def test_old_statistic_accepts_that_error():
    accepted = []
    for case in ALL:
        N, M, D, w, b = case
        E, ref = gc.inputs(N, M, D), gc.oracle(*case)
        norms = np.linalg.norm(E, axis=2)
        big = norms >= np.quantile(norms, 0.75)
        wrong = ref["dE"].copy()
        wrong[big] *= 1.0 + 1e-3
        old = np.abs(wrong - ref["dE"]).max() / np.abs(ref["dE"]).max()
        accepted.append(old <= 1e-4)
    # every case with more than a handful of rows; the old statistic never sees it there
    many = [a for a, c in zip(accepted, ALL) if c[0] * c[1] >= 40]
    assert many and all(many), list(zip(IDS, accepted))


# ------------------------------------------------------------------- helpers with Nc != N
@pytest.mark.parametrize("N,M,D,Nc", gc.HELPER_CASES + [(5, 3, 64, 5)])
def test_cossim_external_centroids_reference(N, M, D, Nc):
    """The plain-torch fp64 get_cossim with external centroids (gc.cossim_torch, the GPU helpers'
    reference) against ge2e_np.get_cossim for Nc < N, Nc > N and Nc = N: the diagonal rule is
    'k == j, where there is such a k' (j < Nc)."""
    E, Eenr = gc.helper_inputs(N, M, D, Nc)
    C = ge2e_np.get_centroids(Eenr)
    got = gc.cossim_torch(torch.tensor(E).double(), torch.tensor(C)).numpy()
    ref = ge2e_np.get_cossim(E, C)
    assert got.shape == ref.shape == (N, M, Nc)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
    # the diagonal really is the leave-one-out cosine, and only there
    plain = np.einsum("jid,kd->jik", ge2e_np._unit(E.astype(np.float64))[0], ge2e_np._unit(C)[0])
    diff = np.abs(ref - plain - 1e-6) > 1e-9
    want = np.zeros((N, M, Nc), bool)
    n = min(N, Nc)
    want[np.arange(n), :, np.arange(n)] = True
    assert np.array_equal(diff, want)


def test_calc_loss_reference_matches_oracle():
    E, Eenr = gc.helper_inputs(5, 3, 64, 9)
    S = 10.0 * ge2e_np.get_cossim(E, ge2e_np.get_centroids(Eenr)) - 5.0
    loss, per = gc.calc_loss_torch(torch.tensor(S))
    # ge2e_np.calc_loss takes the own-speaker entry from the first N columns, like the reference
    o_loss, o_per = ge2e_np.calc_loss(S)
    np.testing.assert_allclose(per.numpy(), o_per, rtol=0, atol=1e-12)
    assert abs(float(loss) - o_loss) <= 1e-12 * abs(o_loss)
