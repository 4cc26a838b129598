"""The GE2E contrast loss kernels (csrc/sv_ge2e_contrast.h behind the `_as` entry points of
include/sv_ge2e.h) against the fp64 reference of tests/contrast_cases.py, off the unit sphere and at
the tile edges of tests/ge2e_cases.py's table, within contrast_cases.BOUNDS (K = 4 times the fp32
torch restatement's own error; tests/test_contrast_cases.py holds the CPU side):

  * the fused path (sv_ge2e_train_as / ops.ge2e_train) on sentinel-filled outputs, the split path
    (ops.ge2e_forward / ge2e_backward, gloss != 1 included), the dispatch outside sv_ge2e_train_ok;
  * the sharded forms, fused and split, with virtual ranks and hand-made exchanges;
  * the helper utils.calc_loss_contrast on a given S (K = N and K > N, a weight on every per value,
    exact ties), the module under both dispatches, the library op under opcheck;
  * two GE2ETrainer steps against the stock-PyTorch port trained with the reference formulas;
  * the softmax path: bit-identical with and without the new argument.
"""
import functools

import numpy as np
import pytest
import torch

import contrast_cases as cc
import recipe
from conftest import model_dims
from oracle import torch_port

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0


def _scalars(w, b):
    return (torch.tensor(w, dtype=torch.float32, device=DEV), torch.tensor(b, dtype=torch.float32, device=DEV))


def _measure(label, case_id, got, ref):
    stats = cc.compare(got, ref)
    print(f"\nMEASURED contrast.{label}.{case_id} {cc.fmt(stats)}")
    return stats


def _train_ok(N, M, D):
    from pytorch_speaker_verification_amd._lib import lib
    return lib().sv_ge2e_train_ok(N, M, D)


def _train(case):
    from pytorch_speaker_verification_amd import ops
    N, M, D, w, b = case
    wt, bt = _scalars(w, b)
    loss, per, dE, dwdb = ops.ge2e_train(torch.tensor(cc.inputs(N, M, D), device=DEV), wt, bt, loss_method="contrast")
    dwdb = dwdb.cpu().numpy()
    return dict(loss=float(loss), per=per.cpu().numpy(), dE=dE.cpu().numpy(), dw=float(dwdb[0]), db=float(dwdb[1]))


def _split(case, gloss=None):
    from pytorch_speaker_verification_amd import ops
    N, M, D, w, b = case
    wt, bt = _scalars(w, b)
    loss, per, st = ops.ge2e_forward(torch.tensor(cc.inputs(N, M, D), device=DEV), wt, bt, "contrast")
    g = None if gloss is None else torch.tensor(gloss, dtype=torch.float32, device=DEV)
    dE, dw, db = ops.ge2e_backward(st, wt, bt, g)
    return dict(loss=float(loss), per=per.cpu().numpy(), dE=dE.cpu().numpy(), dw=float(dw), db=float(db))


# ----------------------------------------------------------------------------------- fused, split
@pytest.mark.parametrize("case", cc.FUSED_CASES, ids=[cc.case_id(c) for c in cc.FUSED_CASES])
def test_fused_kernel_off_sphere(case):
    """sv_ge2e_train_as(SV_GE2E_CONTRAST) on sentinel-filled per / dE / loss / dwdb (an element the
    kernels leave unwritten shows against the reference): within BOUNDS.  The dcos padding columns
    N .. Np - 1 feed F3's sums, so the Np != N cases check them through dE.  ops.ge2e_train runs
    the same call: bit-identical."""
    from pytorch_speaker_verification_amd._lib import call, lib, ptr, stream_of
    N, M, D, w, b = case
    assert _train_ok(N, M, D)
    E = torch.tensor(cc.inputs(N, M, D), device=DEV)
    wt, bt = _scalars(w, b)
    ws = torch.full((lib().sv_ge2e_workspace_size(N, M, D, N) // 4 + 1,), float("nan"), dtype=torch.float32, device=DEV)
    per = torch.full((N, M), SENTINEL, dtype=torch.float32, device=DEV)
    dE = torch.full((N, M, D), SENTINEL, dtype=torch.float32, device=DEV)
    loss = torch.full((), SENTINEL, dtype=torch.float32, device=DEV)
    dwdb = torch.full((2,), SENTINEL, dtype=torch.float32, device=DEV)
    call("sv_ge2e_train_as", 1, ptr(E), N, M, D, ptr(wt), ptr(bt), ptr(loss), ptr(per), ptr(dE), ptr(dwdb), ptr(ws),
         stream_of(E))
    got = dict(loss=float(loss), per=per.cpu().numpy(), dE=dE.cpu().numpy(), dw=float(dwdb[0]), db=float(dwdb[1]))
    stats = _measure("fused", cc.case_id(case), got, cc.reference(*case))
    assert not cc.over(stats, cc.BOUNDS), cc.over(stats, cc.BOUNDS)
    via_ops = _train(case)
    assert via_ops["loss"] == got["loss"] and np.array_equal(via_ops["dE"], got["dE"])
    assert np.array_equal(via_ops["per"], got["per"]) and (via_ops["dw"], via_ops["db"]) == (got["dw"], got["db"])


def test_fused_kernel_sixteen_rows_per_workgroup():
    """BIG_CASE: 2064 rows above 128 speakers, the launcher's 16-row workgroups on a 256-CU device
    (the table's shapes reach 4 and 8 rows), D = 256 (LDS-DMA staging)."""
    assert _train_ok(*cc.BIG_CASE[:3])
    stats = _measure("fused", cc.case_id(cc.BIG_CASE), _train(cc.BIG_CASE), cc.reference_mm(*cc.BIG_CASE))
    assert not cc.over(stats, cc.BOUNDS), cc.over(stats, cc.BOUNDS)


@pytest.mark.parametrize("case", cc.FUSED_CASES + cc.SPLIT_CASES,
                         ids=[cc.case_id(c) for c in cc.FUSED_CASES + cc.SPLIT_CASES])
def test_split_kernels_off_sphere(case):
    """ops.ge2e_forward / ge2e_backward (sv_ge2e_fwd_as / _bwd_as) on every fused and split case,
    the zero-padded (5, 4, 38) included: within BOUNDS."""
    stats = _measure("split", cc.case_id(case), _split(case), cc.reference(*case))
    assert not cc.over(stats, cc.BOUNDS), cc.over(stats, cc.BOUNDS)


@pytest.mark.parametrize("case", cc.SPLIT_CASES, ids=[cc.case_id(c) for c in cc.SPLIT_CASES])
def test_train_outside_the_fused_shapes(case):
    """ops.ge2e_train(loss_method='contrast') where sv_ge2e_train_ok refuses: M = 17, N = 257,
    D = 260 take the split kernels; D = 38 is zero-padded to 40 and runs the fused kernel."""
    N, M, D, w, b = case
    assert _train_ok(N, M, D) == 0
    if case in cc.PADDED_FUSED:
        assert _train_ok(N, M, (D + 3) // 4 * 4)
    stats = _measure("train_dispatch", cc.case_id(case), _train(case), cc.reference(*case))
    assert not cc.over(stats, cc.BOUNDS), cc.over(stats, cc.BOUNDS)


def test_split_backward_with_upstream_gradient():
    case = cc.GLOSS_CASE
    stats = _measure("split_gloss", cc.case_id(case), _split(case, cc.GLOSS), cc.reference(*case, cc.GLOSS))
    assert not cc.over(stats, cc.BOUNDS), cc.over(stats, cc.BOUNDS)


def test_single_speaker_is_refused():
    from pytorch_speaker_verification_amd import ops
    E = torch.tensor(cc.inputs(5, 2, 4)[:1].copy(), device=DEV)
    wt, bt = _scalars(10.0, -5.0)
    for fn in (ops.ge2e_train, ops.ge2e_forward):
        with pytest.raises(ValueError, match="N >= 2"):
            fn(E, wt, bt, loss_method="contrast")


# ------------------------------------------------------------------------------------ sharded forms
def _shard_id(shape, shards):
    return "-".join(map(str, shape)) + "." + "+".join(map(str, shards))


@pytest.mark.parametrize("shape,shards", cc.SHARDED_CASES, ids=[_shard_id(s, h) for s, h in cc.SHARDED_CASES])
def test_fused_shard_kernels_off_sphere(shape, shards):
    """HipFusedShard('contrast') on virtual ranks, one after another, with hand-made exchanges
    (concatenated sums, added reduce buffers); sv_ge2e_shard_rows_as on a sentinel-filled reduce
    buffer.  Concatenated per / dE and the summed loss / (dw, db) against the whole-batch fp64
    reference within BOUNDS; the padding rows of every shard's dC^ exactly zero."""
    from pytorch_speaker_verification_amd._lib import call, ptr, stream_of
    from pytorch_speaker_verification_amd.sharded_ge2e import HipFusedShard
    N, M, D = shape
    w, b = cc.SHARD_W, cc.SHARD_B
    assert HipFusedShard.ok(N, M, D)
    Np = (N + 3) // 4 * 4
    f = HipFusedShard("contrast")
    wt, bt = _scalars(w, b)
    sl = cc.shard_slices(shards)
    Et = torch.tensor(cc.inputs(N, M, D), device=DEV)
    parts = [Et[s0:s0 + nl].contiguous() for s0, nl in sl]
    prep = [f.prep(p, N) for p in parts]
    ssum_all = torch.cat([p[0] for p in prep])
    rows = []
    for p, (s0, nl), (_, ws) in zip(parts, sl, prep):
        per = torch.full((nl, M), SENTINEL, dtype=torch.float32, device=DEV)
        red = torch.full((Np * D + N,), SENTINEL, dtype=torch.float32, device=DEV)
        loss = torch.empty((), dtype=torch.float32, device=DEV)
        dwdb = torch.empty(2, dtype=torch.float32, device=DEV)
        call("sv_ge2e_shard_rows_as", 1, nl, M, D, s0, N, ptr(ssum_all), ptr(wt), ptr(bt), ptr(per), ptr(red),
             ptr(loss), ptr(dwdb), ptr(ws), stream_of(p))
        rows.append((loss, per, red, dwdb))
    for r_ in rows:
        red_h = r_[2].cpu().numpy()
        assert np.isfinite(red_h).all() and not red_h[N * D:Np * D].any()
    red = torch.stack([r_[2] for r_ in rows]).sum(0)
    got = dict(loss=sum(float(r_[0]) for r_ in rows), per=np.concatenate([r_[1].cpu().numpy() for r_ in rows]),
               dE=torch.cat([f.finalize(p, s0, N, red.clone(), ws)
                             for p, (s0, _), (_, ws) in zip(parts, sl, prep)]).cpu().numpy(),
               dw=sum(float(r_[3][0]) for r_ in rows), db=sum(float(r_[3][1]) for r_ in rows))
    stats = _measure("fused_shards", _shard_id(shape, shards), got, cc.reference(N, M, D, w, b))
    assert not cc.over(stats, cc.BOUNDS), cc.over(stats, cc.BOUNDS)
    # HipFusedShard.rows is that call
    l2, per2, red2, dwdb2 = f.rows(parts[-1], sl[-1][0], N, ssum_all, wt, bt, prep[-1][1])
    assert torch.equal(per2, rows[-1][1]) and torch.equal(red2, rows[-1][2]) and torch.equal(dwdb2, rows[-1][3])


@pytest.mark.parametrize("shape,shards", cc.SPLIT_SHARDED_CASES,
                         ids=[_shard_id(s, h) for s, h in cc.SPLIT_SHARDED_CASES])
def test_split_shard_kernels_off_sphere(shape, shards):
    """The same shard lists on HipShardKernels('contrast') (sv_ge2e_fwd_rows_as / _bwd_rows_as)."""
    from pytorch_speaker_verification_amd.sharded_ge2e import HipShardKernels
    N, M, D = shape
    w, b = cc.SHARD_W, cc.SHARD_B
    k = HipShardKernels("contrast")
    wt, bt = _scalars(w, b)
    sl = cc.shard_slices(shards)
    Et = torch.tensor(cc.inputs(N, M, D), device=DEV)
    parts = [Et[s0:s0 + nl].contiguous() for s0, nl in sl]
    ssum_all = torch.cat([k.speaker_sums(p) for p in parts])
    fwd = [k.fwd_rows(p, s0, N, ssum_all, wt, bt) for p, (s0, _) in zip(parts, sl)]
    bwd = [k.bwd_rows(f_[2], wt, bt, None) for f_ in fwd]
    red = torch.stack([r_[0] for r_ in bwd]).sum(0)
    got = dict(loss=sum(float(f_[0]) for f_ in fwd), per=np.concatenate([f_[1].cpu().numpy() for f_ in fwd]),
               dE=torch.cat([k.finalize(f_[2], red.clone()) for f_ in fwd]).cpu().numpy(),
               dw=sum(float(r_[1][0]) for r_ in bwd), db=sum(float(r_[1][1]) for r_ in bwd))
    stats = _measure("split_shards", _shard_id(shape, shards), got, cc.reference(N, M, D, w, b))
    assert not cc.over(stats, cc.BOUNDS), cc.over(stats, cc.BOUNDS)


# ------------------------------------------------------------------------------------------ helper
@functools.lru_cache(maxsize=None)
def _helper_S(N, M, Kc):
    S = (3.0 * np.random.default_rng(4100 + Kc).standard_normal((N, M, Kc))).astype(np.float32)
    S.setflags(write=False)
    return S


@pytest.mark.parametrize("Kc", [5, 9])
def test_helper_on_a_given_S(Kc):
    """utils.calc_loss_contrast forward and autograd (sv_ge2e_calc_contrast / _bwd) on a given fp32 S
    [5, 3, K], K = N and K = N + 4, with a weight on every per value (gper != 0), against fp64 on the
    same S: per within BOUNDS['per_abs'], dS row by row within BOUNDS['dE_row'], zero where the
    reference is zero."""
    from pytorch_speaker_verification_amd.utils import calc_loss_contrast
    N, M = 5, 3
    S = _helper_S(N, M, Kc)
    wts = torch.tensor(np.random.default_rng(78).standard_normal((N, M)))
    Sr = torch.tensor(S, dtype=torch.float64, requires_grad=True)
    per_r, _ = cc.contrast_on_S(Sr)
    assert cc.top_two_gap(Sr) >= cc.GAP_FLOOR
    (per_r.sum() + (per_r * wts).sum()).backward()
    Sg = torch.tensor(S, device=DEV, requires_grad=True)
    loss_g, per_g = calc_loss_contrast(Sg)
    (loss_g + (per_g * wts.float().to(DEV)).sum()).backward()
    d_per = float(np.abs(per_g.detach().cpu().numpy() - per_r.detach().numpy()).max())
    d_loss = abs(float(loss_g.detach()) - float(per_r.detach().sum())) / (N * M) ** 0.5
    d_dS = cc.gc.dE_row(Sg.grad.cpu().numpy(), Sr.grad.numpy())
    print(f"\nMEASURED contrast.helper.K{Kc} per_abs {d_per:.2e} loss_abs {d_loss:.2e} dS_row {d_dS:.2e}")
    assert d_per <= cc.BOUNDS["per_abs"] and d_loss <= cc.BOUNDS["loss_abs"] and d_dS <= cc.BOUNDS["dE_row"]
    assert np.array_equal(Sg.grad.cpu().numpy() != 0, Sr.grad.numpy() != 0)


def test_helper_ties_go_to_the_lowest_k():
    """Exact ties among the off-diagonal maxima (across the 64-lane stride too, K = 70): the
    gradient lands on the lowest tied k, as torch.max(dim)'s."""
    from pytorch_speaker_verification_amd.utils import calc_loss_contrast
    N, M, Kc = 3, 2, 70
    S = np.full((N, M, Kc), -1.0, np.float32)
    S[np.arange(N), :, np.arange(N)] = 0.25
    S[0, 0, [66, 5, 1]] = 1.5        # lowest tied: 1
    S[0, 1, [69, 65]] = 1.5          # 65 (both in the second stride)
    S[1, 0, [1, 64, 0]] = 2.0        # 1 is the diagonal: 0
    S[1, 1, [2, 66]] = 0.5           # 2
    S[2, 0, :] = 0.75                # everything tied, the diagonal too: 0
    S[2, 1, 2:] = 3.0                # 2 is the diagonal: 3
    want = np.array([[1, 65], [0, 2], [0, 3]])
    Sr = torch.tensor(S, dtype=torch.float64, requires_grad=True)
    per_r, idx = cc.contrast_on_S(Sr)
    assert np.array_equal(idx.numpy(), want)
    per_r.sum().backward()
    Sg = torch.tensor(S, device=DEV, requires_grad=True)
    loss_g, per_g = calc_loss_contrast(Sg)
    loss_g.backward()
    got = Sg.grad.cpu().numpy()
    assert np.array_equal(got != 0, Sr.grad.numpy() != 0)
    np.testing.assert_allclose(got, Sr.grad.numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(per_g.detach().cpu().numpy(), per_r.detach().numpy(), rtol=0, atol=cc.BOUNDS["per_abs"])


# ---------------------------------------------------------------------------- module, library op
@pytest.mark.parametrize("dispatch", ["function", "library"])
def test_module_backward_under_both_dispatches(dispatch):
    from pytorch_speaker_verification_amd.speech_embedder_net import GE2ELoss
    case = (7, 16, 36, 10.0, -5.0)
    assert case in cc.FUSED_CASES
    N, M, D, _, _ = case
    mod = GE2ELoss(DEV, loss_method="contrast")
    mod.dispatch = dispatch
    E = torch.tensor(cc.inputs(N, M, D), device=DEV, requires_grad=True)
    loss = mod(E)
    loss.backward()
    ref = cc.reference(*case)
    got = dict(loss=float(loss), per=ref["per"], dE=E.grad.cpu().numpy(), dw=float(mod.w.grad), db=float(mod.b.grad))
    stats = _measure(f"module_{dispatch}", cc.case_id(case), got, ref)
    assert not cc.over(stats, cc.BOUNDS), cc.over(stats, cc.BOUNDS)


def test_opcheck_library_op_with_the_contrast_loss():
    from pytorch_speaker_verification_amd import library
    g = torch.Generator().manual_seed(3)
    E = torch.nn.functional.normalize(torch.randn(3, 4, 32, generator=g), dim=2).to(DEV).requires_grad_()
    w = torch.tensor(10.0, device=DEV, requires_grad=True)
    b = torch.tensor(-5.0, device=DEV, requires_grad=True)
    torch.library.opcheck(library.ge2e_loss, (E, w, b, "contrast"))
    torch.library.opcheck(library.ge2e_loss, (E, w, b), {"loss_method": "contrast"})


# ------------------------------------------------------------------------------------------ trainer
def _port_step(port, w, b, opt, x, N, M):
    """torch_port.train_step with the contrast formulas; returns (loss, the step's top-two gap)."""
    opt.zero_grad()
    per, S, _ = cc.contrast_per(port(x).reshape(N, M, -1), w, b)
    loss = per.sum()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(port.parameters(), 3.0)
    torch.nn.utils.clip_grad_norm_([w, b], 1.0)
    opt.step()
    return float(loss), cc.top_two_gap(S)


@pytest.mark.parametrize("dims,N,M,T", [((40, 96, 2, 24), 3, 3, 5),
                                        ((40, 72, 2, 20), 5, 7, 37),
                                        ((40, 64, 3, 32), 2, 2, 1)])   # N = 2: a single negative
def test_trainer_steps_against_torch_port(dims, N, M, T):
    """Two GE2ETrainer.step with GE2ELoss(loss_method='contrast') at the shapes (and tolerances) of
    test_ragged_training_step_against_torch_port, against oracle.torch_port.SpeechEmbedderPort on the
    host trained with the reference formulas, both clips and SGD.  The port's smallest top-two gap
    over both steps is at least 1e-3 (probed on the CPU: 0.39 / 0.27 and 0.024 / 0.029; N = 2 has
    no second candidate), so the two cannot legitimately differ in k*."""
    from pytorch_speaker_verification_amd.speech_embedder_net import GE2ELoss, SpeechEmbedder
    from pytorch_speaker_verification_amd.trainer import GE2ETrainer
    sd = recipe.make_weights(N * 31 + M * 7 + T, *dims, scale=2.0)
    x = recipe.make_frames(N + M + T, N * M, T, dims[0])
    with model_dims(*dims):
        net = SpeechEmbedder()
    torch_port.load_recipe_weights(net, sd)
    net, ge2e = net.to(DEV), GE2ELoss(DEV, loss_method="contrast")
    tr = GE2ETrainer(net, ge2e, lr=0.01)
    assert tr.ge2e.loss_method == "contrast"
    xd = torch.tensor(x, device=DEV)
    losses = [float(tr.step(xd, N, M)) for _ in range(2)]
    port = torch_port.SpeechEmbedderPort(*dims)
    torch_port.load_recipe_weights(port, sd)
    w = torch.nn.Parameter(torch.tensor(10.0))
    b = torch.nn.Parameter(torch.tensor(-5.0))
    opt = torch.optim.SGD([{"params": port.parameters()}, {"params": [w, b]}], lr=0.01)
    ref = [_port_step(port, w, b, opt, torch.tensor(x), N, M) for _ in range(2)]
    print(f"\nMEASURED contrast.trainer.{N}-{M}-{T} loss {losses} port {[r[0] for r in ref]} gap {[r[1] for r in ref]}")
    assert min(r[1] for r in ref) >= 1e-3
    np.testing.assert_allclose(losses, [r[0] for r in ref], rtol=1e-4)
    got = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    for k, v in port.state_dict().items():
        np.testing.assert_allclose(got[k], v.numpy(), atol=5e-5, err_msg=k)
    np.testing.assert_allclose([ge2e.w.item(), ge2e.b.item()], [w.item(), b.item()], atol=1e-5)


# --------------------------------------------------------------------------------- softmax untouched
@pytest.mark.parametrize("shape", [(129, 11, 256), (7, 16, 36)])
def test_softmax_path_is_bit_identical(shape):
    """ge2e_train(E, w, b), ge2e_train(E, w, b, loss_method='softmax') and sv_ge2e_train_as with
    SV_GE2E_SOFTMAX give the same bits."""
    from pytorch_speaker_verification_amd import ops
    from pytorch_speaker_verification_amd._lib import call, lib, ptr, stream_of
    N, M, D = shape
    E = torch.tensor(cc.gc.inputs(N, M, D), device=DEV)
    wt, bt = _scalars(10.0, -5.0)
    a = ops.ge2e_train(E, wt, bt)
    c = ops.ge2e_train(E, wt, bt, loss_method="softmax")
    ws = torch.empty(lib().sv_ge2e_workspace_size(N, M, D, N) // 4 + 1, dtype=torch.float32, device=DEV)
    d = [torch.empty_like(t) for t in a]
    call("sv_ge2e_train_as", 0, ptr(E), N, M, D, ptr(wt), ptr(bt), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(ws),
         stream_of(E))
    for x, y, z in zip(a, c, d):
        assert torch.equal(x, y) and torch.equal(x, z)
    contrast = ops.ge2e_train(E, wt, bt, loss_method="contrast")
    assert not torch.equal(contrast[0], a[0])
