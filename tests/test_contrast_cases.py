"""CPU side of the GE2E contrast loss tests (tests/contrast_cases.py, tests/test_gpu_contrast.py):

  * the fp64 reference against a loop-form restatement of eq. 7, and where its maximum goes with a
    negative w and with exact ties;
  * the gap floor per case (an fp32 kernel must not be able to pick another column), no all-zero
    reference dE row;
  * the conditioning cap: per case the fp32 restatement stays within BOUNDS / K and picks the
    reference's k*, so BOUNDS is K times the port's error on exactly these inputs;
  * the host-only surface, no GPU: the new C ABI symbols and their argument errors, the Python
    signatures, GE2ELoss(loss_method=...).
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import contrast_cases as cc
from conftest import ROOT

ALL = cc.all_inputs()
IDS = [cc.case_id(c) for c in ALL]

AS_ENTRY_POINTS = ["sv_ge2e_fwd_rows", "sv_ge2e_fwd", "sv_ge2e_bwd_rows", "sv_ge2e_bwd", "sv_ge2e_train",
                   "sv_ge2e_shard_rows"]


# ------------------------------------------------------------------------------------- reference
def test_reference_matches_the_loop_form_of_eq7():
    E = cc.gc.make_offsphere(11, 3, 2, 4)
    for w, b in ((10.0, -5.0), (-2.0, 0.5)):
        per, _, _ = cc.contrast_per(torch.tensor(E, dtype=torch.float64), w, b)
        np.testing.assert_allclose(per.numpy(), cc.contrast_loop(E, w, b), rtol=0, atol=1e-12)


def test_reference_maximum_follows_S_and_ties_go_to_the_lowest_k():
    """A negative w selects the smallest cosine; among equal S the gradient goes to the lowest k."""
    E = torch.tensor(cc.inputs(4, 5, 64), dtype=torch.float64)
    _, S, idx = cc.contrast_per(E, -2.0, 0.5)
    cos = (S - 0.5) / -2.0
    off = cos.masked_fill(cc._eye(4, 5, 4), np.inf)
    assert torch.equal(idx, off.argmin(dim=2))
    S = torch.tensor([[[0.3, 1.5, 1.5, 1.5]], [[1.5, -0.2, 0.7, 1.5]]], dtype=torch.float64, requires_grad=True)
    per, idx = cc.contrast_on_S(S)
    per.sum().backward()
    assert idx.tolist() == [[1], [0]]
    assert (S.grad != 0).tolist() == [[[True, True, False, False]], [[True, True, False, False]]]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_gap_floor_and_live_rows(case):
    """The reference's smallest top-two gap of any row is at least GAP_FLOOR (else: another seed in
    SEED_SHIFT, never a lower floor), and no reference dE row is all zero (dE_row divides by it)."""
    ref = cc.reference(*case)
    print(f"\nMEASURED contrast_cases.gap.{cc.case_id(case)} {ref['gap']:.2e}")
    assert ref["gap"] >= cc.GAP_FLOOR
    assert np.abs(ref["dE"]).reshape(-1, case[2]).max(axis=1).min() > 0


def test_seed_shifts_are_needed():
    """The shifted shapes are below the floor with ge2e_cases' own seed (the table says why each
    shift is there)."""
    for (N, M, D), shift in cc.SEED_SHIFT.items():
        assert shift != 0
        E = torch.tensor(cc.gc.inputs(N, M, D), dtype=torch.float64)
        _, S, _ = cc.contrast_per(E, 10.0, -5.0)
        assert cc.top_two_gap(S) < cc.GAP_FLOOR


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_fp32_port_within_the_cap_and_on_the_same_column(case):
    ref, port = cc.reference(*case), cc.port_f32(*case)
    stats = cc.compare(port, ref)
    print(f"\nMEASURED contrast_cases.port_f32.{cc.case_id(case)} {cc.fmt(stats)}")
    assert not cc.over(stats, cc.BOUNDS, 1.0 / cc.K), cc.over(stats, cc.BOUNDS, 1.0 / cc.K)
    assert np.array_equal(port["kstar"], ref["kstar"])


def test_matrix_product_form_is_the_reference():
    """contrast_per_mm (BIG_CASE's reference) against contrast_per in fp64 at two table cases."""
    for case in ((7, 16, 36, 10.0, -5.0), (4, 5, 64, -2.0, 0.5)):
        a, b = cc.reference(*case), cc._run(*case, 1.0, torch.float64, cc.contrast_per_mm)
        assert np.array_equal(a["kstar"], b["kstar"])
        np.testing.assert_allclose(b["per"], a["per"], rtol=0, atol=1e-12)
        assert cc.gc.dE_row(b["dE"], a["dE"]) <= 1e-12
        assert abs(a["dw"] - b["dw"]) <= 1e-12 and abs(a["db"] - b["db"]) <= 1e-12


def test_big_case_keeps_the_floor_and_the_cap():
    """BIG_CASE under the same three conditions as the table's cases."""
    N, M, D, _, _ = cc.BIG_CASE
    assert N > 128 and N * M > 8 * 256          # beyond one round of 8-row workgroups on 256 CUs
    ref, port = cc.reference_mm(*cc.BIG_CASE), cc.port_f32(*cc.BIG_CASE, cc.contrast_per_mm)
    stats = cc.compare(port, ref)
    print(f"\nMEASURED contrast_cases.port_f32.{cc.case_id(cc.BIG_CASE)} gap {ref['gap']:.2e} {cc.fmt(stats)}")
    assert ref["gap"] >= cc.GAP_FLOOR
    assert np.abs(ref["dE"]).reshape(-1, D).max(axis=1).min() > 0
    assert not cc.over(stats, cc.BOUNDS, 1.0 / cc.K), cc.over(stats, cc.BOUNDS, 1.0 / cc.K)
    assert np.array_equal(port["kstar"], ref["kstar"])


def test_bounds_follow_the_rule():
    assert cc.K == 4 and cc.BOUNDS == {k: 4 * v for k, v in cc.PORT_MAX.items()}


def test_reference_gloss_scales_the_gradient():
    ref1, refg = cc.reference(*cc.GLOSS_CASE), cc.reference(*cc.GLOSS_CASE, cc.GLOSS)
    np.testing.assert_allclose(refg["dE"], cc.GLOSS * ref1["dE"], rtol=1e-12, atol=0)
    assert refg["loss"] == ref1["loss"]


# ------------------------------------------------------------------------------ host-only surface
def _header():
    src = open(os.path.join(ROOT, "include", "sv_ge2e.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_c_abi_has_the_loss_kind_entry_points():
    from pytorch_speaker_verification_amd import _lib
    h, src = _lib.lib(), _header()
    assert re.search(r"SV_GE2E_SOFTMAX\s*=\s*0\b", src) and re.search(r"SV_GE2E_CONTRAST\s*=\s*1\b", src)
    assert re.search(r"#define SV_ABI_VERSION 12\b", src) and h.sv_abi_version() == 12
    names = [n + "_as" for n in AS_ENTRY_POINTS] + ["sv_ge2e_calc_contrast", "sv_ge2e_calc_contrast_bwd"]
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _lib.SIGNATURES and hasattr(h, n), n
    for n in AS_ENTRY_POINTS:   # the sibling is its namesake with one leading int
        res, args = _lib.SIGNATURES[n]
        assert _lib.SIGNATURES[n + "_as"] == (res, [ctypes.c_int] + args), n
    assert _lib.LOSS_METHODS == {"softmax": 0, "contrast": 1}


def _as_args(name, loss, N):
    """Arguments of <name>_as with every pointer NULL: the ints are (loss, N_local = 1, M = 2, D = 4,
    spk_offset = 0, N) in the shard forms (*_rows) and (loss, N, M = 2, D = 4) in the others."""
    from pytorch_speaker_verification_amd import _lib
    _, args = _lib.SIGNATURES[name + "_as"]
    ints = iter([loss, 1, 2, 4, 0, N] if name.endswith("_rows") else [loss, N, 2, 4])
    return [next(ints) if a is ctypes.c_int else None for a in args]


@pytest.mark.parametrize("name", AS_ENTRY_POINTS)
def test_unknown_loss_and_single_speaker_are_refused_before_any_launch(name):
    """No GPU is touched: an unknown loss id is SV_EARG and the contrast loss with N = 1 SV_ESHAPE,
    both returned before the pointer checks (all pointers here are NULL) and so before any launch."""
    from pytorch_speaker_verification_amd import _lib
    f = getattr(_lib.lib(), name + "_as")
    for bad in (2, -1, 7):
        assert f(*_as_args(name, bad, 4)) == -1
    assert f(*_as_args(name, 1, 1)) == -3
    assert f(*_as_args(name, 1, 4)) == -1    # contrast, N fine: now the NULL pointers are the error
    assert f(*_as_args(name, 0, 1)) == -1    # the softmax keeps accepting N = 1 as a shape


def test_helper_refuses_a_row_without_a_negative():
    from pytorch_speaker_verification_amd import _lib
    h = _lib.lib()
    assert h.sv_ge2e_calc_contrast(None, 1, 2, 1, None, None, None) == -1
    assert h.sv_ge2e_calc_contrast(1 << 20, 1, 2, 1, 1 << 20, None, None) == -3   # (no launch: fake pointers)
    assert h.sv_ge2e_calc_contrast_bwd(1 << 20, 1, 2, 1, None, None, 1 << 20, None) == -3
    assert h.sv_ge2e_calc_contrast(1 << 20, 3, 2, 2, 1 << 20, None, None) == -1   # K < N


def test_python_surface():
    from pytorch_speaker_verification_amd import library, ops, sharded_ge2e, speech_embedder_net, train_speech_embedder, utils
    from pytorch_speaker_verification_amd.speech_embedder_net import GE2ELoss
    for fn in (ops.ge2e_forward, ops.ge2e_train, train_speech_embedder.train):
        assert inspect.signature(fn).parameters["loss_method"].default == "softmax"
    assert "loss_method" in inspect.signature(ops.ge2e_backward).parameters
    assert list(inspect.signature(ops.ge2e_train).parameters)[:4] == ["E", "w", "b", "dwdb_out"]
    m = GE2ELoss("cpu", loss_method="contrast")
    assert m.loss_method == "contrast" and m.w.item() == 10.0 and m.b.item() == -5.0
    assert GE2ELoss("cpu").loss_method == "softmax"
    assert list(m.state_dict()) == list(GE2ELoss("cpu").state_dict())
    with pytest.raises(ValueError, match="loss_method"):
        GE2ELoss("cpu", loss_method="triplet")
    with pytest.raises(ValueError, match="loss_method"):
        sharded_ge2e.ShardedGE2E(loss_method="triplet")
    assert sharded_ge2e.ShardedGE2E(loss_method="contrast").k.loss_method == "contrast"
    assert sharded_ge2e.HipFusedShard("contrast").kind == 1 and sharded_ge2e.HipFusedShard().kind == 0
    assert speech_embedder_net.calc_loss_contrast is utils.calc_loss_contrast
    assert 'str loss_method="softmax"' in str(torch.ops.sv.ge2e_loss.default._schema)
    assert library.ge2e_loss is not None


def test_dropin_shims_reexport_the_helper():
    import importlib.util
    from pytorch_speaker_verification_amd import utils
    for mod in ("utils", "speech_embedder_net"):
        spec = importlib.util.spec_from_file_location("dropin_" + mod, os.path.join(ROOT, "dropin", mod + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        assert m.calc_loss_contrast is utils.calc_loss_contrast


def test_library_op_fake_kernel_takes_the_method():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from pytorch_speaker_verification_amd import library
    with FakeTensorMode():
        E = torch.empty(3, 2, 8, device="cuda")
        w, b = torch.empty((), device="cuda"), torch.empty((), device="cuda")
        loss, per = library.ge2e_loss(E, w, b, "contrast")
        assert loss.shape == () and per.shape == (3, 2)
        dE, dw, db = library.ge2e_loss_backward(E, w, b, loss, "contrast")
        assert dE.shape == E.shape and dw.shape == () and db.shape == ()
