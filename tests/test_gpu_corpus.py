"""GPU: training batches cut out of the device-resident corpus (sv_corpus_batch / _bf16,
csrc/sv_corpus.hip) -- the kernel against index arithmetic and against the entry points it replaces
(exact), its clamps, and the paths above it: forward / backward, the fused trainer with a changing
frame count T (bit-identical to the step on the materialised batch, and against the torch port),
and the train() driver on a resident dataset."""
import os
import random

import numpy as np
import pytest
import torch

import recipe
from conftest import golden, model_dims
from oracle import torch_port

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64  # elements of NaN before and after every output (a multiple of 16 bytes in both dtypes)

# (U, F, Tc, B, T)
SHAPES = [(7, 40, 20, 5, 13),          # starts {0, 7, 3, 1, 6}; utterances 0, U - 1 and a repeat
          (3, 8, 9, 1, 9),             # T = Tc
          (11, 64, 33, 70, 1),         # T = 1; B crosses a row block; two mel chunks
          (200, 40, 180, 130, 141)]    # production frame count; odd T; B % 8 != 0


def _corpus(U, F, Tc, seed=0):
    from pytorch_speaker_verification_amd.data_load import DeviceCorpus
    return DeviceCorpus([np.random.default_rng(100 + seed + U + F + Tc).standard_normal((U, F, Tc)).astype(np.float32)],
                        device=DEV)


def _tables(U, F, Tc, B, T):
    if (B, T) == (5, 13):
        utt, start = [0, U - 1, 3, 3, 2], [0, 7, 3, 1, 6]
    else:
        rng = np.random.default_rng(B * 1000 + T)
        utt, start = rng.integers(0, U, B), rng.integers(0, Tc - T + 1, B)
    return (torch.tensor(np.asarray(utt), dtype=torch.int32, device=DEV),
            torch.tensor(np.asarray(start), dtype=torch.int32, device=DEV))


def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _run_kernel(bf16, corpus, utt, start, T, Bp, with_xT=True):
    """(x_tm [T,B,F], xT [F,T,Bp] or None) from the entry point, written inside NaN-filled buffers
    whose guards must come back untouched."""
    from pytorch_speaker_verification_amd._lib import call, ptr, stream_of
    U, F, Tc = corpus.data.shape
    B = utt.shape[0]
    dtype = torch.bfloat16 if bf16 else torch.float32
    xbuf, x = _guarded(T * B * F, dtype)
    tbuf, xT = _guarded(F * T * Bp, dtype)
    call("sv_corpus_batch_bf16" if bf16 else "sv_corpus_batch", ptr(corpus.data), U, F, Tc, ptr(utt), ptr(start), B, T,
         ptr(x), ptr(xT) if with_xT else None, Bp, stream_of(corpus.data))
    torch.cuda.synchronize()
    assert _guards_intact(xbuf) and _guards_intact(tbuf)
    if not with_xT:
        assert bool(torch.isnan(tbuf).all())
        return x.view(T, B, F), None
    return x.view(T, B, F), xT.view(F, T, Bp)


def _replaced_entry_points(bf16, xb, Bp):
    """The same operands by the launches the kernel replaces, on the materialised batch xb [B,T,F]."""
    from pytorch_speaker_verification_amd._lib import call, ptr, stream_of
    B, T, F = xb.shape
    s = stream_of(xb)
    if bf16:
        x_bf = torch.empty((T, B, F), dtype=torch.bfloat16, device=DEV)
        xT = torch.empty((F, T, Bp), dtype=torch.bfloat16, device=DEV)
        call("sv_frames_to_bf16", ptr(xb), B, T, F, ptr(x_bf), ptr(xT), Bp, s)
        return x_bf, xT
    x_tm = torch.empty((T, B, F), dtype=torch.float32, device=DEV)
    call("sv_frames_to_time_major", ptr(xb), ptr(x_tm), B, T, F, s)
    xT = torch.zeros((F, T, Bp), dtype=torch.float32, device=DEV)
    for t in range(T):
        call("sv_transpose", ptr(x_tm[t]), F, B, F, ptr(xT) + 4 * t * Bp, T * Bp, s)
    return x_tm, xT


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_index_arithmetic(shape, bf16):
    U, F, Tc, B, T = shape
    corpus = _corpus(U, F, Tc)
    utt, start = _tables(*shape)
    v = 8 if bf16 else 4
    Bp = (B + v - 1) // v * v
    xb = corpus.frames(utt, start, T)  # [B, T, F] by torch indexing
    want = xb.to(torch.bfloat16) if bf16 else xb
    want_x = want.transpose(0, 1).contiguous()
    want_xT = torch.zeros((F, T, Bp), dtype=want.dtype, device=DEV)
    want_xT[:, :, :B] = want.permute(2, 1, 0)
    x, xT = _run_kernel(bf16, corpus, utt, start, T, Bp)
    assert torch.equal(x, want_x)
    assert torch.equal(xT, want_xT)  # (the padding columns b in [B, Bp) are zero)
    old_x, old_xT = _replaced_entry_points(bf16, xb, Bp)
    assert torch.equal(x, old_x) and torch.equal(xT, old_xT)
    x_only, none = _run_kernel(bf16, corpus, utt, start, T, Bp, with_xT=False)
    assert none is None and torch.equal(x_only, want_x)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_tables_are_clamped_into_the_corpus(bf16):
    """The corpus sits inside a larger allocation with one utterance of NaN before and after it: a
    missing clamp shows as a mismatch (a NaN), never as a read outside the allocation."""
    U, F, Tc, B, T = 6, 40, 20, 8, 13
    corpus = _corpus(U, F, Tc)
    big = torch.full((U + 2, F, Tc), float("nan"), dtype=torch.float32, device=DEV)
    big[1:U + 1] = corpus.data
    corpus.data = big[1:U + 1]
    assert corpus.data.is_contiguous() and corpus.data.data_ptr() % 16 == 0
    bad_utt = torch.tensor([-1, U, 2, -1, U, 0, U - 1, 3], dtype=torch.int32, device=DEV)
    bad_start = torch.tensor([-5, Tc, Tc, -5, 3, -5, Tc, 7], dtype=torch.int32, device=DEV)
    utt, start = bad_utt.clamp(0, U - 1), bad_start.clamp(0, Tc - T)
    assert start.tolist() == [0, 7, 7, 0, 3, 0, 7, 7] and utt.tolist() == [0, U - 1, 2, 0, U - 1, 0, U - 1, 3]
    x, xT = _run_kernel(bf16, corpus, bad_utt, bad_start, T, B)
    want_x, want_xT = _run_kernel(bf16, corpus, utt, start, T, B)
    assert not bool(torch.isnan(x.float()).any()) and not bool(torch.isnan(xT.float()).any())
    assert torch.equal(x, want_x) and torch.equal(xT, want_xT)
    ref = corpus.frames(utt, start, T).transpose(0, 1)
    assert torch.equal(x, ref.to(torch.bfloat16) if bf16 else ref)


def _build(dims, sd_np, precision="f32", schedule="auto"):
    from pytorch_speaker_verification_amd.speech_embedder_net import GE2ELoss, SpeechEmbedder
    with model_dims(*dims):
        net = SpeechEmbedder()
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(torch.as_tensor(sd_np[k]))
    net.precision, net.schedule = precision, schedule
    return net.to(DEV), GE2ELoss(DEV)


def _batch(corpus, B, T, seed):
    from pytorch_speaker_verification_amd.data_load import CorpusBatch
    rng = np.random.default_rng(seed)
    utt = torch.tensor(rng.integers(0, corpus.n_utt, B), dtype=torch.int32, device=DEV)
    start = torch.tensor(rng.integers(0, corpus.n_frames - T + 1, B), dtype=torch.int32, device=DEV)
    return CorpusBatch(corpus, utt, start, T)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_forward_and_backward_are_bit_identical(precision):
    from pytorch_speaker_verification_amd import ops
    dims, B, T = (40, 64, 3, 32), 9, 13
    net, _ = _build(dims, recipe.make_weights(77, *dims, scale=3.0))
    layers = [tuple(p.detach() for p in lp) for lp in net.LSTM_stack.layer_params()]
    w_p, b_p = net.projection.weight.detach(), net.projection.bias.detach()
    batch = _batch(_corpus(17, 40, 30), B, T, 5)
    demb = torch.tensor(np.random.default_rng(9).standard_normal((B, dims[3])).astype(np.float32), device=DEV)
    out = []
    for x in (batch, batch.frames()):
        emb, st = ops.embedder_fwd(precision, x, layers, w_p, b_p)
        grads = ops.embedder_bwd(precision, st, demb, layers, w_p)
        out.append([emb, st.x_tm[0], st.xT0] + list(grads))
    ops.check_persistent_status(wait=True)
    assert len(out[0]) == 3 + 4 * dims[2] + 2
    for i, (a, b) in enumerate(zip(*out)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), i
    assert bool(torch.isfinite(out[0][0]).all())
    emb_nosave, _ = ops.embedder_fwd(precision, batch, layers, w_p, b_p, save=False)  # xT = NULL
    assert torch.equal(emb_nosave, out[0][0])
    net.precision = precision  # the module (autograd path) materialises the batch
    with torch.no_grad():
        assert torch.equal(net(batch), net(batch.frames())) and torch.equal(net(batch), out[0][0])


def test_test_driver_on_a_resident_dataset(tmp_path, capsys):
    """test() under the same seeds on the host loader and on a resident dataset: the same batches,
    so the same printed EER lines and the same average."""
    from pytorch_speaker_verification_amd import data_load
    from pytorch_speaker_verification_amd import train_speech_embedder as tse
    from pytorch_speaker_verification_amd.hparam import hparam as hp
    g = golden("eer.npz")
    d = tmp_path / "test"
    recipe.make_speaker_dir(str(d), int(g["n_spk"]), int(g["data_seed"]))
    ckpt = os.path.join(os.path.dirname(__file__), "golden", "ref_small_checkpoint.pth")
    saved = {k: dict(v) for k, v in hp.items() if isinstance(v, dict)}
    saved_top = {k: v for k, v in hp.items() if not isinstance(v, dict)}
    out = []
    try:
        hp.device = "cuda"
        hp.data.nmels, hp.model.hidden, hp.model.num_layer, hp.model.proj = [int(v) for v in g["dims"]]
        hp.training = False
        hp.data.test_path = str(d)
        hp.test.N, hp.test.M, hp.test.epochs, hp.test.num_workers = int(g["N"]), int(g["M"]), 2, 0
        for resident in (False, True):
            random.seed(4)
            np.random.seed(4)
            torch.manual_seed(4)
            ds = data_load.SpeakerDatasetResident(data_load.DeviceCorpus(str(d), device=DEV)) if resident else None
            capsys.readouterr()
            out.append((tse.test(ckpt, dataset=ds), capsys.readouterr().out))
    finally:
        for k, v in saved.items():
            hp[k].update(v)
        for k, v in saved_top.items():
            hp[k] = v
    assert out[0] == out[1] and "EER" in out[0][1] and np.isfinite(out[0][0])


@pytest.mark.parametrize("precision,schedule,chunks", [("f32", "auto", None), ("bf16", "auto", None),
                                                       ("bf16", "persist", None), ("bf16", "auto", [(0, 5), (5, 9)])])
def test_trainer_with_changing_T_is_bit_identical(precision, schedule, chunks, monkeypatch):
    """Three steps with T = 11, 12, 9 on CorpusBatch objects against a second trainer from the same
    init on the materialised batches: loss and every parameter after each step."""
    from pytorch_speaker_verification_amd import trainer as trainer_mod
    if chunks:
        monkeypatch.setattr(trainer_mod, "bf16_row_chunks", lambda *a, **k: list(chunks))
    dims, N, M = (40, 64, 3, 32), 3, 3
    sd = recipe.make_weights(31, *dims, scale=3.0)
    corpus = _corpus(17, 40, 30)
    trs = [trainer_mod.GE2ETrainer(*_build(dims, sd, precision, schedule), lr=0.01) for _ in range(2)]
    for i, T in enumerate((11, 12, 9)):
        batch = _batch(corpus, N * M, T, 40 + i)
        la = trs[0].step(batch, N, M)
        lb = trs[1].step(batch.frames(), N, M)
        assert torch.equal(la, lb) and bool(torch.isfinite(la)), (i, float(la), float(lb))
        assert torch.equal(trs[0].flat_p, trs[1].flat_p), i
    for tr in trs:
        tr.check()


def test_trainer_with_changing_T_against_torch_port():
    """The same changing-T steps (T = 11 then 9) against the stock PyTorch port on the host, at the
    tolerances of test_ragged_training_step_against_torch_port for these dims."""
    from pytorch_speaker_verification_amd.trainer import GE2ETrainer
    dims, N, M = (40, 96, 2, 24), 3, 3
    sd = recipe.make_weights(131, *dims, scale=2.0)
    corpus = _corpus(17, 40, 30)
    net, ge2e = _build(dims, sd)
    tr = GE2ETrainer(net, ge2e, lr=0.01)
    port = torch_port.SpeechEmbedderPort(*dims)
    torch_port.load_recipe_weights(port, sd)
    w = torch.nn.Parameter(torch.tensor(10.0))
    b = torch.nn.Parameter(torch.tensor(-5.0))
    opt = torch.optim.SGD([{"params": port.parameters()}, {"params": [w, b]}], lr=0.01)
    losses, ref = [], []
    for i, T in enumerate((11, 9)):
        batch = _batch(corpus, N * M, T, 60 + i)
        losses.append(float(tr.step(batch, N, M)))
        ref.append(float(torch_port.train_step(port, w, b, opt, batch.frames().cpu(), N, M)))
    np.testing.assert_allclose(losses, ref, rtol=1e-4)
    got = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    for k, v in port.state_dict().items():
        np.testing.assert_allclose(got[k], v.numpy(), atol=5e-5, err_msg=k)
    np.testing.assert_allclose([ge2e.w.item(), ge2e.b.item()], [w.item(), b.item()], atol=1e-5)


LENGTHS, DRIVER_SEED = (9, 11, 12), 0  # (a seed whose 12 batches draw more than one length: asserted below)


def test_train_driver_on_a_resident_dataset(tmp_path, monkeypatch):
    from pytorch_speaker_verification_amd import data_load
    from pytorch_speaker_verification_amd import train_speech_embedder as tse
    from pytorch_speaker_verification_amd.hparam import hparam as hp
    from pytorch_speaker_verification_amd.trainer import GE2ETrainer
    g = golden("eer.npz")
    d = tmp_path / "train"
    recipe.make_speaker_dir(str(d), 12, 5)
    saved = {k: dict(v) for k, v in hp.items() if isinstance(v, dict)}
    saved_top = {k: v for k, v in hp.items() if not isinstance(v, dict)}
    seen = []
    orig = GE2ETrainer.step

    def recording_step(self, x, N, M, probe=None):
        xm = x.frames() if isinstance(x, data_load.CorpusBatch) else x
        seen.append(xm.detach().float().cpu().clone())
        return orig(self, x, N, M, probe)

    monkeypatch.setattr(GE2ETrainer, "step", recording_step)

    def run(tag, epochs, resident, **kw):
        hp.train.epochs = epochs
        hp.train.checkpoint_dir = str(tmp_path / tag)
        hp.train.log_file = str(tmp_path / tag / "Stats")
        random.seed(3)
        np.random.seed(3)
        torch.manual_seed(3)
        del seen[:]
        dataset = data_load.SpeakerDatasetResident(data_load.DeviceCorpus(str(d), device=DEV)) if resident else None
        path = tse.train(str(tmp_path / "none.model"), dataset=dataset, **kw)
        lines = open(hp.train.log_file).read().strip().splitlines()
        return list(seen), path, sorted(os.listdir(hp.train.checkpoint_dir)), lines

    try:
        hp.device = "cuda"
        hp.data.nmels, hp.model.hidden, hp.model.num_layer, hp.model.proj = [int(v) for v in g["dims"]]
        hp.training = True
        hp.data.train_path = str(d)
        hp.train.N, hp.train.M, hp.train.num_workers = 4, 5, 0
        hp.train.log_interval, hp.train.checkpoint_interval = 1, 2
        hp.train.restore = False
        host, _, _, host_lines = run("host", 2, False)
        res, _, _, res_lines = run("resident", 2, True)
        var, path, files, lines = run("var", 4, True, lengths=LENGTHS, crop="random", seed=DRIVER_SEED)
        with pytest.raises(ValueError):
            tse.train(str(tmp_path / "none.model"), lengths=LENGTHS)  # the host loader has one length
    finally:
        for k, v in saved.items():
            hp[k].update(v)
        for k, v in saved_top.items():
            hp[k] = v
    # the resident run sees the host loader's batches, bit for bit and in its order
    assert len(host) == len(res) == 6 and all(tuple(x.shape) == (20, 160, 40) for x in host)
    assert all(torch.equal(a, b) for a, b in zip(host, res))
    assert [ln.split("\t", 1)[1] for ln in host_lines] == [ln.split("\t", 1)[1] for ln in res_lines]  # same losses
    # variable lengths
    Ts = [int(x.shape[1]) for x in var]
    assert len(var) == 12 and all(T in LENGTHS for T in Ts) and len(set(Ts)) >= 2, Ts
    assert all(tuple(x.shape) == (20, T, 40) for x, T in zip(var, Ts))
    assert "ckpt_epoch_2_batch_id_3.pth" in files and "ckpt_epoch_4_batch_id_3.pth" in files
    assert os.path.basename(path) == "final_epoch_4_batch_id_3.model"
    assert len(lines) == 12 and "Epoch:1[1/3],Iteration:1" in lines[0]
    first = float(lines[0].split("Loss:")[1].split()[0])
    last = float(lines[-1].split("Loss:")[1].split()[0])
    assert np.isfinite(last) and last < first, (first, last)
