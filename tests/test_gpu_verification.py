"""GPU: the fused trial scorer (sv_trial_hist, csrc/sv_trials.hip) against the numpy oracle
(verification_ref.py) -- exact counts on dyadic inputs at the shapes where tiling goes wrong, the
under- / overflow / NaN slots and accumulation, a sandwich between fp64 counts on real-valued unit
rows -- and the surface above it: corpus_eer, the d-vector builders, evaluate, test(protocol="corpus")."""
import itertools

import numpy as np
import pytest
import torch

import recipe
import verification_ref as R
from conftest import model_dims

pytestmark = pytest.mark.gpu
DEV = "cuda"
DELTA = 2e-5  # fp32 dot product of unit vectors, any order: D 2^-24 = 1.53e-5 at D = 256; the rest: the slot rule


def _V():
    from pytorch_speaker_verification_amd import verification
    return verification


def _dev(x, sliced=False):
    """x on the device; sliced: as a column slice of a wider tensor (row stride D + 8, 16 B in)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    if not sliced:
        return t
    wide = torch.full((t.shape[0], t.shape[1] + 8), float("nan"), dtype=t.dtype, device=DEV)
    wide[:, 4:4 + t.shape[1]] = t
    return wide[:, 4:4 + t.shape[1]]


def _label_kinds(rng, na, nb):
    """all equal; all distinct within an operand (row i and row i of the other share a label); a few
    speakers with some rows -1."""
    some = lambda n: np.where(rng.random(n) < 0.2, -1, rng.integers(0, 5, n)).astype(np.int32)  # noqa: E731
    return {"equal": (np.zeros(na, np.int32), np.zeros(nb, np.int32)),
            "distinct": (np.arange(na, dtype=np.int32), np.arange(nb, dtype=np.int32)),
            "some-1": (some(na), some(nb))}


# rectangular (Na, Nb) and symmetric (U, None): one row, tile edge +- 1, more than one tile each way
SHAPES = [(1, 1), (127, 129), (130, 257), (1, None), (2, None), (129, None), (300, None)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}" if s[1] else f"sym{s[0]}")
def test_counts_are_exact_on_dyadic_inputs(shape):
    """Entries k / 8, k in [-8, 8]: every dot product is exact in fp32 in any order, and with
    [lo, hi) = [-P, P), P the power of two >= D, and bins a power of two so is the slot.  Counts
    equal the oracle slot for slot, for every D, grid, label kind, bin count and row stride."""
    V = _V()
    na, nb = shape
    sym = nb is None
    rng = np.random.default_rng(7 + na + (nb or 0))
    n_cases = 0
    for D in (4, 36, 256):
        span = float(1 << int(np.ceil(np.log2(D))))
        a = R.dyadic_rows(rng, na, D)
        b = None if sym else R.dyadic_rows(rng, nb, D)
        s = R.scores(a, b)
        assert np.abs(s).max() <= span
        for kind, (la, lb) in _label_kinds(rng, na, na if sym else nb).items():
            live, target = R.pairs(la, None if sym else lb)
            non, tar = R.split(s, live, target)
            for bins, grid, sliced in itertools.product((1, 64, 8192), (0, 1, 3), (False, True)):
                if sliced and grid != 0:
                    continue
                lo32, hi32, inv = V.bin_params(bins, -span, span)
                want = R.hist_of_scores(non, tar, lo32, inv, bins)
                h = V.trial_histograms(_dev(a, sliced), _dev(la), None if sym else _dev(b, sliced),
                                       None if sym else _dev(lb), bins=bins, lo=-span, hi=span, grid=grid)
                assert h.counts.dtype == np.int64 and h.counts.shape == (2, bins + 2)
                assert np.array_equal(h.counts, want), (D, kind, bins, grid, sliced)
                assert int(h.counts.sum()) == int(live.sum())
                assert (h.lo, h.hi, h.bins) == (-span, span, bins)
                n_cases += 1
    assert n_cases == 3 * 3 * (9 + 3)


def test_one_workgroup_flushes_mid_run():
    """grid = 1 over 23 * 24 / 2 = 276 tiles: more than the 256 tiles between two flushes of the
    workgroup's 32-bit histograms (csrc/sv_trials.hip), so the counts pass through a mid-run flush."""
    V = _V()
    rng = np.random.default_rng(11)
    U, D, bins = 23 * 128, 4, 64
    a = R.dyadic_rows(rng, U, D)
    lab = rng.integers(0, 3, U).astype(np.int32)
    lo32, _, inv = V.bin_params(bins, -4.0, 4.0)
    live, target = R.pairs(lab)
    want = R.hist_of_scores(*R.split(R.scores(a), live, target), lo32, inv, bins)
    da, dl = _dev(a), _dev(lab)
    for grid in (1, 2, 0):
        h = V.trial_histograms(da, dl, bins=bins, lo=-4.0, hi=4.0, grid=grid)
        assert np.array_equal(h.counts, want), grid
    assert int(want.sum()) == U * (U - 1) // 2


def test_row_offsets_past_2_31_elements():
    """2^21 + 130 rows at a row stride of 1024 floats: the last 130 rows start past element 2^31 of
    the allocation (8.6 GB, of which only the first D columns are ever written or read)."""
    V = _V()
    rng = np.random.default_rng(13)
    na, nb, lda, D, bins = (1 << 21) + 130, 3, 1024, 4, 64
    a, b = R.dyadic_rows(rng, na, D), R.dyadic_rows(rng, nb, D)
    la, lb = rng.integers(0, 3, na).astype(np.int32), np.arange(nb, dtype=np.int32)
    wide = torch.empty((na, lda), dtype=torch.float32, device=DEV)
    view = wide[:, :D]
    view.copy_(torch.from_numpy(a))
    assert V._rows(view, "a") is view and (na - 1) * lda >= 1 << 31
    lo32, _, inv = V.bin_params(bins, -4.0, 4.0)
    h = V.trial_histograms(view, _dev(la), _dev(b), _dev(lb), bins=bins, lo=-4.0, hi=4.0)
    assert np.array_equal(h.counts, R.hist(a, la, b, lb, lo32, inv, bins)) and int(h.counts.sum()) == na * nb
    # the rows past 2^31 alone, through a view that starts there
    tail = view[1 << 21:]
    h = V.trial_histograms(tail, _dev(la[1 << 21:]), _dev(b), _dev(lb), bins=bins, lo=-4.0, hi=4.0)
    assert np.array_equal(h.counts, R.hist(a[1 << 21:], la[1 << 21:], b, lb, lo32, inv, bins))


def test_slots_nan_and_accumulation():
    from pytorch_speaker_verification_amd._lib import call, lib, ptr, stream_of
    V = _V()
    rng = np.random.default_rng(5)
    na, nb, D, bins = 70, 131, 8, 16
    a, b = R.dyadic_rows(rng, na, D), R.dyadic_rows(rng, nb, D)
    a[3, 1] = np.nan  # every pair of row 3 scores NaN: slot 0
    la, lb = rng.integers(0, 3, na).astype(np.int32), rng.integers(0, 3, nb).astype(np.int32)
    lo, hi = -0.5, 0.75
    lo32, hi32, inv = V.bin_params(bins, lo, hi)
    s = R.scores(a, b)
    live, target = R.pairs(la, lb)
    h = V.trial_histograms(_dev(a), _dev(la), _dev(b), _dev(lb), bins=bins, lo=lo, hi=hi)
    assert np.array_equal(h.counts, R.hist(a, la, b, lb, lo32, inv, bins))
    for row, cls in ((0, live & ~target), (1, target)):
        with np.errstate(invalid="ignore"):
            below, above = (s < lo) | np.isnan(s), s >= hi
        assert h.counts[row, 0] == (cls & below).sum() > nb // 3  # (row 3's NaN pairs are in there)
        assert h.counts[row, -1] == (cls & above).sum() > 0
        assert h.counts[row, 1:-1].sum() == (cls & ~below & ~above).sum() > 0
    assert h.counts[:, 0].sum() >= nb
    # the kernel adds into hist: a second call on the same buffer doubles every slot
    da, dla, db, dlb = _dev(a), _dev(la), _dev(b), _dev(lb)
    hist = torch.zeros(int(lib().sv_trial_hist_size(bins)) // 8, dtype=torch.int64, device=DEV)
    for _ in range(2):
        call("sv_trial_hist", ptr(da), D, ptr(dla), na, ptr(db), D, ptr(dlb), nb, D, 0, float(lo32), float(inv), bins,
             ptr(hist), 0, stream_of(da))
    assert np.array_equal(hist.view(2, bins + 2).cpu().numpy(), 2 * h.counts)


@pytest.fixture(scope="module")
def real():
    """The real-valued inputs and their fp64 scores by class, computed once."""
    x, lab = R.speaker_rows()
    live, target = R.pairs(lab)
    non, tar = R.split(R.scores(x), live, target)
    non.setflags(write=False)
    tar.setflags(write=False)
    return x, lab, non, tar


def test_real_valued_counts_lie_between_the_fp64_counts(real):
    """12 speakers x 25 utterances, D = 256, unit rows, 256 bins on [-1, 1): at every edge e the kernel's
    count of scores >= e lies between the fp64 counts of scores >= e + DELTA and >= e - DELTA, per class."""
    V = _V()
    x, lab, non, tar = real
    assert abs(R.eer_sorted(non, tar)[0] - 0.1397) < 5e-5
    h = V.trial_histograms(_dev(x), _dev(lab), bins=256)
    assert h.n_nontarget == non.size == 41250 and h.n_target == tar.size == 3600
    edges = h.edges()
    assert np.array_equal(edges, -1.0 + np.arange(257) / 128.0)
    acc_non, acc_tar, _, _ = V._accepted(h)
    near = 0
    for got, ref in ((acc_non, non), (acc_tar, tar)):
        lo_cnt, hi_cnt = R.count_ge(ref, edges + DELTA), R.count_ge(ref, edges - DELTA)
        print("kernel - fp64 count at the edges: max", int(np.abs(got - R.count_ge(ref, edges)).max()))
        assert np.all(lo_cnt <= got) and np.all(got <= hi_cnt)
        near += int((hi_cnt - lo_cnt).sum())
    share = near / float(non.size + tar.size)
    print("share of pairs within DELTA of an edge:", share)
    assert share <= 0.01  # (0.52 % in numpy: the sandwich leaves a miscount nowhere to hide)


def _widening(non, tar, thr):
    allp = np.concatenate([non, tar])
    return int((np.abs(allp - thr) <= DELTA).sum()) / float(min(non.size, tar.size))


def test_corpus_eer_on_the_real_valued_inputs(real):
    V = _V()
    x, lab, non, tar = real
    e, thr, far, frr, e_lo, e_hi, res = V.corpus_eer(_dev(x), _dev(lab), bins=4096, passes=2)
    want = R.eer_sorted(non, tar)[0]
    w = _widening(non, tar, thr)
    print(f"eer {e} in [{e_lo}, {e_hi}], oracle {want}, widening {w}, resolution {res}")
    assert res == pytest.approx(2.0 / 4096 / 4096 * 2, rel=1e-6)
    assert e_lo <= e <= e_hi and e == (far + frr) / 2
    assert e_lo - w <= want <= e_hi + w
    assert e_hi - e_lo <= 10 * w  # the second pass resolved the crossing to a handful of pairs


@pytest.mark.parametrize("seed", range(4))
def test_corpus_eer_on_dyadic_inputs(seed):
    """Entries k / 32, D = 8: scores are multiples of 2^-10 inside [-0.5, 0.5], exact in fp32, and the
    second pass' range (two first-pass bins, 2^-10 wide) holds exactly one such value."""
    V = _V()
    rng = np.random.default_rng(seed)
    n_spk, per, D = 6, 20, 8
    base = rng.choice([-4, 4], size=(n_spk, 1, D))
    rows = ((base + rng.integers(-4, 5, size=(n_spk, per, D))) / 32.0).reshape(-1, D).astype(np.float32)
    lab = np.repeat(np.arange(n_spk, dtype=np.int32), per)
    live, target = R.pairs(lab)
    non, tar = R.split(R.scores(rows), live, target)
    want = R.eer_sorted(non, tar)[0]
    da, dl = _dev(rows), _dev(lab)
    e, thr, far, frr, e_lo, e_hi, res = V.corpus_eer(da, dl, passes=2)
    assert e_lo <= want <= e_hi
    hs = V._passes(da, dl, None, None, 4096, 2)
    assert len(hs) == 2 and hs[1].hi - hs[1].lo == 2.0 ** -10 and res == 2.0 ** -22
    inside = np.unique(np.concatenate([non, tar])[(np.concatenate([non, tar]) >= hs[1].lo)
                                                  & (np.concatenate([non, tar]) < hs[1].hi)])
    assert inside.size == 1
    assert e == want
    one = V.corpus_eer(da, dl, passes=1)
    assert one[4] <= want <= one[5] and one[6] == 2.0 ** -11 and one[5] - one[4] >= e_hi - e_lo


# ----------------------------------------------------------------------------- the public surface, toy dims
DIMS = (40, 64, 2, 32)


@pytest.fixture(scope="module")
def toy():
    from pytorch_speaker_verification_amd.data_load import DeviceCorpus
    from pytorch_speaker_verification_amd.speech_embedder_net import SpeechEmbedder
    with model_dims(*DIMS):
        net = SpeechEmbedder()
    sd = recipe.make_weights(21, *DIMS, scale=3.0)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(torch.as_tensor(sd[k]))
    net = net.to(DEV).eval()
    rng = np.random.default_rng(9)
    mean = rng.standard_normal((3, 1, 40, 1))
    corpus = DeviceCorpus([(mean[k] + rng.standard_normal((4, 40, 180))).astype(np.float32) for k in range(3)],
                          device=DEV)
    return net, corpus


def test_corpus_dvectors_equal_the_module_bit_for_bit(toy):
    V = _V()
    net, corpus = toy
    ids = torch.arange(12)
    with torch.no_grad():
        want = net(corpus.frames(ids, torch.zeros_like(ids), 160))
        late = corpus.frames(ids, torch.full_like(ids, 20), 150)
        want_late = torch.cat([net(late[i:i + 5]) for i in range(0, 12, 5)])  # (the same batches)
    d = V.corpus_dvectors(net, corpus)
    assert d.shape == (12, 32) and d.dtype == torch.float32 and torch.equal(d, want)
    assert torch.equal(V.corpus_dvectors(net, corpus, T=150, start=20, batch=5), want_late)
    assert torch.allclose(d.norm(dim=1), torch.ones(12, device=DEV), atol=1e-6)
    with pytest.raises(ValueError):
        V.corpus_dvectors(net, corpus, T=170, start=11)


def test_utterance_dvectors_equal_embed_windows_and_a_numpy_mean(toy):
    from pytorch_speaker_verification_amd import dvector
    V = _V()
    net, corpus = toy
    lengths = [40, 180, 99, 60]  # one window; many; a ragged tail; a window that ends exactly at T
    frames = torch.cat([corpus.data[u, :, :T].T for u, T in enumerate(lengths)]).contiguous()  # [n_frames, 40]
    frame_off = np.concatenate([[0], np.cumsum(lengths)])
    got = V.utterance_dvectors(net, frames, frame_off, win=40, hop=20)
    starts, part_off = V.utterance_windows(frame_off, 40, 20)
    assert list(np.diff(part_off)) == [1, 8, 3, 2]
    windows = torch.stack([frames[s:s + 40] for s in starts])
    emb = dvector.embed_windows(net, windows).cpu().numpy().astype(np.float64)
    want = np.stack([emb[a:b].mean(axis=0) for a, b in zip(part_off[:-1], part_off[1:])])
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert got.shape == (4, 32) and got.dtype == torch.float32
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-6
    with pytest.raises(ValueError, match="utterance 0 has 40 frames"):
        V.utterance_dvectors(net, frames, frame_off, win=41, hop=20)


def _check_against_oracle(r, non, tar, p_target=0.01):
    """evaluate's dict against the sorted fp64 scores: the class sizes exactly; the EER exactly when
    the pair that decides it is alone within DELTA of the threshold (no fp32 / fp64 reordering can
    then touch it), else inside the interval widened as for corpus_eer; minDCF between the fp64 bounds
    of the DELTA sandwich (the cost rises with FAR and with FRR)."""
    assert (r["n_target"], r["n_nontarget"]) == (tar.size, non.size)
    want = R.eer_sorted(non, tar)[0]
    n_near = int((np.abs(np.concatenate([non, tar]) - r["threshold"]) <= DELTA).sum())
    w = n_near / float(min(non.size, tar.size))
    print(r, "oracle eer", want, "pairs near the threshold", n_near)
    assert r["eer_lo"] <= r["eer"] <= r["eer_hi"] and r["eer_lo"] - w <= want <= r["eer_hi"] + w
    if n_near == 1:
        assert r["eer"] == want
    edges = -1.0 + np.arange(4097) / 2048.0
    far_hi, frr_lo = R.rates_at(non, tar, edges - DELTA)
    far_lo, frr_hi = R.rates_at(non, tar, edges + DELTA)
    norm = min(p_target, 1.0 - p_target)
    lower = np.min(p_target * frr_lo + (1.0 - p_target) * far_lo) / norm
    upper = np.min(p_target * frr_hi + (1.0 - p_target) * far_hi) / norm
    assert lower - 1e-12 <= r["min_dcf"] <= upper + 1e-12


def test_evaluate_in_both_protocols_against_the_oracle(toy, tmp_path, capsys):
    from pytorch_speaker_verification_amd import data_load
    from pytorch_speaker_verification_amd import train_speech_embedder as tse
    from pytorch_speaker_verification_amd.hparam import hparam as hp
    V = _V()
    net, corpus = toy
    d = V.corpus_dvectors(net, corpus).cpu().numpy().astype(np.float64)
    lab = np.repeat(np.arange(3, dtype=np.int32), 4)
    # all pairs of utterances
    live, target = R.pairs(lab)
    non, tar = R.split(R.scores(d), live, target)
    assert (non.size, tar.size) == (48, 18)
    r = V.evaluate(net, corpus)
    assert sorted(r) == ["eer", "eer_hi", "eer_lo", "min_dcf", "n_nontarget", "n_target", "threshold"]
    _check_against_oracle(r, non, tar)
    # enrol on the first two utterances of a speaker, test the other two against all three models
    models = np.stack([d[4 * k:4 * k + 2].mean(axis=0) for k in range(3)])
    models /= np.linalg.norm(models, axis=1, keepdims=True)
    tests = np.concatenate([d[4 * k + 2:4 * k + 4] for k in range(3)])
    live, target = R.pairs(np.repeat(np.arange(3), 2), np.arange(3))
    non, tar = R.split(R.scores(tests, models), live, target)
    assert (non.size, tar.size) == (12, 6)
    _check_against_oracle(V.evaluate(net, corpus, enroll=2, p_target=0.05), non, tar, 0.05)
    with pytest.raises(ValueError, match="no test utterance"):
        V.evaluate(net, corpus, enroll=4)
    # test(protocol="corpus") loads the checkpoint and returns evaluate's EER
    ckpt = str(tmp_path / "toy.pth")
    torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, ckpt)
    ds = data_load.SpeakerDatasetResident(corpus, utter_num=4)
    old_device = hp.device
    try:
        hp.device = DEV
        with model_dims(*DIMS):
            capsys.readouterr()
            got = tse.test(ckpt, dataset=ds, protocol="corpus")
            out = capsys.readouterr().out
            with pytest.raises(ValueError, match="resident"):
                tse.test(ckpt, dataset=[], protocol="corpus")
    finally:
        hp.device = old_device
    assert got == r["eer"] and out.count("\n") == 2 and "corpus EER" in out


def test_train_evaluates_after_each_checkpoint(tmp_path, capsys):
    """train(eval_corpus=...): one extra line per checkpoint on stdout and in the log file, with
    evaluate's figures for the weights just saved; the training itself -- every other log line, the
    saved model -- is what it is without the evaluation."""
    import os
    import random

    from conftest import golden
    from pytorch_speaker_verification_amd import data_load
    from pytorch_speaker_verification_amd import train_speech_embedder as tse
    from pytorch_speaker_verification_amd.hparam import hparam as hp
    from pytorch_speaker_verification_amd.speech_embedder_net import SpeechEmbedder
    V = _V()
    g = golden("eer.npz")
    d = tmp_path / "train"
    recipe.make_speaker_dir(str(d), 12, 5)
    saved = {k: dict(v) for k, v in hp.items() if isinstance(v, dict)}
    saved_top = {k: v for k, v in hp.items() if not isinstance(v, dict)}

    def run(tag, **kw):
        hp.train.checkpoint_dir = str(tmp_path / tag)
        hp.train.log_file = str(tmp_path / tag / "Stats")
        random.seed(3)
        np.random.seed(3)
        torch.manual_seed(3)
        corpus = data_load.DeviceCorpus(str(d), device=DEV)
        capsys.readouterr()
        path = tse.train(str(tmp_path / "none.model"), dataset=data_load.SpeakerDatasetResident(corpus),
                         **({"eval_corpus": corpus} if kw.get("evaluate") else {}))
        return path, open(hp.train.log_file).read().splitlines(), capsys.readouterr().out, corpus

    try:
        hp.device = "cuda"
        hp.data.nmels, hp.model.hidden, hp.model.num_layer, hp.model.proj = [int(v) for v in g["dims"]]
        hp.training = True
        hp.data.train_path = str(d)
        hp.train.N, hp.train.M, hp.train.num_workers, hp.train.epochs = 4, 5, 0, 2
        hp.train.log_interval, hp.train.checkpoint_interval = 1, 2
        hp.train.restore = False
        plain_path, plain_lines, _, _ = run("plain")
        path, lines, out, corpus = run("eval", evaluate=True)
        net = SpeechEmbedder()
        net.load_state_dict(torch.load(os.path.join(hp.train.checkpoint_dir, "ckpt_epoch_2_batch_id_3.pth"),
                                       weights_only=True))
        r = V.evaluate(net.to(DEV).eval(), corpus)
    finally:
        for k, v in saved.items():
            hp[k].update(v)
        for k, v in saved_top.items():
            hp[k] = v
    extra = [ln for ln in lines if "corpus EER" in ln]
    rest = [ln for ln in lines if "corpus EER" not in ln]
    assert len(extra) == 1 and len(rest) == len(plain_lines) == 6
    assert [ln.split("\t", 1)[1] for ln in rest] == [ln.split("\t", 1)[1] for ln in plain_lines]
    assert lines.index(extra[0]) == 6  # after the checkpoint of epoch 2
    assert extra[0].startswith("Epoch:2\tcorpus EER:{0:.4f} [".format(r["eer"])) and extra[0] in out
    assert "minDCF:{0:.4f}".format(r["min_dcf"]) in extra[0]
    assert "trials:{0}+{1}".format(r["n_target"], r["n_nontarget"]) in extra[0]
    a, b = torch.load(plain_path, weights_only=True), torch.load(path, weights_only=True)
    assert all(torch.equal(a[k], b[k]) for k in a)
