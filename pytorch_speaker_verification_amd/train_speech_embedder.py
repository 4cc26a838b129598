"""Drop-in training / EER-evaluation driver (reference train_speech_embedder.py:19-160).

``train(model_path)``
    The reference loop (:19-90): preprocessed dataset -> DataLoader(N speakers, drop_last) ->
    per batch one GE2E step -> periodic log line and checkpoints.  The step body (:44-65) runs
    as ``GE2ETrainer.step`` (HIP kernels, no autograd graph, no host sync); the log line keeps
    the reference's format; checkpoints keep its file names and state_dict keys.  Batches are
    copied host->device on a side stream ahead of use (DevicePrefetcher).  The reference's
    per-batch row permutation (:48-57) is value-neutral (rows are independent; tested bitwise),
    so only its ``random.sample`` draw is kept, which keeps seeded runs on the reference's
    data order.
``test(model_path)``
    EER evaluation (:92-154) on the GPU: enrollment / verification halves, verification
    centroids from get_centroids, get_cossim(verification, enrollment centroids), the 50-point
    threshold sweep on device (exact integer counts, sv_eer_counts) and the reference's float32
    FAR/FRR/EER selection.  Returns the average EER (the reference only prints it).

``train`` takes ``loss_method="softmax"``: ``"contrast"`` trains with the GE2E paper's contrast loss
(eq. 7), which the reference does not implement, through the same step (GE2ELoss.loss_method).

Both take ``dataset=None``: a given dataset replaces the configured one -- the way to train or
evaluate the reference's raw-waveform configuration (``data_preprocessed: false``) on decoded audio,
with ``data_load.SpeakerDatasetWaveforms``, whose batches are made on the GPU and skip the pinned copy.

A ``data_load.SpeakerDatasetResident`` (the preprocessed corpus kept on the device) is served by
``data_load.ResidentBatches``: per step two int32 tables go to the device and the forward cuts its
operands out of the corpus -- with the default arguments the host loader's batches, bit for bit and in
its order.  ``train`` then also takes ``lengths`` (the frame counts T to draw from, one per batch;
None = 160 always; ``data_load.batch_lengths`` gives the paper's [140, 180] on the GEMMs' fast grid),
``crop`` ("head" | "random") and ``seed`` (of the private RNG both are drawn from).

``test(..., protocol="corpus")`` (a resident dataset) runs ``verification.evaluate`` on the dataset's
whole corpus instead -- every pair of utterances, one EER -- prints one line and returns that EER;
``train(..., eval_corpus=corpus)`` runs it on ``corpus`` after every checkpoint and adds one line to
stdout and the log file.  The default protocol and the existing log line are unchanged.

``test(..., protocol="corpus", cohort=c, top_k=k)`` and ``train(..., eval_corpus=corpus, eval_cohort=c,
eval_top_k=k)`` hand a cohort to ``evaluate``: the figures are then those of the AS-normalised scores
(adaptive symmetric score normalisation, verification.py), and the line says so.  The cohort -- a
DeviceCorpus or a tensor of unit speaker models -- must not contain the evaluated speakers.
"""
from __future__ import annotations

import os
import random
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

from ._lib import call, ptr, stream_of
from .data_load import (TRAIN_FRAMES, DevicePrefetcher, ResidentBatches, SpeakerDatasetTIMIT,
                        SpeakerDatasetTIMITPreprocessed)
from .hparam import hparam as hp
from .speech_embedder_net import GE2ELoss, SpeechEmbedder
from .trainer import GE2ETrainer
from .utils import get_centroids, get_cossim

EER_THRESHOLDS = [0.01 * i + 0.5 for i in range(50)]  # :134


def _dataset():
    return SpeakerDatasetTIMITPreprocessed() if hp.data.data_preprocessed else SpeakerDatasetTIMIT()


def _value_neutral_perm(n):
    """The reference's random.sample permutation (:48-52 / :114-119): drawn for RNG parity."""
    return random.sample(range(0, n), n)


def _loader(dataset, split, pin_memory):
    """The reference's DataLoader (:26-27 / :97); a dataset whose items are already on the device
    (on_device) is read in this process and not pinned, and so are a resident dataset's items (utterance
    ids: its draws from the global RNG streams stay in this process)."""
    on_device = getattr(dataset, "on_device", False) or getattr(dataset, "resident", False)
    return DataLoader(dataset, batch_size=split.N, shuffle=True, num_workers=0 if on_device else split.num_workers,
                      drop_last=True, pin_memory=pin_memory and not on_device)


def train(model_path, dataset=None, loss_method="softmax", lengths=None, crop="head", seed=0, eval_corpus=None,
          eval_cohort=None, eval_top_k=300):
    if eval_cohort is not None and eval_corpus is None:
        raise ValueError("train: eval_cohort needs eval_corpus")
    device = torch.device(hp.device)
    train_dataset = _dataset() if dataset is None else dataset
    loader = _loader(train_dataset, hp.train, True)
    resident = getattr(train_dataset, "resident", False)
    if not resident and (lengths is not None or crop != "head"):
        raise ValueError("train: lengths and crop need a resident dataset (data_load.SpeakerDatasetResident)")
    embedder_net = SpeechEmbedder().to(device)
    if hp.train.restore:
        embedder_net.load_state_dict(torch.load(model_path, weights_only=True))
    ge2e_loss = GE2ELoss(device, loss_method=loss_method)
    trainer = GE2ETrainer(embedder_net, ge2e_loss, lr=hp.train.lr)
    os.makedirs(hp.train.checkpoint_dir, exist_ok=True)
    N, M = hp.train.N, hp.train.M
    embedder_net.train()
    iteration = 0
    e = batch_id = 0
    on_fetch = lambda: _value_neutral_perm(N * M)  # noqa: E731
    if resident:  # one object for all epochs: its private RNG runs on
        batches = ResidentBatches(loader, train_dataset.corpus, lengths, crop, seed, on_fetch=on_fetch)
    for e in range(hp.train.epochs):
        total_loss = torch.zeros((), device=device)
        if not resident:
            batches = DevicePrefetcher(loader, device, on_fetch=on_fetch)
        for batch_id, mel_db_batch in enumerate(batches):
            # (a resident batch is N * M rows already)
            x = mel_db_batch if resident else mel_db_batch.reshape(N * M, mel_db_batch.size(2), mel_db_batch.size(3))
            loss = trainer.step(x, N, M)
            total_loss = total_loss + loss
            iteration += 1
            if (batch_id + 1) % hp.train.log_interval == 0:
                mesg = "{0}\tEpoch:{1}[{2}/{3}],Iteration:{4}\tLoss:{5:.4f}\tTLoss:{6:.4f}\t\n".format(
                    time.ctime(), e + 1, batch_id + 1, len(train_dataset) // N, iteration, float(loss),
                    float(total_loss) / (batch_id + 1))
                print(mesg)
                if hp.train.log_file is not None:
                    with open(hp.train.log_file, "a") as f:
                        f.write(mesg)
        if hp.train.checkpoint_dir is not None and (e + 1) % hp.train.checkpoint_interval == 0:
            ckpt = os.path.join(hp.train.checkpoint_dir, f"ckpt_epoch_{e + 1}_batch_id_{batch_id + 1}.pth")
            torch.save({k: v.detach().cpu() for k, v in embedder_net.state_dict().items()}, ckpt)
            if eval_corpus is not None:
                mesg = _corpus_line(embedder_net, eval_corpus, "Epoch:{0}\t".format(e + 1), eval_cohort, eval_top_k)
                print(mesg)
                if hp.train.log_file is not None:
                    with open(hp.train.log_file, "a") as f:
                        f.write(mesg)
    save_path = os.path.join(hp.train.checkpoint_dir, f"final_epoch_{e + 1}_batch_id_{batch_id + 1}.model")
    torch.save({k: v.detach().cpu() for k, v in embedder_net.state_dict().items()}, save_path)
    print("\nDone, trained model saved at", save_path)
    return save_path


def eer_from_sim(sim):
    """(EER, threshold, FAR, FRR) of one batch: counts on device, the reference's float32
    selection on the host (train_speech_embedder.py:134-149)."""
    N, M2, Nc = sim.shape
    thr = torch.tensor(EER_THRESHOLDS, dtype=torch.float32, device=sim.device)
    cnt = torch.empty((2, len(EER_THRESHOLDS)), dtype=torch.float32, device=sim.device)
    call("sv_eer_counts", ptr(sim), N, M2, Nc, ptr(thr), len(EER_THRESHOLDS), ptr(cnt[0]), ptr(cnt[1]),
         stream_of(sim))
    n_all, n_diag = cnt.cpu().numpy()
    f32 = np.float32
    diff, best = f32(1.0), (f32(0), 0.0, f32(0), f32(0))
    for i, t in enumerate(EER_THRESHOLDS):
        far = f32(f32(f32(f32(n_all[i] - n_diag[i]) / f32(N - 1.0)) / f32(M2)) / f32(N))
        frr = f32(f32(f32(f32(M2 * N) - n_diag[i]) / f32(M2)) / f32(N))
        d = f32(abs(f32(far - frr)))
        if diff > d:
            diff = d
            best = (f32(f32(far + frr) / f32(2.0)), t, far, frr)
    return best


def _as_norm_note(r):
    return "AS-norm top {0} of {1}".format(r["top_k"], r["n_cohort"]) if "score_norm" in r else ""


def _corpus_line(embedder_net, corpus, prefix="", cohort=None, top_k=300):
    """One line with verification.evaluate's figures on `corpus` (all pairs of its utterances; with a
    cohort those of the AS-normalised scores, and one more field that says so)."""
    from .verification import evaluate
    with torch.no_grad():
        r = evaluate(embedder_net, corpus, cohort=cohort, top_k=top_k)
    return "{0}corpus EER:{1:.4f} [{2:.4f}, {3:.4f}]\tthres:{4:.4f}\tminDCF:{5:.4f}\ttrials:{6}+{7}\t{8}\n".format(
        prefix, r["eer"], r["eer_lo"], r["eer_hi"], r["threshold"], r["min_dcf"], r["n_target"], r["n_nontarget"],
        _as_norm_note(r) + "\t" if cohort is not None else "")


def test(model_path, dataset=None, protocol="batches", cohort=None, top_k=300):
    if protocol not in ("batches", "corpus"):
        raise ValueError(f"unknown protocol {protocol!r} (expected 'batches' or 'corpus')")
    if cohort is not None and protocol != "corpus":
        raise ValueError("test: a cohort (AS-norm) needs protocol='corpus'")
    device = torch.device(hp.device)
    test_dataset = _dataset() if dataset is None else dataset
    if protocol == "corpus":
        if not getattr(test_dataset, "resident", False):
            raise ValueError("test: protocol='corpus' needs a resident dataset (data_load.SpeakerDatasetResident)")
        from .verification import evaluate
        embedder_net = SpeechEmbedder()
        embedder_net.load_state_dict(torch.load(model_path, weights_only=True))
        embedder_net = embedder_net.to(device).eval()
        with torch.no_grad():
            r = evaluate(embedder_net, test_dataset.corpus, cohort=cohort, top_k=top_k)
        print("\ncorpus EER : {0:.4f} in [{1:.4f}, {2:.4f}] (thres:{3:.4f}, minDCF:{4:.4f}, {5} target and {6} "
              "non-target trials{7})".format(r["eer"], r["eer_lo"], r["eer_hi"], r["threshold"], r["min_dcf"],
                                             r["n_target"], r["n_nontarget"],
                                             ", " + _as_norm_note(r) if cohort is not None else ""))
        return float(r["eer"])
    loader = _loader(test_dataset, hp.test, False)
    embedder_net = SpeechEmbedder()
    embedder_net.load_state_dict(torch.load(model_path, weights_only=True))
    embedder_net = embedder_net.to(device).eval()
    N, M = hp.test.N, hp.test.M
    assert M % 2 == 0
    avg_EER = np.float32(0.0)
    with torch.no_grad():
        for e in range(hp.test.epochs):
            batch_avg_EER = np.float32(0.0)
            batch_id = 0
            for batch_id, mel_db_batch in enumerate(loader):
                if getattr(test_dataset, "resident", False):  # utterance ids [N, M] -> their first 160 frames
                    ids = mel_db_batch.reshape(-1)
                    mel_db_batch = test_dataset.corpus.frames(ids, torch.zeros_like(ids), TRAIN_FRAMES).reshape(
                        N, M, TRAIN_FRAMES, -1)
                mel = mel_db_batch.to(device)
                enroll, verif = torch.split(mel, M // 2, dim=1)
                enroll = enroll.reshape(N * M // 2, enroll.size(2), enroll.size(3))
                verif = verif.reshape(N * M // 2, verif.size(2), verif.size(3))
                _value_neutral_perm(verif.size(0))
                e_emb = embedder_net(enroll).reshape(N, M // 2, -1)
                v_emb = embedder_net(verif).reshape(N, M // 2, -1)
                sim = get_cossim(v_emb, get_centroids(e_emb))
                EER, thr, FAR, FRR = eer_from_sim(sim)
                batch_avg_EER = np.float32(batch_avg_EER + EER)
                print("\nEER : %0.2f (thres:%0.2f, FAR:%0.2f, FRR:%0.2f)" % (EER, thr, FAR, FRR))
            avg_EER = np.float32(avg_EER + np.float32(batch_avg_EER / (batch_id + 1)))
    avg_EER = np.float32(avg_EER / hp.test.epochs)
    print("\n EER across {0} epochs: {1:.4f}".format(hp.test.epochs, avg_EER))
    return float(avg_EER)


if __name__ == "__main__":
    if hp.training:
        train(hp.model.model_path)
    else:
        test(hp.model.model_path)
