"""Drop-in data loading (reference data_load.py:19-85).

``SpeakerDatasetTIMITPreprocessed`` serves [M, 160, nmels] float32 utterance stacks from the
offline-preprocessed ``speakerK.npy`` files ([utterances, nmels, 180], data_preprocess.py:46-54)
with the reference's sampling semantics and RNG consumption (so a seeded run draws the same
batches): with shuffle, a speaker chosen by ``random.sample`` independently of ``idx``
(data_load.py:70-71) and M utterances drawn WITH replacement by ``np.random.randint`` (:77);
without shuffle, file ``idx`` of ``os.listdir`` order and utterances [utter_start, +M) (:73,79).
Frames are truncated to 160 (:82) and transposed to [M, frames, mels] (:84).

``SpeakerDatasetWaveforms`` is the raw-waveform dataset (``SpeakerDatasetTIMIT``, data_load.py:19-46)
on decoded audio: the reference's sampling and RNG consumption, and ``features.mel_db_fixed`` (trim,
fix_length, mel magnitude in dB, on the GPU) in place of ``utils.mfccs_and_spec(f, wav_process=True)``.

``DevicePrefetcher`` overlaps the pinned host->device copy of batch k+1 with step k on a side
HIP stream; a batch that is already on the device passes through.  ``SpeakerDatasetTIMIT`` itself
(wav files, librosa) stays out of scope here: there is no audio decoder.

``DeviceCorpus`` keeps the whole preprocessed corpus on the device (28.8 KB per utterance of
[40, 180] fp32); ``SpeakerDatasetResident`` samples it as ``SpeakerDatasetTIMITPreprocessed`` samples
the files but yields utterance ids, and ``ResidentBatches`` turns them into ``CorpusBatch`` objects --
two int32 tables per step, the frame count T drawn per batch (``batch_lengths``: the paper's
[140, 180] on the GEMMs' fast grid) -- from which the forward cuts its operands in one launch.
"""
from __future__ import annotations

import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from . import features
from .hparam import hparam as hp

TRAIN_FRAMES = 160  # data_load.py:82 ("TODO implement variable length batch size")


class SpeakerDatasetTIMITPreprocessed(Dataset):
    def __init__(self, shuffle=True, utter_start=0):
        split = hp.train if hp.training else hp.test
        self.path = hp.data.train_path if hp.training else hp.data.test_path
        self.utter_num = split.M
        self.file_list = os.listdir(self.path)
        self.shuffle = shuffle
        self.utter_start = utter_start

    def __len__(self):
        return len(self.file_list)

    def _speaker_file(self, idx):
        names = os.listdir(self.path)  # re-listed per item, as the reference does (:68)
        return random.sample(names, 1)[0] if self.shuffle else names[idx]

    def _utterances(self, utters):
        if self.shuffle:
            return utters[np.random.randint(0, utters.shape[0], self.utter_num)]
        return utters[self.utter_start:self.utter_start + self.utter_num]

    def __getitem__(self, idx):
        utters = np.load(os.path.join(self.path, self._speaker_file(idx)))
        picked = self._utterances(utters)[:, :, :TRAIN_FRAMES]
        return torch.tensor(np.ascontiguousarray(picked.transpose(0, 2, 1)))


class SpeakerDatasetTIMIT(Dataset):
    """Raw-wav dataset (data_load.py:19-46): needs librosa STFT/mel features (utils.py:138-164),
    which are offline DSP outside the GPU training path."""

    def __init__(self):
        raise NotImplementedError("raw-wav featurisation (librosa) is out of scope: run the reference's "
                                  "data_preprocess.py once and set data.data_preprocessed: true, or decode the "
                                  "audio yourself and use SpeakerDatasetWaveforms")


class SpeakerDatasetWaveforms(Dataset):
    """SpeakerDatasetTIMIT (data_load.py:19-46) on decoded audio.  `speakers` is a sequence of lists
    of mono fp32 waveforms (1-D arrays or tensors, host or device) at hp.data.sr, one list per
    speaker; utterance_number defaults to hp.train.M or hp.test.M by hp.training (:23-28).  The
    speaker order is shuffled once (:30); item idx shuffles that speaker's utterance order and takes
    the first utterance_number (:39-40) -- the reference's draws from `random`, so a seeded run
    picks what the reference picks -- and returns features.mel_db_fixed of them, a cuda float32
    tensor [M, T, nmels] (:42-46, utils.mfccs_and_spec(f, wav_process=True)[1] per utterance).

    Items live on the GPU: use it with num_workers=0 and without pin_memory (train / test of
    train_speech_embedder do, for a dataset with on_device set).  Audio decoding and resampling are
    the caller's."""

    on_device = True

    def __init__(self, speakers, utterance_number=None):
        if utterance_number is None:
            utterance_number = hp.train.M if hp.training else hp.test.M
        self.utterance_number = utterance_number
        self.speakers = [list(utterances) for utterances in speakers]
        random.shuffle(self.speakers)

    def __len__(self):
        return len(self.speakers)

    def __getitem__(self, idx):
        utterances = list(self.speakers[idx])  # (the reference globs a fresh list per item, :38)
        random.shuffle(utterances)
        return features.mel_db_fixed(utterances[0:self.utterance_number])


class DevicePrefetcher:
    """Iterates a DataLoader yielding device tensors; the copy of the next batch (pinned host
    memory, non_blocking) runs on a side stream while the caller works on the current one."""

    def __init__(self, loader, device, on_fetch=None):
        self.loader, self.device = loader, torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.on_fetch = on_fetch  # called right after each host batch is drawn (RNG-order hook)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        it = iter(self.loader)
        nxt = self._fetch(it)
        while nxt is not None:
            cur, ev = nxt
            torch.cuda.current_stream(self.device).wait_event(ev)
            cur.record_stream(torch.cuda.current_stream(self.device))
            nxt = self._fetch(it)
            yield cur

    def _fetch(self, it):
        try:
            host = next(it)
        except StopIteration:
            return None
        if self.on_fetch is not None:
            self.on_fetch()
        if host.is_cuda:  # made on the device (SpeakerDatasetWaveforms): ordered behind its producer
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(host.device))
            return host, ev
        if not host.is_pinned():
            host = host.pin_memory()
        with torch.cuda.stream(self.stream):
            dev = host.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return dev, ev


# ----------------------------------------------------------------------------- resident corpus
def batch_lengths(B, lo=140, hi=180):
    """The frame counts T in [lo, hi] (the GE2E paper's TI-SV range, arXiv 1710.10467 §3.2) with
    T * B % 256 == 0 for a batch of B rows: off that grid the input-projection, dx and dW GEMMs
    (M or K = T * B) leave the 256-wide tiles for the fallback ones -- correct, but slower.
    ValueError if no T qualifies."""
    out = [T for T in range(lo, hi + 1) if (T * B) % 256 == 0]
    if not out:
        raise ValueError(f"no T in [{lo}, {hi}] has T * {B} % 256 == 0")
    return out


class DeviceCorpus:
    """Every utterance of a preprocessed corpus in one tensor on the device.

    source: a directory of ``speakerK.npy`` files ([utterances, nmels, frames] float32,
    data_preprocess.py:46-54), read in ``os.listdir`` order (the reference's speaker order), or a
    sequence of such arrays / tensors, one per speaker (``features.preprocess_speaker`` outputs).
    device: None = hp.device.

      data         [U, nmels, frames] float32, all speakers' utterances, one allocation
      speaker_off  host int64 [S + 1]: speaker k owns utterances speaker_off[k] : speaker_off[k + 1]
      names        the speakers' names (file names, or "speaker<k>" for a sequence)

    ValueError if the speakers disagree on nmels or frames."""

    def __init__(self, source, device=None):
        device = torch.device(hp.device if device is None else device)
        if isinstance(source, (str, os.PathLike)):
            self.names = os.listdir(source)
            parts = [np.load(os.path.join(source, n), mmap_mode="r") for n in self.names]
        else:
            parts = list(source)
            self.names = [f"speaker{k}" for k in range(len(parts))]
        if not parts:
            raise ValueError("DeviceCorpus: no speakers")
        for n, p in zip(self.names, parts):
            if p.ndim != 3 or p.shape[0] < 1:
                raise ValueError(f"DeviceCorpus: {n} is not [utterances >= 1, nmels, frames] (shape {tuple(p.shape)})")
            if tuple(p.shape[1:]) != tuple(parts[0].shape[1:]):
                raise ValueError(f"DeviceCorpus: {n} has (nmels, frames) = {tuple(p.shape[1:])}, "
                                 f"{self.names[0]} has {tuple(parts[0].shape[1:])}")
        self.speaker_off = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
        self.data = torch.empty((int(self.speaker_off[-1]),) + tuple(parts[0].shape[1:]), dtype=torch.float32,
                                device=device)
        for k, p in enumerate(parts):  # speaker by speaker: never a second host copy of the corpus
            src = p if torch.is_tensor(p) else torch.from_numpy(np.array(p, dtype=np.float32))  # (a file: mapped)
            self.data[int(self.speaker_off[k]):int(self.speaker_off[k + 1])].copy_(src)

    n_utt = property(lambda self: self.data.shape[0])
    nmels = property(lambda self: self.data.shape[1])
    n_frames = property(lambda self: self.data.shape[2])

    def frames(self, utt, start, T):
        """[B, T, nmels]: utterance utt[b], frames start[b] : start[b] + T, by plain torch indexing on
        the device ``data`` lives on (the CPU included).  ValueError for an index outside the corpus."""
        utt = torch.as_tensor(utt, dtype=torch.int64).reshape(-1).to(self.data.device)
        start = torch.as_tensor(start, dtype=torch.int64).reshape(-1).to(self.data.device)
        if utt.shape != start.shape:
            raise ValueError("DeviceCorpus.frames: utt and start differ in length")
        if not 1 <= T <= self.n_frames:
            raise ValueError(f"DeviceCorpus.frames: T = {T} outside [1, {self.n_frames}]")
        if utt.numel() and (int(utt.min()) < 0 or int(utt.max()) >= self.n_utt or int(start.min()) < 0
                            or int(start.max()) > self.n_frames - T):
            raise ValueError("DeviceCorpus.frames: an utterance or a start outside the corpus")
        t = start[:, None] + torch.arange(T, device=self.data.device)[None, :]
        return self.data[utt[:, None], :, t].contiguous()  # [B, T, nmels]


class CorpusBatch:
    """A training batch that is still in the corpus: row b is utterance utt[b], frames start[b] :
    start[b] + T (utt, start int32 [B] on the corpus' device).  ops.embedder_forward(_bf16) and
    GE2ETrainer.step take it in place of x [B, T, nmels] and cut the LSTM's operands straight out of
    ``corpus.data`` (sv_corpus_batch); ``frames()`` materialises that x."""

    def __init__(self, corpus, utt, start, T):
        self.corpus, self.utt, self.start, self.T = corpus, utt, start, int(T)

    shape = property(lambda self: (self.utt.shape[0], self.T, self.corpus.nmels))
    device = property(lambda self: self.corpus.data.device)

    def frames(self):
        return self.corpus.frames(self.utt, self.start, self.T)

    def rows(self, r0, r1):
        """Rows r0 : r1 as a batch of their own (views of the tables)."""
        return CorpusBatch(self.corpus, self.utt[r0:r1], self.start[r0:r1], self.T)


class SpeakerDatasetResident(Dataset):
    """SpeakerDatasetTIMITPreprocessed on a DeviceCorpus: the same sampling and the same draws from
    ``random`` and ``np.random`` (one ``random.sample`` over the speaker names, then
    ``np.random.randint(0, U_k, M)``; without shuffle speaker ``idx`` and utterances
    [utter_start, +M)), but an item is the M global utterance ids, int64 [M] -- the frames stay on
    the device.  utter_num: None = hp.train.M or hp.test.M by hp.training."""

    resident = True

    def __init__(self, corpus, shuffle=True, utter_start=0, utter_num=None):
        if utter_num is None:
            utter_num = hp.train.M if hp.training else hp.test.M
        self.corpus, self.shuffle, self.utter_start, self.utter_num = corpus, shuffle, utter_start, utter_num

    def __len__(self):
        return len(self.corpus.names)

    def __getitem__(self, idx):
        names = self.corpus.names
        k = names.index(random.sample(names, 1)[0]) if self.shuffle else idx
        lo, hi = int(self.corpus.speaker_off[k]), int(self.corpus.speaker_off[k + 1])
        if self.shuffle:
            ids = lo + np.random.randint(0, hi - lo, self.utter_num)
        else:
            ids = np.arange(lo, hi)[self.utter_start:self.utter_start + self.utter_num]
        return torch.as_tensor(ids, dtype=torch.int64)


class ResidentBatches:
    """DevicePrefetcher's place for a resident dataset: iterates a DataLoader of utterance ids
    [N, M] and yields CorpusBatch objects.  Per batch it draws one length T from ``lengths`` (None:
    always TRAIN_FRAMES) and the rows' first frames -- crop "head": 0, the reference's batches;
    "random": uniform in [0, frames - T] per row, the paper's -- from a private
    ``random.Random(seed)``, so the global RNG streams see what the host loader's run sees.  The
    two tables travel as one pinned int32 [2, B] block, copied non-blocking on this object's own
    stream ahead of use, with an event the consuming stream waits on: the only host-to-device
    traffic of a step.  (A corpus on the CPU is served without streams: the tests' reference.)"""

    def __init__(self, loader, corpus, lengths=None, crop="head", seed=0, on_fetch=None):
        if crop not in ("head", "random"):
            raise ValueError(f"unknown crop {crop!r} (expected 'head' or 'random')")
        self.lengths = [TRAIN_FRAMES] if lengths is None else [int(T) for T in lengths]
        if not self.lengths or min(self.lengths) < 1 or max(self.lengths) > corpus.n_frames:
            raise ValueError(f"lengths {self.lengths} outside [1, {corpus.n_frames}], the corpus' frame count")
        self.loader, self.corpus, self.crop, self.on_fetch = loader, corpus, crop, on_fetch
        self.rng = random.Random(seed)
        self.device = corpus.data.device
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        it = iter(self.loader)
        nxt = self._fetch(it)
        while nxt is not None:
            cur, ev = nxt
            if ev is not None:
                main = torch.cuda.current_stream(self.device)
                main.wait_event(ev)
                cur.utt.record_stream(main)  # (utt and start are views of one block)
            nxt = self._fetch(it)
            yield cur

    def _fetch(self, it):
        try:
            ids = next(it)
        except StopIteration:
            return None
        if self.on_fetch is not None:
            self.on_fetch()
        B = ids.numel()
        T = self.rng.choice(self.lengths) if len(self.lengths) > 1 else self.lengths[0]
        table = torch.empty((2, B), dtype=torch.int32, pin_memory=self.stream is not None)
        table[0] = ids.reshape(-1)
        if self.crop == "head":
            table[1] = 0
        else:
            table[1] = torch.tensor([self.rng.randint(0, self.corpus.n_frames - T) for _ in range(B)], dtype=torch.int32)
        if self.stream is None:
            return CorpusBatch(self.corpus, table[0], table[1], T), None
        with torch.cuda.stream(self.stream):
            dev = table.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return CorpusBatch(self.corpus, dev[0], dev[1], T), ev
