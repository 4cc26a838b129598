"""Corpus-scale speaker verification: one EER and one minDCF over a whole held-out set.

``train_speech_embedder.test`` repeats the reference's toy protocol (batches of 4 speakers, a
50-point threshold grid, leave-one-out centroids).  This module scores every utterance of a corpus
against every other one, or against every enrolled speaker model, and derives the ROC from the two
score distributions -- the scores themselves are never kept: ``sv_trial_hist`` (csrc/sv_trials.hip)
bins every fp32 dot product in the epilogue of the scoring GEMM into a target and a non-target
histogram (U utterances give U^2 / 2 trials; at U = 100 000 the score matrix would be 20 GB).

  trial_histograms   the kernel: two histograms of all pairs of rows of one or two matrices
  cohort_stats       mean and std of every row's top-K scores against a cohort (sv_cohort_topk_stats)
  cohort_models, as_norm, norm_range
                     adaptive score normalisation (AS-norm): the usual cohort, a trial side's (mu, 1 / sigma),
                     and the range of the normalised score that the first histogram pass covers
  roc, eer, min_dcf  FAR / FRR at the bin edges, the equal error rate with an interval that
                     contains the sorted-scores EER, the normalised minimum detection cost
  corpus_eer         histogram passes that zoom into the FAR / FRR crossing
  corpus_dvectors    unit d-vectors of every utterance of a data_load.DeviceCorpus
  utterance_dvectors the GE2E paper's sliding-window inference for ragged log-mel frames
  evaluate           d-vectors -> trials -> {eer, threshold, eer_lo, eer_hi, min_dcf, ...}

Scores are cosines only if the rows are unit vectors: the kernel takes rows as they are, and
corpus_dvectors / utterance_dvectors / evaluate produce unit rows.  There is no CPU path for the
histograms; the ROC arithmetic on a TrialHist is plain numpy on the host.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import call, lib, ptr, stream_of
from .data_load import TRAIN_FRAMES, CorpusBatch

MAX_BINS, MAX_D = 8192, 1024  # include/sv_ge2e.h: sv_trial_hist's SV_ESHAPE limits
MAX_COHORT = 65535             # sv_cohort_topk_stats' (16-bit bin counters)


class TrialHist:
    """Two score histograms: ``counts`` int64 [2, bins + 2], row 0 non-targets, row 1 targets; slot 0
    holds the scores below ``lo`` (and NaN), slots 1 .. bins the ``bins`` equal bins of [lo, hi), slot
    bins + 1 the scores at or above ``hi``.  ``lo`` and ``hi`` are the fp32 values the kernel saw."""

    def __init__(self, counts, lo, hi, bins):
        counts = np.asarray(counts, dtype=np.int64)
        if counts.shape != (2, int(bins) + 2):
            raise ValueError(f"TrialHist: counts {counts.shape} is not [2, bins + 2] with bins = {bins}")
        self.counts, self.lo, self.hi, self.bins = counts, float(lo), float(hi), int(bins)

    n_nontarget = property(lambda self: int(self.counts[0].sum()))
    n_target = property(lambda self: int(self.counts[1].sum()))
    width = property(lambda self: (self.hi - self.lo) / self.bins)

    def edges(self):
        """The bins + 1 bin edges, float64."""
        return self.lo + (self.hi - self.lo) * (np.arange(self.bins + 1, dtype=np.float64) / self.bins)


def bin_params(bins, lo, hi):
    """(lo, hi, inv_width) as the kernel gets them: lo and hi rounded to fp32, inv_width the fp32
    rounding of bins / (hi - lo) of those two, computed in fp64."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    if not (np.isfinite(lo32) and np.isfinite(hi32) and hi32 > lo32):
        raise ValueError(f"trial_histograms: need finite lo < hi in fp32 (got {lo}, {hi})")
    return lo32, hi32, np.float32(bins / (float(hi32) - float(lo32)))


def _rows(t, name):
    """A [N, D'] fp32 device view the kernel can read in place (unit column stride, row stride a
    multiple of 4, 16-byte aligned, D' = D rounded up to a multiple of 4), or such a copy: zero
    columns change no dot product."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"trial_histograms: {name} must be a device tensor (the trial kernels have no CPU path)")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"trial_histograms: {name} must be float32 [N >= 1, D >= 1] (got {t.dtype} {tuple(t.shape)})")
    N, D = t.shape
    if D > MAX_D:
        raise ValueError(f"trial_histograms: D = {D} above the kernel's limit {MAX_D}")
    ok = D % 4 == 0 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= D and t.data_ptr() % 16 == 0
    if not ok:
        pad = torch.zeros((N, (D + 3) // 4 * 4), dtype=torch.float32, device=t.device)
        pad[:, :D] = t
        t = pad
    return t


def _labels(lab, n, dev, name):
    if not torch.is_tensor(lab) or lab.dtype != torch.int32 or lab.device != dev or lab.shape != (n,):
        raise ValueError(f"trial_histograms: {name} must be an int32 [{n}] tensor on {dev}")
    return lab.contiguous()


def _norm(norm, n, dev, name):
    """(mu, inv) of one trial side as float32 [n] contiguous tensors on dev."""
    try:
        mu, inv = norm
    except (TypeError, ValueError):
        raise ValueError(f"trial_histograms: {name} must be a pair (mu, inv)") from None
    for t in (mu, inv):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != dev or t.shape != (n,):
            raise ValueError(f"trial_histograms: {name} must hold two float32 [{n}] tensors on {dev}")
    return mu.contiguous(), inv.contiguous()


def trial_histograms(a, lab_a, b=None, lab_b=None, bins=4096, lo=-1.0, hi=1.0, grid=0, norm_a=None, norm_b=None):
    """The histograms of s = a[i] . b[j] over all pairs (sv_trial_hist, include/sv_ge2e.h has the slot
    rule): a [Na, D], b [Nb, D] float32 device tensors -- rows may be strided views -- with int32 labels
    on the same device; a pair is a target when its labels are equal, and a row with a negative label
    takes part in no pair.  b=None is the symmetric mode: the pairs i < j of a alone.  grid: the
    number of workgroups, 0 = automatic (the counts do not depend on it).  Returns a TrialHist on
    the host.  Raises on CPU tensors: there is no CPU path.

    norm_a = (mu, inv), float32 [Na] each (and norm_b for b; in symmetric mode norm_a serves both
    sides): the histograms of z = 0.5 ((s - mu_a[i]) inv_a[i] + (s - mu_b[j]) inv_b[j]) instead
    (sv_trial_hist_norm; as_norm makes the pairs).  [lo, hi) is then a range of z: norm_range."""
    if (b is None) != (lab_b is None):
        raise ValueError("trial_histograms: give b and lab_b together, or neither (symmetric mode)")
    if b is None and norm_b is not None:
        raise ValueError("trial_histograms: the symmetric mode takes norm_a for both sides")
    if b is not None and (norm_a is None) != (norm_b is None):
        raise ValueError("trial_histograms: give norm_a and norm_b together, or neither")
    bins = int(bins)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"trial_histograms: bins = {bins} outside [1, {MAX_BINS}]")
    lo32, hi32, inv_width = bin_params(bins, lo, hi)
    a = _rows(a, "a")
    lab_a = _labels(lab_a, a.shape[0], a.device, "lab_a")
    symmetric = b is None
    if symmetric:
        b, lab_b = a, lab_a
    else:
        b = _rows(b, "b")
        if b.device != a.device or b.shape[1] != a.shape[1]:
            raise ValueError(f"trial_histograms: a {tuple(a.shape)} on {a.device} and b {tuple(b.shape)} on {b.device} "
                             "differ in D or device")
        lab_b = _labels(lab_b, b.shape[0], a.device, "lab_b")
    if norm_a is not None:
        norm_a = _norm(norm_a, a.shape[0], a.device, "norm_a")
        norm_b = norm_a if symmetric else _norm(norm_b, b.shape[0], a.device, "norm_b")
    with torch.cuda.device(a.device):
        hist = torch.zeros(int(lib().sv_trial_hist_size(bins)) // 8, dtype=torch.int64, device=a.device)
        if norm_a is None:
            call("sv_trial_hist", ptr(a), a.stride(0), ptr(lab_a), a.shape[0], ptr(b), b.stride(0), ptr(lab_b),
                 b.shape[0], a.shape[1], int(symmetric), float(lo32), float(inv_width), bins, ptr(hist), int(grid),
                 stream_of(a))
        else:
            call("sv_trial_hist_norm", ptr(a), a.stride(0), ptr(lab_a), a.shape[0], ptr(b), b.stride(0), ptr(lab_b),
                 b.shape[0], a.shape[1], int(symmetric), float(lo32), float(inv_width), bins, ptr(norm_a[0]),
                 ptr(norm_a[1]), ptr(norm_b[0]), ptr(norm_b[1]), ptr(hist), int(grid), stream_of(a))
    return TrialHist(hist[:2 * (bins + 2)].view(2, bins + 2).cpu().numpy(), lo32, hi32, bins)


# ----------------------------------------------------------------------------- AS-norm
def cohort_stats(x, cohort, top_k, grid=0):
    """(mean, std), float32 [N] on the device: for every row of x [N, D] the mean and the population
    standard deviation (divisor top_k) of the top_k largest of its scores x[i] . cohort[c] over the rows
    of cohort [Nc, D] (sv_cohort_topk_stats: an exact radix select inside the scoring GEMM, no score
    written).  Operands as trial_histograms' (float32 device tensors, rows may be strided views);
    Nc <= 65 535.  A row with a NaN score gets NaN.  grid: the number of workgroups, 0 = automatic
    (the results do not depend on it).  ValueError for top_k outside [1, Nc]."""
    x, cohort = _rows(x, "x"), _rows(cohort, "cohort")
    if cohort.device != x.device or cohort.shape[1] != x.shape[1]:
        raise ValueError(f"cohort_stats: x {tuple(x.shape)} on {x.device} and cohort {tuple(cohort.shape)} on "
                         f"{cohort.device} differ in D or device")
    n, nc, top_k = x.shape[0], cohort.shape[0], int(top_k)
    if nc > MAX_COHORT:
        raise ValueError(f"cohort_stats: {nc} cohort rows above the kernel's limit {MAX_COHORT}")
    if not 1 <= top_k <= nc:
        raise ValueError(f"cohort_stats: top_k = {top_k} outside [1, Nc = {nc}]")
    with torch.cuda.device(x.device):
        out = torch.empty((2, n), dtype=torch.float32, device=x.device)
        call("sv_cohort_topk_stats", ptr(x), x.stride(0), n, ptr(cohort), cohort.stride(0), nc, x.shape[1], top_k,
             ptr(out[0]), ptr(out[1]), int(grid), stream_of(x))
    return out[0], out[1]


def cohort_models(d, speaker_off):
    """The usual cohort, one row per speaker: the renormalised mean of each speaker's unit d-vectors
    (d [U, proj], speaker s owns rows speaker_off[s] : speaker_off[s + 1]; sv_dvec_align)."""
    from .ops import dvec_align
    off = torch.from_numpy(np.asarray(speaker_off, dtype=np.int32)).to(d.device)
    with torch.cuda.device(d.device):
        return _unit_rows(dvec_align(d.contiguous(), off))


def as_norm(x, cohort, top_k, std_floor=1e-5):
    """(mu, inv) of one trial side for trial_histograms' norm_a / norm_b: cohort_stats' mean, and
    inv = 1 / max(std, std_floor)."""
    mu, sd = cohort_stats(x, cohort, top_k)
    return mu, 1.0 / torch.clamp(sd, min=float(std_floor))


def norm_range(norm_a, norm_b=None, s_max=1.0):
    """(lo, hi): a range [lo, hi) that contains z = 0.5 ((s - mu_a[i]) inv_a[i] + (s - mu_b[j]) inv_b[j])
    for every pair (i, j) and every |s| <= s_max, given inv > 0 (norm_b=None: norm_a on both sides).  z
    rises with s, so each side's extremes are taken at s = -s_max and s = +s_max; the sum of the sides'
    extremes, in fp64, is widened by 2^-20 of its size for the kernel's five fp32 roundings (2^-22
    would do) and rounded outwards to fp32.  It is where the first histogram pass of normalised scores
    looks, as [-1, 1) is for cosines; typically tens of units wide."""
    lo = hi = 0.0
    for mu, inv in (norm_a, norm_a if norm_b is None else norm_b):
        mu, inv = mu.double(), inv.double()
        lo += 0.5 * float(((-s_max - mu) * inv).min())
        hi += 0.5 * float(((s_max - mu) * inv).max())
    pad = 2.0 ** -20 * max(abs(lo), abs(hi), 1.0)
    return (float(np.nextafter(np.float32(lo - pad), np.float32(-np.inf))),
            float(np.nextafter(np.float32(hi + pad), np.float32(np.inf))))


# ----------------------------------------------------------------------------- ROC arithmetic (host)
def _accepted(h):
    """(accepted non-targets, accepted targets) int64 [bins + 1] at every edge (score >= edge: the
    bins from that edge up plus the overflow slot), and the two class sizes.  ValueError for an
    empty class: its error rate is undefined."""
    n_non, n_tar = h.n_nontarget, h.n_target
    if n_non == 0 or n_tar == 0:
        raise ValueError(f"the trials hold {n_tar} target and {n_non} non-target pairs: FAR and FRR need both classes")
    acc = np.cumsum(h.counts[:, :0:-1], axis=1)[:, ::-1]  # [2, bins + 1]: slots k + 1 .. bins + 1
    return acc[0], acc[1], n_non, n_tar


def roc(h):
    """(edges, far, frr) float64 [bins + 1]: a trial is accepted when its score is >= the edge, so
    far[k] = #(non-targets >= edge k) / #non-targets and frr[k] = #(targets < edge k) / #targets; the
    underflow slot (NaN scores included) is rejected at every edge, the overflow slot accepted."""
    acc_non, acc_tar, n_non, n_tar = _accepted(h)
    return h.edges(), acc_non / float(n_non), (n_tar - acc_tar) / float(n_tar)


def _crossing(far, frr):
    """k in [-1, bins]: FAR >= FRR at edge k and FAR < FRR at edge k + 1, where edge -1 is -inf
    (FAR 1, FRR 0) and edge bins + 1 is +inf (FAR 0, FRR 1).  FAR - FRR never increases with the
    threshold, so k is unique."""
    return int(np.count_nonzero(far >= frr)) - 1


def eer(h):
    """(eer, threshold, far, frr, eer_lo, eer_hi).  The threshold is the first edge that minimises
    |FAR - FRR| (a later edge replaces the choice only if it is strictly better: the reference's
    sweep, train_speech_embedder.py:138), eer = (FAR + FRR) / 2 there.

    [eer_lo, eer_hi] contains the EER of the same scores computed from the sorted scores (thresholds
    at every distinct score and above the largest, any minimiser of |FAR - FRR|).  Derivation: with
    a trial accepted when score >= theta, FAR(theta) never increases and FRR(theta) never decreases,
    so g = FAR - FRR never increases.  Let e_k <= e_{k+1} be the neighbouring edges (with -inf and
    +inf as outermost edges) with g(e_k) >= 0 > g(e_{k+1}).  A theta < e_k has g(theta) >= g(e_k) >= 0;
    if it minimises |g| then g(theta) = g(e_k), and as FAR(theta) - FAR(e_k) >= 0 >= FRR(theta) -
    FRR(e_k) are then equal, both rates are those at e_k.  The same holds above e_{k+1}.  So every
    minimiser has the rates of some theta in [e_k, e_{k+1}], where FAR(e_{k+1}) <= FAR <= FAR(e_k)
    and FRR(e_k) <= FRR <= FRR(e_{k+1}):
        eer_lo = (FAR(e_{k+1}) + FRR(e_k)) / 2,   eer_hi = (FAR(e_k) + FRR(e_{k+1})) / 2.
    The slot rule is monotone in the score, so "slot > k" is "score >= theta_k" for some theta_k within
    rounding of edge k; the argument runs on those theta_k, whatever the rounding at an edge."""
    edges, far, frr = roc(h)
    diff = np.abs(far - frr)
    best = int(np.argmin(diff))  # (the first minimum)
    k = _crossing(far, frr)
    far_lo, frr_lo = (1.0, 0.0) if k < 0 else (far[k], frr[k])
    far_hi, frr_hi = (0.0, 1.0) if k >= h.bins else (far[k + 1], frr[k + 1])
    return (float((far[best] + frr[best]) / 2), float(edges[best]), float(far[best]), float(frr[best]),
            float((far_hi + frr_lo) / 2), float((far_lo + frr_hi) / 2))


def min_dcf(h, p_target=0.01, c_miss=1.0, c_fa=1.0):
    """The normalised minimum detection cost: min over the edges of
    (c_miss p_target FRR + c_fa (1 - p_target) FAR) / min(c_miss p_target, c_fa (1 - p_target))."""
    if not 0.0 < p_target < 1.0 or c_miss <= 0 or c_fa <= 0:
        raise ValueError("min_dcf: need 0 < p_target < 1 and positive costs")
    _, far, frr = roc(h)
    return float(np.min(c_miss * p_target * frr + c_fa * (1.0 - p_target) * far)
                 / min(c_miss * p_target, c_fa * (1.0 - p_target)))


def _zoom(h):
    """The next pass's (lo, hi): the two bins around the FAR / FRR crossing of h -- the bin that holds
    it and its lower neighbour (the upper one at the bottom of the range) -- or None when the crossing
    lies in the under- or overflow slot or the new edges would no longer differ in fp32."""
    _, far, frr = roc(h)
    k = _crossing(far, frr)
    if k < 0 or k >= h.bins:
        return None
    j0 = max(0, min(k - 1, h.bins - 2))
    e = h.edges()
    lo, hi = np.float32(e[j0]), np.float32(e[min(j0 + 2, h.bins)])
    return (float(lo), float(hi)) if hi > lo and (hi - lo) / h.bins > 0 else None


def _passes(a, lab_a, b, lab_b, bins, passes, norm_a=None, norm_b=None, lo=None, hi=None):
    """The histograms of the passes that ran: the first over [lo, hi) -- by default [-1, 1), with
    norm_a norm_range's -- each further one over _zoom of the one before, everything outside carried
    by its under- and overflow slots.  passes=None: 2, with norm_a 3."""
    if passes is None:
        passes = 2 if norm_a is None else 3
    if passes < 1:
        raise ValueError("passes must be >= 1")
    if (lo is None) != (hi is None):
        raise ValueError("give lo and hi together, or neither")
    if lo is None:
        lo, hi = (-1.0, 1.0) if norm_a is None else norm_range(norm_a, norm_b)
    kw = {} if norm_a is None else {"norm_a": norm_a, "norm_b": norm_b}
    hs = [trial_histograms(a, lab_a, b, lab_b, bins=bins, lo=lo, hi=hi, **kw)]
    while len(hs) < passes:
        z = _zoom(hs[-1])
        if z is None:
            break
        hs.append(trial_histograms(a, lab_a, b, lab_b, bins=bins, lo=z[0], hi=z[1], **kw))
    return hs


def corpus_eer(a, lab_a, b=None, lab_b=None, bins=4096, passes=None, norm_a=None, norm_b=None, lo=None, hi=None):
    """(eer, threshold, far, frr, eer_lo, eer_hi, resolution) of all trials of unit rows a (and b):
    pass 1 bins the cosines over [-1, 1); each further pass reruns the kernel with [lo, hi) set to the
    two bins around the crossing of the pass before (after two passes of 4096 bins a range about
    2.4e-7 wide), the scores outside it carried by the under- and overflow slots, whose counts
    enter FAR and FRR exactly.  The tuple is eer() of the last pass plus its bin width.  A crossing
    outside the first range ends the passes early.

    norm_a (norm_b) = (mu, inv): the trials of the AS-normalised score z (trial_histograms).  Pass 1
    then covers norm_range(norm_a, norm_b) -- or the given [lo, hi) -- a range W of tens of units.

    passes=None is 2 passes for cosines and 3 for normalised scores: bins of W / 4096, then W / 2^23,
    then W / 2^34 (2.3e-9 at W = 40, below the spacing of fp32 values of z wherever |z| > 0.02: the
    last pass separates every pair of distinct normalised scores there)."""
    h = _passes(a, lab_a, b, lab_b, bins, passes, norm_a, norm_b, lo, hi)[-1]
    return eer(h) + (h.width,)


# ----------------------------------------------------------------------------- d-vectors
@torch.no_grad()
def corpus_dvectors(net, corpus, T=TRAIN_FRAMES, start=0, precision="f32", batch=None):
    """[U, proj] unit-norm d-vectors of every utterance of a data_load.DeviceCorpus, frames start :
    start + T of each: batches of ``batch`` utterances (None: embed_windows' defaults) as CorpusBatch
    objects through the forward that saves no state, so the frames are cut out of the corpus on the
    device and nothing is gathered on the host.  Raises PersistentRecurrenceError as embed_windows does."""
    from .dvector import bf16_batch
    from .ops import check_persistent_status, embedder_forward, embedder_forward_bf16
    if precision not in ("f32", "bf16"):
        raise ValueError(f"precision must be 'f32' or 'bf16', got {precision!r}")
    if not 1 <= T <= corpus.n_frames or not 0 <= start <= corpus.n_frames - T:
        raise ValueError(f"corpus_dvectors: frames {start} : {start + T} outside the corpus' {corpus.n_frames}")
    dev = corpus.data.device
    layers = net.LSTM_stack.layer_params()
    if batch is None:
        batch = bf16_batch(layers[0][1].shape[1]) if precision == "bf16" else 16384
    fwd, kw = (embedder_forward_bf16, {}) if precision == "bf16" else (embedder_forward, {"products": net.f32_products})
    utt = torch.arange(corpus.n_utt, dtype=torch.int32, device=dev)
    first = torch.full((corpus.n_utt,), int(start), dtype=torch.int32, device=dev)
    out = []
    with torch.cuda.device(dev):
        for i in range(0, corpus.n_utt, batch):
            cb = CorpusBatch(corpus, utt[i:i + batch], first[i:i + batch], T)
            emb, _ = fwd(cb, layers, net.projection.weight, net.projection.bias, save=False, schedule=net.schedule, **kw)
            out.append(emb)
        check_persistent_status(wait=True)
    return out[0] if len(out) == 1 else torch.cat(out)


def utterance_windows(frame_off, win=160, hop=80):
    """(starts int32 [S], part_off int32 [n_utt + 1]): the first row of every window of every utterance
    of a ragged batch of time-major frames (frame_off [n_utt + 1] row offsets) -- j = 0, hop, ... while
    j + win <= T, so a window that ends exactly at T is kept (this module's rule; the export's strict
    '<' is dvector.window_starts') -- and the window offsets of the utterances.  ValueError naming the
    first utterance shorter than win."""
    frame_off = np.asarray(frame_off, dtype=np.int64)
    if win < 1 or hop < 1:
        raise ValueError("utterance_windows: win and hop must be >= 1")
    starts, part_off = [], [0]
    for u, (a, b) in enumerate(zip(frame_off[:-1], frame_off[1:])):
        if b - a < win:
            raise ValueError(f"utterance {u} has {b - a} frames, fewer than one window of {win}")
        s = np.arange(0, b - a - win + 1, hop, dtype=np.int64)
        starts.append(a + s)
        part_off.append(part_off[-1] + s.size)
    starts = np.concatenate(starts) if starts else np.zeros(0, dtype=np.int64)
    return starts.astype(np.int32), np.asarray(part_off, dtype=np.int32)


def _unit_rows(x64):
    """fp64 rows -> unit rows, fp32."""
    return (x64 / x64.norm(dim=1, keepdim=True)).to(torch.float32)


@torch.no_grad()
def utterance_dvectors(net, frames, frame_off, win=160, hop=80, precision="f32"):
    """The GE2E paper's inference (arXiv 1710.10467 section 3.2) for a ragged batch: frames
    [n_frames, nmels] time-major log-mel rows on the device and frame_off [n_utt + 1] (features.logmel's
    outputs); every utterance is cut into windows of ``win`` frames every ``hop`` frames
    (utterance_windows), all windows are embedded in one embed_windows call, each utterance's unit
    window d-vectors are averaged (sv_dvec_align, one part per utterance) and the mean is
    renormalised.  Returns [n_utt, proj] float32 on the device.  ValueError for an utterance shorter
    than win; PersistentRecurrenceError as embed_windows."""
    from .dvector import embed_windows
    from .ops import dvec_align
    starts, part_off = utterance_windows(frame_off, win, hop)
    dev = frames.device
    idx = torch.from_numpy(starts.astype(np.int64)).to(dev)[:, None] + torch.arange(win, device=dev)[None, :]
    emb = embed_windows(net, frames[idx], precision=precision)
    with torch.cuda.device(dev):
        mean = dvec_align(emb.contiguous(), torch.from_numpy(part_off).to(dev))
    return _unit_rows(mean)


def enroll_split(speaker_off, k):
    """The enrol=k protocol's tables from speaker_off [S + 1] (speaker s owns utterances speaker_off[s] :
    speaker_off[s + 1]): (enroll_idx int64, enroll_off int32 [S + 1], test_idx int64, test_lab int32) --
    a speaker's first k utterances (all of them if it has no more) make its model, rows
    enroll_off[s] : enroll_off[s + 1] of enroll_idx; every remaining utterance is a test labelled
    with its speaker.  A speaker with <= k utterances gives a model and no tests."""
    speaker_off = np.asarray(speaker_off, dtype=np.int64)
    if k < 1:
        raise ValueError("enroll_split: k must be >= 1")
    enroll, off, test, lab = [], [0], [], []
    for s, (a, b) in enumerate(zip(speaker_off[:-1], speaker_off[1:])):
        m = min(a + k, b)
        enroll.append(np.arange(a, m))
        off.append(off[-1] + m - a)
        test.append(np.arange(m, b))
        lab.append(np.full(b - m, s))
    return (np.concatenate(enroll).astype(np.int64), np.asarray(off, dtype=np.int32),
            np.concatenate(test).astype(np.int64), np.concatenate(lab).astype(np.int32))


def trials_of(d, speaker_off, enroll=None):
    """(a, lab_a, b, lab_b) for trial_histograms from the unit d-vectors d [U, proj] of a corpus.
    enroll=None: all pairs of utterances (b, lab_b None: symmetric), label = speaker.  enroll=k: the
    tests of enroll_split against all S speaker models, a model the renormalised mean of the
    speaker's first k unit d-vectors (sv_dvec_align)."""
    from .ops import dvec_align
    dev = d.device
    speaker_off = np.asarray(speaker_off, dtype=np.int64)
    S = speaker_off.shape[0] - 1
    if enroll is None:
        lab = np.repeat(np.arange(S, dtype=np.int32), np.diff(speaker_off))
        return d, torch.from_numpy(lab).to(dev), None, None
    e_idx, e_off, t_idx, t_lab = enroll_split(speaker_off, enroll)
    if t_idx.size == 0:
        raise ValueError(f"enroll={enroll} leaves no test utterance: no speaker has more than {enroll}")
    with torch.cuda.device(dev):
        models = _unit_rows(dvec_align(d[torch.from_numpy(e_idx).to(dev)].contiguous(), torch.from_numpy(e_off).to(dev)))
    return (d[torch.from_numpy(t_idx).to(dev)].contiguous(), torch.from_numpy(t_lab).to(dev), models,
            torch.arange(S, dtype=torch.int32, device=dev))


def evaluate(net, corpus, enroll=None, T=TRAIN_FRAMES, precision="f32", bins=4096, passes=None, p_target=0.01,
             cohort=None, top_k=300, std_floor=1e-5):
    """Verification quality of ``net`` on a data_load.DeviceCorpus: a dict with eer, threshold, eer_lo,
    eer_hi (corpus_eer on the trials), min_dcf (of the first pass, all of [-1, 1), at p_target with unit
    costs), n_target and n_nontarget.  The d-vectors are corpus_dvectors(net, corpus, T, precision=...).

    enroll=None: every pair of utterances is a trial (symmetric mode), a target when both are one
    speaker's.  enroll=k: a speaker's first k utterances make its model (the mean of their unit
    d-vectors, renormalised) and every remaining utterance is scored against all S models; a speaker
    with <= k utterances gives a model and no tests.

    Unlike test(), the own-speaker score uses the enrolment model as it stands: there is no
    leave-one-out centroid, no batches of hp.test.N speakers and no 50-point threshold grid, so the
    two figures are not comparable.

    cohort: adaptive symmetric score normalisation (AS-norm).  Either a float32 [Nc, proj] device
    tensor of unit rows, or a DeviceCorpus, which is embedded with corpus_dvectors (same T and
    precision) and reduced to one model per speaker with cohort_models.  Both sides of every trial --
    the utterances, or with enroll=k the tests and the speaker models -- get the mean and std of their
    top_k cohort scores (cohort_stats), inv = 1 / max(std, std_floor), and the trials are those of
    z = 0.5 ((s - mu_e) inv_e + (s - mu_t) inv_t): three zoom passes by default, the first over
    norm_range.  threshold and min_dcf are then on the scale of z, and the dict also carries
    score_norm = "as-norm", top_k, n_cohort and range, the first pass's (lo, hi).  ValueError for
    top_k > Nc.  The cohort must not contain the evaluated speakers: their own utterances among the
    top scores shrink the normalised target scores.  That is the caller's responsibility; nothing
    here can check it.  Without cohort the dict is the un-normalised one, unchanged."""
    d = corpus_dvectors(net, corpus, T=T, precision=precision)
    a, lab_a, b, lab_b = trials_of(d, corpus.speaker_off, enroll)
    if cohort is None:
        hs = _passes(a, lab_a, b, lab_b, bins, passes)
        extra = {}
    else:
        if not torch.is_tensor(cohort):
            cohort = cohort_models(corpus_dvectors(net, cohort, T=T, precision=precision), cohort.speaker_off)
        norm_a = as_norm(a, cohort, top_k, std_floor)
        norm_b = None if b is None else as_norm(b, cohort, top_k, std_floor)
        hs = _passes(a, lab_a, b, lab_b, bins, passes, norm_a, norm_b)
        extra = {"score_norm": "as-norm", "top_k": int(top_k), "n_cohort": int(cohort.shape[0]),
                 "range": (hs[0].lo, hs[0].hi)}
    e, thr, _, _, e_lo, e_hi = eer(hs[-1])
    return {"eer": e, "threshold": thr, "eer_lo": e_lo, "eer_hi": e_hi, "min_dcf": min_dcf(hs[0], p_target),
            "n_target": hs[0].n_target, "n_nontarget": hs[0].n_nontarget, **extra}
