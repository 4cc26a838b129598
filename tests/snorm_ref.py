"""Numpy oracle for adaptive score normalisation (pytorch_speaker_verification_amd/verification.py,
csrc/sv_snorm.hip, sv_trial_hist_norm of csrc/sv_trials.hip): sort-based top-K statistics in fp64,
the normalisation step of include/sv_ge2e.h applied literally in np.float32 and the same in fp64, and
the header's order-preserving key of a score."""
import numpy as np

import verification_ref as R


def topk_stats(scores_fp64, k):
    """(mean, std) float64 [N] of the k largest entries of every row of scores_fp64 [N, Nc]: a sort (NaN
    sorts last, i.e. largest), the mean and the population standard deviation (divisor k) in fp64."""
    s = np.sort(np.asarray(scores_fp64, dtype=np.float64), axis=1)[:, -int(k):]
    with np.errstate(invalid="ignore"):
        return s.mean(axis=1), s.std(axis=1)


def normalise(s, mu_a, inv_a, mu_b, inv_b):
    """z [Na, Nb] float32 of the scores s [Na, Nb]: za = (s - mu_a[i]) * inv_a[i], zb = (s - mu_b[j]) *
    inv_b[j], z = 0.5f * (za + zb), every operation rounded to fp32 on its own."""
    f = np.float32
    s = np.asarray(s).astype(f)
    mu_a, inv_a = np.asarray(mu_a).astype(f)[:, None], np.asarray(inv_a).astype(f)[:, None]
    mu_b, inv_b = np.asarray(mu_b).astype(f)[None, :], np.asarray(inv_b).astype(f)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        za = ((s - mu_a).astype(f) * inv_a).astype(f)
        zb = ((s - mu_b).astype(f) * inv_b).astype(f)
        return (f(0.5) * (za + zb).astype(f)).astype(f)


def as_norm_fp64(s, mu_a, inv_a, mu_b, inv_b):
    """The same in fp64."""
    d = np.float64
    s = np.asarray(s, dtype=d)
    return 0.5 * ((s - np.asarray(mu_a, dtype=d)[:, None]) * np.asarray(inv_a, dtype=d)[:, None]
                  + (s - np.asarray(mu_b, dtype=d)[None, :]) * np.asarray(inv_b, dtype=d)[None, :])


def normalised_hist(s, live, target, norm_a, norm_b, lo, inv_width, n_bins):
    """counts int64 [2, n_bins + 2] of the fp32-normalised scores by class (verification_ref's slot rule)."""
    z = normalise(s, *norm_a, *norm_b)
    return R.hist_of_scores(*R.split(z, live, target), lo, inv_width, n_bins)


def key32(s):
    """The order-preserving uint32 key of fp32 scores that the header defines: all bits flipped if the
    sign bit is set, else the sign bit flipped; NaN takes 0xffffffff."""
    s = np.asarray(s, dtype=np.float32)
    u = s.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(s), np.uint32(0xFFFFFFFF), k)
