"""Soft outputs: what the decoder knows about a shot besides its prediction, and the logical error rate that is left when the least
certain shots are discarded.  This file is the definition; the kernels of csrc/soft.hip (qd_soft_fold, qd_soft_weigh, qd_soft_tally) equal
it bit for bit, as csrc/shrink.hip equals shrink.py.  numpy only.

A soft record is one int64[6] per shot, FIELDS = ("weight", "faults", "events", "iters", "post", "tail"):

    weight  sum of w_j over the faults j of the committed space-time correction C (decoder.corrections), w = fault_weights(priors): the
            log-likelihood cost of the correction in units of 2^-16 nat.  A heavy correction is an unlikely one.
    faults  |C|, the number of faults in the correction.
    events  the number of detector bytes of the shot with the low bit set (the syndrome's weight).
    iters   the BP iterations over all windows: the sum of `status & QD_STATUS_ITER_MASK`.
    post    the number of windows whose output came from the post-processor (QD_STATUS_OSD).
    tail    the sum over the windows of `(status >> 20) & 0xFFF`, the top twelve bits of the status word.  Relay-BP writes the leg that
            produced the returned candidate there (QD_STATUS_RELAY_LEG_SHIFT), so for Relay-BP this is a sum of leg indices.  For BP-OSD and
            BP-LSD these bits are the post-processor's pivot count, saturating at 4095 per window, wherever the decoder reports one; a decoder
            that reports none leaves them zero and the field is zero.

Bits 14 .. 19 of a status word (grid, exactness, convergence, inconsistency, zero syndrome) enter no field but `post` (bit 17).

Every field is a non-negative "larger = less certain" score except that `weight` can be negative where priors exceed 1/2.  A histogram of a
field has BINS bins of width 2^shift (bin_of); selection_curve reads the acceptance curve off it.
"""
from __future__ import annotations

import math

import numpy as np

FIELDS = ("weight", "faults", "events", "iters", "post", "tail")
BINS = 1024                      # QD_SOFT_BINS
WEIGHT_ONE = 1 << 16             # the weight of a fault with p = 1 / (1 + e): one nat
_W_MAX = 2 ** 31 - 1

STATUS_ITER_MASK = 0x3FFF        # QD_STATUS_ITER_MASK
STATUS_OSD = 1 << 17             # QD_STATUS_OSD
STATUS_TAIL_SHIFT, STATUS_TAIL_MASK = 20, 0xFFF


def fault_weights(priors):
    """int32 [n]: rint(log((1 - p) / p) * 2^16), computed in float64 and clipped to +-(2^31 - 1).  p = 0.5 gives 0; p outside (0, 1) raises
    ValueError (such a fault has no finite cost).  The host makes this table once; the device never computes a logarithm."""
    p = np.asarray(priors, dtype=np.float64).reshape(-1)
    if p.size and not bool(np.all((p > 0.0) & (p < 1.0))):
        raise ValueError("fault weights need priors inside (0, 1)")
    with np.errstate(over="ignore"):             # (a subnormal prior: the quotient overflows, the weight clips)
        w = np.rint(np.log((1.0 - p) / p) * float(WEIGHT_ONE))
    return np.clip(w, -float(_W_MAX), float(_W_MAX)).astype(np.int64).astype(np.int32)


def _host(a):
    """numpy view of an array-like; device tensors are copied to the host (no torch import here)."""
    if hasattr(a, "detach") and hasattr(a, "cpu"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def status_fields(status):
    """(iters, post, tail) int64 arrays of status words (any integer array; the words are taken as int32 bit patterns)."""
    s = _host(status).astype(np.int64) & 0xFFFFFFFF
    return s & STATUS_ITER_MASK, (s >> 17) & 1, (s >> STATUS_TAIL_SHIFT) & STATUS_TAIL_MASK


def soft_mirror(corr_bits, det, statuses, weights):
    """int64 [N, 6] soft records.  corr_bits: [N, n] array of 0 / 1 (or anything np.asarray unpacks to one, e.g. the PackedSamples that
    sliding_window_corrections returns), the committed correction; det: [N, ndet] detector bytes, of which the low bit counts; statuses: the
    (window, status words) pairs that plan.decode(stats=...) yields -- the pairs of one window, laid end to end in the order given, are the
    shots 0 .. N - 1; weights: int [n] (fault_weights)."""
    c = (_host(corr_bits).astype(np.int64) & 1)
    d = _host(det)
    d = d.astype(np.int64) & 1
    w = np.asarray(weights, dtype=np.int64).reshape(-1)
    if c.ndim != 2 or d.ndim != 2 or c.shape[0] != d.shape[0] or c.shape[1] != w.shape[0]:
        raise ValueError("corrections %s, detectors %s and %d weights do not go together" % (c.shape, d.shape, w.shape[0]))
    N = c.shape[0]
    out = np.zeros((N, len(FIELDS)), dtype=np.int64)
    out[:, 0] = c @ w
    out[:, 1] = c.sum(axis=1)
    out[:, 2] = d.sum(axis=1)
    at = {}
    for k, st in statuses:
        it, post, tail = status_fields(_host(st).reshape(-1))
        a = at.get(int(k), 0)
        if a + it.shape[0] > N:
            raise ValueError("window %d reports more than %d status words" % (k, N))
        out[a:a + it.shape[0], 3] += it
        out[a:a + it.shape[0], 4] += post
        out[a:a + it.shape[0], 5] += tail
        at[int(k)] = a + it.shape[0]
    if any(a != N for a in at.values()):
        raise ValueError("status words for %s shots per window, the batch has %d" % (sorted(at.items()), N))
    return out


def _shift_for(top):
    """The smallest shift that puts the value `top` (>= 0) into the BINS bins: top >> shift <= BINS - 1."""
    top, s = max(int(top), 0), 0
    while (top >> s) > BINS - 1:
        s += 1
    return s


def default_shifts(weights, priors, ndet, nwindows, max_iter):
    """int32 [6] bin widths 2^shift, a function of the arguments alone (never of the data): `weight` the smallest shift that puts four times the
    expected weight of the sampled fault set, 4 * sum_j p_j w_j, into the BINS bins; `faults` and `events` the smallest that hold n and ndet;
    `iters` nwindows * max_iter; `post` 0 (there are at most nwindows post-processed windows); `tail` nwindows * 4095."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    p = np.asarray(priors, dtype=np.float64).reshape(-1)
    if w.shape != p.shape:
        raise ValueError("%d weights, %d priors" % (w.shape[0], p.shape[0]))
    expect = float(np.sum(p * w))
    return np.array([_shift_for(math.ceil(4.0 * max(expect, 0.0))), _shift_for(w.shape[0]), _shift_for(ndet), _shift_for(int(nwindows) * int(max_iter)),
                     0, _shift_for(int(nwindows) * 4095)], dtype=np.int32)


def bin_of(value, shift):
    """clip(value >> shift, 0, BINS - 1) as int64: negative values go to bin 0, values of BINS * 2^shift and more to the last bin."""
    v = np.asarray(value, dtype=np.int64)
    return np.clip(v >> np.int64(shift), 0, BINS - 1)


def histogram(soft, shifts, fail=None):
    """int64 [6, 2, BINS] of soft records [N, 6]: plane 0 counts every shot's bin, plane 1 the shots with fail[b] true (None: plane 1 stays zero).
    What qd_soft_tally adds to its histogram."""
    soft = np.asarray(soft, dtype=np.int64).reshape(-1, len(FIELDS))
    h = np.zeros((len(FIELDS), 2, BINS), dtype=np.int64)
    f = None if fail is None else np.asarray(fail).astype(bool).reshape(-1)
    for i in range(len(FIELDS)):
        b = bin_of(soft[:, i], int(shifts[i]))
        h[i, 0] = np.bincount(b, minlength=BINS)
        if f is not None:
            h[i, 1] = np.bincount(b[f], minlength=BINS)
    return h


def selection_curve(hist_field):
    """hist_field: int [2, nbins] (all shots, failing shots) of one field.  Returns (kept, errors, pL, sigma): accepting the shots of bins
    <= t keeps kept[t] shots (int64) of which errors[t] fail (int64); pL[t] = errors / kept with its binomial standard deviation sigma[t], NaN
    where nothing is kept.  The last entry is the whole set."""
    h = np.asarray(hist_field, dtype=np.int64)
    if h.ndim != 2 or h.shape[0] != 2:
        raise ValueError("a field's histogram is [2, bins]")
    kept, errors = np.cumsum(h[0]), np.cumsum(h[1])
    k = kept.astype(np.float64)
    pL = np.divide(errors.astype(np.float64), k, out=np.full(k.shape, np.nan), where=kept > 0)
    sigma = np.sqrt(np.divide(pL * (1.0 - pL), k, out=np.full(k.shape, np.nan), where=kept > 0))
    return kept, errors, pL, sigma


__all__ = ["FIELDS", "BINS", "WEIGHT_ONE", "fault_weights", "status_fields", "soft_mirror", "default_shifts", "bin_of", "histogram", "selection_curve"]
