"""Shrinking failing fault sets to 1-minimal ones: take a fault set the decoder fails on and remove faults while it keeps failing (the
greedy search of LDPC error-floor / trapping-set studies).  What is left bounds the exponent of pL ~ p^t for this decoder by its weight, and
its residual S xor C is an undetectable logical fault of weight about 2 |S|: an upper bound on the circuit-level distance.

Host side, numpy only: the definition, the result record and `shrink_mirror`, the CPU reference of the step kernels (csrc/shrink.hip,
decoder.device.FaultShrinker), which must produce the same trials in the same order and the same final sets, bit for bit.

The definition.  A model has check matrix H (m x n) and observable matrix L (k x n), columns as in detector_error_model_to_matrix; a decoder
D maps detector bits to k predicted observables.  A fault set S FAILS iff D(H S) != L S in any observable.  Every parent set E walks alone:

  state:     S = E, last = -1, quiet = 0, w = |S|
  trial 0:   the set S itself, no fault removed.  If it does not fail the parent ends with fails = False and S = E.
  otherwise repeat:
    if quiet >= w the parent ends as MINIMAL (this covers w = 0);
    j = the smallest member of S above `last`, wrapping to the smallest member of S when there is none;
    the trial is S \\ {j};
    if it fails:  S <- S \\ {j}, w <- w - 1, quiet <- 0;   if it does not:  quiet <- quiet + 1;   in both cases last <- j.

At the end the last |S| trials removed each member of S once from the same S and none of them failed: S is 1-minimal.  Every trial after
trial 0 either removes a fault or raises `quiet`, so a parent of |E| faults makes at most |E| (|E| + 1) / 2 + 1 trials (`trial_bound`).
Per parent the outputs are the final S, `fails`, `minimal` and the number of trials.  A trial is one decode; the parents advance together,
one trial each per round, so the decoder sees batches -- and since it returns the same bits for a row whatever batch the row sits in, the
walk of a parent does not depend on the other parents.
"""
from __future__ import annotations

import dataclasses

import numpy as np

STATE_WORDS = 8                 # QD_SHRINK_STATE: int32 per parent -- last, quiet, w, trials, flags, pending fault, start weight, 0
FLAG_FAILS, FLAG_MINIMAL, FLAG_ENDED = 1, 2, 4      # QD_SHRINK_FAILS, QD_SHRINK_MINIMAL, QD_SHRINK_ENDED


@dataclasses.dataclass
class ShrinkResult:
    """What a shrink returns, one entry per parent.  sets: the final sets, bool [P, n] (or packed int32 [P, ceil(n / 32)] words, bit j & 31 of
    word j >> 5 = fault j, where the caller passed packed sets); fails: trial 0 failed; minimal: the walk ended with `quiet >= w` (False for a
    parent that does not fail); start_weight, weight: |E| and the final |S|; trials: decodes spent on the parent, trial 0 included."""
    sets: np.ndarray
    fails: np.ndarray
    minimal: np.ndarray
    start_weight: np.ndarray
    weight: np.ndarray
    trials: np.ndarray


def trial_bound(weight):
    """|E| (|E| + 1) / 2 + 1: no parent of |E| faults makes more trials."""
    w = np.asarray(weight, dtype=np.int64)
    return w * (w + 1) // 2 + 1


def pack_sets(bits, words=None):
    """bool [P, n] -> int32 [P, words] (default ceil(n / 32)), padding bits zero."""
    bits = np.asarray(bits).astype(bool)
    if bits.ndim != 2:
        raise ValueError("fault sets must be a [parents, faults] array")
    n = bits.shape[1]
    words = (n + 31) // 32 if words is None else int(words)
    if 32 * words < n:
        raise ValueError("%d words cannot hold %d faults" % (words, n))
    pad = np.zeros((bits.shape[0], 32 * words), np.uint8)
    pad[:, :n] = bits
    return np.packbits(pad, axis=1, bitorder="little").view("<i4").reshape(bits.shape[0], words)


def unpack_sets(words, n):
    """int32 [P, words] -> bool [P, n]."""
    w = np.ascontiguousarray(words, dtype=np.int32)
    if w.ndim != 2 or 32 * w.shape[1] < n:
        raise ValueError("packed sets of shape %s cannot hold %d faults" % (w.shape, n))
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :n].astype(bool)


def shrink_mirror(fault_sets, fails, rounds=False):
    """The definition in the module docstring.  fault_sets: bool [P, n]; fails: a callable bool [A, n] -> bool [A].  All live parents advance
    one trial per round, in ascending parent order, so the callable sees batches.  Returns a ShrinkResult (sets bool [P, n]); rounds=True:
    (result, log), log[r] = (parents int64 [A], faults int64 [A]) of round r: the live parents and the fault each one's trial removes, -1 for
    trial 0."""
    S = np.array(fault_sets, dtype=bool)
    if S.ndim != 2:
        raise ValueError("fault_sets must be a [parents, faults] array")
    P, n = S.shape
    last = np.full(P, -1, np.int64)
    quiet = np.zeros(P, np.int64)
    w = S.sum(axis=1).astype(np.int64)
    start = w.copy()
    trials = np.zeros(P, np.int64)
    failed = np.zeros(P, bool)
    minimal = np.zeros(P, bool)
    cur = np.full(P, -1, np.int64)
    live = np.arange(P, dtype=np.int64)
    log = []
    while live.size:
        T = S[live].copy()
        rem = cur[live] >= 0
        T[np.flatnonzero(rem), cur[live][rem]] = False
        verdict = np.asarray(fails(T)).astype(bool).reshape(-1)
        if verdict.shape[0] != live.size:
            raise ValueError("the predicate returned %d verdicts for %d trials" % (verdict.shape[0], live.size))
        if rounds:
            log.append((live.copy(), cur[live].copy()))
        trials[live] += 1
        alive = np.ones(live.size, bool)
        for i, p in enumerate(live):
            j = int(cur[p])
            if j < 0:
                if not verdict[i]:
                    alive[i] = False
                    continue
                failed[p] = True
            else:
                if verdict[i]:
                    S[p, j] = False
                    w[p] -= 1
                    quiet[p] = 0
                else:
                    quiet[p] += 1
                last[p] = j
            if quiet[p] >= w[p]:
                minimal[p] = True
                alive[i] = False
                continue
            members = np.flatnonzero(S[p])
            above = members[members > last[p]]
            cur[p] = above[0] if above.size else members[0]
        live = live[alive]
    res = ShrinkResult(S, failed, minimal, start, w, trials)
    return (res, log) if rounds else res


def is_one_minimal(fault_set, fails):
    """True iff the set fails and none of its one-fault-removed children does (one call of `fails` on |S| + 1 rows)."""
    s = np.asarray(fault_set, dtype=bool).reshape(-1)
    members = np.flatnonzero(s)
    rows = np.repeat(s[None, :], members.size + 1, axis=0)
    rows[np.arange(1, members.size + 1), members] = False
    v = np.asarray(fails(rows)).astype(bool).reshape(-1)
    return bool(v[0]) and not v[1:].any()
