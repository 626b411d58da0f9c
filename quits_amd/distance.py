"""An estimate of the code or circuit-level distance from random information sets (the method of QDistRnd; Stim has no counterpart): put
the columns of H in a random order, eliminate, and every dependent column closes a kernel vector; the lightest one that flips an observable
is kept.  It needs no decoder, no sampling and no truncated space; what it finds certifies itself (H e = 0, L e != 0) and bounds the
distance FROM ABOVE.  It is never a lower bound: a trial that finds nothing light says nothing.

Host side, numpy only: the definition, the result record, `distance_mirror` (the CPU reference of the kernels, csrc/distance.hip) and
`kernel_vector`, which regenerates a witness from a record; then `DistanceEstimator`, the device class, and the calls.  The text below is
the definition: the mirror and the kernels must produce the same records and the same histogram, bit for bit.

The definition.  H (detectors x faults) and L (observables x faults) have one column per fault; the columns of H are taken mod 2 with
duplicates summed.  obs(j) is the mask of the SELECTED observables column j of L flips (bit i = the i-th selected observable; `observables`
selects at most 64 rows of L, default all of them).  A code with more than 64 logicals is covered by running disjoint selections and taking
the minimum: any logical vector flips at least one of them.

  limits       1 .. 65535 detectors, at least one fault, at most 64 selected observables: ValueError beyond.
  order        key(t, j) = word j & 3 of Philox4x32-10(key = (seed lo, seed hi), counter = (t lo, t hi, j >> 2, 4)) -- the last counter
               words 0 .. 3 belong to the samplers and Relay-BP.  The order of trial t is the faults sorted by (key, j) ascending.
  pivots       a column is a pivot iff it is not in the span of the columns before it in the order.  This names no pivot row and no
               elimination strategy: the mirror and the kernels are free in both.
  candidates   for every non-pivot column j, e(t, j) = {j} + the unique set of earlier pivots that sums to h_j; w = |e|,
               o = XOR of obs over e.  Dependent columns met before the rank is complete are candidates like any other; a fault without
               detectors is a candidate of weight 1 in every trial (and counts iff its mask is non-zero).
  record       rec[t] = min over the candidates with o != 0 of w * 2^32 + j, a uint64; NO_RECORD (2^64 - 1) if the trial has none.  Ties
               in weight go to the lowest fault index.
  histogram    hist[64], uint64: the candidates with o != 0 by weight over all trials run; bin 63 holds every weight >= 63.

rec[t] is a function of (H, L, observables, seed, t) alone: not of the batch, the grid or the trials run before it.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import time

import numpy as np

from .search import MAX_DETECTORS, MAX_OBSERVABLES, _matrices

NO_RECORD = 0xFFFFFFFFFFFFFFFF          # the record of a trial without a logical candidate
HIST_BINS = 64
STREAM = 4                              # last Philox counter word of the column keys
_M64 = np.uint64(63)


@dataclasses.dataclass
class DistanceResult:
    """What an estimate returns.  weight: the lightest undetectable logical fault set found, or None -- an UPPER bound on the distance, never
    a lower one: more trials can only lower it, and no number of trials proves it tight.  witnesses: int64 arrays of fault indices,
    ascending, and masks: what each flips (bit i = the i-th selected observable) -- the lightest records in (trial, fault) order, at most
    `keep` of them, regenerated on the host with `kernel_vector`, passed through `check_vector`, equal fault sets kept once.  trials: the
    trials that ran, first_trial .. : trials 0 .. trials - 1 of `seed`, so the result is reproducible from (seed, trials); first_trial: the
    first trial that reached `weight`; hist: the histogram of the module docstring over those trials; records: the uint64 record of every
    trial (keep_records=True, else None); rank: the GF(2) rank of H; seconds."""
    weight: int | None
    witnesses: list
    masks: list
    trials: int
    first_trial: int | None
    hist: np.ndarray
    records: np.ndarray | None
    rank: int
    seed: int
    observables: list
    seconds: float = 0.0

    def to_json(self) -> dict:
        return {"weight": self.weight, "witnesses": [[int(j) for j in w] for w in self.witnesses], "masks": [int(m) for m in self.masks],
                "trials": int(self.trials), "first_trial": self.first_trial, "hist": [int(x) for x in self.hist],
                "records": None if self.records is None else [int(x) for x in self.records], "rank": int(self.rank), "seed": int(self.seed),
                "observables": list(self.observables), "seconds": float(self.seconds)}


@dataclasses.dataclass
class DistanceModel:
    """The tables both engines read.  ndet, n; col_ptr int64 [n + 1], col_rows int32: the detectors of every fault, ascending (CSC of H mod 2);
    fault_obs uint64 [n]; observables: the selected rows of L."""
    ndet: int
    n: int
    col_ptr: np.ndarray
    col_rows: np.ndarray
    fault_obs: np.ndarray
    observables: list


def prepare(H, L, observables=None) -> DistanceModel:
    """Check the limits and lay out the tables of the module docstring."""
    H, L = _matrices((H, L))
    ndet, n = H.shape
    if ndet > MAX_DETECTORS:
        raise ValueError("%d detectors: the estimate holds at most %d" % (ndet, MAX_DETECTORS))
    if observables is None:
        if L.shape[0] > MAX_OBSERVABLES:
            raise ValueError("%d observables: at most %d are searched at a time -- pass a selection, observables=[...]" % (L.shape[0], MAX_OBSERVABLES))
        observables = list(range(L.shape[0]))
    observables = [int(i) for i in observables]
    if len(observables) > MAX_OBSERVABLES:
        raise ValueError("%d observables selected: at most %d are searched at a time" % (len(observables), MAX_OBSERVABLES))
    if len(set(observables)) != len(observables) or any(not 0 <= i < L.shape[0] for i in observables):
        raise ValueError("observables must be distinct row indices of L (0 .. %d)" % (L.shape[0] - 1))
    if ndet < 1 or n < 1:
        raise ValueError("the model has %d detectors and %d faults: nothing to estimate" % (ndet, n))
    fault_obs = np.zeros(n, np.uint64)
    Lr = L.tocsr()
    for bit, i in enumerate(observables):
        row = Lr.indices[Lr.indptr[i]:Lr.indptr[i + 1]][Lr.data[Lr.indptr[i]:Lr.indptr[i + 1]] % 2 != 0]
        fault_obs[row] |= np.uint64(1 << bit)
    Hc = H.copy()                                        # (the caller's matrix stays as it is)
    Hc.sum_duplicates()
    Hc.data = (Hc.data % 2).astype(np.uint8)
    Hc.eliminate_zeros()
    Hc.sort_indices()
    return DistanceModel(ndet, n, Hc.indptr.astype(np.int64), Hc.indices.astype(np.int32), fault_obs, observables)


def trial_order(n, seed, t) -> np.ndarray:
    """The column order of trial t (module docstring): int64 [n]."""
    from .strata import philox4x32_10
    seed, t = int(seed), int(t)
    words = philox4x32_10(t & 0xFFFFFFFF, (t >> 32) & 0xFFFFFFFF, np.arange((n + 3) // 4, dtype=np.uint64), STREAM, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    keys = np.stack(words, axis=1).reshape(-1)[:n]
    return np.argsort(keys, kind="stable")               # stable: equal keys stay in ascending j


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------
class _Elimination:
    """One trial's elimination, by detector.  Row d of `state` is column d of the row transform R (ndet bits) followed by 64 mask bits: for
    any column h, the XOR of the rows in its support is (R h, mask of the pivots that make up R h).  R h lies inside the pivot rows iff h
    is dependent, and then its set bits name those pivots.  Words of 64 bits; the pivot row of an independent column is its HIGHEST free bit
    (the kernels take the lowest: the definition does not care)."""

    def __init__(self, m: DistanceModel):
        self.m = m
        self.q = (m.ndet + 63) // 64
        self.state = np.zeros((m.ndet, self.q + 1), np.uint64)
        d = np.arange(m.ndet)
        self.state[d, d >> 6] = np.uint64(1) << (d.astype(np.uint64) & _M64)
        self.free = np.zeros(self.q, np.uint64)          # rows without a pivot
        for k in range(self.q):
            self.free[k] = np.uint64((1 << min(64, m.ndet - 64 * k)) - 1)
        self.pivot_of_row = np.full(m.ndet, -1, np.int64)
        self.rank = 0

    def reduce(self, j):
        m = self.m
        rows = m.col_rows[m.col_ptr[j]:m.col_ptr[j + 1]]
        v = np.bitwise_xor.reduce(self.state[rows], axis=0) if len(rows) else np.zeros(self.q + 1, np.uint64)
        v[self.q] ^= m.fault_obs[j]
        return v

    def step(self, j):
        """Take column j: None if it became a pivot, else (weight, mask, reduced vector)."""
        v = self.reduce(j)
        out = v[:self.q] & self.free
        nz = np.flatnonzero(out)
        if not len(nz):
            w = 1 + sum(int(x).bit_count() for x in v[:self.q])
            return w, int(v[self.q]), v
        k = int(nz[-1])
        r = 64 * k + int(out[k]).bit_length() - 1
        bit = np.uint64(1) << np.uint64(r & 63)
        v[k] ^= bit
        hit = np.flatnonzero(self.state[:, k] & bit)
        self.state[hit] ^= v
        self.free[k] ^= bit
        self.pivot_of_row[r] = j
        self.rank += 1
        return None


def _run_trial(m: DistanceModel, seed, t, hist):
    el = _Elimination(m)
    best = NO_RECORD
    for j in trial_order(m.n, seed, t):
        got = el.step(int(j))
        if got is not None and got[1]:
            hist[min(got[0], HIST_BINS - 1)] += np.uint64(1)
            best = min(best, (got[0] << 32) + int(j))
    return best, el.rank


def distance_mirror(H, L, trials, seed=0, trial0=0, observables=None):
    """The definition of the module docstring in numpy: (records uint64 [trials], hist uint64 [64]) of trials trial0 .. trial0 + trials - 1.
    The CPU reference of the kernels."""
    m = H if isinstance(H, DistanceModel) else prepare(H, L, observables)
    rec, hist = np.zeros(int(trials), np.uint64), np.zeros(HIST_BINS, np.uint64)
    for i in range(int(trials)):
        rec[i] = _run_trial(m, seed, int(trial0) + i, hist)[0]
    return rec, hist


def mirror_rank(H, L=None, observables=None) -> int:
    """The GF(2) rank of H, from one trial's elimination."""
    m = H if isinstance(H, DistanceModel) else prepare(H, L, observables)
    return _run_trial(m, 0, 0, np.zeros(HIST_BINS, np.uint64))[1]


def kernel_vector(H, L, seed, t, j, observables=None):
    """The candidate e(t, j) of the module docstring: (faults int64 ascending, mask).  ValueError if column j is a pivot of trial t."""
    m = H if isinstance(H, DistanceModel) else prepare(H, L, observables)
    j = int(j)
    if not 0 <= j < m.n:
        raise ValueError("fault %d is outside 0 .. %d" % (j, m.n - 1))
    el = _Elimination(m)
    for c in trial_order(m.n, seed, t):
        got = el.step(int(c))
        if int(c) == j:
            break
    if got is None:
        raise ValueError("fault %d is a pivot of trial %d: it closes no kernel vector" % (j, int(t)))
    rows = [64 * k + b for k in range(el.q) for b in range(64) if (int(got[2][k]) >> b) & 1]
    return np.sort(np.array([j] + [int(el.pivot_of_row[r]) for r in rows], dtype=np.int64)), got[1]


def check_vector(H, L, e, mask, observables) -> None:
    """Raise AssertionError unless H e = 0 and L[observables] e = mask != 0 (mod 2), e distinct faults in ascending order."""
    H, L = _matrices((H, L))
    e = np.asarray(e, dtype=np.int64)
    assert len(e) and np.all(np.diff(e) > 0) and e[0] >= 0 and e[-1] < H.shape[1], "faults must be distinct, ascending and in range"
    x = np.zeros(H.shape[1], np.int64)
    x[e] = 1
    assert not (np.asarray(H @ x).reshape(-1) % 2).any(), "H e != 0"
    lo = np.asarray(L @ x).reshape(-1) % 2
    got = sum(int(lo[i]) << bit for bit, i in enumerate(observables))
    assert got == int(mask) and got != 0, "L e = %#x, expected %#x" % (got, int(mask))


def _result(H, L, m: DistanceModel, trials, records, first, hist, rank, seed, keep, t0) -> DistanceResult:
    """records: every trial's record or None, first: (weight, [(trial, fault), ...]) the lightest in trial order, or None."""
    weight, wit, masks = None, [], []
    if first is not None:
        weight = first[0]
        seen = set()
        for t, j in first[1][:max(0, int(keep))]:
            e, mask = kernel_vector(m, None, seed, t, j)
            assert len(e) == weight, "record of trial %d says weight %d, its vector has %d faults" % (t, weight, len(e))
            check_vector(H, L, e, mask, m.observables)
            if tuple(e) not in seen:
                seen.add(tuple(e))
                wit.append(e)
                masks.append(mask)
    return DistanceResult(weight, wit, masks, int(trials), None if first is None else first[1][0][0], hist, records, int(rank), int(seed),
                          list(m.observables), time.perf_counter() - t0)


def _lightest(records, trial0, keep, so_far):
    """Fold a batch of records into (weight, [(trial, fault)]): the first `keep` lightest in trial order."""
    live = records != np.uint64(NO_RECORD)
    if not live.any():
        return so_far
    w = int(records[live].min() >> np.uint64(32))
    if so_far is not None and so_far[0] < w:
        return so_far
    if so_far is None or w < so_far[0]:
        so_far = (w, [])
    room = max(1, int(keep)) - len(so_far[1])
    idx = np.flatnonzero(live & ((records >> np.uint64(32)) == np.uint64(w)))[:max(0, room)]
    so_far[1].extend((int(trial0) + int(i), int(records[i] & np.uint64(0xFFFFFFFF))) for i in idx)
    return so_far


def estimate_distance_mirror(model, trials=64, seed=0, keep=16, keep_records=False, observables=None) -> DistanceResult:
    """`estimate_distance` on the CPU through `distance_mirror`: for tests and small models, called by name."""
    t0 = time.perf_counter()
    H, L = _matrices(model)
    m = prepare(H, L, observables)
    rec, hist = distance_mirror(m, None, trials, seed)
    return _result(H, L, m, len(rec), rec if keep_records else None, _lightest(rec, 0, keep, None), hist, mirror_rank(m), seed, keep, t0)


# ---- the device ---------------------------------------------------------------------------------------------------------------------------
class DistanceEstimator:
    """The trials on the device (csrc/distance.hip): one workgroup per trial, the row transform by detector in LDS.  Everything is allocated
    here, before any launch; a model whose transform (or whose order, while it is sorted) does not fit in LDS raises NotImplementedError."""

    def __init__(self, m: DistanceModel, device=None):
        from . import _lib
        import torch
        self.L = _lib.require_distance(_lib.require_gpu())
        self.m = m
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.h = C.c_void_p()
        cp = np.ascontiguousarray(m.col_ptr, dtype=np.int64)
        cr = np.ascontiguousarray(m.col_rows, dtype=np.int32)
        fo = np.ascontiguousarray(m.fault_obs, dtype=np.uint64)
        rc = self.L.qd_isd_create(m.ndet, m.n, cp.ctypes.data, cr.ctypes.data, fo.ctypes.data, self.device, C.byref(self.h))
        if rc == _lib.QD_ECAPACITY:
            raise NotImplementedError("quits_amd: distance estimate: " + self.L.qd_last_error().decode(errors="replace"))
        _lib.check(rc)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.qd_isd_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def info(self) -> dict:
        from . import _lib
        v = np.zeros(8, np.int64)
        _lib.check(self.L.qd_isd_info(self.h, v.ctypes.data))
        return {"lds_bytes": int(v[0]), "threads": int(v[1]), "workspace_bytes": int(v[2]), "trials_in_flight": int(v[3]), "rank": int(v[4]),
                "columns_per_block": int(v[5])}

    def run(self, seed, trial0, ntrials) -> np.ndarray:
        """The records of trials trial0 .. trial0 + ntrials - 1 (uint64); the device histogram grows by their candidates."""
        from . import _lib
        import torch
        out = torch.empty(max(1, int(ntrials)), dtype=torch.int64, device="cuda:%d" % self.device)
        _lib.check(self.L.qd_isd_run(self.h, int(seed) & NO_RECORD, int(trial0), int(ntrials), out.data_ptr(), None))
        torch.cuda.synchronize(self.device)
        return out[:int(ntrials)].cpu().numpy().view(np.uint64)

    def hist(self) -> np.ndarray:
        from . import _lib
        h = np.zeros(HIST_BINS, np.uint64)
        _lib.check(self.L.qd_isd_hist(self.h, h.ctypes.data))
        return h

    def reset(self):
        from . import _lib
        _lib.check(self.L.qd_isd_reset(self.h))


def estimate_distance(model, trials=1 << 16, seed=0, *, target=None, max_seconds=None, batch=None, keep=16, keep_records=False,
                      observables=None) -> DistanceResult:
    """The estimate of the module docstring on the device.  model: an (H, L) pair, circuit text, a Circuit, .dem text or a DEM.  Trials
    0, 1, ... of `seed` run in batches of `batch` (default: eight launches' worth of trials in flight, at least 1024); the run stops after
    `trials`, after the first batch whose lightest weight is <= target, or after the first batch that ends past max_seconds -- only at
    batch boundaries, and `trials` of the result is what ran.  There is no CPU fall-back: without the library or a device this raises;
    `distance_mirror` is the CPU reference, called by name."""
    t0 = time.perf_counter()
    trials = int(trials)
    if trials < 1:
        raise ValueError("trials must be at least 1")
    if batch is not None and int(batch) < 1:
        raise ValueError("batch must be at least 1")
    if int(keep) < 0:
        raise ValueError("keep must not be negative")
    H, L = _matrices(model)
    m = prepare(H, L, observables)
    est = DistanceEstimator(m)
    try:
        batch = max(1024, 8 * est.info()["trials_in_flight"]) if batch is None else int(batch)
        parts, first, done = [], None, 0
        while done < trials:
            cnt = min(batch, trials - done)
            rec = est.run(seed, done, cnt)
            first = _lightest(rec, done, keep, first)
            if keep_records:
                parts.append(rec)
            done += cnt
            if target is not None and first is not None and first[0] <= int(target):
                break
            if max_seconds is not None and time.perf_counter() - t0 > float(max_seconds):
                break
        return _result(H, L, m, done, np.concatenate(parts) if keep_records else None, first, est.hist(), est.info()["rank"], seed, keep, t0)
    finally:
        est.close()


def estimate_code_distance(hx, hz, lx, lz, **kw):
    """(dx_result, dz_result) of a CSS code.  dx bounds the lightest X-type logical: a vector of ker hz that anticommutes with some row of
    lz, the model (hz, lz); dz the lightest Z-type logical: the model (hx, lx).  Keywords as `estimate_distance`; `observables` applies to
    both."""
    return estimate_distance((hz, lz), **kw), estimate_distance((hx, lx), **kw)
