"""A directed search for light undetectable logical faults: a breadth-first search over small detection-event sets with a visited set.  It
needs no decoder and no sampling; what it finds certifies itself (H e = 0, L e != 0) and bounds the circuit-level distance from above.

This is Stim's hypergraph search (`search_for_undetectable_logical_errors`) restated from memory and FIXED HERE: where Stim differs, this
text decides.  Host side, numpy only: the definition, the result record and `search_mirror`, the CPU reference of the kernels
(csrc/logical_search.hip, `LogicalSearcher`), which must produce the same level sizes, outcome and logical masks.

The definition.  H (detectors x faults) and L (observables x faults) have the columns of detector_error_model_to_matrix (merged faults);
priors are not used.  dets(j) is the support of column j of H, obs(j) the mask of the SEARCHED observables column j of L flips (bit i =
the i-th searched observable; `observables` selects at most 64 rows of L, default all of them).

  parameters   max_event_set K (1 .. 8, default 6), max_fault_degree D (1 .. 16, default 6), no_increase (Stim's
               dont_explore_edges_increasing_symptom_degree), max_weight, max_states, keep (witnesses returned), observables.
  limits       at most 65535 detectors and at most 64 searched observables: ValueError beyond.
  admitted     fault j is admitted iff 1 <= |dets(j)| <= D.  A fault without detectors and with obs(j) != 0 is an undetectable logical
               fault of weight 1: it enters level 1 as the state (empty, obs(j)) and the result is `found` at level 1.  A fault without
               detectors and with obs(j) = 0 is ignored.
  states       (S, o): S a sorted set of at most K detectors, o a mask.  (empty, 0) is never a state.
  level 1      the distinct (dets(j), obs(j)) over admitted faults with |dets(j)| <= K (and the weight-1 states above).
  level l + 1  for every level-l state with S != empty and every admitted fault j that contains min(S): S' = S xor dets(j),
               o' = o xor obs(j); dropped if |S'| > K, if no_increase and |S'| > |S|, if (S', o') = (empty, 0), or if the state already
               belongs to a level <= l + 1.  So level sizes are properties of the input, not of the traversal order.
  stop rules   checked after each whole level l, in this order:
               1. the running total of distinct states exceeds max_states: the level is discarded, outcome `capacity`,
                  levels_completed = l - 1 (a level completes IFF the total through it is at most max_states);
               2. the level holds states (empty, o != 0): outcome `found`, weight = l, logical_masks = every such o, ascending;
               3. the level is empty: outcome `space` (the truncated space holds no undetectable logical fault), levels_completed = l - 1;
               4. l = max_weight: outcome `weight`.
  witnesses    for each of the first `keep` masks the parents are followed back to level 1; the faults of odd multiplicity, ascending,
               are the witness e: H e = 0, L[observables] e = o, every fault admitted (or the detector-less fault of a weight-1 result),
               len(e) <= weight and len(e) = weight (mod 2).

Which parent a state keeps when several reach it at the same level is NOT fixed: the witness may differ between the mirror and the device,
and between two runs on the device.  Every other field of the result is deterministic.

`capacity` and `weight` say nothing about the distance; `space` says there is no undetectable logical fault INSIDE THE TRUNCATED SPACE
(event sets of at most K detectors, faults of at most D), which is not a lower bound on the distance either.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import time

import numpy as np

MAX_EVENT_SET, MAX_FAULT_DEGREE, MAX_DETECTORS, MAX_OBSERVABLES = 8, 16, 65535, 64
EMPTY = 0xFFFF                          # an empty detector slot of a state record
NO_PARENT = 0xFFFFFFFF                  # the parent index of a level-1 state
RECORD_BYTES = 32                       # QD_SEARCH_RECORD: two words of eight 16-bit detectors, the mask, parent and fault
RECORD = np.dtype([("w0", "<u8"), ("w1", "<u8"), ("mask", "<u8"), ("parent", "<u4"), ("fault", "<u4")])
SEARCH_POOL, SEARCH_TABLE, SEARCH_STAGE, SEARCH_FOUND = 1, 2, 4, 8       # QD_SEARCH_OVER_*: the overflow flags of the counters
FOUND_CAP = 1 << 16                     # (empty, o) states a level can report
DEFAULT_STAGE = 1 << 23                 # staged candidates per chunk (40 bytes each)


@dataclasses.dataclass
class LogicalSearchResult:
    """What a search returns.  outcome: 'found', 'space', 'capacity' or 'weight' (the stop rules of the module docstring); weight: the level
    of a `found` result, else None; levels_completed, level_sizes, total_states: the completed levels; logical_masks: every mask of the found
    level, ascending (bit i = the i-th searched observable); witnesses: int64 arrays of fault indices, one per mask of the first `keep`;
    the limits used (max_event_set, max_fault_degree, no_increase, max_weight, max_states, observables); candidates: per completed level,
    the (state, fault) pairs that passed the size tests and were looked up in the visited set (None from the mirror); seconds."""
    outcome: str
    weight: int | None
    levels_completed: int
    level_sizes: list
    total_states: int
    logical_masks: list
    witnesses: list
    max_event_set: int
    max_fault_degree: int
    no_increase: bool
    max_weight: int | None
    max_states: int | None
    observables: list
    candidates: list | None = None
    seconds: float = 0.0

    def to_json(self) -> dict:
        d = dataclasses.asdict(self)
        d["witnesses"] = [[int(j) for j in w] for w in self.witnesses]
        d["logical_masks"] = [int(m) for m in self.logical_masks]
        return d


@dataclasses.dataclass
class SearchModel:
    """The tables both engines read.  n, ndet; K, D; fault_dets uint16 [n, D] (sorted, EMPTY-padded; all EMPTY for a fault that is not
    admitted); fault_obs uint64 [n]; row_ptr int64 [ndet + 1], row_faults int32: the admitted faults of every detector, ascending (CSR);
    free_logicals: the faults without detectors and with a non-zero mask; observables: the searched rows of L."""
    n: int
    ndet: int
    K: int
    D: int
    no_increase: bool
    fault_dets: np.ndarray
    fault_obs: np.ndarray
    row_ptr: np.ndarray
    row_faults: np.ndarray
    free_logicals: np.ndarray
    observables: list

    @property
    def max_row(self) -> int:
        return int(np.diff(self.row_ptr).max()) if self.ndet else 0


def _matrices(model):
    """(H, L) as scipy csc matrices from an (H, L) pair, circuit text, a Circuit, .dem text or a DEM."""
    from scipy.sparse import csc_matrix
    if isinstance(model, (tuple, list)) and len(model) == 2:
        H, L = model
    else:
        from .decoder.base import detector_error_model_to_matrix
        H, L, _ = detector_error_model_to_matrix(model)
    H, L = csc_matrix(H), csc_matrix(L)
    if H.shape[1] != L.shape[1]:
        raise ValueError("H has %d columns and L %d: both must have one column per fault" % (H.shape[1], L.shape[1]))
    return H, L


def prepare(H, L, max_event_set=6, max_fault_degree=6, no_increase=False, observables=None) -> SearchModel:
    """Check the limits and lay out the tables of the module docstring."""
    K, D = int(max_event_set), int(max_fault_degree)
    if not 1 <= K <= MAX_EVENT_SET:
        raise ValueError("max_event_set = %d is outside 1 .. %d" % (K, MAX_EVENT_SET))
    if not 1 <= D <= MAX_FAULT_DEGREE:
        raise ValueError("max_fault_degree = %d is outside 1 .. %d" % (D, MAX_FAULT_DEGREE))
    H, L = _matrices((H, L))
    ndet, n = H.shape
    if ndet > MAX_DETECTORS:
        raise ValueError("%d detectors: the search holds at most %d (16-bit detector slots)" % (ndet, MAX_DETECTORS))
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
        raise ValueError("the model has %d detectors and %d faults: nothing to search" % (ndet, n))
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
    deg = np.diff(Hc.indptr)
    admitted = (deg >= 1) & (deg <= D)
    fault_dets = np.full((n, D), EMPTY, np.uint16)
    for j in np.flatnonzero(admitted):
        fault_dets[j, :deg[j]] = Hc.indices[Hc.indptr[j]:Hc.indptr[j + 1]]
    Hr = Hc[:, np.flatnonzero(admitted)].tocsr()
    Hr.sort_indices()
    row_faults = np.flatnonzero(admitted)[Hr.indices].astype(np.int32)
    free = np.flatnonzero((deg == 0) & (fault_obs != 0))
    return SearchModel(n, ndet, K, D, bool(no_increase), fault_dets, fault_obs, Hr.indptr.astype(np.int64), row_faults, free, observables)


def level_one(m: SearchModel) -> np.ndarray:
    """The level-1 candidates as records (duplicates included: the visited set removes them): (dets(j), obs(j)) of every admitted fault of
    at most K detectors, and (empty, obs(j)) of every detector-less fault with a non-zero mask."""
    deg = (m.fault_dets != EMPTY).sum(axis=1)
    js = np.concatenate([np.flatnonzero((deg >= 1) & (deg <= m.K)), m.free_logicals]).astype(np.int64)
    slots = np.full((len(js), 8), EMPTY, np.uint16)
    w = min(m.D, 8)
    slots[:, :w] = m.fault_dets[js, :w]
    rec = np.zeros(len(js), RECORD)
    rec["w0"], rec["w1"] = _pack(slots)
    rec["mask"], rec["parent"], rec["fault"] = m.fault_obs[js], NO_PARENT, js
    return rec


def _pack(slots):
    s = np.ascontiguousarray(slots, dtype="<u2")
    w = s.view("<u8")
    return w[:, 0].copy(), w[:, 1].copy()


def _unpack(w0, w1):
    w = np.empty((len(w0), 2), "<u8")
    w[:, 0], w[:, 1] = w0, w1
    return w.view("<u2")


def witness_of(chain) -> np.ndarray:
    """The faults of odd multiplicity in a parent chain, ascending."""
    f, c = np.unique(np.asarray(chain, dtype=np.int64), return_counts=True)
    return f[c % 2 == 1]


def check_witness(H, L, e, mask, observables, weight, max_fault_degree) -> None:
    """Raise AssertionError unless `e` meets the witness contract of the module docstring."""
    H, L = _matrices((H, L))
    e = np.asarray(e, dtype=np.int64)
    assert len(e) and np.all(np.diff(e) > 0) and e[0] >= 0 and e[-1] < H.shape[1], "faults must be distinct, ascending and in range"
    x = np.zeros(H.shape[1], np.int64)
    x[e] = 1
    assert not ((H @ x) % 2).any(), "H e != 0"
    lo = np.asarray((L @ x) % 2).reshape(-1)
    got = sum(int(lo[i]) << bit for bit, i in enumerate(observables))
    assert got == int(mask) and got != 0, "L e = %#x, expected %#x" % (got, int(mask))
    deg = np.diff(H.tocsc().indptr)[e]
    assert np.all(deg <= max_fault_degree) and (np.all(deg >= 1) or weight == 1), "a fault of the witness is not admitted"
    assert len(e) <= weight and (weight - len(e)) % 2 == 0, "len(e) = %d against weight %d" % (len(e), weight)


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------
class _MirrorEngine:
    """The breadth-first search in numpy: the pool is an array of records in level order, the visited set the lexicographically sorted keys."""

    PAIRS = 1 << 22              # (state, fault) pairs expanded at a time

    def __init__(self, m: SearchModel, max_states):
        self.m, self.max_states = m, max_states
        self.pool = np.zeros(0, RECORD)
        self.keys = np.zeros((0, 3), np.uint64)          # sorted keys of the pool
        self.frontier = (0, 0)
        self.candidates = None

    @staticmethod
    def _keys(rec):
        return np.stack([rec["w0"], rec["w1"], rec["mask"]], axis=1)

    def _new(self, rec):
        """The records of `rec` whose state is neither in the pool nor earlier in `rec`."""
        if not len(rec):
            return rec
        k = self._keys(rec)
        order = np.lexsort((k[:, 2], k[:, 1], k[:, 0]))
        ks = k[order]
        first = np.ones(len(ks), bool)
        first[1:] = (ks[1:] != ks[:-1]).any(axis=1)
        rec, k = rec[order[first]], ks[first]
        allk = np.concatenate([self.keys, k])
        src = np.concatenate([np.zeros(len(self.keys), bool), np.ones(len(k), bool)])
        order = np.lexsort((allk[:, 2], allk[:, 1], allk[:, 0]))
        allk, src = allk[order], src[order]
        eq = np.zeros(len(allk), bool)
        eq[1:] = (allk[1:] == allk[:-1]).all(axis=1)
        dup = eq.copy()
        dup[:-1] |= eq[1:]
        self.keys = allk[~(src & dup)]
        return rec[~dup[src]]            # (src rows keep the order of k, which is sorted)

    def _append(self, parts):
        """Close a level: True (and the pool grows) iff the total stays within max_states."""
        new = np.concatenate(parts) if parts else np.zeros(0, RECORD)
        if self.max_states is not None and len(self.pool) + len(new) > self.max_states:
            return None
        self.frontier = (len(self.pool), len(self.pool) + len(new))
        self.pool = np.concatenate([self.pool, new])
        return len(new)

    def start(self):
        return self._append([self._new(level_one(self.m))])

    def step(self):
        m = self.m
        lo, hi = self.frontier
        parts = []
        rowlen = np.diff(m.row_ptr)
        pos = lo
        while pos < hi:
            # a chunk of states whose rows hold about PAIRS faults
            first = _unpack(self.pool["w0"][pos:hi], self.pool["w1"][pos:hi])[:, 0]
            cnt = np.where(first != EMPTY, rowlen[np.minimum(first, m.ndet - 1)], 0)
            take = max(1, int(np.searchsorted(np.cumsum(cnt), self.PAIRS, side="right")))
            cnt = cnt[:take]
            st = self.pool[pos:pos + take]
            slots = _unpack(st["w0"], st["w1"])
            ps = np.repeat(np.arange(take), cnt)
            off = np.arange(len(ps)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            pf = m.row_faults[m.row_ptr[np.minimum(first[:take], m.ndet - 1)][ps] + off].astype(np.int64)
            a = np.concatenate([slots[ps], m.fault_dets[pf]], axis=1)
            a.sort(axis=1)
            eq = (a[:, 1:] == a[:, :-1]) & (a[:, 1:] != EMPTY)
            a[:, 1:][eq] = EMPTY
            a[:, :-1][eq] = EMPTY
            a.sort(axis=1)
            size = (a != EMPTY).sum(axis=1)
            mask = st["mask"][ps] ^ m.fault_obs[pf]
            keep = (size <= m.K) & ~((size == 0) & (mask == 0))
            if m.no_increase:
                keep &= size <= (slots != EMPTY).sum(axis=1)[ps]
            rec = np.zeros(int(keep.sum()), RECORD)
            rec["w0"], rec["w1"] = _pack(a[keep][:, :8])
            rec["mask"], rec["parent"], rec["fault"] = mask[keep], (pos + ps)[keep], pf[keep]
            parts.append(self._new(rec))
            pos += take
        return self._append(parts)

    def found(self):
        lo, hi = self.frontier
        lvl = self.pool[lo:hi]
        idx = np.flatnonzero((lvl["w0"] == np.uint64(0xFFFFFFFFFFFFFFFF)) & (lvl["w1"] == np.uint64(0xFFFFFFFFFFFFFFFF)))
        return [(int(lvl["mask"][i]), lo + int(i)) for i in idx]

    def chain(self, idx):
        out = []
        while idx != NO_PARENT:
            out.append(int(self.pool["fault"][idx]))
            idx = int(self.pool["parent"][idx])
        return out

    def close(self):
        pass


def _drive(engine, m: SearchModel, max_weight, max_states, keep, t0) -> LogicalSearchResult:
    """The host loop of both engines: one level per call, the stop rules in the order of the module docstring."""
    sizes, total, level = [], 0, 0
    outcome, weight, masks, witnesses = None, None, [], []
    while outcome is None:
        level += 1
        new = engine.start() if level == 1 else engine.step()
        if new is None:
            outcome = "capacity"
            break
        found = engine.found()
        if found:
            sizes.append(new)
            total += new
            outcome, weight = "found", level
            found.sort()
            masks = [f[0] for f in found]
            witnesses = [witness_of(engine.chain(idx)) for _, idx in found[:max(0, int(keep))]]
            break
        if new == 0:
            outcome = "space"
            break
        sizes.append(new)
        total += new
        if max_weight is not None and level >= max_weight:
            outcome = "weight"
    cand = getattr(engine, "candidates", None)
    return LogicalSearchResult(outcome, weight, len(sizes), sizes, total, masks, witnesses, m.K, m.D, m.no_increase,
                               None if max_weight is None else int(max_weight), None if max_states is None else int(max_states),
                               list(m.observables), None if cand is None else list(cand[:len(sizes)]), time.perf_counter() - t0)


def _check_run_limits(max_weight, max_states, keep):
    if max_weight is not None and int(max_weight) < 1:
        raise ValueError("max_weight must be at least 1")
    if max_states is not None and int(max_states) < 1:
        raise ValueError("max_states must be at least 1")
    if int(keep) < 0:
        raise ValueError("keep must not be negative")


def search_mirror(H, L, max_event_set=6, max_fault_degree=6, no_increase=False, max_weight=None, max_states=None, keep=16,
                  observables=None) -> LogicalSearchResult:
    """The definition of the module docstring in numpy: the CPU reference of the kernels.  max_states=None: no limit."""
    t0 = time.perf_counter()
    _check_run_limits(max_weight, max_states, keep)
    m = prepare(H, L, max_event_set, max_fault_degree, no_increase, observables)
    return _drive(_MirrorEngine(m, None if max_states is None else int(max_states)), m, max_weight, max_states, keep, t0)


# ---- the device ---------------------------------------------------------------------------------------------------------------------------
def _pow2_at_least(x: int) -> int:
    return 1 << max(0, int(x) - 1).bit_length()


def default_table_size(max_states: int, stage_states: int = DEFAULT_STAGE) -> int:
    """Slots of the visited table: the power of two that keeps it at most half full.  It holds the pool's states and the winners of the
    chunk in flight, so a level that overflows the pool never fills the table first."""
    return _pow2_at_least(2 * (int(max_states) + int(stage_states)))


def search_memory_bytes(max_states, table_size=None, stage_states=DEFAULT_STAGE) -> int:
    """What a search of `max_states` states allocates on the device: the pool (32 bytes a state), the visited table (4 bytes a slot) and
    the staging area of a chunk (a record and its table slot: 40 bytes a candidate), plus the list of found states.  The model's own
    tables (a few hundred kilobytes) come on top."""
    table_size = default_table_size(max_states, stage_states) if table_size is None else int(table_size)
    return RECORD_BYTES * int(max_states) + 4 * table_size + (RECORD_BYTES + 8) * int(stage_states) + 4 * FOUND_CAP


def default_max_states(free_bytes, stage_states=DEFAULT_STAGE) -> int:
    """The largest max_states whose search_memory_bytes is at most half of `free_bytes` (and whose pool indices stay 32-bit)."""
    budget = int(free_bytes) // 2
    hi = min(budget // RECORD_BYTES, NO_PARENT - 1 - int(stage_states))
    lo = 0
    while lo < hi:                                       # search_memory_bytes is monotone in max_states
        mid = (lo + hi + 1) // 2
        if search_memory_bytes(mid, None, stage_states) <= budget:
            lo = mid
        else:
            hi = mid - 1
    if lo < 1:
        raise RuntimeError("quits_amd: %d free bytes on the device do not hold a search" % int(free_bytes))
    return lo


class LogicalSearcher:
    """The search on the device (csrc/logical_search.hip): a pool of state records in level order, an open-addressing table of pool
    indices, a staging area per chunk of the frontier.  Everything is allocated here, before any launch: a failed allocation raises.
    table_size (a power of two) and chunk_states (frontier states per chunk) are for tests; stage_states sizes the staging area."""

    def __init__(self, m: SearchModel, max_states, table_size=None, chunk_states=None, stage_states=None, device=None):
        from . import _lib
        import torch
        self.L = _lib.require_search(_lib.require_gpu())
        self.m, self.max_states = m, int(max_states)
        self.device = torch.cuda.current_device() if device is None else int(device)
        max_row = max(1, m.max_row)
        if stage_states is None:
            stage_states = DEFAULT_STAGE if chunk_states is None else min(DEFAULT_STAGE, max(1024, int(chunk_states) * max_row))
        self.stage_states = max(int(stage_states), max_row, 1)
        self.chunk_states = max(1, self.stage_states // max_row) if chunk_states is None else int(chunk_states)
        if self.chunk_states < 1 or self.chunk_states * max_row > self.stage_states:
            raise ValueError("chunk_states = %d times the longest row (%d faults) exceeds the %d staged candidates" % (self.chunk_states, max_row, self.stage_states))
        self.table_size = default_table_size(self.max_states, self.stage_states) if table_size is None else int(table_size)
        if self.table_size < 2 or self.table_size & (self.table_size - 1):
            raise ValueError("table_size must be a power of two")
        if self.max_states + self.stage_states > NO_PARENT - 1:
            raise ValueError("max_states = %d: pool and staging indices must stay below 2^32 - 2" % self.max_states)
        self.bytes = search_memory_bytes(self.max_states, self.table_size, self.stage_states)
        self.h = C.c_void_p()
        row_ptr = np.ascontiguousarray(m.row_ptr, dtype=np.int64)
        row_faults = np.ascontiguousarray(m.row_faults, dtype=np.int32)
        fd = np.ascontiguousarray(m.fault_dets, dtype=np.uint16)
        fo = np.ascontiguousarray(m.fault_obs, dtype=np.uint64)
        _lib.check(self.L.qd_search_create(m.ndet, m.n, row_ptr.ctypes.data, row_faults.ctypes.data, fd.ctypes.data, fo.ctypes.data, m.K, m.D,
                                           int(m.no_increase), self.max_states, self.table_size, self.stage_states, self.device, C.byref(self.h)))
        self.candidates = []
        self._seen = 0
        self._frontier = (0, 0)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.qd_search_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def reset(self):
        from . import _lib
        _lib.check(self.L.qd_search_reset(self.h))
        self.candidates, self._seen, self._frontier = [], 0, (0, 0)

    def counters(self):
        from . import _lib
        c = np.zeros(8, np.uint64)
        _lib.check(self.L.qd_search_counters(self.h, c.ctypes.data))
        return {"pool": int(c[0]), "staged": int(c[1]), "found": int(c[2]), "flags": int(c[3]), "candidates": int(c[4])}

    def _close_level(self):
        c = self.counters()
        if c["flags"] & ~SEARCH_POOL:
            what = [name for bit, name in ((SEARCH_TABLE, "the visited table is full (%d slots)" % self.table_size),
                                           (SEARCH_STAGE, "the staging area overflowed (%d candidates)" % self.stage_states),
                                           (SEARCH_FOUND, "more than %d undetectable logical states in one level" % FOUND_CAP)) if c["flags"] & bit]
            raise RuntimeError("quits_amd: logical search: " + "; ".join(what))
        if c["flags"] & SEARCH_POOL or c["pool"] > self.max_states:
            return None
        new = c["pool"] - self._frontier[1]
        self._frontier = (self._frontier[1], c["pool"])
        self.candidates.append(c["candidates"] - self._seen)
        self._seen = c["candidates"]
        return new

    def start(self):
        from . import _lib
        rec = np.ascontiguousarray(level_one(self.m))
        _lib.check(self.L.qd_search_seed(self.h, rec.ctypes.data, len(rec), None))
        return self._close_level()

    def step(self):
        from . import _lib
        _lib.check(self.L.qd_search_level(self.h, self.chunk_states, None))
        return self._close_level()

    def found(self):
        from . import _lib
        nf = self.counters()["found"]
        if not nf:
            return []
        masks, idx = np.zeros(nf, np.uint64), np.zeros(nf, np.uint32)
        _lib.check(self.L.qd_search_found(self.h, nf, masks.ctypes.data, idx.ctypes.data))
        return [(int(a), int(b)) for a, b in zip(masks, idx)]

    def chain(self, idx):
        from . import _lib
        cap = len(self.candidates) + 1
        faults, n = np.zeros(cap, np.int32), C.c_int32(0)
        _lib.check(self.L.qd_search_chain(self.h, int(idx), cap, faults.ctypes.data, C.byref(n)))
        return faults[:n.value].tolist()


def find_undetectable_logical_errors(model, max_event_set=6, max_fault_degree=6, no_increase=False, max_weight=None, max_states=None,
                                     keep=16, observables=None, table_size=None, chunk_states=None) -> LogicalSearchResult:
    """The search of the module docstring on the device.  model: an (H, L) pair, circuit text, a Circuit, .dem text or a DEM.  max_states
    defaults to the largest value for which `search_memory_bytes` is at most half of the device's free memory.  table_size and
    chunk_states are for tests (a small table makes long probe chains, a small chunk splits a level's duplicates over several chunks).
    There is no CPU fall-back: without the library or a device this raises; `search_mirror` is the CPU reference, called by name."""
    t0 = time.perf_counter()
    _check_run_limits(max_weight, max_states, keep)
    H, L = _matrices(model)
    m = prepare(H, L, max_event_set, max_fault_degree, no_increase, observables)
    from . import _lib
    _lib.require_search(_lib.require_gpu())
    if max_states is None:
        import torch
        max_states = default_max_states(torch.cuda.mem_get_info()[0])
    eng = LogicalSearcher(m, max_states, table_size, chunk_states)
    try:
        return _drive(eng, m, max_weight, max_states, keep, t0)
    finally:
        eng.close()
