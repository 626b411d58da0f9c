"""Crafted models that take the logical-fault search to the limits of its state record -- event sets of 5 to 8 detectors, faults of up to
16, detector 65534 of 65535, all 64 mask bits, a level of 65 536 and of 65 537 undetectable states, level 1 seeded in several chunks -- and,
on the numpy mirror alone, the proof that every model reaches the edge it is meant for.  tests/test_gpu_search_limits.py runs the same
models on the device and compares state by state.  No GPU and no fixture file: every model comes from a fixed seed."""
import time
import types

import numpy as np
import pytest
from scipy.sparse import csc_matrix

from quits_amd import search as ls

NDET = ls.MAX_DETECTORS                # every model has 65535 detectors, so 65534 is the last legal one
GROUP = 16                             # QD_SEARCH_GROUP: the lanes that stride over one row
# The detectors the crafted faults draw from: both ends of the 16-bit range, both sides of every byte boundary and of the sign bit.
POOL = np.array([0, 1, 2, 255, 256, 257, 4095, 4096, 16384, 21845, 32767, 32768, 32769, 32770, 43690, 49151, 49152, 61440, 65280, 65530,
                 65531, 65532, 65533, 65534])


def crafted(seed, n, degrees, hot, twins=False, weight=2.0):
    """(H, L): n faults, fault j flips degrees[j mod len] detectors of POOL (the first `hot` of a shuffled POOL are drawn `weight` times as
    often as the others, so rows are both longer and shorter than GROUP) and about half of 64 observables; row 63 is forced onto every
    third fault.  twins: two more faults, a copy of fault 0 with its mask and a copy of fault 1 with mask bit 32 flipped."""
    rng = np.random.default_rng(seed)
    p = np.ones(len(POOL))
    p[rng.permutation(len(POOL))[:hot]] = weight
    cols = [np.sort(rng.choice(POOL, size=degrees[j % len(degrees)], replace=False, p=p / p.sum())) for j in range(n)]
    obs = rng.random((64, n)) < 0.5
    obs[63, ::3] = True
    if twins:
        cols += [cols[0], cols[1]]
        obs = np.concatenate([obs, obs[:, :2]], axis=1)
        obs[32, -1] ^= True
    return _csc(cols, NDET), csc_matrix(obs.astype(np.uint8))


def _csc(cols, rows):
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    indices = np.concatenate(cols) if len(cols) else np.zeros(0, np.int64)
    return csc_matrix((np.ones(len(indices), np.uint8), indices, indptr), shape=(rows, len(cols)))


def line():
    """Nine detectors 65534, 65533, ..., 65526 in a line: a fault per adjacent pair, a fault of one detector at each end, the observable
    (row 63 of 64) on the first end.  The only undetectable logical fault is the whole line: ten faults."""
    top = NDET - 1
    cols = [np.array([top])] + [np.array([top - i - 1, top - i]) for i in range(8)] + [np.array([top - 8])]
    obs = np.zeros((64, len(cols)), np.uint8)
    obs[63, 0] = 1
    return _csc(cols, NDET), csc_matrix(obs)


def found_list(N):
    """One detector, fault 0 on it; faults 1 .. N without detectors, fault j with the mask j: N undetectable states in level 1."""
    j = np.arange(N + 1)
    return _csc([np.array([0])] + [np.zeros(0, np.int64)] * N, 1), csc_matrix(((j[None, :] >> np.arange(17)[:, None]) & 1).astype(np.uint8))


# name: (the model, the search's options, the edges asserted by test_model_reaches_its_edges)
RANDOM_EDGES = ("sizes", "deep", "high_first", "bit32", "rows", "chunks")
K8_DEGREES = [2, 3, 4, 6, 8, 16, 5, 7, 3, 4, 11, 2]
MODELS = {
    "k5": (lambda: crafted(7, 48, [1, 2, 3, 4, 5, 2, 3, 10], 3, twins=True), dict(max_event_set=5, max_fault_degree=10), RANDOM_EDGES + ("twins",)),
    "k6": (lambda: crafted(3, 54, [2, 3, 4, 5, 6, 3, 4, 12], 4), dict(max_event_set=6, max_fault_degree=12, max_weight=4), RANDOM_EDGES),
    "k7": (lambda: crafted(26, 54, [2, 3, 4, 5, 7, 6, 3], 4), dict(max_event_set=7, max_fault_degree=7, max_weight=3), RANDOM_EDGES),
    "k8": (lambda: crafted(5, 60, K8_DEGREES, 4), dict(max_event_set=8, max_fault_degree=16, max_weight=3), RANDOM_EDGES + ("degree16",)),
    "k8_no_increase": (lambda: crafted(5, 60, K8_DEGREES, 4), dict(max_event_set=8, max_fault_degree=16, max_weight=4, no_increase=True),
                       RANDOM_EDGES + ("degree16", "no_increase")),
    "line": (line, dict(max_event_set=2, max_fault_degree=2), ("line",)),
}
POOL_LIMIT = 4096                      # states of a model: what keeps the state-by-state comparison on the device to a second or two
_REFERENCE = {}


def columns(H, L):
    """Per fault the set of its detectors and its 64-bit mask, straight from the matrices (not through ls.prepare)."""
    H, L = csc_matrix(H), csc_matrix(L)
    dets = [frozenset(H.indices[H.indptr[j]:H.indptr[j + 1]].tolist()) for j in range(H.shape[1])]
    obs = [sum(1 << int(i) for i in L.indices[L.indptr[j]:L.indptr[j + 1]]) for j in range(L.shape[1])]
    return dets, obs


def state_of(ref, chain):
    """(S, o) of a parent chain: the xor of its faults' columns of H and of L."""
    S, o = set(), 0
    for j in chain:
        S ^= ref.dets[j]
        o ^= ref.obs[j]
    return tuple(sorted(S)), o


def reference(name):
    """The mirror's run of a model, computed once and shared: the matrices, the options, the SearchModel, the result, the engine with its
    pool, the bounds of every level in the pool and the set of (S, o) of every level."""
    if name not in _REFERENCE:
        make, opts, edges = MODELS[name]
        H, L = make()
        kw = dict(opts)
        max_weight = kw.pop("max_weight", None)
        m = ls.prepare(H, L, **kw)
        eng = ls._MirrorEngine(m, None)
        res = ls._drive(eng, m, max_weight, None, 16, time.perf_counter())
        bounds = np.concatenate([[0], np.cumsum(res.level_sizes)]).tolist()
        slots = ls._unpack(eng.pool["w0"], eng.pool["w1"])
        states = [(tuple(int(d) for d in row if d != ls.EMPTY), int(mask)) for row, mask in zip(slots, eng.pool["mask"])]
        dets, obs = columns(H, L)
        _REFERENCE[name] = types.SimpleNamespace(name=name, H=H, L=L, opts=opts, edges=edges, m=m, res=res, eng=eng, bounds=bounds, slots=slots,
                                                 states=states, dets=dets, obs=obs,
                                                 levels=[set(states[a:b]) for a, b in zip(bounds[:-1], bounds[1:])])
    return _REFERENCE[name]


# What the mirror gave for these seeds, frozen: (outcome, weight, level sizes).  The edges below are what is required of a model; these
# rows only say that it is still the same model.
FROZEN = {
    "k5": ("found", 2, [43, 170]),
    "k6": ("weight", None, [48, 177, 711, 2769]),
    "k7": ("weight", None, [54, 350, 2060]),
    "k8": ("weight", None, [50, 311, 1851]),
    "k8_no_increase": ("found", 4, [50, 116, 346, 1000]),
    "line": ("found", 10, [10, 9, 8, 7, 6, 5, 4, 3, 2, 1]),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_model_is_the_frozen_one(name):
    ref = reference(name)
    assert (ref.res.outcome, ref.res.weight, ref.res.level_sizes) == FROZEN[name]
    assert ref.H.shape[0] == NDET == 65535 and ref.L.shape[0] == 64
    assert ref.res.total_states == len(ref.eng.pool) <= POOL_LIMIT
    assert all(len(lv) == n for lv, n in zip(ref.levels, ref.res.level_sizes)), "a state twice in a level"
    assert len(set().union(*ref.levels)) == ref.res.total_states, "a state in two levels"


@pytest.mark.parametrize("name", list(MODELS))
def test_every_mirror_record_is_the_xor_of_its_chain(name):
    """Pins the mirror, the reference of the device tests: every pool record gives back its own (S, mask) from the columns of H and L along
    its parent chain, the chain is as long as the record's level, and every fault of it is admitted."""
    ref = reference(name)
    D = ref.m.D
    for level, (a, b) in enumerate(zip(ref.bounds[:-1], ref.bounds[1:]), start=1):
        for idx in range(a, b):
            chain = ref.eng.chain(idx)
            assert len(chain) == level
            assert all(1 <= len(ref.dets[j]) <= D for j in chain)
            assert state_of(ref, chain) == ref.states[idx]
            S = ref.states[idx][0]
            assert list(S) == sorted(set(S)) and len(S) <= ref.m.K and ref.states[idx] != ((), 0)


def check_edge(ref, edge):
    """Assert one of the edges a model is meant for, on the mirror's pool."""
    m, res, K = ref.m, ref.res, ref.m.K
    size = np.array([len(S) for S, _ in ref.states])
    masks = np.array([o for _, o in ref.states], dtype=np.uint64)
    first = np.array([S[0] if S else -1 for S, _ in ref.states])
    expanded = np.arange(len(size)) < ref.bounds[-2]                      # every level but the last was expanded
    degree = np.array([len(d) for d in ref.dets])
    admitted = (degree >= 1) & (degree <= m.D)
    if edge == "top":               # the last legal detector and the last mask bit
        assert any(d == 65534 for S, _ in ref.states for d in S), "no state holds detector 65534"
        assert (masks >> np.uint64(63)).any(), "no mask has bit 63"
    elif edge == "sizes":           # every size of an event set, the largest often
        assert all((size == k).any() for k in range(1, K + 1)) and (size == K).sum() >= 16
    elif edge == "deep":            # expanded states with a second word: removals and insertions cross the w0 / w1 boundary, the cut at K
        assert (expanded & (size >= 5)).any() and (expanded & (size == K)).any()
    elif edge == "high_first":      # min(S) with the top bit set, as a row index and in the 16-bit comparisons
        assert (expanded & (first >= 32768)).any()
    elif edge == "bit32":
        assert ((masks >> np.uint64(32)) & np.uint64(1)).any(), "no mask has bit 32"
    elif edge == "rows":            # lanes of a group with two faults, one fault and none, on rows that are expanded
        rows = np.diff(m.row_ptr)[first[expanded & (first >= 0)]]
        assert rows.max() > GROUP and 0 < rows.min() < GROUP
    elif edge == "chunks":          # stage_states = max_row seeds level 1 in at least three chunks
        assert m.n > m.max_row > GROUP and len(ls.level_one(m)) > 2 * m.max_row
    elif edge == "degree16":        # an admitted fault of 16 detectors, and a state that came by one
        assert m.D == 16 and (degree[admitted] == 16).any()
        assert (degree[ref.eng.pool["fault"][ref.bounds[1]:].astype(np.int64)] == 16).any(), "no state came by a fault of 16"
    elif edge == "twins":           # a pair of faults that cancels to (empty, 0) and a pair that is a weight-2 logical fault
        n = m.n
        assert ref.dets[n - 2] == ref.dets[0] and ref.obs[n - 2] == ref.obs[0]
        assert ref.dets[n - 1] == ref.dets[1] and ref.obs[n - 1] ^ ref.obs[1] == 1 << 32
        assert res.outcome == "found" and res.weight == 2 and 1 << 32 in res.logical_masks
        seeds = ls.level_one(m)["fault"].tolist()           # seeded in chunks of max_row, the copy of fault 0 meets a pool record of an earlier chunk
        assert seeds.index(n - 2) // m.max_row > seeds.index(0) // m.max_row and len(seeds) == res.level_sizes[0] + 1
    elif edge == "no_increase":     # the rule changes the levels after the first
        free = ls.search_mirror(ref.H, ref.L, **{k: v for k, v in ref.opts.items() if k != "no_increase"})
        assert free.level_sizes[0] == res.level_sizes[0] and free.level_sizes[1:] != res.level_sizes[1:]
    elif edge == "line":            # (empty, 1 << 63) appears by cancellation at the deepest level, from detectors 65526 .. 65534
        assert (res.outcome, res.weight, res.logical_masks) == ("found", 10, [1 << 63])
        assert [w.tolist() for w in res.witnesses] == [list(range(10))]
        assert first[expanded].min() == 65526 and (size == 2).sum() >= 16
    else:
        raise AssertionError("no such edge: " + edge)


@pytest.mark.parametrize("name", list(MODELS))
def test_model_reaches_its_edges(name):
    ref = reference(name)
    for edge in ("top",) + ref.edges:
        check_edge(ref, edge)


@pytest.mark.parametrize("N", [65536, 65537])
def test_found_list_models_hold_n_undetectable_states_in_level_one(N):
    H, L = found_list(N)
    res = ls.search_mirror(H, L, keep=2)
    assert (res.outcome, res.weight, res.level_sizes) == ("found", 1, [N + 1])
    assert res.logical_masks == list(range(1, N + 1)) and [w.tolist() for w in res.witnesses] == [[1], [2]]
    assert (N == ls.FOUND_CAP) or (N == ls.FOUND_CAP + 1)


def sixty_five_observables():
    """The k7 model with a 65th observable on every second fault, and the selection of rows 1 .. 64 of it: row 64 is mask bit 63."""
    from scipy.sparse import vstack
    H, L = MODELS["k7"][0]()
    extra = np.zeros((1, L.shape[1]), np.uint8)
    extra[0, ::2] = 1
    return H, csc_matrix(vstack([L, csc_matrix(extra)])), list(range(1, 65))


def test_sixty_five_observables_need_a_selection():
    H, L, rows = sixty_five_observables()
    opts = MODELS["k7"][1]
    with pytest.raises(ValueError, match="pass a selection"):
        ls.search_mirror(H, L, **opts)
    res = ls.search_mirror(H, L, observables=rows, **opts)
    assert res.observables == rows and res.outcome == "weight" and res.level_sizes[0] == FROZEN["k7"][2][0]
    m = ls.prepare(H, L, opts["max_event_set"], opts["max_fault_degree"], observables=rows)
    dets, obs = columns(H, L)
    assert [int(o) for o in m.fault_obs] == [o >> 1 for o in obs] and any(o >> 64 for o in obs)      # row 0 is dropped, row 64 is bit 63
