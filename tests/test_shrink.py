"""quits_amd.shrink on the host: the mirror of the fault-set shrinker against brute force and against its own definition, the edge cases, and
the library's new entry points (no GPU needed to see that they are there)."""
import itertools

import numpy as np
import pytest

from quits_amd import shrink


def _monotone(T):
    """Fails iff the set holds at least two members of T: a superset of a failing set fails."""
    return lambda rows: (np.asarray(rows, bool)[:, T].sum(axis=1) >= 2)


def _mod3(rows):
    """Fails iff the sum of the members is no multiple of 3: not monotone."""
    rows = np.asarray(rows, bool)
    return (rows * np.arange(rows.shape[1])[None, :]).sum(axis=1) % 3 != 0


def _children(s):
    members = np.flatnonzero(s)
    rows = np.repeat(s[None, :], members.size, axis=0)
    rows[np.arange(members.size), members] = False
    return rows


@pytest.mark.parametrize("n", [1, 2, 5, 9, 12])
def test_mirror_finds_a_minimal_failing_subset_of_a_monotone_predicate(n):
    """Every subset of n <= 12 faults as a parent: a failing parent ends on a failing subset of itself none of whose proper subsets fails
    (enumerated), a parent that does not fail stays as it is."""
    rng = np.random.default_rng(n)
    T = np.flatnonzero(rng.random(n) < 0.6)
    fails = _monotone(T)
    parents = np.array(list(itertools.product([False, True], repeat=n)), dtype=bool)
    if n == 12:
        parents = parents[rng.choice(parents.shape[0], 300, replace=False)]
    res = shrink.shrink_mirror(parents, fails)
    want = fails(parents)
    assert np.array_equal(res.fails, want) and np.array_equal(res.minimal, want)
    assert np.array_equal(res.sets[~want], parents[~want]) and (res.trials[~want] == 1).all()
    assert not (res.sets & ~parents).any() and np.array_equal(res.weight, res.sets.sum(axis=1)) and np.array_equal(res.start_weight, parents.sum(axis=1))
    assert (res.trials <= shrink.trial_bound(res.start_weight)).all()
    for s in res.sets[want]:
        assert fails(s[None, :])[0]
        members = np.flatnonzero(s)
        for r in range(members.size):                               # brute force: no proper subset fails
            for sub in itertools.combinations(members, r):
                t = np.zeros(n, bool)
                t[list(sub)] = True
                assert not fails(t[None, :])[0]
        assert s.sum() == 2                                         # ... which here means exactly two members of T


def test_mirror_on_a_predicate_that_is_not_monotone():
    """sum of members % 3 != 0: the result fails and none of its children does; the trials stay within the bound; every trial removes the next
    member in cyclic order, replayed here from the log alone."""
    rng = np.random.default_rng(5)
    n = 40
    parents = rng.random((60, n)) < 0.3
    res, log = shrink.shrink_mirror(parents, _mod3, rounds=True)
    start = _mod3(parents)
    assert np.array_equal(res.fails, start) and np.array_equal(res.minimal, start)
    assert (res.trials <= shrink.trial_bound(parents.sum(axis=1))).all() and res.trials.sum() == sum(p.size for p, _ in log)
    for s, f in zip(res.sets, res.fails):
        assert shrink.is_one_minimal(s, _mod3) == bool(f)
        if f:
            assert _mod3(s[None, :])[0] and not _mod3(_children(s)).any()
    S = parents.copy()
    last = np.full(parents.shape[0], -1)
    for r, (par, flt) in enumerate(log):
        assert np.array_equal(par, np.sort(par))
        if r == 0:
            assert np.array_equal(par, np.arange(parents.shape[0])) and (flt == -1).all()
            continue
        for p, j in zip(par, flt):
            members = np.flatnonzero(S[p])
            above = members[members > last[p]]
            assert j == (above[0] if above.size else members[0]), "parent %d, round %d" % (p, r)
            t = S[p].copy()
            t[j] = False
            if _mod3(t[None, :])[0]:
                S[p] = t
            last[p] = j
    assert np.array_equal(S, res.sets)


def test_edge_cases():
    """The empty set, a singleton, a parent that does not fail, and members in the last word only (the search wraps)."""
    n = 70
    always = lambda rows: np.ones(len(rows), bool)
    never = lambda rows: np.zeros(len(rows), bool)
    empty = np.zeros((1, n), bool)
    r = shrink.shrink_mirror(empty, always)
    assert r.fails[0] and r.minimal[0] and r.trials[0] == 1 and r.weight[0] == 0
    r = shrink.shrink_mirror(empty, never)
    assert not r.fails[0] and not r.minimal[0] and r.trials[0] == 1
    single = np.zeros((1, n), bool)
    single[0, 33] = True
    r = shrink.shrink_mirror(single, lambda rows: np.asarray(rows)[:, 33])          # fails only with fault 33
    assert r.fails[0] and r.minimal[0] and r.trials[0] == 2 and r.sets[0, 33] and r.weight[0] == 1
    r = shrink.shrink_mirror(single, always)                                         # fails without it too
    assert r.minimal[0] and r.trials[0] == 2 and r.weight[0] == 0
    quiet = np.zeros((1, n), bool)
    quiet[0, [3, 9]] = True
    r = shrink.shrink_mirror(quiet, never)
    assert not r.fails[0] and np.array_equal(r.sets, quiet) and r.trials[0] == 1
    tail = np.zeros((1, n), bool)
    tail[0, [64, 66, 69]] = True
    wrap = lambda rows: np.asarray(rows)[:, 69] & ~(np.asarray(rows)[:, 66] & ~np.asarray(rows)[:, 64])       # 69, but not 66 without 64
    res, log = shrink.shrink_mirror(tail, wrap, rounds=True)
    assert [int(f[0]) for _, f in log] == [-1, 64, 66, 69, 64, 69] and res.minimal[0]
    assert np.flatnonzero(res.sets[0]).tolist() == [69] and res.trials[0] == 6
    assert shrink.trial_bound(3) == 7
    with pytest.raises(ValueError):
        shrink.shrink_mirror(np.zeros(4, bool), always)


def test_pack_and_unpack():
    rng = np.random.default_rng(0)
    for n in (1, 31, 32, 33, 65):
        bits = rng.random((5, n)) < 0.5
        w = shrink.pack_sets(bits)
        assert w.dtype == np.int32 and w.shape == (5, (n + 31) // 32) and np.array_equal(shrink.unpack_sets(w, n), bits)
        assert np.array_equal(shrink.unpack_sets(shrink.pack_sets(bits, 4), n), bits)
    with pytest.raises(ValueError):
        shrink.pack_sets(np.zeros((1, 65), bool), 2)


def test_library_exports_and_version():
    from quits_amd import _lib
    L = _lib.load()
    assert L.qd_version() >= 114 and _lib.require_shrink(L) is L
    for name in ("qd_shrink_begin", "qd_shrink_step"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert (_lib.SHRINK_STATE, _lib.SHRINK_FAILS, _lib.SHRINK_MINIMAL, _lib.SHRINK_ENDED) == (shrink.STATE_WORDS, shrink.FLAG_FAILS, shrink.FLAG_MINIMAL, shrink.FLAG_ENDED)

    class Old:
        def qd_version(self):
            return 113
    with pytest.raises(RuntimeError, match="114"):
        _lib.require_shrink(Old())


def test_public_functions_are_exported():
    from quits_amd import simulation
    for name in ("shrink_fault_sets", "get_minimal_failures", "get_relay_minimal_failures", "MinimalFailuresResult"):
        assert hasattr(simulation, name)
