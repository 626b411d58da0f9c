"""The random information-set estimate of the distance, host side (quits_amd/distance.py): the numpy mirror against a dense brute-force
restatement of the definition written here, known code distances, bounds on circuit-level models, the trial0 and tie rules, the refusals,
the version gate, the command line and the kernel's resources.  No GPU."""
import json

import numpy as np
import pytest
from scipy.sparse import csc_matrix

import helpers
from quits_amd import distance as qd
from test_search import matrices

NONE = np.uint64(qd.NO_RECORD)


def synthetic_6x14():
    """6 x 14 with a zero column that carries a mask (3), two equal columns (4, 9), a duplicated row (rows 1 and 4) and a column of weight 6
    (7); two observables."""
    rng = np.random.default_rng(614)
    H = (rng.random((6, 14)) < 0.35).astype(np.uint8)
    H[:, 3] = 0
    H[:, 9] = H[:, 4]
    H[:, 7] = 1
    H[4] = H[1]
    L = (rng.random((2, 14)) < 0.4).astype(np.uint8)
    L[:, 3] = (1, 0)
    L[:, 9] = L[:, 4] ^ np.array([0, 1], np.uint8)          # the two equal columns differ in their mask: a weight-2 logical
    assert H[:, 7].sum() == 6 and not H[:, 3].any() and np.array_equal(H[1], H[4])
    return csc_matrix(H), csc_matrix(L)


def rep3_code():
    """The HGP rep-3 code: the fixture's hx is 9 x 18 of rank 8 (its rows sum to zero), so one row never gets a pivot."""
    cd = helpers.code("hgp_rep3")
    assert cd["hx"].shape == (9, 18) and cd["lx"].shape[0] == 2
    return csc_matrix(cd["hx"]), csc_matrix(cd["lx"])


def dense_reference(H, L, trials, seed, observables=None):
    """The definition on dense 0/1 arrays: the pivots in [I | H-columns-in-order] style, a column at a time, the pivot row of an independent
    column being the one with the MOST ones left in the columns still to come (ties: the highest index) -- nothing like the mirror's or the
    kernels' rule.  Returns (records, hist, candidates per trial as {fault: (support, mask)})."""
    H = np.asarray(csc_matrix(H).todense()) % 2
    L = np.asarray(csc_matrix(L).todense()) % 2
    m, n = H.shape
    obs = list(range(L.shape[0])) if observables is None else list(observables)
    fobs = [sum(int(L[i, j]) << b for b, i in enumerate(obs)) for j in range(n)]
    rec, hist, cands = np.zeros(trials, np.uint64), np.zeros(64, np.uint64), []
    for t in range(trials):
        order = [int(j) for j in qd.trial_order(n, seed, t)]
        A = H[:, order].astype(np.uint8)                     # row-reduced in place, column by column
        prow, pcol = [], []                                   # pivot rows and the faults that own them
        best, cand = int(NONE), {}
        for pos, j in enumerate(order):
            col = A[:, pos]
            free = [r for r in range(m) if col[r] and r not in prow]
            if free:
                r = max(free, key=lambda r: (int(A[r, pos + 1:].sum()), r))
                for i in range(m):
                    if i != r and A[i, pos]:
                        A[i] ^= A[r]
                prow.append(r)
                pcol.append(j)
                continue
            e = sorted([j] + [pcol[prow.index(r)] for r in range(m) if col[r]])
            mask = 0
            for f in e:
                mask ^= fobs[f]
            cand[j] = (e, mask)
            if mask:
                hist[min(len(e), 63)] += np.uint64(1)
                best = min(best, (len(e) << 32) + j)
        rec[t] = best
        cands.append(cand)
    return rec, hist, cands


@pytest.mark.parametrize("make", [rep3_code, synthetic_6x14])
def test_every_candidate_against_a_dense_reference(make):
    H, L = make()
    trials, seed = 32, 5
    rec, hist = qd.distance_mirror(H, L, trials, seed=seed)
    ref_rec, ref_hist, cands = dense_reference(H, L, trials, seed)
    assert np.array_equal(rec, ref_rec) and np.array_equal(hist, ref_hist)
    assert hist.sum() > 0 and (rec != NONE).any()
    Hd = np.asarray(H.todense()) % 2
    for t in range(trials):
        for j, (e, mask) in cands[t].items():
            got, gmask = qd.kernel_vector(H, L, seed, t, j)
            assert got.tolist() == e and gmask == mask
            x = np.zeros(H.shape[1], np.int64)
            x[got] = 1
            assert not ((Hd @ x) % 2).any()
            if mask:
                qd.check_vector(H, L, got, mask, [0, 1][:L.shape[0]])
        pivots = [j for j in range(H.shape[1]) if j not in cands[t]]
        assert len(pivots) == qd.mirror_rank(H, L)
        with pytest.raises(ValueError, match="pivot"):
            qd.kernel_vector(H, L, seed, t, pivots[0])


def test_the_synthetic_model_holds_what_it_should():
    H, L = synthetic_6x14()
    rec, hist = qd.distance_mirror(H, L, 16, seed=1)
    assert np.all(rec == np.uint64((1 << 32) + 3))           # the detector-less fault 3 with its mask: weight 1 in every trial
    assert hist[1] == 16 and hist[2:].sum() > 0
    e, mask = qd.kernel_vector(H, L, 1, 0, 3)
    assert e.tolist() == [3] and mask == 1


CODES = [("bb72", 6), ("bb90", 10), ("bb144", 12), ("hgp225", 6)]


@pytest.mark.parametrize("name,d", CODES)
@pytest.mark.parametrize("basis", ["x", "z"])
def test_known_code_distances(name, d, basis):
    """64 trials of seed 1 reach the known distance in both bases (every fixture holds both logicals)."""
    cd = helpers.code(name)
    H, L = cd["h" + basis], cd["l" + basis]
    assert L.shape[0] > 0
    res = qd.estimate_distance_mirror((H, L), trials=64, seed=1)
    assert res.weight == d and res.trials == 64 and 0 <= res.first_trial < 64
    assert len(res.witnesses) >= 1 and len(res.witnesses) == len(res.masks)
    for e, mask in zip(res.witnesses, res.masks):
        assert len(e) == d
        qd.check_vector(H, L, e, mask, res.observables)
    assert int(res.hist[:d].sum()) == 0 and int(res.hist[d]) >= 1


@pytest.mark.parametrize("name,exact", [("bb72_custom_r0_p0.003", True), ("bb72_custom_r2_xbasis_mixed", True), ("bb72_custom_r6_p0.003", False)])
def test_bounds_on_circuit_level_models(name, exact):
    """256 trials of seed 1.  The search proves 6 on the first two models; on the six-round one it proves nothing, so 6 is an upper bound there."""
    H, L = matrices(name)
    res = qd.estimate_distance_mirror((H, L), trials=256, seed=1, keep=4)
    assert res.weight <= 6 and (not exact or res.weight == 6)
    assert len(res.witnesses) >= 1
    for e, mask in zip(res.witnesses, res.masks):
        qd.check_vector(H, L, e, mask, res.observables)


def test_trial0_splits_a_run():
    H, L = matrices("bb72_custom_r0_p0.003")
    whole, hw = qd.distance_mirror(H, L, 8, seed=3)
    a, ha = qd.distance_mirror(H, L, 3, seed=3)
    b, hb = qd.distance_mirror(H, L, 5, seed=3, trial0=3)
    assert np.array_equal(whole, np.concatenate([a, b])) and np.array_equal(hw, ha + hb)
    assert not np.array_equal(whole, qd.distance_mirror(H, L, 8, seed=4)[0])


def test_ties_go_to_the_lowest_fault():
    """Faults 2 and 5 are equal columns (no detector) and both logical: weight 1 twice in every trial, whatever the order; the record names
    fault 2.  With their masks taken away the lightest are {0, 1} (equal columns, masks differ) and ties are again by fault index."""
    H = csc_matrix(np.array([[1, 1, 0, 1, 0, 0], [1, 1, 0, 0, 1, 0]], np.uint8))
    L = csc_matrix(np.array([[1, 0, 1, 0, 0, 1]], np.uint8))
    rec, hist = qd.distance_mirror(H, L, 8, seed=0)
    assert np.all(rec == np.uint64((1 << 32) + 2)) and hist[1] == 16
    ref = dense_reference(H, L, 8, 0)
    assert np.array_equal(rec, ref[0]) and np.array_equal(hist, ref[1])
    L0 = csc_matrix(np.array([[1, 0, 0, 0, 0, 0]], np.uint8))
    rec, hist = qd.distance_mirror(H, L0, 8, seed=0)
    ref = dense_reference(H, L0, 8, 0)
    assert np.array_equal(rec, ref[0]) and np.array_equal(hist, ref[1])
    for t in range(8):
        w, j = int(rec[t]) >> 32, int(rec[t]) & 0xFFFFFFFF
        assert j == min(f for f, (e, mask) in ref[2][t].items() if mask and len(e) == w)


def test_limits_raise_value_errors():
    H, L = rep3_code()
    wide = csc_matrix(np.ones((65, H.shape[1]), np.uint8))
    with pytest.raises(ValueError, match="pass a selection"):
        qd.distance_mirror(H, wide, 1)
    with pytest.raises(ValueError, match="at most 64"):
        qd.distance_mirror(H, wide, 1, observables=list(range(65)))
    assert len(qd.distance_mirror(H, wide, 2, observables=list(range(64)))[0]) == 2
    for bad in ([0, 0], [2], [-1]):
        with pytest.raises(ValueError, match="distinct row indices"):
            qd.distance_mirror(H, L, 1, observables=bad)
    with pytest.raises(ValueError, match="nothing to estimate"):
        qd.distance_mirror(csc_matrix((0, 4), dtype=np.uint8), csc_matrix((1, 4), dtype=np.uint8), 1)
    with pytest.raises(ValueError, match="nothing to estimate"):
        qd.distance_mirror(csc_matrix((4, 0), dtype=np.uint8), csc_matrix((1, 0), dtype=np.uint8), 1)
    tall = csc_matrix((np.ones(2, np.uint8), ([0, 65535], [0, 1])), shape=(65536, 2))
    with pytest.raises(ValueError, match="65535"):
        qd.distance_mirror(tall, csc_matrix(np.ones((1, 2), np.uint8)), 1)
    with pytest.raises(ValueError, match="one column per fault"):
        qd.distance_mirror(H, L[:, :-1], 1)
    with pytest.raises(ValueError, match="pass a selection"):
        qd.estimate_distance((H, wide))                      # checked before the device is looked for
    with pytest.raises(ValueError, match="trials"):
        qd.estimate_distance((H, L), trials=0)


def test_a_selection_changes_masks_not_pivots():
    H, L = rep3_code()
    assert L.shape[0] == 2
    both, _ = qd.distance_mirror(H, L, 16, seed=2)
    for sel in ([0], [1], [1, 0]):
        m = qd.prepare(H, L, sel)
        assert int(m.fault_obs.max()) < (1 << len(sel))
        fulls, parts = dense_reference(H, L, 4, 2)[2], dense_reference(H, L, 4, 2, sel)[2]
        for full, part in zip(fulls, parts):
            assert sorted(full) == sorted(part)               # the same non-pivot columns
            for j in full:
                assert full[j][0] == part[j][0]
                assert part[j][1] == sum(((full[j][1] >> i) & 1) << b for b, i in enumerate(sel))
    one, _ = qd.distance_mirror(H, L, 16, seed=2, observables=[0])
    assert np.all(one >= both)                               # fewer observables: fewer logical candidates


def test_every_input_form_gives_the_same_records():
    from quits_amd.dem import Circuit
    name = "hgprep3_zxcoloration_r3_p0.001"
    H, L = matrices(name)
    text = helpers.circuit_text(name)
    a = qd.estimate_distance_mirror((H, L), trials=4, seed=1, keep_records=True)
    b = qd.estimate_distance_mirror(text, trials=4, seed=1, keep_records=True)
    c = qd.estimate_distance_mirror(Circuit(text), trials=4, seed=1, keep_records=True)
    assert np.array_equal(a.records, b.records) and np.array_equal(a.records, c.records) and a.weight == 3
    out = a.to_json()
    assert json.loads(json.dumps(out))["weight"] == 3 and len(out["records"]) == 4 and len(out["hist"]) == 64


def test_version_gate_and_exports():
    from quits_amd import _lib, simulation
    L = _lib.load()
    assert L.qd_version() >= 117 and _lib.require_distance(L) is L
    for name in ("qd_isd_create", "qd_isd_destroy", "qd_isd_info", "qd_isd_run", "qd_isd_hist", "qd_isd_reset"):
        assert name in _lib.EXPORTS and hasattr(L, name)

    class Old:
        def qd_version(self):
            return 116
    with pytest.raises(RuntimeError, match="117 -- rebuild it"):
        _lib.require_distance(Old())
    assert simulation.estimate_distance is qd.estimate_distance and simulation.estimate_code_distance is qd.estimate_code_distance


def test_command_line_prints_the_result_as_json(tmp_path, capsys):
    from quits_amd.__main__ import main
    name = "hgprep3_zxcoloration_r3_p0.001"
    path = tmp_path / "c.stim"
    path.write_text(helpers.circuit_text(name))
    assert main(["distance", "--circuit", str(path), "--trials", "8", "--seed", "1", "--keep", "2", "--mirror"]) == 0
    out = json.loads(capsys.readouterr().out)
    assert out["weight"] == 3 and out["trials"] == 8 and out["seed"] == 1 and 1 <= len(out["witnesses"]) <= 2
    H, L = matrices(name)
    for e, mask in zip(out["witnesses"], out["masks"]):
        qd.check_vector(H, L, e, mask, out["observables"])
    assert main(["distance", "--circuit", str(path), "--observables", "7", "--mirror"]) == 1


def test_distance_kernel_uses_no_scratch(tmp_path):
    """The transform and the block's reduced columns live in LDS: no indexed register array, no scratch."""
    from test_api import _resource_usage
    kern = dict(_resource_usage(tmp_path, "distance.hip"))
    names = [n for n in kern if "qd_isd_" in n]
    assert len(names) >= 1, kern
    assert all(kern[n] == 0 for n in names), kern
