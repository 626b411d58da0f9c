"""The random information-set estimate of the distance on the device (csrc/distance.hip) against the numpy mirror
(quits_amd.distance.distance_mirror): records and histogram bit for bit at the shapes where the kernel can go wrong, the invariances that
keep the grid and the batch out of the results, the calls end to end and the capacity refusal."""
import numpy as np
import pytest
from scipy.sparse import csc_matrix

import helpers
from quits_amd import distance as qd
from test_distance import rep3_code, synthetic_6x14
from test_search import matrices

pytestmark = pytest.mark.gpu


def synthetic(m, n, w, seed):
    """m x n, column weight w (the rng.choice recipe of the decoder's synthetic graphs), four random observables."""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([rng.choice(m, size=w, replace=False) for _ in range(n)])
    H = csc_matrix((np.ones(n * w, np.uint8), (rows, np.repeat(np.arange(n), w))), shape=(m, n))
    return H, csc_matrix((rng.random((4, n)) < 0.5).astype(np.uint8))


def heavy_40x600():
    """40 x 600: column 17 has weight 16; 600 columns of weight 3 on 40 rows complete the rank within the first tenth of the order, so nearly
    the whole walk is the all-candidates phase."""
    H, L = synthetic(40, 600, 3, 40600)
    H = H.tolil()
    H[:, 17] = 0
    H[np.arange(0, 32, 2), 17] = 1
    return csc_matrix(H), L


def code(name, basis="x"):
    cd = helpers.code(name)
    return csc_matrix(cd["h" + basis]), csc_matrix(cd["l" + basis])


def device_run(H, L, trials, seed=1, trial0=0, observables=None):
    est = qd.DistanceEstimator(qd.prepare(H, L, observables))
    try:
        return est.run(seed, trial0, trials), est.hist(), est.info()
    finally:
        est.close()


def compare(H, L, trials, seed=1, observables=None):
    rec, hist, info = device_run(H, L, trials, seed, 0, observables)
    ref_rec, ref_hist = qd.distance_mirror(H, L, trials, seed=seed, observables=observables)
    assert np.array_equal(rec, ref_rec), (rec[:8], ref_rec[:8], info)
    assert np.array_equal(hist, ref_hist), (hist, ref_hist, info)
    assert info["rank"] == qd.mirror_rank(H, L, observables)
    return info


CASES = {
    "rep3_m9": (rep3_code, 64),                                              # less than one word, a row without a pivot; one wavefront a trial
    "synthetic_6x14": (synthetic_6x14, 64),                                  # zero column, equal columns, duplicated row
    "m32": (lambda: synthetic(32, 96, 3, 32), 32),                           # exactly one word
    "m64": (lambda: synthetic(64, 192, 3, 64), 32),                          # exactly two words, the last one-wavefront size
    "m65": (lambda: synthetic(65, 195, 3, 65), 32),                          # one bit into the third word, the first 256-thread size
    "bb72_code": (lambda: code("bb72"), 64),                                 # 36 x 72: partial last word, m = n / 2
    "bb144_code": (lambda: code("bb144"), 64),                               # 72 x 144
    "bb72_r0": (lambda: matrices("bb72_custom_r0_p0.003"), 64),              # 72 x 432, rank 66: rows that never get a pivot
    "heavy_40x600": (heavy_40x600, 32),                                      # a column of weight 16; the all-candidates phase
    "bb72_r6": (lambda: matrices("bb72_custom_r6_p0.003"), 8),               # 288 x 2592: 1024 threads, 41 column blocks, 4096 sorted words
    "headline": (lambda: matrices("bb144_custom_r12_p0.003"), 2),            # 1008 x 9504, rank 1002: the LDS budget at its edge
}


@pytest.mark.parametrize("key", list(CASES))
def test_device_equals_the_mirror(key):
    make, trials = CASES[key]
    H, L = make()
    info = compare(H, L, trials)
    if key == "headline":
        assert H.shape == (1008, 9504) and info["rank"] == 1002 and info["threads"] == 1024 and 128 * 1024 < info["lds_bytes"] <= 160 * 1024
    if key in ("rep3_m9", "m64"):
        assert info["threads"] == 64 and info["trials_in_flight"] >= 16
    if key == "m65":
        assert info["threads"] == 256
    if key == "heavy_40x600":
        assert int(np.diff(H.indptr).max()) == 16 and info["rank"] == 40 and info["columns_per_block"] >= 16


def test_results_do_not_depend_on_batch_grid_or_history():
    H, L = matrices("bb72_custom_r0_p0.003")
    m = qd.prepare(H, L)
    ref, ref_hist = qd.distance_mirror(m, None, 64, seed=1)
    est = qd.DistanceEstimator(m)
    try:
        assert np.array_equal(est.run(1, 0, 64), ref) and np.array_equal(est.hist(), ref_hist)
        assert np.array_equal(est.run(1, 0, 64), ref) and np.array_equal(est.hist(), ref_hist + ref_hist)       # a second run adds
        est.reset()
        assert not est.hist().any()
        a, b = est.run(1, 0, 3), est.run(1, 3, 5)                                                              # trial0 splits a run
        assert np.array_equal(np.concatenate([a, b]), ref[:8])
        assert np.array_equal(est.hist(), qd.distance_mirror(m, None, 8, seed=1)[1])
        for batch in (1, 7, 64):
            est.reset()
            got = np.concatenate([est.run(1, t, min(batch, 64 - t)) for t in range(0, 64, batch)])
            assert np.array_equal(got, ref) and np.array_equal(est.hist(), ref_hist), batch
        hi = est.run((1 << 32) + 1, 0, 8)                                                                      # the high key word
        assert not np.array_equal(hi, ref[:8]) and np.array_equal(hi, qd.distance_mirror(m, None, 8, seed=(1 << 32) + 1)[0])
        far = est.run(1, (1 << 32) + 5, 4)                                                                     # the high trial word
        assert np.array_equal(far, qd.distance_mirror(m, None, 4, seed=1, trial0=(1 << 32) + 5)[0])
    finally:
        est.close()
    for batch in (1, 7, 64):
        res = qd.estimate_distance((H, L), trials=64, seed=1, batch=batch, keep_records=True, keep=1)
        assert np.array_equal(res.records, ref) and np.array_equal(res.hist, ref_hist) and res.trials == 64


def test_estimate_distance_end_to_end():
    H, L = code("bb144")
    res = qd.estimate_distance((H, L), trials=64, seed=1)
    ref = qd.estimate_distance_mirror((H, L), trials=64, seed=1)
    assert res.weight == 12 and res.first_trial == ref.first_trial and res.trials == 64 and res.rank == ref.rank == 66
    assert len(res.witnesses) == len(ref.witnesses) >= 1
    for e, mask, e2 in zip(res.witnesses, res.masks, ref.witnesses):
        qd.check_vector(H, L, e, mask, res.observables)
        assert len(e) == 12 and np.array_equal(e, e2)
    assert np.array_equal(res.hist, ref.hist) and res.records is None


def test_target_stops_at_a_batch_boundary():
    H, L = matrices("bb72_custom_r0_p0.003")
    res = qd.estimate_distance((H, L), trials=4096, seed=1, target=6, batch=16, keep=2)
    assert res.weight == 6 and res.trials % 16 == 0 and 16 <= res.trials < 4096
    assert res.trials - 16 <= res.first_trial < res.trials                   # the batch that reached the target was the last
    again = qd.estimate_distance((H, L), trials=res.trials, seed=1, keep=2)   # reproducible from (seed, trials)
    assert again.weight == 6 and again.first_trial == res.first_trial and np.array_equal(again.hist, res.hist)
    for e, mask in zip(res.witnesses, res.masks):
        qd.check_vector(H, L, e, mask, res.observables)
    slow = qd.estimate_distance((H, L), trials=4096, seed=1, max_seconds=0.0, batch=16, keep=0)
    assert slow.trials == 16 and slow.witnesses == []


def test_estimate_code_distance_of_bb72():
    cd = helpers.code("bb72")
    dx, dz = qd.estimate_code_distance(cd["hx"], cd["hz"], cd["lx"], cd["lz"], trials=64, seed=1)
    assert (dx.weight, dz.weight) == (6, 6)
    qd.check_vector(cd["hz"], cd["lz"], dx.witnesses[0], dx.masks[0], dx.observables)
    qd.check_vector(cd["hx"], cd["lx"], dz.witnesses[0], dz.masks[0], dz.observables)


def test_capacity_is_refused_before_any_launch():
    """9900 x 133320 (the stored matrices of the circuit's detector error model): a transform of 12 MB."""
    H, L, _ = helpers.dem_matrices("qlp1020_cardinal_r20_p0.003")
    assert H.shape == (9900, 133320) and L.shape[0] == 136
    with pytest.raises(NotImplementedError, match=r"takes (\d+) bytes of LDS, a CU holds 163840") as exc:
        qd.estimate_distance((H, L), trials=4, observables=range(64))
    import re
    assert int(re.search(r"takes (\d+) bytes", str(exc.value)).group(1)) > 163840


def test_the_qlp_code_runs_with_a_selection():
    """450 x 1020, 136 logicals: 64 at a time."""
    cd = helpers.code("qlp1020")
    H, L = csc_matrix(cd["hx"]), csc_matrix(cd["lx"])
    with pytest.raises(ValueError, match="pass a selection"):
        qd.estimate_distance((H, L), trials=4)
    compare(H, L, 4, observables=range(64))
