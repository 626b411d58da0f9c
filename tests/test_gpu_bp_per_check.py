"""The per-check work around the two edge loops of the several-checks-per-lane min-sum kernel (bp_scatter_wide.hip): a check's state
is ONE register set (the gather walk reads what was sent, commits what it found, the scatter pass sends that), the argmin edge's sign
is picked as a mask by one v_bfe_i32 and applied as (dlt ^ m) - m, its address is a 24-bit multiply-add, the convergence vote is one
XOR per round into the sign bit of a per-lane word with one flag byte per wavefront, and the certificate's running maximum is one
non-canonicalising v_max_f32.  What those edits can get wrong, and the case that would show it -- three paths (default,
QD_BP_NO_FAST_START=1, QD_NO_SCATTER=1) bit for bit against each other and against the double-precision oracle on the device's
grid: hard decisions, status words (iteration counts included), OSD-0 outputs, posteriors of the first shots that do not converge:

  position   rows of weight 35 and 36 (64 of each: the sign pick in the second word, both word boundaries) with priors spread over three
             decades, sampled syndromes (both values of a check's syndrome, both parities of the incoming signs) and the all-ones one.
             A check's walk order is a permutation of its faults that the layout chooses (graph_layout.hip, scatter_walk) and Python
             cannot see; what is shown on the CPU is that over the passes the argmin lies at every index of the row in COLUMN order,
             0, 3, 4, 31, 32, 34 and the last among them, on rows of either weight.
  zero       all priors equal on rows of weight 2, 4, 33 and 64: min1 = min2 on every check of the first pass, the correction adds 0.
  state      the window of test_gpu_bp_argmin_keys.py whose rounds cross the key bound midway (max_iter 4 and 7: a key walk that does
             not hold is followed by the compare walk, which commits into the set the key walk left alone), and QD_SCATTER_M2_LIMIT=1
             (every shot with a defect goes through the recheck pass).
  vote       256 checks of weight 4 on <128,8,2,2> (two wavefronts, two rounds each, every lane taken) and 256 shots, shot b with
             the single defect b: after the first iteration no hard decision has moved, so check b is the ONLY unsatisfied check of
             the vote -- in turn every lane of every round of every wavefront, the last lane of the last wavefront and the lanes that
             are unsatisfied in round 1 only among them.  A vote that misses one reports that shot converged.
  maximum    the vote's matrix with the four faults of check 5 a hundred times less likely than the rest: the largest second minimum
             of the first pass belongs to that check alone -- one lane of the first 64 slots, a wavefront's first round -- and every
             other check of the pass, the lane's second round included, stays far below it.  At max_iter 1 the first pass is all the
             default path's certificate sees; QD_SCATTER_M2_LIMIT sits at that value, so the running maximum must keep what it met
             first.  (A parked shot comes back with the same outputs: the case pins the inputs and would show a maximum that turns
             into garbage, not one that is lost.)
  shapes     one case under QD_SCATTER_CPL1=1; qlp1020 W = 3 at max_iter 3 (three sign words, the compare form only).

The conditions named above are asserted on the CPU by an integer flooding min-sum in numpy (test_crafted_conditions_hold)."""
import ctypes
import functools

import numpy as np
import pytest
from scipy.sparse import csc_matrix, csr_matrix

import helpers
import oracle as orc
import test_gpu_bp_argmin_keys as keys
import test_gpu_bp_scatter_reset as reset

SWITCHES = reset.SWITCHES
PATHS = reset.PATHS
SHOTS = 64
ONES_SHOTS = 4
NLLR = 6
EQ_ROWS = [64] * 8 + [33] * 8 + [4] * 40 + [2] * 72
VOTE_CHECKS = 256
MAX_CHECK = 5
MUST_BE_ARGMIN = {36: (0, 3, 4, 31, 32, 34, 35), 35: (0, 3, 4, 31, 32, 34)}


@functools.lru_cache(maxsize=None)
def _matrix(which):
    if which == "w35_36":
        return helpers.synthetic_window([36] * 64 + [35] * 64, 3, 6, 41001)
    if which in ("eq", "vote", "maxfirst"):          # every fault in two checks, all priors equal
        rows = EQ_ROWS if which == "eq" else [4] * VOTE_CHECKS
        rng = np.random.default_rng(41002 if which == "eq" else 41003)
        H = helpers._place(rng, rows, np.full(sum(rows) // 2, 2, dtype=np.int64))
        H = H[:, rng.permutation(H.shape[1])]
        pri = np.full(H.shape[1], 0.02 if which == "eq" else 0.01)
        if which == "maxfirst":
            pri[:] = 0.03
            pri[np.flatnonzero(H[MAX_CHECK])] = 3e-4
        return csc_matrix(H), pri
    if which == "bound":
        return keys._matrix("bound")
    assert which == "qlp1020_w3"
    w = helpers.window_set("qlp1020_cardinal_r20_p0.003", 3, 1)[0]
    return w["H"], np.asarray(w["priors"], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _window(which, synd):
    H, pri = _matrix(which)
    if synd == "ones":
        s = np.ones((ONES_SHOTS, H.shape[0]), dtype=np.uint8)
    elif synd == "single":
        s = np.eye(H.shape[0], dtype=np.uint8)
    else:
        s = np.ascontiguousarray(orc.sample_dem(H, H[:1], pri, seed=53, shot0=0, B=SHOTS)[0]).astype(np.uint8)
    s.setflags(write=False)
    return H, pri, s


def _minsum(H, pri, s, max_iter):
    """Integer flooding min-sum on the device's grid rule (as test_gpu_bp_argmin_keys._minsum_min2), per shot and gather pass, in the
    checks' own order: {(shot, pass): min1, min2, argmin (index of the first smallest magnitude among the row's faults in column
    order), unsat (the checks whose hard-decision parity differs from the syndrome: the pass's vote)}."""
    k = orc.grid_bits(pri, max_iter)[0]
    P = np.rint(np.log((1.0 - pri) / pri) * 2.0 ** k).astype(np.int64)
    R = csr_matrix(H)
    R.sort_indices()
    ptr, c = R.indptr, R.indices
    deg = np.diff(ptr)
    r = np.repeat(np.arange(R.shape[0]), deg)
    within = np.arange(len(c)) - ptr[r]
    out = {}
    for b in range(s.shape[0]):
        if not s[b].any():
            continue
        L, msg = P.copy(), np.zeros(len(c), dtype=np.int64)
        for t in range(max_iter + 1):
            bm = L[c] - msg
            unsat = (np.add.reduceat((L[c] <= 0).astype(np.int64), ptr[:-1]) & 1) != s[b]
            if t >= 1 and not unsat.any():
                break
            mag, sgn = np.abs(bm), (bm <= 0).astype(np.int64)
            order = np.lexsort((within, mag, r))
            min1, min2 = mag[order][ptr[:-1]], mag[order][ptr[:-1] + 1]
            out[(b, t)] = dict(min1=min1, min2=min2, argmin=within[order][ptr[:-1]], unsat=unsat)
            neg = (s[b][r].astype(np.int64) ^ (np.add.reduceat(sgn, ptr[:-1]) & 1)[r] ^ sgn) == 1
            new = np.where(mag == min1[r], min2[r], min1[r])
            msg = np.where(neg, -new, new)
            L = P + np.bincount(c, weights=msg, minlength=len(P)).astype(np.int64)
    return out


@functools.lru_cache(maxsize=None)
def _first_pass_top(which, max_iter):
    """The largest second minimum of gather pass 0 (priors alone: the same for every shot), in the grid units of `max_iter`."""
    H, pri, s = _window(which, "sampled")
    sim = _minsum(H, pri, s, max_iter)
    return max(int(v["min2"].max()) for (b, t), v in sim.items() if t == 0), sim


def test_crafted_conditions_hold():
    """The inputs of the crafted cases, on the CPU."""
    # position: every index of a row is an argmin somewhere, on rows of weight 36 and of weight 35
    H, pri, s = _window("w35_36", "sampled")
    deg = np.diff(csr_matrix(H).indptr)
    sim = _minsum(H, pri, s, 3)
    for w, need in MUST_BE_ARGMIN.items():
        seen = set()
        for v in sim.values():
            seen |= set(v["argmin"][deg == w].tolist())
        assert set(need) <= seen, (w, sorted(set(need) - seen))
    assert 0 < s.sum() < s.size and {0, 1} <= set(s[:, deg == 36].ravel().tolist())
    # zero: min1 = min2 on every check of the first pass, on all four weights
    H, pri, s = _window("eq", "sampled")
    assert sorted(np.diff(csr_matrix(H).indptr).tolist(), reverse=True) == EQ_ROWS
    sim = _minsum(H, pri, s, 3)
    first = [v for (b, t), v in sim.items() if t == 0]
    assert first and all((v["min1"] == v["min2"]).all() for v in first)
    # state: rounds that cross the key bound after passes under it (the CPU test of test_gpu_bp_argmin_keys.py shows the rest)
    H, pri, s = _window("bound", "sampled")
    for max_iter in (4, 7):
        m2, _ = keys._minsum_min2(H, pri, s, max_iter)
        over = {key: (v.reshape(2, 64) >= keys.KEY_BOUND).any(axis=1) for key, v in m2.items()}
        assert any(over[(b, t)][r] and not over[(b, 0)][r] for (b, t) in over for r in range(2) if t >= 1), max_iter
    # vote: shot b's only unsatisfied check after the first iteration is check b, and no shot is done
    H, pri, s = _window("vote", "single")
    assert H.shape[0] == VOTE_CHECKS and np.array_equal(s, np.eye(VOTE_CHECKS, dtype=np.uint8))
    sim = _minsum(H, pri, s, 1)
    for b in range(VOTE_CHECKS):
        assert np.array_equal(np.flatnonzero(sim[(b, 1)]["unsat"]), [b]), b
    # maximum: the first pass's largest second minimum is check 5's alone, the other checks' lie far below
    top, sim = _first_pass_top("maxfirst", 1)
    first = next(v["min2"] for (b, t), v in sorted(sim.items()) if t == 0)
    assert MAX_CHECK < 64 and int(np.argmax(first)) == MAX_CHECK and first[MAX_CHECK] == top and np.sort(first)[-2] * 2 < top


@functools.lru_cache(maxsize=None)
def _reference(which, synd, max_iter):
    """The oracle in double precision on the device's grid, on the CPU, as test_gpu_bp_scatter_reset._reference gives it."""
    H, pri, s = _window(which, synd)
    shots = np.arange(len(s))
    g, form = orc.device_arithmetic(H, pri, "minimum_sum", "parallel", max_iter, 1.0)
    prm = orc.make_params("minimum_sum", "parallel", max_iter, "osd_0", 0, 1.0, form)
    ref, flags = g.decode_batch(np.ascontiguousarray(s), prm)
    soft = {}
    for b in np.flatnonzero(flags[:, 0] == 0)[:NLLR]:
        conv, dec, llr, it = g.bp(s[b], prm)
        assert not conv and it == flags[b, 1]
        assert float(np.abs(llr).max()) * 2.0 ** orc.grid_bits(pri, max_iter)[0] < 2.0 ** 23, (which, synd, max_iter)
        soft[int(b)] = (dec, llr)
    return shots, ref, flags, soft


def _run(monkeypatch, which, synd, env, max_iter):
    import torch
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    H, pri, s = _window(which, synd)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wg = WindowGraph(H, pri)
    dec = BatchDecoder(wg, max_iter=max_iter, osd_method="osd_0")
    det = torch.from_numpy(np.array(s)).cuda()
    out = {}
    bits, status = dec.decode(det, stage=1)
    out[1] = (unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy())
    failed = np.flatnonzero(((out[1][1] >> 16) & 1) == 0)[:NLLR]
    out["llr"] = {int(b): dec.failed_llr(int(b)).cpu().numpy() for b in failed}
    bits, status = dec.decode(det, stage=3)
    out[3] = (unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy())
    arr = (ctypes.c_int32 * 14)()
    assert wg._L.qd_graph_info_ex(wg._h, arr, 14) == 0
    return out, dec.info(), (int(arr[12]), int(arr[13]), 3 if wg.info()["max_row_weight"] > 64 else 2)


def _paths(monkeypatch, which, synd, max_iter, extra_env=None, shape=(128, 2, 2)):
    ref4 = _reference(which, synd, max_iter)
    cpl1 = "QD_SCATTER_CPL1" in (extra_env or {})
    outs = {}
    for tag, env in PATHS:
        outs[tag], info, ran = _run(monkeypatch, which, synd, dict(env, **(extra_env or {})), max_iter)
        assert info["scatter_kernel"] == (tag != "gather") and info["scatter_wide_kernel"] == (tag != "gather" and not cpl1), (tag, info)
        assert info["bp_fast_start"] == (tag == "default"), (tag, info)
        if tag != "gather":
            assert ran[1:] == shape[1:] and shape[0] in (None, ran[0]), (which, tag, ran)
    reset._same(outs["default"], outs["gather"], "default path against the gather kernel")
    reset._same(outs["generic"], outs["gather"], "QD_BP_NO_FAST_START=1 against the gather kernel")
    for tag in ("default", "generic", "gather"):
        reset._against_oracle(ref4, outs[tag], tag, True)
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [1, 2, 3, 50])
@pytest.mark.parametrize("synd", ["sampled", "ones"])
@pytest.mark.parametrize("which", ["w35_36", "eq"])
def test_per_check_positions_and_zero_corrections(gpu, monkeypatch, which, synd, max_iter):
    """Rows of weight 35 and 36 with the argmin all over both sign words; rows of weight 2, 4, 33, 64 with min1 = min2."""
    _paths(monkeypatch, which, synd, max_iter)


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [4, 7])
def test_per_check_rewalk_commits_into_the_one_set(gpu, monkeypatch, max_iter):
    """Rounds that trip the key bound midway: the compare walk behind a key walk that did not hold commits the check's state."""
    _paths(monkeypatch, "bound", "sampled", max_iter)


@pytest.mark.gpu
def test_per_check_with_recheck_pass(gpu, monkeypatch):
    """QD_SCATTER_M2_LIMIT = 1: every shot with a defect is parked and comes back from the gather kernel's recheck pass."""
    _paths(monkeypatch, "w35_36", "sampled", 50, extra_env={"QD_SCATTER_M2_LIMIT": "1"})


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [1, 2])
def test_per_check_vote_sees_every_lane_of_every_round(gpu, monkeypatch, max_iter):
    """256 shots with one defect each: the check that alone keeps the shot from converging visits every lane of both rounds of both
    wavefronts; at max_iter 1 the vote is the thin last pass's (default path) or the loop's (QD_BP_NO_FAST_START=1)."""
    outs = _paths(monkeypatch, "vote", "single", max_iter, shape=(128, 2, 2))
    if max_iter == 1:
        st = outs["default"][1][1]
        assert not ((st >> 16) & 1).any() and ((st & 0x3FFF) == 1).all()


@pytest.mark.gpu
def test_per_check_maximum_met_in_the_first_pass(gpu, monkeypatch):
    """QD_SCATTER_M2_LIMIT at the first pass's largest second minimum, met in one lane's first round only; max_iter 1."""
    top = _first_pass_top("maxfirst", 1)[0]
    _paths(monkeypatch, "maxfirst", "sampled", 1, extra_env={"QD_SCATTER_M2_LIMIT": str(top)})


@pytest.mark.gpu
def test_per_check_one_check_per_lane(gpu, monkeypatch):
    """QD_SCATTER_CPL1=1: the same text with one check per lane."""
    _paths(monkeypatch, "w35_36", "sampled", 50, extra_env={"QD_SCATTER_CPL1": "1"}, shape=(None, 1, 2))


@pytest.mark.gpu
def test_per_check_three_sign_words(gpu, monkeypatch):
    """qlp1020 W = 3 at max_iter 3: <512,4,3,3>, the sign pick over three words, the compare form only."""
    _paths(monkeypatch, "qlp1020_w3", "sampled", 3, shape=(512, 3, 3))
