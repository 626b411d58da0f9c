"""The gather pass of the several-checks-per-lane min-sum kernel (bp_scatter_wide.hip) finds a check's two minima and its argmin edge
from position-carrying keys where rows have at most 64 faults (bp_scatter_edge.h, QS_EDGE_K): key = |bm| + (1 + k / 64) for edge k
of the check's walk, the two smallest keys kept with the v_med3 / v_min the magnitudes used to go through, magnitude = floor(key) - 1
and position = 64 * fraction at the walk's end.  A key is exact below 2^18, i.e. for a second minimum below 2^18 - 1 grid units; a
wavefront whose round ends with a second key at or above that walks the round again in the compare form and stays there.

What can go wrong, and the case that would show it (three paths -- default, QD_BP_NO_FAST_START=1, QD_NO_SCATTER=1 -- bit for bit
against each other and against the double-precision oracle on the device's grid: hard decisions, status words, OSD-0 outputs,
exported posteriors):

  ties       Several edges share the minimum: the first must win and min2 must equal min1.  Windows with ALL PRIORS EQUAL, where every
             magnitude of the early passes ties; row weights 4, 32, 33, 36, 64 and one degree-mixed round (29..36), so that the first
             and last positions of both sign words and position 63, the last one six bits hold, are argmin positions.
  bound      The exactness bound from both sides in one run.  The grid rule gives fine grids for a small max_iter: at max_iter 3 a
             prior of 9 LLR units is 294 912 grid units, above 2^18 - 1, at max_iter 4..7 it is 147 456, below it.  The window has one
             round of weight-24 checks and one of weight-4 checks, 70 % of the faults at 9 units and 30 % at 2.9: _minsum_min2, integer
             flooding min-sum in numpy, shows ON THE CPU (test_bound_window_lies_on_both_sides_of_the_key_limit) that some 64-check
             round of some pass holds second minima on both sides of the bound (lanes that pass and lanes that fail under one ballot),
             that in some pass one round fails while the other passes (both forms run between two barriers), and that no shot trips the
             certificate's m2_limit.  At max_iter 3 the weight-4 round is over the bound from pass 0 on; at 4 and 7 every shot begins
             under it and rounds cross it midway, so a sticky bit is set after passes in the key form -- at 7 it lives through up to seven
             more passes, some of them back under the bound.  The same window at max_iter 50 is on a grid of 2^-11 (a prior of 9 units is
             18 432): the simulation's largest second minimum there is 75 438, so that case stays in the key form for fifty iterations.
  degenerate Rows of weight 2 and 3 among rows of weight 12 in one round: the lightest rows the kernel ever sees.  A check with two edges
             has exactly two keys, and lanes past their degree enter QS_BIG keys from the third position on.  A row of ONE fault has no
             second minimum: the library keeps such a window off the scatter kernel altogether (graph_layout.hip, scatter_form), which
             test_rows_of_one_fault_stay_off_the_scatter_kernel holds on to -- "fewer than two real edges" cannot reach the key form.
  recheck    QD_SCATTER_M2_LIMIT low on the bound window: the certificate (the largest second minimum a workgroup met, collected from
             whichever form produced it) parks the same shots for the gather kernel's recheck pass as before.
  bb72       a fixture window: bb72 r6 at max_iter 50, 64 sampled shots."""
import ctypes
import functools

import numpy as np
import pytest
from scipy.sparse import csc_matrix, csr_matrix

import helpers
import oracle as orc

SWITCHES = ("QD_NO_SCATTER", "QD_BP_NO_FAST_START", "QD_SCATTER_M2_LIMIT", "QD_SCATTER_CPL1")
PATHS = (("default", {}), ("generic", {"QD_BP_NO_FAST_START": "1"}), ("gather", {"QD_NO_SCATTER": "1"}))
SHOTS = 64
ONES_SHOTS = 4         # the all-ones syndrome is one syndrome: a few copies, so that more than one workgroup runs it
NLLR = 6               # posteriors are read back one shot at a time: the first NLLR shots that did not converge
KEY_BOUND = 2 ** 18 - 1        # a second minimum at or above this many grid units has a key of 2^18 or more
TIES = {               # name: row weights, heaviest first; all priors equal
    "t4": [4] * 128,
    "t32": [32] * 96,
    "t33": [33] * 96,
    "t36": [36] * 96,
    "t64": [64] * 72,
    "t29_36": [w for w in range(36, 28, -1) for _ in range(8)],
}
BOUND_ROWS = [24] * 64 + [4] * 64          # slots are sorted by degree: round 0 the weight-24 checks, round 1 the weight-4 checks
STRONG, WEAK = 1.0 / (1.0 + np.exp(9.0)), 0.05
LIGHT_ROWS = {"degenerate": [3, 3, 3, 3, 2, 2, 2, 2], "one_fault": [2, 2, 2, 2, 1, 1, 1, 1]}     # beside 56 rows of weight 12
SHAPES = {name: (128, 2, 2) for name in list(TIES) + ["bound", "degenerate"]}
SHAPES["bb72"] = (256, 2, 2)


def _matrix(which):
    if which in TIES:
        H, _ = helpers.synthetic_window(TIES[which], 3, 6, 20270 + sorted(TIES).index(which))
        return H, np.full(H.shape[1], 0.01)
    if which == "bound":
        H, _ = helpers.synthetic_window(BOUND_ROWS, 3, 6, 20280)
        rng = np.random.default_rng(20281)
        return H, np.where(rng.random(H.shape[1]) < 0.3, WEAK, STRONG)
    if which in LIGHT_ROWS:
        H, pri = helpers.synthetic_window([12] * 56, 3, 6, 20290)
        rng = np.random.default_rng(20291)
        D = H.toarray()
        extra = np.zeros((8, D.shape[1]), dtype=D.dtype)
        for i, w in enumerate(LIGHT_ROWS[which]):
            extra[i, rng.choice(D.shape[1], size=w, replace=False)] = 1
        D = np.concatenate([D, extra], axis=0)[rng.permutation(64)]
        assert sorted(D.sum(axis=1).tolist()) == sorted(LIGHT_ROWS[which]) + [12] * 56
        return csc_matrix(D), pri
    assert which == "bb72"
    H, _, pri = helpers.dem_matrices("bb72_custom_r6_p0.003")
    return H, np.asarray(pri, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _window(which, synd):
    H, pri = _matrix(which)
    if synd == "ones":
        s = np.ones((ONES_SHOTS, H.shape[0]), dtype=np.uint8)
    else:
        s = np.ascontiguousarray(orc.sample_dem(H, H[:1], pri, seed=53, shot0=0, B=SHOTS)[0]).astype(np.uint8)
    s.setflags(write=False)
    return H, pri, s


def _minsum_min2(H, pri, s, max_iter):
    """Integer flooding min-sum on the device's grid rule, magnitudes and signs, one shot at a time: {(shot, pass): second minimum of every
    check, in the library's slot order (degree-descending, stable), so that entries 64 r .. 64 r + 63 are round r of a wavefront} for
    every gather pass a kernel path can run (0 .. the pass that finds the shot converged, or max_iter), and the certificate's bound.
    A message's magnitude is min2 where the edge's own magnitude equals min1 and min1 elsewhere (a tied minimum has min2 = min1)."""
    k = orc.grid_bits(pri, max_iter)[0]
    P = np.rint(np.log((1.0 - pri) / pri) * 2.0 ** k).astype(np.int64)
    R = csr_matrix(H)
    R.sort_indices()
    ptr, c = R.indptr, R.indices
    deg = np.diff(ptr)
    assert deg.min() >= 2
    r = np.repeat(np.arange(R.shape[0]), deg)
    slots = np.argsort(-deg, kind="stable")
    m2_limit = ((1 << 23) - int(np.abs(P).max())) // int(H.sum(axis=0).max()) - 1
    out = {}
    for b in range(s.shape[0]):
        if not s[b].any():
            continue                     # an all-zero syndrome returns without running BP
        L, msg = P.copy(), np.zeros(len(c), dtype=np.int64)
        for t in range(max_iter + 1):
            bm = L[c] - msg
            if t >= 1 and np.array_equal(np.add.reduceat((L[c] <= 0).astype(np.int64), ptr[:-1]) & 1, s[b]):
                break
            mag, sgn = np.abs(bm), (bm <= 0).astype(np.int64)
            sm = mag[np.lexsort((mag, r))]
            min1, min2 = sm[ptr[:-1]], sm[ptr[:-1] + 1]
            out[(b, t)] = min2[slots]
            neg = (s[b][r].astype(np.int64) ^ (np.add.reduceat(sgn, ptr[:-1]) & 1)[r] ^ sgn) == 1
            new = np.where(mag == min1[r], min2[r], min1[r])
            msg = np.where(neg, -new, new)
            L = P + np.bincount(c, weights=msg, minlength=len(P)).astype(np.int64)
    return out, m2_limit


@pytest.mark.parametrize("max_iter", [3, 4, 7, 50])
def test_bound_window_lies_on_both_sides_of_the_key_limit(max_iter):
    """The inputs of the `bound` cases, on the CPU: second minima at or above 2^18 - 1 and below it inside one 64-check round of one pass,
    a pass in which one round has such a check and the other has none, and no shot near the certificate's bound; at max_iter 4 and 7
    rounds that cross the bound after passes under it, at 7 with at least five passes behind the crossing; at 50 none at all."""
    H, pri, s = _window("bound", "sampled")
    m2, m2_limit = _minsum_min2(H, pri, s, max_iter)
    rounds = {key: (v.reshape(2, 64) >= KEY_BOUND).any(axis=1) for key, v in m2.items()}
    mixed = [key for key, v in m2.items() if ((v.reshape(2, 64) >= KEY_BOUND).any(axis=1) & (v.reshape(2, 64) < KEY_BOUND).any(axis=1)).any()]
    split = [key for key, a in rounds.items() if a.sum() == 1]
    passes = {b: 1 + max(t for bb, t in m2 if bb == b) for b in {b for b, _ in m2}}
    # (shot, round, first pass over the bound, passes from there on) of the rounds that begin under the bound
    late = [(b, r, t, passes[b] - t) for b in passes for r in range(2) if not rounds[(b, 0)][r]
            for t in [min((t for t in range(passes[b]) if rounds[(b, t)][r]), default=None)] if t is not None]
    top = max(int(v.max()) for v in m2.values())
    print("bound window, max_iter %d: %d shot-passes, %d with a round on both sides of the bound, %d with one round over it and one under, %d rounds "
          "cross it midway (most passes from there on: %d), largest second minimum %d (m2_limit %d)" % (
              max_iter, len(m2), len(mixed), len(split), len(late), max([x[3] for x in late], default=0), top, m2_limit))
    assert top < m2_limit
    if max_iter == 50:
        assert top < KEY_BOUND
        return
    assert mixed and split
    assert max_iter == 3 or late
    assert max_iter != 7 or max(x[3] for x in late) >= 5


@functools.lru_cache(maxsize=None)
def _reference(which, synd, max_iter):
    """The oracle in double precision on the device's grid, on the CPU: (OSD-0 outputs, flags, {shot: (hard decisions, posteriors)} of
    the first NLLR shots BP leaves unconverged).  Checked here: with max_iter > 1 some shot runs more than one iteration."""
    H, pri, s = _window(which, synd)
    g, form = orc.device_arithmetic(H, pri, "minimum_sum", "parallel", max_iter, 1.0)
    prm = orc.make_params("minimum_sum", "parallel", max_iter, "osd_0", 0, 1.0, form)
    ref, flags = g.decode_batch(s, prm)
    print("%s / %s / max_iter %d: oracle iterations min %d max %d, converged %d of %d" % (
        which, synd, max_iter, flags[:, 1].min(), flags[:, 1].max(), int(flags[:, 0].sum()), len(flags)))
    # (the all-ones syndrome of an odd row weight with equal priors is met by the first iteration's hard decisions)
    assert max_iter == 1 or synd == "ones" or int(flags[:, 1].max()) > 1, (which, synd, max_iter)
    soft = {}
    for b in np.flatnonzero(flags[:, 0] == 0)[:NLLR]:
        conv, dec, llr, it = g.bp(s[b], prm)
        assert not conv and it == flags[b, 1]
        # the device adds grid units in int32 and float: exact, and so comparable bit for bit, below 2^23 units
        assert float(np.abs(llr).max()) * 2.0 ** orc.grid_bits(pri, max_iter)[0] < 2.0 ** 23, (which, synd, max_iter, float(np.abs(llr).max()))
        soft[int(b)] = (dec, llr)
    return ref, flags, soft


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
    # which instantiation ran: entries 12 and 13 of qd_graph_info_ex are the wide kernel's lanes and checks per lane; rows of at most
    # 64 faults take two sign words -- the instantiations that walk in the key form
    arr = (ctypes.c_int32 * 14)()
    assert wg._L.qd_graph_info_ex(wg._h, arr, 14) == 0
    if "QD_NO_SCATTER" not in env:
        assert wg.info()["max_row_weight"] <= 64
        assert (int(arr[12]), int(arr[13]), 2) == SHAPES[which], (which, list(arr))
    return out, dec.info()


def _same(a, b, what):
    for stage in (1, 3):
        bad = np.flatnonzero((a[stage][0] != b[stage][0]).any(axis=1) | (a[stage][1] != b[stage][1]))
        assert bad.size == 0, "%s, stage %d: %d shots differ, first %s" % (what, stage, bad.size, bad[:8])
    assert sorted(a["llr"]) == sorted(b["llr"]), what
    for k in a["llr"]:
        assert np.array_equal(a["llr"][k], b["llr"][k]), "%s: posteriors of shot %d differ" % (what, k)


def _against_oracle(ref3, out, tag):
    ref, flags, soft = ref3
    bits, status = out[3]
    assert np.array_equal((status >> 16) & 1, flags[:, 0]), tag
    assert np.array_equal(status & 0x3FFF, flags[:, 1]), tag
    assert np.array_equal(bits, ref), tag
    assert sorted(out["llr"]) == sorted(soft), tag
    for b, (dec, llr) in soft.items():
        assert np.array_equal(out[1][0][b], dec), (tag, b)
        assert np.array_equal(out["llr"][b].astype(np.float64), llr), (tag, b)      # exact: the grid's posteriors fit a float


def _paths(monkeypatch, which, synd, max_iter, extra_env=None):
    ref3 = _reference(which, synd, max_iter)
    outs = {}
    for tag, env in PATHS:
        if extra_env and tag != "gather":
            env = dict(env, **extra_env)
        outs[tag], info = _run(monkeypatch, which, synd, env, max_iter)
        assert info["scatter_wide_kernel"] == (tag != "gather"), (tag, info)       # the wide scatter kernel really ran
        assert info["bp_fast_start"] == (tag == "default"), (tag, info)
    _same(outs["default"], outs["gather"], "default path against the gather kernel")
    _same(outs["generic"], outs["gather"], "QD_BP_NO_FAST_START=1 against the gather kernel")
    for tag in ("default", "generic", "gather"):
        _against_oracle(ref3, outs[tag], tag)
    st = outs["default"][1][1]
    run = st[(st >> 19) & 1 == 0]
    assert run.size and (run & 0x3FFF).min() >= 1 and (run & 0x3FFF).max() <= max_iter
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [3, 50])
@pytest.mark.parametrize("synd", ["sampled", "ones"])
@pytest.mark.parametrize("which", list(TIES))
def test_argmin_keys_on_tied_minima(gpu, monkeypatch, which, synd, max_iter):
    """All priors equal: every magnitude of the early passes ties, on every row-weight pattern of the module's table."""
    _paths(monkeypatch, which, synd, max_iter)


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [3, 4, 7, 50])
@pytest.mark.parametrize("synd", ["sampled", "ones"])
def test_argmin_keys_across_the_bound(gpu, monkeypatch, synd, max_iter):
    """Second minima on both sides of 2^18 - 1 inside a round and between the rounds of a pass (shown on the CPU by
    test_bound_window_lies_on_both_sides_of_the_key_limit); at max_iter 4 and 7 the bound is crossed midway."""
    _paths(monkeypatch, "bound", synd, max_iter)


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [3, 50])
@pytest.mark.parametrize("synd", ["sampled", "ones"])
def test_argmin_keys_rows_without_a_second_edge(gpu, monkeypatch, synd, max_iter):
    """Rows of weight 2 and 3 beside rows of weight 12 in one round."""
    _paths(monkeypatch, "degenerate", synd, max_iter)


@pytest.mark.gpu
def test_rows_of_one_fault_stay_off_the_scatter_kernel(gpu, monkeypatch):
    """A window with a row of one fault is decoded by the gather kernel: no check without a second edge reaches the key form."""
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    H, pri = _matrix("one_fault")
    info = BatchDecoder(WindowGraph(H, pri), max_iter=3, osd_method="osd_0").info()
    assert not info["scatter_wide_kernel"], info


@pytest.mark.gpu
@pytest.mark.parametrize("limit", ["500000", "1"])
def test_argmin_keys_forced_recheck(gpu, monkeypatch, limit):
    """QD_SCATTER_M2_LIMIT among the window's second minima (500 000: the simulation's largest at max_iter 3 is 884 736, the first pass's
    294 912, so the shots that iterate on trip it and the others do not; 1: every shot with a defect): the parked shots come back from the
    gather kernel's recheck pass."""
    _paths(monkeypatch, "bound", "sampled", 3, extra_env={"QD_SCATTER_M2_LIMIT": limit})


@pytest.mark.gpu
def test_argmin_keys_fixture_window(gpu, monkeypatch):
    """bb72 r6, the whole history as one window (288 checks: <256,8,2,2>), max_iter 50."""
    _paths(monkeypatch, "bb72", "sampled", 50)
