"""BP-LSD (qd_lsd0_kernel<NR>, lsd_kernels.hip) at its kernel bounds and on crafted cluster structures: the post-processor alone on given soft
information -- BatchDecoder(wg, max_iter=1, osd_method=method, osd_order=order).osd0(syndromes, llr) -- against the oracle's Graph.lsd(.., fixed=True)
(integer candidate costs; order 0 through the same call), every shot of every case: corrections bit for bit, the status word whole (bits 20..31 =
min(pivots, 4095); bit 18 = the oracle's `inconsistent`, which must equal H ref != s recomputed here; bit 17 set; the low 16 bits as the staging
kernel left them: zero), and info()["post_kernel"] == "qd_lsd0_kernel".

One wavefront decodes one shot; lane l owns the checks l NR .. l NR + NR - 1; NR = 8, 16, 24, 32 by the number of checks (lsd_nr, restated in
LSD_NR).  Every window is seeded and synthetic (or composed of committed fixture windows), its GF(2) rank computed on the CPU.  On the random sparse
windows of the OSD edges file LSD is bimodal: a shot whose posteriors point at its faults ends after a round with nothing to sweep, any other shot
percolates into one cluster that pivots nearly every check.  The regime in between -- several clusters, some of them swept -- needs a window
with locality: _banded_window.

  A  both sides of every bound of lsd_nr: m = 512 | 513, 1024 | 1025, 1536 | 1537, 2048 | 2049 (2049: the LSD methods are refused with QD_ECAPACITY,
     OSD-0 takes the window).  Banded windows, rank-deficient by three appended rows; 24 shots of 12 faults each (32 at 2048 checks, where fewer of them
     percolate to nearly every check) with noisy posteriors that point at 80 % of them, and two shots with a dependent check spoiled; lsd_0, lsd_cs 1,
     lsd_cs 3, lsd_e 4.
  B  the two extremes on one sparse window per instantiation (m = 400, 900, 1400, 2048): percolating shots (one cluster, pivots in every Q plane,
     more than 64 candidate positions; half of them sampled faults, half the syndrome of every second fault) and one inconsistent shot that takes in
     every fault of the window; lsd_0, lsd_cs 64, lsd_e 10 (lsd_e 15 at m = 400).
  C  crafted soft information per instantiation: all LLRs equal, a three-value alphabet, +-0 and tiny values of both signs, random LLRs with random
     syndromes on sparse windows; equal priors with equal LLRs on _twins_window, where two candidates share the winning cost in every cluster and the
     earlier must win (on the sparse windows a cluster's candidates reach hundreds of rows and seldom tie at the minimum); lsd_cs 1 / 12 / 64 and lsd_e 10.
  D  cluster structure on windows where the path can be reasoned out: _precondition_d says, case by case, what is built, and asserts it on the oracle's
     counters.
  E  state carried by a resident wavefront and by the workspace from shot to shot and from call to call.
  F  block-diagonal windows composed of the committed fixture windows (1296, 1708, 2016 checks): DEM-shaped clusters at NR = 24 / 32 under a higher order.

CASES is the table of all of them; _precondition asserts, on the oracle alone and before anything is compared, that a case holds what it is there for
(minimum counts, not tolerances).  test_every_case_holds_what_it_is_there_for runs the table without a GPU."""
import functools
from collections import namedtuple

import numpy as np
import pytest
from scipy.sparse import block_diag, csc_matrix

import helpers
import oracle as orc
from test_gpu_osd_higher_order_edges import _priors, _sampled, _sparse_window, _spoil

KERNEL = "qd_lsd0_kernel"
LSD_NR = ((512, 8), (1024, 16), (1536, 24), (2048, 32))          # lsd_nr (lsd_kernels.hip): checks up to .. -> checks per lane; beyond the last: refused
ST = {k: i for i, k in enumerate(helpers.LSD_STATS)}


def _lsd_nr(m):
    return next((nr for bound, nr in LSD_NR if m <= bound), 0)


def _banded_window(m, n, dependent, band, seed):
    """A seeded m x n parity-check matrix (dense uint8) with locality, and its priors: fault j sits on 2..4 checks drawn from the `band` consecutive
    checks that start at j (m - dependent) // n (a ring: past the last independent check the band goes on at check 0); each of the last `dependent`
    checks is the sum of two of the others."""
    rng = np.random.default_rng(seed)
    mb = m - dependent
    H = np.zeros((m, n), dtype=np.uint8)
    for j in range(n):
        H[((j * mb) // n + rng.choice(band, size=rng.integers(2, 5), replace=False)) % mb, j] = 1
    for d in range(dependent):
        a, b = rng.choice(mb, size=2, replace=False)
        H[mb + d] = H[a] ^ H[b]
    assert H[:mb].sum(axis=1).min() >= 1 and H.sum(axis=1).max() <= 255 and 2 <= H.sum(axis=0).min() and H.sum(axis=0).max() <= 4 + dependent
    return H, _priors(rng, n)


def _fixture_window(rows):
    """The block-diagonal windows of test_gpu_parity.py (test_bplsd_wide_windows, test_osd0_many_pivot_kernel_wide_windows): bb144 (1008 checks) next to
    bb72 (288), to its own first 700 checks, or to itself."""
    Ha, _, pa = helpers.dem_matrices("bb144_custom_r12_p0.003")
    if rows == 1296:
        Hb, _, pb = helpers.dem_matrices("bb72_custom_r6_p0.003")
    elif rows == 1708:
        Hb, pb = csc_matrix(Ha)[:700], pa
    else:
        Hb, pb = Ha, pa
    H = np.asarray(block_diag([Ha, Hb]).todense(), dtype=np.uint8)
    assert H.shape[0] == rows
    return H, np.concatenate([pa, pb])


def _wide_column_window(m, n, wide, weight, seed):
    """A sparse window with `wide` further faults of column weight `weight` (on checks chosen at random) behind its n faults."""
    H, pri = _sparse_window(m, n, 0, seed)
    rng = np.random.default_rng(seed + 1)
    W = np.zeros((m, wide), dtype=np.uint8)
    for k in range(wide):
        W[rng.choice(m, size=weight, replace=False), k] = 1
    return np.concatenate([H, W], axis=1), np.concatenate([pri, _priors(rng, wide)])


def _absorbing_window():
    """64 x 129: a 64 x 128 sparse window and, last, one fault on the checks 3, 12, 21, 30, 39 -- five lanes of the NR = 8 instantiation."""
    H, pri = _sparse_window(64, 128, 0, 64128)
    col = np.zeros((64, 1), dtype=np.uint8)
    col[[3, 12, 21, 30, 39]] = 1
    return np.concatenate([H, col], axis=1), np.concatenate([pri, [0.01]])


def _staircase_window(blocks):
    """`blocks` disjoint blocks of four checks c0..c3 and five faults: x on c0 c1, y on c1 c2, z on c2 c3, w on c3 alone, v on c0 c2.  The faults z + w
    have the syndrome c2, y + z + w the syndrome c1, x + y + z + w the syndrome c0: a cluster seeded there has to take them one by one."""
    block = np.array([[1, 0, 0, 0, 1], [1, 1, 0, 0, 0], [0, 1, 1, 0, 1], [0, 0, 1, 1, 0]], dtype=np.uint8)
    H = np.asarray(block_diag([block] * blocks).todense(), dtype=np.uint8)
    return H, _priors(np.random.default_rng(blocks), H.shape[1])


def _island_window():
    """99 x 387: three checks that share three faults pairwise (rank 2: the syndrome 1 0 0 is outside their column space), next to the 96 x 384 banded window."""
    tri = np.array([[1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=np.uint8)
    H, pri = _banded_window(96, 384, 0, 8, 96)
    return np.asarray(block_diag([tri, H]).todense(), dtype=np.uint8), np.concatenate([[0.01, 0.02, 0.03], pri])


def _twins_window(blocks):
    """`blocks` disjoint blocks of three checks and four faults: p on c0 c1, q on c1 c2, and twice the same fault, r and r', on c0 c2.  With one prior and
    one LLR a block with the syndrome c0 c2 is decoded as follows: the cluster of c0 takes p (lowest index), the cluster of c2 takes q and absorbs it
    -- valid, LSD-0 says p + q; the growth stage adds r and, from order 2 on, r', both dependent; flipping either replaces p + q (two weights) by one
    fault (one weight): two candidates share the winning cost and r, the earlier, must win."""
    block = np.array([[1, 0, 1, 1], [1, 1, 0, 0], [0, 1, 1, 1]], dtype=np.uint8)
    H = np.asarray(block_diag([block] * blocks).todense(), dtype=np.uint8)
    return H, np.full(H.shape[1], 0.01)


PAIR_ROWS = (5, 300, 590)          # the checks u < t < r of _last_pair_window


def _last_pair_window():
    """600 x 664, built so that the one candidate that beats LSD-0 is the pair of the 63rd and the 64th candidate position of a cluster.  Checks u, t, r;
    faults A on u, T on t r, D on r, 62 copies of A, x on u t, y on t r (a copy of T); A, its copies and T dear (p = 1e-4), x and y cheaper (0.05), D cheap (0.3);
    every other check has one fault of its own.  Syndrome u r, posteriors in the order A, T, D, the copies, x, y: LSD-0 says A + D with T a pivot that is off.
    The growth stage of order 64 adds the 62 copies, x (the clusters meet) and y, all dependent: 64 positions.  A copy alone costs what A saves; x alone
    = A + T + D switches T on; y alone switches T on; a copy with anything switches something dear on; x + y = A + D saves A."""
    u, t, r = PAIR_ROWS
    core = np.zeros((600, 67), dtype=np.uint8)
    core[u, 0] = 1                      # A
    core[[t, r], 1] = 1                 # T
    core[r, 2] = 1                      # D
    core[u, 3:65] = 1                   # the copies of A
    core[[u, t], 65] = 1                # x
    core[[t, r], 66] = 1                # y
    rest = np.setdiff1d(np.arange(600), PAIR_ROWS)
    own = np.zeros((600, 597), dtype=np.uint8)
    own[rest, np.arange(597)] = 1
    pri = np.concatenate([[1e-4, 1e-4, 0.3], np.full(62, 1e-4), [0.05, 0.05], np.full(597, 0.01)])
    return np.concatenate([core, own], axis=1), pri


def _growth_order_window():
    """7 x 6, built so that the clusters of a round are in one order by (size, id) and in the other by id.  f0 on checks 0 2, f1 on 1 2 3, fb on 5 6, gA on 3,
    g on 3 6, and a fault of its own for check 4; syndrome 0 1 5 (that of f0 + f1 + fb + g); posteriors f0 = f1 = fb < gA < g.  Round 1: cluster 0 takes f0,
    cluster 1 takes f1 and absorbs it (two faults, checks 0..3, the syndrome moved to check 3), cluster 5 takes fb (one fault, the syndrome moved to check 6).
    Round 2 by (size, id): cluster 5 first -- its best fault is g, which absorbs cluster 1 and settles both checks: 4 faults, 4 pivots.  By id cluster 1 would
    go first, take gA and be valid, then cluster 5 would take g: the same correction, but 5 faults and 5 pivots in the status word."""
    H = np.zeros((7, 6), dtype=np.uint8)
    for j, rows in enumerate(([0, 2], [1, 2, 3], [5, 6], [3], [3, 6], [4])):
        H[rows, j] = 1
    return H, np.array([0.01, 0.01, 0.01, 0.02, 0.02, 0.01])


def _two_chains_window():
    """Two copies of a repetition-code chain with a doubled fault (4 checks x 6 faults each, the toy of test_oracle.py), side by side: 8 x 12, rank 8."""
    chain = np.array([[1, 1, 0, 0, 0, 0], [0, 1, 1, 1, 0, 0], [0, 0, 1, 1, 1, 0], [0, 0, 0, 0, 1, 1]], dtype=np.uint8)
    return np.asarray(block_diag([chain, chain]).todense(), dtype=np.uint8), np.array([0.01, 0.01, 0.001, 0.2, 0.01, 0.01] * 2)


WINDOWS = {          # name: (generator, its arguments)
    # A: banded, n = 4 m (8200 at 2048; 3 m at 2049, see the test there), three dependent rows
    "a512": (_banded_window, (512, 2048, 3, 8, 512)), "a513": (_banded_window, (513, 2052, 3, 8, 520)),
    "a1024": (_banded_window, (1024, 4096, 3, 8, 1331)), "a1025": (_banded_window, (1025, 4100, 3, 8, 1025)),
    "a1536": (_banded_window, (1536, 6144, 3, 8, 1643)), "a1537": (_banded_window, (1537, 6148, 3, 8, 1944)),
    "a2048": (_banded_window, (2048, 8200, 3, 8, 2955)), "a2049": (_banded_window, (2049, 6147, 3, 8, 2049)),
    # B: sparse, n about 2 m (3 m at 400 checks: with fewer faults no cluster there holds more than 64 candidate positions), three dependent rows
    "b400": (_sparse_window, (400, 1203, 3, 400)), "b900": (_sparse_window, (900, 1803, 3, 900)),
    "b1400": (_sparse_window, (1400, 2803, 3, 1400)), "b2048": (_sparse_window, (2048, 4100, 3, 2048)),
    # C: sparse, four dependent rows
    "c300": (_sparse_window, (300, 613, 4, 300)), "c800": (_sparse_window, (800, 1613, 4, 800)),
    "c1300": (_sparse_window, (1300, 2613, 4, 1300)), "c1800": (_sparse_window, (1800, 3613, 4, 1800)),
    "w510": (_twins_window, (170,)), "w1020": (_twins_window, (340,)), "w1530": (_twins_window, (510,)), "w2040": (_twins_window, (680,)),
    # D
    "t5x8": (_sparse_window, (5, 8, 0, 58)), "t40x63": (_sparse_window, (40, 63, 0, 4063)), "d70x73": (_sparse_window, (70, 73, 3, 7373)),
    "ones2048": (_sparse_window, (2048, 4100, 0, 20480)), "absorb": (_absorbing_window, ()), "chains": (_two_chains_window, ()), "order": (_growth_order_window, ()),
    "near96": (_banded_window, (96, 384, 0, 8, 96)), "stairs": (_staircase_window, (256,)),
    "pair64": (_last_pair_window, ()), "island": (_island_window, ()), "wide600": (_wide_column_window, (600, 1200, 8, 12, 600)),
    # E
    "e200": (_sparse_window, (200, 800, 3, 200)),
    # F
    "f1296": (_fixture_window, (1296,)), "f1708": (_fixture_window, (1708,)), "f2016": (_fixture_window, (2016,)),
}


def _dependent(name):
    gen, args = WINDOWS[name]
    return args[2] if gen in (_banded_window, _sparse_window) else 0


@functools.lru_cache(maxsize=None)
def _window(name):
    """(H as csc, priors, H dense, rank); read-only."""
    gen, args = WINDOWS[name]
    H, pri = gen(*args)
    H, pri = np.ascontiguousarray(H), np.ascontiguousarray(pri, dtype=np.float64)
    Hs = csc_matrix(H)
    rank = orc.Graph(Hs, pri).rank()
    H.setflags(write=False)
    pri.setflags(write=False)
    return Hs, pri, H, rank


def _syndromes(H, e):
    return (e.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)


def _pointed(rng, H, pri, shots, faults, hit=0.8, noise=1.0, push=8.0):
    """`faults` faults per shot, their syndromes, and posteriors = prior LLR + N(0, noise) with `push` taken off a fraction `hit` of the true faults."""
    n = H.shape[1]
    e = np.zeros((shots, n), dtype=np.uint8)
    for b in range(shots):
        e[b, rng.choice(n, size=faults, replace=False)] = 1
    llr = (np.log((1 - pri) / pri)[None, :] + noise * rng.normal(size=e.shape)).astype(np.float32)
    llr[e.astype(bool) & (rng.random(e.shape) < hit)] -= push
    return _syndromes(H, e), llr


@functools.lru_cache(maxsize=None)
def _inputs(name, soft, shots):
    """(syndromes, LLRs as float32, priors) of a case; read-only."""
    Hs, pri, H, rank = _window(name)
    m, n = H.shape
    dep = _dependent(name)
    rng = np.random.default_rng([m, n, shots, sum(map(ord, soft))])
    if soft == "mix":                 # part A: the last two shots leave the column space
        synd, llr = _pointed(rng, H, pri, shots, 12)
        _spoil(synd, m, dep, range(shots - 2, shots))
    elif soft == "percolate":         # part B: the second half are syndromes of every second fault (any syndrome of the column space); the last shot leaves it
        synd, llr = _sampled(rng, H, pri, shots)
        synd[shots // 2:] = _syndromes(H, (rng.random((shots - shots // 2, n)) < 0.5).astype(np.uint8))
        _spoil(synd, m, dep, [shots - 1])
    elif soft == "sampled":
        synd, llr = _sampled(rng, H, pri, shots)
    elif soft == "zero_inside":       # the third shot: no check unsatisfied
        synd, llr = _sampled(rng, H, pri, shots)
        synd[2] = 0
    elif soft == "ties":
        synd, _ = _sampled(rng, H, pri, shots)
        llr = np.full((shots, n), 2.5, np.float32)
    elif soft == "few_values":
        synd, _ = _sampled(rng, H, pri, shots)
        llr = rng.choice(np.array([-1.0, 0.25, 3.0], np.float32), size=(shots, n))
    elif soft == "negzero":
        synd, _ = _sampled(rng, H, pri, shots)
        llr = rng.choice(np.array([0.0, -0.0, 1e-30, -1e-30, 1e-42, -1e-42, 1.0], np.float32), size=(shots, n))
    elif soft == "equal_costs":       # the syndrome c0 c2 in 60 blocks of the twins window
        synd = np.zeros((shots, m), np.uint8)
        for b in range(shots):
            k = rng.choice(m // 3, size=60, replace=False)
            synd[b, 3 * k] = synd[b, 3 * k + 2] = 1
        llr = np.full((shots, n), 1.5, np.float32)
    elif soft == "deep":
        synd = (rng.random((shots, m)) < 0.3).astype(np.uint8)
        llr = rng.normal(size=(shots, n)).astype(np.float32)
    elif soft == "all_ones":
        synd = np.ones((shots, m), np.uint8)
        llr = (np.log((1 - pri) / pri)[None, :] + rng.normal(size=(shots, n))).astype(np.float32)
    elif soft == "absorb":            # the syndrome of the last fault, which has the lowest LLR (second shot: plus two distant faults)
        e = np.zeros((shots, n), np.uint8)
        e[:, n - 1] = 1
        e[1, [5, 77]] = 1
        synd = _syndromes(H, e)
        llr = rng.uniform(2.0, 6.0, size=(shots, n)).astype(np.float32)
        llr[:, n - 1] = -5.0
    elif soft == "growth_order":      # (see _growth_order_window) shot 1: check 4 unsatisfied too
        synd = np.zeros((shots, m), np.uint8)
        synd[:, [0, 1, 5]] = 1
        synd[1, 4] = 1
        llr = np.tile(np.array([-5.0, -5.0, -5.0, 0.5, 0.6, 3.0], np.float32), (shots, 1))
    elif soft == "one_chain":         # checks 1, 2 of the first chain (shot 0) or of the second (shot 1), posteriors that prefer fault 2
        synd = np.zeros((shots, m), np.uint8)
        synd[0, [1, 2]] = 1
        synd[1, [5, 6]] = 1
        llr = np.tile(np.array([3.0, 3.0, 0.5, 1.0, 3.0, 3.0] * 2, np.float32), (shots, 1))
    elif soft == "neighbours":        # two faults 24 columns (6 checks) apart and a third one far away, all pointed at
        e = np.zeros((shots, n), np.uint8)
        for b in range(shots):
            j = int(rng.integers(0, n - 40))
            e[b, [j, j + 24, (j + n // 2) % n]] = 1
        synd = _syndromes(H, e)
        llr = (np.log((1 - pri) / pri)[None, :] + rng.normal(size=e.shape)).astype(np.float32)
        llr[e.astype(bool)] -= 12.0
    elif soft == "last_pair":         # (see _last_pair_window) shot 1: a few of the other checks unsatisfied too
        synd = np.zeros((shots, m), np.uint8)
        synd[:, [PAIR_ROWS[0], PAIR_ROWS[2]]] = 1
        synd[1, [40, 41, 450]] = 1
        llr = np.full((shots, n), 4.0, np.float32)
        llr[:, :67] = np.concatenate([[-10.0, -9.0, -8.0], np.full(62, -5.0), [-4.0, -3.0]]).astype(np.float32)
    elif soft == "island":            # check 0 alone among the three dependent ones, and twelve faults of the banded part with posteriors that point at most of them
        synd, llr = _pointed(rng, H, pri, shots, 12)
        synd[:, :3] = [1, 0, 0]
    elif soft == "many_invalid":      # in 200 of the 256 blocks the last 1..4 faults of the chain x y z w, pointed at: a cluster per block, 1..4 rounds each
        e = np.zeros((shots, n), np.uint8)
        for b in range(shots):
            for k in rng.choice(n // 5, size=200, replace=False):
                e[b, 5 * k + 4 - rng.integers(1, 5):5 * k + 4] = 1
        synd = _syndromes(H, e)
        llr = np.where(e.astype(bool), -5.0, 5.0).astype(np.float32) + rng.uniform(-1, 1, size=e.shape).astype(np.float32)
    elif soft == "wide_first":        # a wide fault with the lowest LLR of all next to the one true fault
        wide = np.flatnonzero(H.sum(axis=0) >= 12)
        e = np.zeros((shots, n), np.uint8)
        llr = (np.log((1 - pri) / pri)[None, :] + rng.normal(size=e.shape)).astype(np.float32)
        for b in range(shots):
            F = wide[b % len(wide)]
            # g: a light fault whose lowest check r is one of F's -- the cluster seeded at r grows first
            r, g = [(r, j) for r in np.flatnonzero(H[:, F]) for j in np.flatnonzero(H[r]) if H[:, j].sum() <= 4 and H[:r, j].sum() == 0][b // len(wide)]
            e[b, g] = 1
            llr[b, F], llr[b, g] = -9.0, -8.0
        synd = _syndromes(H, e)
    elif soft == "state":             # part E: percolating, local, zero and inconsistent shots in a seeded shuffle
        synd, llr = _sampled(rng, H, pri, shots)
        kind = rng.integers(0, 4, size=shots)
        sl, ll = _pointed(rng, H, pri, shots, 3, hit=1.0)
        local = kind == 1
        synd[local], llr[local] = sl[local], ll[local]
        synd[kind == 2] = 0
        _spoil(synd, m, dep, np.flatnonzero(kind == 3))
    elif soft == "local":
        synd, llr = _pointed(rng, H, pri, shots, 3, hit=1.0)
    elif soft == "dem":               # part F: faults at four times their priors, noisy posteriors that lean towards them
        e = (rng.random((shots, n)) < np.minimum(4 * pri, 0.4)).astype(np.uint8)
        synd = _syndromes(H, e)
        llr = (rng.normal(size=(shots, n)) + 2.0).astype(np.float32)
        llr[:3] = np.log((1 - pri) / pri).astype(np.float32)
        llr[e.astype(bool)] -= 3.0
    else:
        raise KeyError(soft)
    synd, llr = np.ascontiguousarray(synd, dtype=np.uint8), np.ascontiguousarray(llr, dtype=np.float32)
    for x in (synd, llr, pri):
        x.setflags(write=False)
    return synd, llr, pri


@functools.lru_cache(maxsize=None)
def _reference(name, soft, shots, method, order):
    """The oracle on the CPU: (corrections, stats [shots, 10] in the order of helpers.LSD_STATS, H ref != s per shot); read-only.  Asserted here for every
    case: the oracle's `inconsistent` is H ref != s, and its clusters add up (every seed ends valid, absorbed, or -- in a flagged shot only -- retired)."""
    Hs, _, H, rank = _window(name)
    synd, llr, pri = _inputs(name, soft, shots)
    ref, st = helpers.oracle_lsd_parallel(Hs, pri, synd, llr, method, order)
    bad = (_syndromes(H, ref) != synd).any(axis=1)
    assert np.array_equal(st[:, ST["inconsistent"]].astype(bool), bad), (name, soft, method, order)
    seeds = synd.sum(axis=1)
    retired = seeds - st[:, ST["clusters"]] - st[:, ST["merges"]]
    assert (retired >= 0).all() and (retired[~bad] == 0).all() and (retired[bad] > 0).all(), (name, soft, retired)
    assert (st[:, ST["pivots"]] <= rank).all() and (st[:, ST["replaced"]] <= st[:, ST["swept"]]).all() and (st[:, ST["swept"]] <= st[:, ST["clusters"]]).all()
    for x in (ref, st, bad):
        x.setflags(write=False)
    return ref, st, bad


Case = namedtuple("Case", "part name soft shots method order")
ORDERS_A = (("lsd_0", 0), ("lsd_cs", 1), ("lsd_cs", 3), ("lsd_e", 4))
ORDERS_B = (("lsd_0", 0), ("lsd_cs", 64), ("lsd_e", 10))
ORDERS_C = (("lsd_cs", 1), ("lsd_cs", 12), ("lsd_cs", 64), ("lsd_e", 10))
BOUND_WINDOWS = ("a512", "a513", "a1024", "a1025", "a1536", "a1537", "a2048")
PLANES_B = {"b400": 5, "b900": 13, "b1400": 21, "b2048": 31}          # Q planes a percolating shot fills, and then some

CASES = (
    [Case("A", w, "mix", 34 if w == "a2048" else 26, me, o) for w in BOUND_WINDOWS for me, o in ORDERS_A]
    + [Case("B", w, "percolate", 8, me, o) for w in PLANES_B for me, o in ORDERS_B] + [Case("B", "b400", "percolate", 8, "lsd_e", 15)]
    + [Case("C", w, soft, 8, me, o) for w in ("c300", "c800", "c1300", "c1800") for soft in ("ties", "few_values", "negzero", "deep") for me, o in ORDERS_C]
    + [Case("C", w, "equal_costs", 4, me, o) for w in ("w510", "w1020", "w1530", "w2040") for me, o in ORDERS_C]
    + [Case("D", w, "sampled", 16, me, o) for w in ("t5x8", "t40x63") for me, o in (("lsd_0", 0), ("lsd_cs", 3), ("lsd_e", 4))]
    + [Case("D", "d70x73", "zero_inside", 16, me, o) for me, o in (("lsd_0", 0), ("lsd_cs", 3), ("lsd_e", 4))]
    + [Case("D", "ones2048", "all_ones", 2, me, o) for me, o in (("lsd_0", 0), ("lsd_cs", 3))]
    + [Case("D", "absorb", "absorb", 2, me, o) for me, o in (("lsd_0", 0), ("lsd_cs", 3), ("lsd_e", 4))]
    + [Case("D", "order", "growth_order", 2, me, o) for me, o in (("lsd_0", 0), ("lsd_cs", 3))]
    + [Case("D", "chains", "one_chain", 2, me, o) for me, o in (("lsd_cs", 15), ("lsd_e", 15))]
    + [Case("D", "near96", "neighbours", 16, me, o) for me, o in (("lsd_cs", 6), ("lsd_e", 6))]
    + [Case("D", "pair64", "last_pair", 2, "lsd_cs", 64)]
    + [Case("D", "island", "island", 12, me, o) for me, o in (("lsd_cs", 3), ("lsd_e", 4))]
    + [Case("D", "stairs", "many_invalid", 4, me, o) for me, o in (("lsd_0", 0), ("lsd_cs", 3))]
    + [Case("D", "wide600", "wide_first", 16, me, o) for me, o in (("lsd_0", 0), ("lsd_cs", 3))]
    + [Case("F", w, "dem", 12, me, o) for w in ("f1296", "f1708", "f2016") for me, o in (("lsd_cs", 1), ("lsd_e", 6))]
)
STATE_WINDOW, STATE_ORDER = "e200", ("lsd_cs", 3)          # part E: its shot count follows the device's compute units


def _id(c):
    return "%s-%s-%s-%s%d" % (c.part, c.name, c.soft, c.method, c.order)


def _col(st, key):
    return st[:, ST[key]]


def _precondition(c):
    """What the case is there for, asserted on the oracle alone.  Returns a line for the record."""
    Hs, pri0, H, rank = _window(c.name)
    m, n = H.shape
    synd, llr, pri = _inputs(c.name, c.soft, c.shots)
    ref, st, bad = _reference(c.name, c.soft, c.shots, c.method, c.order)
    piv, high = _col(st, "pivots"), c.order > 0
    what = ""
    if c.part == "A":
        assert rank == m - 3 and not bad[:-2].any() and bad[-2:].all(), (c, rank, bad)
        few, most = int((piv[:-2] < m / 2).sum()), int((piv[:-2] > m - 64).sum())          # (the spoiled shots reach the rank in any case)
        assert few >= 2 and most >= 2, (c, piv)
        what = "%d shots with pivots < m / 2, %d with pivots > m - 64" % (few, most)
        if high:
            several, replaced = int((_col(st, "swept") >= 2).sum()), int((_col(st, "replaced") > 0).sum())
            assert several >= 2 and replaced >= 4, (c, _col(st, "swept"), _col(st, "replaced"))
            what += ", %d with two or more swept clusters, %d with a replaced solution" % (several, replaced)
    elif c.part == "B":
        assert m - 6 <= rank <= m - 3 and not bad[:-1].any() and bad[-1], (c, rank, bad)
        full = int((piv[:-1] > 64 * PLANES_B[c.name]).sum())
        assert full >= 3 and (_col(st, "clusters")[:-1][piv[:-1] > 64 * PLANES_B[c.name]] == 1).all(), (c, piv, _col(st, "clusters"))
        assert _col(st, "added")[-1] == n, (c, st[-1])          # the inconsistent shot takes in every fault before its cluster is retired
        what = "%d shots with one cluster of more than %d pivots, the spoiled one adds all %d faults in %d rounds" % (full, 64 * PLANES_B[c.name], n, st[-1, ST["rounds"]])
        if high:
            assert _col(st, "max_candidates")[:-1].max() > 64 and (_col(st, "replaced") > 0).any(), (c, _col(st, "max_candidates"))
            what += ", up to %d candidate positions in a cluster" % _col(st, "max_candidates").max()
    elif c.part == "C":
        if c.soft == "equal_costs":
            # (see _twins_window) every cluster is swept and replaced; from order 2 on it has the two tied candidates, and the earlier one is in the solution
            assert len(set(pri.tolist())) == 1 and len(set(llr.ravel().tolist())) == 1 and not bad.any()
            ref0, st0, _ = _reference(c.name, c.soft, c.shots, "lsd_0", 0)
            k = np.flatnonzero(synd[0, ::3])
            assert ref0[0, 4 * k].all() and ref0[0, 4 * k + 1].all() and ref0[0].sum() == 120 and (_col(st0, "clusters") == 60).all()
            assert (_col(st, "swept") == 60).all() and (_col(st, "replaced") == 60).all() and (_col(st, "max_candidates") == min(c.order, 2)).all()
            assert ref[0, 4 * k + 2].all() and ref[0].sum() == 60
            return_tied = 60 if c.order >= 2 else 0
            what = "60 clusters, %d of them with two candidates tied at the minimum" % return_tied
        else:
            assert 3 <= m - rank <= 6, (c, rank)
            if c.soft == "deep":
                assert bad.sum() > c.shots // 2, (c, bad)
            else:
                assert not bad.any() and (_col(st, "swept") > 0).sum() >= 2 and (_col(st, "replaced") > 0).any(), (c, bad, _col(st, "swept"), _col(st, "replaced"))
            what = "%d inconsistent, %d replaced, up to %d candidate positions" % (bad.sum(), (_col(st, "replaced") > 0).sum(), _col(st, "max_candidates").max())
    elif c.part == "D":
        what = _precondition_d(c, H, rank, synd, llr, ref, st, bad)
    elif c.part == "F":
        assert not bad.any() and (_col(st, "clusters") >= 2).all() and (_col(st, "swept") >= 2).sum() >= 6 and (_col(st, "replaced") > 0).sum() >= 2, (c, st)
        what = "%d..%d clusters, %d shots with a replaced solution" % (_col(st, "clusters").min(), _col(st, "clusters").max(), (_col(st, "replaced") > 0).sum())
    return "%-44s %4d x %-5d rank %4d NR %2d, %2d shots: %s" % (_id(c), m, n, rank, _lsd_nr(m), c.shots, what)


def _precondition_d(c, H, rank, synd, llr, ref, st, bad):
    m, n = H.shape
    seeds = synd.sum(axis=1)
    if c.name in ("t5x8", "t40x63"):
        assert m < 64 and not bad.any() and (_col(st, "pivots") > 0).all()
        return "fewer checks than lanes"
    if c.soft == "zero_inside":
        assert rank == m - 3 and seeds[2] == 0 and (seeds[[1, 3]] > 0).all() and not st[2].any() and not bad.any()
        return "shot 2 has no unsatisfied check"
    if c.soft == "all_ones":
        assert rank == m == 2048 and (seeds == m).all() and not bad.any() and (_col(st, "clusters") + _col(st, "merges") == m).all()
        return "2048 seeds, %s clusters at the end" % _col(st, "clusters").tolist()
    if c.soft == "absorb":
        # lsd_0, shot 0: cluster 3 (lowest id, all sizes 0) takes the fault, its four other checks are seeds of four clusters -- one step, four absorbed
        assert seeds[0] == 5 and H[:, n - 1].sum() == 5 and (llr[:, n - 1] < llr[:, :n - 1].min(axis=1)).all() and not bad.any()
        ref0, st0, _ = _reference(c.name, c.soft, c.shots, "lsd_0", 0)
        assert st0[0, ST["added"]] == 1 and st0[0, ST["merges"]] == 4 and st0[0, ST["pivots"]] == 1 and st0[0, ST["rounds"]] == 1 and st0[0, ST["clusters"]] == 1
        assert ref0[0, n - 1] == 1 and ref0[0].sum() == 1
        assert st0[1, ST["merges"]] >= 4
        if c.order:
            assert _col(st, "grown")[0] == c.order and st[0, ST["added"]] == 1 + c.order
        return "one growth step absorbs four clusters"
    if c.soft == "growth_order":
        ref0, st0, _ = _reference(c.name, c.soft, c.shots, "lsd_0", 0)
        assert ref0[0].tolist() == [1, 1, 1, 0, 1, 0] and ref0[1].tolist() == [1, 1, 1, 0, 1, 1] and not bad.any()
        assert [st0[0, ST[k]] for k in ("rounds", "added", "pivots", "merges", "clusters")] == [2, 4, 4, 2, 1]
        assert [st0[1, ST[k]] for k in ("rounds", "added", "pivots", "merges", "clusters")] == [2, 5, 5, 2, 2]
        return "round 2 grows cluster 5 (one fault) before cluster 1 (two): 4 pivots, not 5"
    if c.soft == "one_chain":
        # the cluster of a chain can take the chain's six faults and no more: the growth stage asks for up to 15 and runs dry
        ref0, st0, _ = _reference(c.name, c.soft, c.shots, "lsd_0", 0)
        assert (_col(st0, "added") == 1).all() and (_col(st, "added") == 6).all() and (_col(st, "grown") == 5).all() and c.order == 15
        assert (_col(st, "pivots") == 4).all() and (_col(st, "max_candidates") == 2).all() and (_col(st, "replaced") == 1).all() and not bad.any()
        return "growth stage ends with the chain's 6 faults added, 5 of them grown, order 15"
    if c.soft == "neighbours":
        # every fault is pointed at: LSD-0 ends with valid clusters apart; the growth stage makes two of them meet
        ref0, st0, _ = _reference(c.name, c.soft, c.shots, "lsd_0", 0)
        met = int(((_col(st0, "clusters") >= 2) & (_col(st, "merges") > _col(st0, "merges")) & (_col(st0, "rounds") <= 2)).sum())
        assert met >= 3 and not bad.any(), (c, _col(st0, "clusters"), _col(st, "merges") - _col(st0, "merges"))
        return "%d shots in which the growth stage merges valid clusters" % met
    if c.soft == "last_pair":
        assert _lsd_nr(m) == 16 and not bad.any() and c.order == 64
        ref0, st0, _ = _reference(c.name, c.soft, c.shots, "lsd_0", 0)
        assert np.flatnonzero(ref0[0]).tolist() == [0, 2] and st0[0, ST["pivots"]] == 3 and st0[0, ST["clusters"]] == 2
        assert np.flatnonzero(ref[0]).tolist() == [65, 66] and ref[1, [65, 66]].all() and not ref[1, :65].any()
        assert (_col(st, "max_candidates") == 64).all() and (_col(st, "grown") >= 64).all() and (_col(st, "replaced") == 1).all() and (_col(st, "merges") == 1).all()
        return "the winning candidate is the pair of positions 63 and 64 of 64"
    if c.soft == "island":
        # the cluster of check 0 takes the three faults of its island and is retired; the clusters of the banded part are swept all the same
        swept = int((_col(st, "swept") > 0).sum())
        assert rank == m - 1 and bad.all() and (_col(st, "clusters") >= 1).all() and swept >= c.shots // 2 and (_col(st, "replaced") > 0).sum() >= 2, (c, st)
        return "a retired cluster in every shot, swept clusters next to it in %d" % swept
    if c.soft == "many_invalid":
        # a round grows no more clusters than its list holds, the lists shrink, and round 1 grows at most `seeds` clusters: more than
        # (added - seeds) / (rounds - 1) clusters are still invalid after round 1
        ref0, st0, _ = _reference(c.name, c.soft, c.shots, "lsd_0", 0)
        live = (_col(st0, "added") - seeds) / np.maximum(_col(st0, "rounds") - 1, 1)
        assert (seeds == 200).all() and (_col(st0, "rounds") == 4).all() and (_col(st0, "merges") == 0).all()
        assert (live > 64).all() and not bad.any() and (_col(st0, "clusters") == 200).all(), (c, live)
        return "at least %s clusters invalid after round 1" % np.ceil(live).astype(int).tolist()
    if c.soft == "wide_first":
        # the wide fault F has the lowest LLR of all and touches the one seed r... so the first growth step takes it, and its eleven other checks, all free, join
        # at once: more than QL_NB = 8 checks to rescan
        assert _lsd_nr(m) == 16 and H.sum(axis=0).max() == 12 and not bad.any()
        for b in range(c.shots):
            F = int(np.argmin(llr[b]))
            assert H[:, F].sum() == 12 and (H[:, F] & synd[b]).sum() >= 1 and (H[:, F] & (1 - synd[b])).sum() >= 9, (c, b)
        ref0, st0, _ = _reference(c.name, c.soft, c.shots, "lsd_0", 0)
        assert (_col(st0, "added") == 2).all() and (_col(st0, "pivots") == 2).all() and (ref0.sum(axis=1) == 1).all()
        return "a fault of weight 12 joins first: nine or more free checks at once"
    raise KeyError(c)


def _device(name, method, order, *batches):
    """One decoder, one osd0 call per (syndromes, LLRs) batch in turn: [(corrections, status words as uint32), ...] on the host.  The decoder lives in this
    frame alone: nothing a failing assertion keeps alive holds a device handle."""
    import torch
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    Hs, pri = _window(name)[:2]
    wg = WindowGraph(Hs, pri)
    dec = BatchDecoder(wg, max_iter=1, osd_method=method, osd_order=order)
    kernel = dec.info()["post_kernel"]
    assert kernel == KERNEL, (name, method, order, kernel)
    out = []
    for synd, llr in batches:
        bits, status = dec.osd0(torch.tensor(synd, device="cuda"), torch.tensor(llr, device="cuda"))        # (copies: the cached inputs are read-only)
        out.append((unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy().view(np.uint32)))
    return out


def _expected_status(st, bad):
    return ((1 << 17) | (bad.astype(np.int64) << 18) | (np.minimum(_col(st, "pivots"), 4095) << 20)).astype(np.uint32)


def _assert_same(tag, err, status, ref, st, bad):
    for b in range(len(ref)):
        assert np.array_equal(err[b], ref[b]), (tag, b, np.flatnonzero(err[b] != ref[b])[:8], st[b])
    assert np.array_equal((status >> 20) & 0xFFF, np.minimum(_col(st, "pivots"), 4095)), tag
    assert np.array_equal(((status >> 18) & 1).astype(bool), bad), tag
    assert ((status >> 17) & 1).all() and not (status & 0xFFFF).any(), tag
    assert np.array_equal(status, _expected_status(st, bad)), tag


def _compare(c):
    print(_precondition(c))
    ref, st, bad = _reference(c.name, c.soft, c.shots, c.method, c.order)
    synd, llr, _ = _inputs(c.name, c.soft, c.shots)
    (err, status), = _device(c.name, c.method, c.order, (synd, llr))
    _assert_same(_id(c), err, status, ref, st, bad)


def test_case_table_covers_every_instantiation_and_bound():
    assert [nr for _, nr in LSD_NR] == [8, 16, 24, 32]
    sizes = {_window_shape(w)[0] for w in BOUND_WINDOWS + ("a2049",)}          # a2049: the window of the refusal test
    for bound, nr in LSD_NR:
        assert {bound, bound + 1} <= sizes and _lsd_nr(bound) == nr and _lsd_nr(bound + 1) == dict(LSD_NR).get(bound + 512, 0)
    for part, windows in (("B", PLANES_B), ("C", ("c300", "c800", "c1300", "c1800")), ("C, equal costs", ("w510", "w1020", "w1530", "w2040"))):
        assert [_lsd_nr(_window_shape(w)[0]) for w in windows] == [8, 16, 24, 32], part
    assert [_lsd_nr(_window_shape(w)[0]) for w in ("f1296", "f1708", "f2016")] == [24, 32, 32]
    assert len({_id(c) for c in CASES}) == len(CASES)


def _window_shape(name):
    gen, args = WINDOWS[name]
    return (args[0], args[1]) if gen in (_banded_window, _sparse_window, _wide_column_window) else (3 * args[0], 4 * args[0]) if gen is _twins_window else _window(name)[2].shape


def test_every_case_holds_what_it_is_there_for():
    """The whole table on the oracle alone (no GPU): every case's preconditions, and those of part E at a nominal 32 compute units (the device test
    asserts them again for the shots it runs)."""
    for c in CASES:
        print(_precondition(c))
    print(_precondition_state(4 * 8 * 32 + 5))


# ---- the device ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_lsd_case(gpu, case):
    _compare(case)


@pytest.mark.gpu
def test_window_of_2049_checks_is_refused_for_lsd_only(gpu):
    """lsd_nr(2049) = 0: qd_decoder_create refuses the LSD methods with QD_ECAPACITY (-4) and names LSD; OSD-0 takes the same window.  (6147 faults: OSD-0's
    own layout sorts the columns in LDS, 8 bytes for each of the next power of two, and takes 8192 of them beside the row state of 2049 checks, not 16384.)"""
    from quits_amd._lib import QdError
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    Hs, pri, H, rank = _window("a2049")
    assert H.shape == (2049, 6147) and rank == 2046 and _lsd_nr(2049) == 0 and _lsd_nr(2048) == 32
    wg = WindowGraph(Hs, pri)
    for method, order in (("lsd_0", 0), ("lsd_cs", 1), ("lsd_e", 4)):
        with pytest.raises(QdError) as exc:
            BatchDecoder(wg, max_iter=1, osd_method=method, osd_order=order)
        code, text = exc.value.code, str(exc.value)
        del exc
        assert code == -4 and "LSD" in text, (method, code, text)
    dec = BatchDecoder(wg, max_iter=1, osd_method="osd_0")
    assert dec.info()["post_kernel"].startswith("qd_osd0"), dec.info()


def _precondition_state(shots):
    name, (method, order) = STATE_WINDOW, STATE_ORDER
    m, n = _window(name)[2].shape
    ref, st, bad = _reference(name, "state", shots, method, order)
    piv, seeds = _col(st, "pivots"), _inputs(name, "state", shots)[0].sum(axis=1)
    kinds = {"three planes": int((piv > 128).sum()), "one plane": int(((piv > 0) & (piv <= 64)).sum()), "zero": int((seeds == 0).sum()), "inconsistent": int(bad.sum())}
    assert all(v >= shots // 8 for v in kinds.values()), kinds
    ref2, st2, bad2 = _reference(name, "local", 8, method, order)
    assert (_col(st2, "pivots") <= 16).all() and (_col(st2, "pivots") > 0).all() and not bad2.any()
    return "E-%s-state: %d x %d, %d shots: %s; then 8 shots of at most %d pivots" % (name, m, n, shots, kinds, _col(st2, "pivots").max())


@pytest.mark.gpu
def test_state_of_a_resident_wavefront_and_of_the_workspace(gpu):
    """Eight wavefronts per compute unit stay resident and take shots from a work counter; each keeps its Q planes, pivot columns and sweep lists in a
    workspace slot from shot to shot, and a plane is cleared only when a shot's pivot count first reaches it.  More than four shots per wavefront, of
    four kinds in a seeded shuffle (percolating: more than 128 pivots, three planes; local; zero; inconsistent); the same call twice on one decoder
    (identical output), then eight local shots on the same decoder, over whatever the big calls left in the slots."""
    import torch
    shots = 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    print(_precondition_state(shots))
    method, order = STATE_ORDER
    ref, st, bad = _reference(STATE_WINDOW, "state", shots, method, order)
    ref3, st3, bad3 = _reference(STATE_WINDOW, "local", 8, method, order)
    big, small = _inputs(STATE_WINDOW, "state", shots)[:2], _inputs(STATE_WINDOW, "local", 8)[:2]
    (err, status), (err2, status2), (err3, status3) = _device(STATE_WINDOW, method, order, big, big, small)
    _assert_same("state, first call", err, status, ref, st, bad)
    assert np.array_equal(err, err2) and np.array_equal(status, status2)
    _assert_same("state, small call after the big ones", err3, status3, ref3, st3, bad3)
