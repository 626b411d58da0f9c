"""Higher-order OSD (osd_cs / osd_e) at its kernel boundaries and on crafted inputs: the post-processor alone, on given soft information,
against the oracle's osd_w (integer candidate costs), bit for bit and status word for status word.

Two device forms exist: the panel kernel qd_osdcs_kernel (osd_cs.hip: three instantiations chosen by qd_osdcs_layout) and the row form of
qd_osd0_reg_kernel (osd_kernels.hip: QD_OSDCS_OLD=1, and every window the layout refuses).  The other GPU tests run them on fixture windows
(m = 252, 1008, 1350, 1708; posteriors BP made from sampled syndromes) only.  Here every window is synthetic and seeded (_sparse_window:
column weight 3..4, row weight far below 255, priors over two decades so that the integer fault weights differ; `dependent` appended rows,
each the sum of two earlier ones, make the window rank-deficient), the GF(2) rank is computed on the CPU, and every case asserts on the
oracle alone that it holds what it is there for, before anything is compared.

  A  both sides of every bound of qd_osdcs_layout (restated in _panel_variant): m 512 | 513, 1024 | 1025, 1408 | 1409 (all six rank-deficient
     by three appended rows: a.rank < m with a full last Q word); n 4096 | 4097 at m = 256, 10240 | 10241 at m = 576, and the largest n the
     LDS takes at m = 1025 | one more.  osd_cs 3 and osd_e 4 (osd_cs 1 at the LDS bound), half of the shots of a rank-deficient window
     with a syndrome outside the column space.
  B  crafted soft information on one window per instantiation (m = 192, 640, 1100, rank-deficient by four): all LLRs equal, a three-value
     alphabet, +-0 and tiny values, random LLRs with random syndromes (mostly inconsistent), and equal priors with equal LLRs, where many
     candidates tie on cost and the earliest must win.
  C  sweep and elimination edges on the smallest instantiation: fewer non-pivot columns than the order, none at all, windows of fewer
     than 64 checks and faults, the last pivot in the last, partial batch of 64 columns; the largest orders (osd_e 15, osd_cs 64) on the
     second instantiation.
  D  shot-to-shot state of a persistent workgroup: more shots than workgroups, inconsistent and consistent syndromes following each other
     within a workgroup.

Every comparison: corrections bit for bit; status bits 20..31 = min(pivots, 4095); bit 18 = (H ref != syndrome) computed here from the
oracle's correction; bit 17 set; BatchDecoder.info()["post_kernel"] names the form the case is there for.  Wherever the panel kernel takes
the window the row form runs too and must return the same bits and status words.

Two notes on the windows: a 70 x 73 window with n - rank = 3 has full row rank, so no syndrome is inconsistent on it -- part D runs a second
70 x 73 window, of rank 67 (three dependent rows); and the largest orders run on a 576 x 1203 window of their own (the 576-check windows of
part A have 10240 faults: the oracle's 32767 candidates would take seconds each)."""
import functools

import numpy as np
import pytest
from scipy.sparse import csc_matrix

import helpers
import oracle as orc

pytestmark = pytest.mark.gpu

PANEL, ROWS = "qd_osdcs_kernel", "qd_osd0_reg_kernel<row form>"
LDS_BYTES = 160 * 1024          # QD_LDS_BYTES
SHAPES = {1: (256, 2, 8, 16), 2: (512, 2, 16, 20), 3: (512, 3, 22, 40)}     # cs_shape: threads, Q columns per thread, words per column, sorted items per thread


def _panel_variant(m, n):
    """qd_osdcs_layout (osd_cs.hip) restated: the instantiation that takes an m x n window, 0 = none (the row form runs)."""
    var = 1 if m <= 512 else (2 if m <= 1024 else (3 if m <= 1408 else 0))
    if var == 0 or n >= 65535:
        return 0
    T, CPT, NWD, IPT = SHAPES[var]
    if n > T * IPT:
        return 0
    al = lambda x: (x + 15) & ~15
    npiv, out_bytes = T * CPT, 4 * ((n + 31) // 32)
    o_var = 2 * 64 * (NWD + 1) * 8 + 2 * npiv * 8 + 64 * NWD * 8 + 2 * NWD * 8 + NWD * 64 * 2 + 2 * npiv * 2 + 2048       # CsLds<T, CPT, NWD>::o_var
    total = max(o_var + 2 * al(out_bytes) + al(2 * n), al(8 * n) + 2048)
    return var if total <= LDS_BYTES else 0


# the largest n whose 8-byte sort keys and 2048 bytes of splitters and counters fit the LDS: the bound of the third instantiation (20480 = 512 x 40
# items would not fit); 20224 by hand
NMAX3 = max(n for n in range(20000, 20481) if _panel_variant(1025, n) == 3)

WINDOWS = {          # name: (checks, faults, dependent rows among the checks, seed)
    "m512": (512, 1031, 3, 512), "m513": (513, 1031, 3, 513), "m1024": (1024, 2055, 3, 1024), "m1025": (1025, 2055, 3, 1025),
    "m1408": (1408, 2821, 3, 1408), "m1409": (1409, 2821, 3, 1409),
    "n4096": (256, 4096, 0, 4096), "n4097": (256, 4097, 0, 4097), "n10240": (576, 10240, 0, 10240), "n10241": (576, 10241, 0, 10241),
    "nmax": (1025, NMAX3, 0, 20224), "nmax1": (1025, NMAX3 + 1, 0, 20225),
    "b192": (192, 397, 4, 192), "b640": (640, 1293, 4, 640), "b1100": (1100, 2213, 4, 1100),
    "c70x73": (70, 73, 0, 7073), "c70x70": (70, 70, 0, 7002), "t5x8": (5, 8, 0, 58), "t40x63": (40, 63, 0, 4063),
    "m576": (576, 1203, 0, 576), "d70x73": (70, 73, 3, 7373),
}


def _priors(rng, n):
    return 10.0 ** rng.uniform(-3.5, -1.5, size=n)          # integer weights round(log(1 / p) * 2^18) from 0.9e6 to 2.1e6


def _sparse_window(m, n, dependent, seed):
    """A seeded m x n parity-check matrix (dense uint8) and its priors.  Every fault sits on 3 or 4 of the first m - dependent checks, dealt from
    shuffled decks of those checks so that the row weights differ by a few at most; each of the last `dependent` checks is the sum of two of the
    others."""
    rng = np.random.default_rng(seed)
    mb = m - dependent
    cw = rng.integers(3, 5, size=n)
    total = int(cw.sum())
    deck = np.concatenate([rng.permutation(mb) for _ in range(total // mb + 1)])[:total]
    start = np.concatenate([[0], np.cumsum(cw)])
    H = np.zeros((m, n), dtype=np.uint8)
    for j in range(n):
        rows = deck[start[j]:start[j + 1]]
        if len(set(rows.tolist())) < len(rows):               # a fault that straddles two decks may meet a check twice
            rows = rng.choice(mb, size=cw[j], replace=False)
        H[rows, j] = 1
    for d in range(dependent):
        a, b = rng.choice(mb, size=2, replace=False)
        H[mb + d] = H[a] ^ H[b]
    assert H.sum(axis=1).min() >= 1 and H.sum(axis=1).max() <= 255 and 3 <= H.sum(axis=0).min() and H.sum(axis=0).max() <= 4 + dependent
    return H, _priors(rng, n)


def _last_batch_window():
    """H = [A | I] with 96 checks: A has 135 faults of weight 3..4 on 90 of the checks and six zero rows; 231 faults, not a multiple of 64."""
    rng = np.random.default_rng(96231)
    A90, _ = _sparse_window(90, 135, 0, 96135)
    zero = np.sort(rng.choice(96, size=6, replace=False))
    A = np.zeros((96, 135), dtype=np.uint8)
    A[np.setdiff1d(np.arange(96), zero)] = A90
    return np.concatenate([A, np.eye(96, dtype=np.uint8)], axis=1), _priors(rng, 231), zero


@functools.lru_cache(maxsize=None)
def _window(name):
    """(H as csc, priors, H dense, rank); read-only."""
    if name == "last":
        H, pri, _ = _last_batch_window()
    else:
        H, pri = _sparse_window(*WINDOWS[name])
    Hs = csc_matrix(H)
    rank = orc.Graph(Hs, pri).rank()
    H.setflags(write=False)
    pri.setflags(write=False)
    return Hs, pri, H, rank


def _sampled(rng, H, pri, shots):
    """Faults drawn at twice their priors (four per shot at the least), their syndromes, and noisy posteriors that lean towards half of them: with the
    other half left at its prior OSD-0 often settles on a costlier fault set than the sweep finds (posteriors that point at every fault leave the sweep
    nothing to win)."""
    e = (rng.random((shots, H.shape[1])) < np.maximum(2.0 * pri, 4.0 / H.shape[1])).astype(np.uint8)
    synd = (e.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)
    llr = (np.log((1 - pri) / pri)[None, :] + 2.0 * rng.normal(size=e.shape)).astype(np.float32)
    llr[e.astype(bool) & (rng.random(e.shape) < 0.5)] -= 4.0
    return synd, llr


def _spoil(synd, m, dependent, which):
    """Flip the bit of one dependent check in the shots `which`: a dependent check's bit is fixed by two others, so the syndrome leaves the column space."""
    assert dependent > 0
    for k, b in enumerate(which):
        synd[b, m - 1 - (k % dependent)] ^= 1


@functools.lru_cache(maxsize=None)
def _inputs(name, soft, shots):
    """(syndromes, LLRs as float32, priors) of a case; read-only.  soft: 'sampled' (the second half of a rank-deficient window's shots spoiled),
    'mixed' (a seeded half of the shots spoiled), or one of part B's crafted sets."""
    Hs, pri, H, rank = _window(name)
    m, n = H.shape
    dep = WINDOWS[name][2] if name in WINDOWS else 0
    rng = np.random.default_rng([m, n, shots, sum(map(ord, soft))])
    synd, llr = _sampled(rng, H, pri, shots)
    if soft == "sampled":
        if dep:
            _spoil(synd, m, dep, range(shots // 2, shots))
    elif soft == "mixed":
        _spoil(synd, m, dep, np.flatnonzero(rng.random(shots) < 0.5))
    elif soft == "ties":
        llr = np.full((shots, n), 2.5, np.float32)
    elif soft == "few_values":
        llr = rng.choice(np.array([-1.0, 0.25, 3.0], np.float32), size=(shots, n))
    elif soft == "negzero":
        llr = rng.choice(np.array([0.0, -0.0, 1e-30, -1e-30, 1.0], np.float32), size=(shots, n))
    elif soft == "deep":
        synd = (rng.random((shots, m)) < 0.3).astype(np.uint8)
        llr = rng.normal(size=(shots, n)).astype(np.float32)
    elif soft == "equal_costs":
        pri = np.full(n, 0.01)
        llr = np.full((shots, n), 1.5, np.float32)
    elif soft == "last_batch":
        # the 135 faults of A first, then the identity block, and within it the faults of A's zero rows last of all: they alone reach those
        # six checks, so the elimination runs through every column and its last pivots come from the batch of 231 - 192 = 39 columns
        zero = _last_batch_window()[2]
        llr = rng.uniform(-2.0, 2.0, size=(shots, n)).astype(np.float32)
        llr[:, 135:] = rng.uniform(5.0, 6.0, size=(shots, 96)).astype(np.float32)
        llr[:, 135 + zero] = rng.uniform(10.0, 11.0, size=(shots, 6)).astype(np.float32)
        synd = (rng.random((shots, m)) < 0.3).astype(np.uint8)
    else:
        raise KeyError(soft)
    synd, llr = np.ascontiguousarray(synd), np.ascontiguousarray(llr)
    for x in (synd, llr, pri):
        x.setflags(write=False)
    return synd, llr, pri


def _candidates(method, order, n, rank):
    w = min(order, n - rank)
    return (1 << w) - 1 if method == "osd_e" else (n - rank) + w * (w - 1) // 2


@functools.lru_cache(maxsize=None)
def _reference(name, soft, shots, method, order):
    """The oracle on the CPU: (corrections, pivots, inconsistent, winners).  Asserted here, on the oracle alone: the elimination reaches the window's
    rank and the sweep looks at the number of candidates the window's rank and the order give."""
    Hs, _, H, rank = _window(name)
    synd, llr, pri = _inputs(name, soft, shots)
    ref, st = helpers.oracle_osd_w_parallel(Hs, pri, synd, llr, method, order)
    bad = ((ref.astype(np.int64) @ H.T.astype(np.int64)) % 2 != synd).any(axis=1)
    assert (st[:, 0] == rank).all(), (name, soft, st[:, 0], rank)
    assert (st[:, 2] == _candidates(method, order, H.shape[1], rank)).all(), (name, soft, method, order, st[:, 2])
    print("%-7s %-11s %-6s %2d: %d x %d, rank %d, %d shots, oracle: %d inconsistent, %d with a winning candidate, %d candidates per shot" % (
        name, soft, method, order, H.shape[0], H.shape[1], rank, shots, int(bad.sum()), int((st[:, 1] > 0).sum()), int(st[0, 2])))
    for x in (ref, st, bad):
        x.setflags(write=False)
    return ref, st[:, 0], bad, st[:, 1]


def _device(name, soft, shots, method, order, monkeypatch, rows):
    import torch
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    Hs = _window(name)[0]
    synd, llr, pri = _inputs(name, soft, shots)
    if rows:
        monkeypatch.setenv("QD_OSDCS_OLD", "1")
    else:
        monkeypatch.delenv("QD_OSDCS_OLD", raising=False)
    wg = WindowGraph(Hs, pri)
    dec = BatchDecoder(wg, max_iter=1, osd_method=method, osd_order=order)
    kernel = dec.info()["post_kernel"]
    bits, status = dec.osd0(torch.tensor(synd, device="cuda"), torch.tensor(llr, device="cuda"))        # (copies: the cached inputs are read-only)
    return unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy(), kernel


def _compare(name, soft, shots, method, order, monkeypatch, variant):
    """One case on the device, in the form the window takes by default (variant 1..3: the panel kernel, 0: the row form) and, where that is the
    panel kernel, in the row form too, against the oracle."""
    m, n = _window(name)[2].shape
    assert _panel_variant(m, n) == variant, (name, _panel_variant(m, n))
    ref, pivots, bad, _ = _reference(name, soft, shots, method, order)
    err, status, kernel = _device(name, soft, shots, method, order, monkeypatch, rows=False)
    print("%-7s %-11s %-6s %2d: post_kernel %s%s" % (name, soft, method, order, kernel, " (instantiation %d), and the row form" % variant if variant else ""))
    assert kernel == (PANEL if variant else ROWS), (name, kernel)
    for b in range(shots):
        assert np.array_equal(err[b], ref[b]), (name, soft, method, order, b, np.flatnonzero(err[b] != ref[b])[:8])
    assert np.array_equal((status >> 20) & 0xFFF, np.minimum(pivots, 4095)), (name, soft, method, order)
    assert np.array_equal(((status >> 18) & 1).astype(bool), bad), (name, soft, method, order)
    assert ((status >> 17) & 1).all()
    if variant:
        err2, status2, kernel2 = _device(name, soft, shots, method, order, monkeypatch, rows=True)
        assert kernel2 == ROWS, (name, kernel2)
        assert np.array_equal(err, err2) and np.array_equal(status, status2), (name, soft, method, order)


# ---- A: both sides of every bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,order", [("osd_cs", 3), ("osd_e", 4)])
@pytest.mark.parametrize("name,variant", [("m512", 1), ("m513", 2), ("m1024", 2), ("m1025", 3), ("m1408", 3), ("m1409", 0),
                                          ("n4096", 1), ("n4097", 0), ("n10240", 2), ("n10241", 0)])
def test_both_sides_of_every_instantiation_bound(gpu, monkeypatch, name, variant, method, order):
    """Eight shots per window.  The m windows are rank-deficient by their three appended rows (asserted), so the elimination ends by a.rank < m with
    the last Q word of the instantiation full at 512, 1024 and 1408; four of their eight syndromes are outside the column space."""
    m, n, dep, _ = WINDOWS[name]
    rank = _window(name)[3]
    _, _, bad, winners = _reference(name, "sampled", 8, method, order)
    if dep:
        assert m - dep - 2 <= rank <= m - dep, (name, rank)
        assert not bad[:4].any() and bad[4:].all(), (name, bad)
    else:
        assert rank == m and not bad.any(), (name, rank, bad)
    assert (winners > 0).any(), (name, "no candidate ever beat OSD-0: the sweep is not exercised")
    _compare(name, "sampled", 8, method, order, monkeypatch, variant)


@pytest.mark.parametrize("name,variant", [("nmax", 3), ("nmax1", 0)])
def test_largest_window_the_lds_sort_takes(gpu, monkeypatch, name, variant):
    """al(8 n) + 2048 <= 160 KB: n = 20224 sorts in LDS (third instantiation, one workgroup per CU), 20225 goes to the row form.  Two shots, osd_cs 1
    (the oracle takes about a second per shot here: 19 200 single-column candidates over 20 224 faults)."""
    assert NMAX3 == 20224 and 8 * NMAX3 + 2048 == LDS_BYTES
    _, _, bad, winners = _reference(name, "sampled", 2, "osd_cs", 1)
    assert _window(name)[3] == 1025 and not bad.any() and (winners > 0).any()
    _compare(name, "sampled", 2, "osd_cs", 1, monkeypatch, variant)


# ---- B: crafted soft information ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", ["ties", "few_values", "negzero", "deep", "equal_costs"])
@pytest.mark.parametrize("name,variant", [("b192", 1), ("b640", 2), ("b1100", 3)])
def test_crafted_soft_information(gpu, monkeypatch, name, variant, soft):
    """16 shots, osd_cs 2, one window per instantiation, each rank-deficient by 4 (asserted: 3..6).
    ties -- one LLR: the sample sort's keys differ in the fault index alone (splitters, buckets and the rank sort all decide on the low word);
    few_values -- three LLRs: tie groups of hundreds of faults that straddle buckets;
    negzero -- +0, -0 and +-1e-30 must order as the oracle's '<' on doubles orders them (+-0 tie, on the fault index);
    deep -- random LLRs and random syndromes of density 0.3: outside the column space for most shots (asserted: more than half);
    equal_costs -- one prior and one LLR: every candidate costs a multiple of one weight, so many tie and the earliest must win.  That ties occur
    at the minimum is asserted on the oracle: priors moved by a relative 1e-6 at random can reorder none but exactly tied candidates, and four such
    perturbations do not crown the same candidate in some shot."""
    m = WINDOWS[name][0]
    assert 3 <= m - _window(name)[3] <= 6
    _, _, bad, winners = _reference(name, soft, 16, "osd_cs", 2)
    if soft == "deep":
        assert bad.sum() > 8, (name, bad)
    else:
        assert not bad.any(), (name, soft, bad)
    assert (winners > 0).any(), (name, soft)
    if soft == "equal_costs":
        Hs = _window(name)[0]
        synd, llr, pri = _inputs(name, soft, 16)
        rng = np.random.default_rng(m)
        w = np.array([helpers.oracle_osd_w_parallel(Hs, pri * (1.0 + 1e-6 * rng.uniform(-1, 1, size=len(pri))), synd, llr, "osd_cs", 2)[1][:, 1] for _ in range(4)])
        tied = int(((w != w[0]).any(axis=0) & (w > 0).all(axis=0)).sum())
        print("%-7s equal_costs: %d of 16 shots with candidates tied at the minimum (shown by perturbed priors)" % (name, tied))
        assert tied > 0, (name, w)
    _compare(name, soft, 16, "osd_cs", 2, monkeypatch, variant)


# ---- C: sweep and elimination edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,order,candidates", [("osd_cs", 7, 6), ("osd_e", 7, 7)])
def test_fewer_non_pivot_columns_than_the_order(gpu, monkeypatch, method, order, candidates):
    """70 x 73 of rank 70: w = min(order, n - rank) = 3 -- three singles and three pairs, or the seven subsets of three columns."""
    assert _window("c70x73")[3] == 70
    _, _, bad, winners = _reference("c70x73", "sampled", 16, method, order)
    assert _candidates(method, order, 73, 70) == candidates and not bad.any() and (winners > 0).any()
    _compare("c70x73", "sampled", 16, method, order, monkeypatch, 1)


@pytest.mark.parametrize("method,order", [("osd_cs", 3), ("osd_e", 4)])
def test_no_non_pivot_column_at_all(gpu, monkeypatch, method, order):
    """70 x 70 invertible: nothing to sweep (no candidates, asserted), the answer is OSD-0's."""
    Hs, pri, H, rank = _window("c70x70")
    assert rank == 70
    ref, _, bad, winners = _reference("c70x70", "sampled", 16, method, order)
    synd, llr, _ = _inputs("c70x70", "sampled", 16)
    g = orc.Graph(Hs, pri)
    assert _candidates(method, order, 70, 70) == 0 and not bad.any() and not winners.any()
    assert all(np.array_equal(ref[b], g.osd0(synd[b], llr[b].astype(np.float64), stop_early=True)[0]) for b in range(16))
    _compare("c70x70", "sampled", 16, method, order, monkeypatch, 1)


@pytest.mark.parametrize("method,order", [("osd_cs", 3), ("osd_e", 4)])
@pytest.mark.parametrize("name", ["t5x8", "t40x63"])
def test_windows_of_less_than_one_batch(gpu, monkeypatch, name, method, order):
    """5 x 8 and 40 x 63: fewer checks than a Q word has bits, fewer faults than a batch has columns (one bucket, eight samples for eight keys)."""
    _, _, bad, winners = _reference(name, "sampled", 16, method, order)
    assert not bad.any() and (winners > 0).any()
    _compare(name, "sampled", 16, method, order, monkeypatch, 1)


@pytest.mark.parametrize("method,order", [("osd_cs", 3), ("osd_e", 4)])
def test_last_pivot_in_the_last_partial_batch(gpu, monkeypatch, method, order):
    """[A | I] with 96 checks and 231 faults, the identity columns of A's six zero rows sorted last: 96 pivots (asserted), the last of them from the
    fourth batch, which has 39 columns; `npiv >= rank` and `base + 64 >= n` come true in the same batch."""
    Hs, pri, H, rank = _window("last")
    zero = _last_batch_window()[2]
    assert H.shape == (96, 231) and rank == 96 and not H[zero, :135].any() and H[:, :135].sum(axis=0).min() >= 3
    _, pivots, bad, winners = _reference("last", "last_batch", 8, method, order)
    llr = _inputs("last", "last_batch", 8)[1]
    assert (np.sort(np.argsort(llr, axis=1, kind="stable")[:, -6:], axis=1) == 135 + zero).all()
    assert (pivots == 96).all() and not bad.any() and (winners > 0).any()
    _compare("last", "last_batch", 8, method, order, monkeypatch, 1)


@pytest.mark.parametrize("method,order,candidates", [("osd_e", 15, 32767), ("osd_cs", 64, 627 + 2016)])
def test_largest_orders_on_the_second_instantiation(gpu, monkeypatch, method, order, candidates):
    """osd_e 15 (the documented maximum: 32767 patterns) and osd_cs 64 (2016 pairs) on a 576 x 1203 window, two shots each."""
    assert _window("m576")[3] == 576
    _, _, bad, winners = _reference("m576", "sampled", 2, method, order)
    assert _candidates(method, order, 1203, 576) == candidates and not bad.any() and (winners > 0).any()
    _compare("m576", "sampled", 2, method, order, monkeypatch, 2)


# ---- D: shot-to-shot state --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant,per_cu,rounds,extra,order", [("d70x73", 1, 5, 2, 3, 3), ("b1100", 3, 1, 1, 5, 1)])
def test_more_shots_than_workgroups(gpu, monkeypatch, name, variant, per_cu, rounds, extra, order):
    """The smallest instantiation runs five workgroups per CU (2 x that + 3 shots: every workgroup decodes two or three), the largest one (one per
    CU + 5 shots: five workgroups decode two).  A workgroup takes shots b, b + workgroups, ...: with a syndrome outside the column space in every
    second shot all shots of a workgroup would be of one kind, so a seeded half of the shots is spoiled instead, and it is asserted that some workgroup
    decodes a consistent shot right after an inconsistent one and the other way round.  Every shot has its own syndrome and LLRs: a flag, a pivot count
    or a table left over from the shot before shows in the shot after."""
    import torch
    blocks = torch.cuda.get_device_properties(0).multi_processor_count * per_cu
    shots = blocks * rounds + extra
    m = WINDOWS[name][0]
    assert 3 <= m - _window(name)[3] <= 6
    _, _, bad, winners = _reference(name, "mixed", shots, "osd_cs", order)
    after_bad, after_good = int((bad[:-blocks] & ~bad[blocks:]).sum()), int((~bad[:-blocks] & bad[blocks:]).sum())
    print("%-7s mixed: %d workgroups; a consistent shot follows an inconsistent one %d times, the reverse %d times" % (name, blocks, after_bad, after_good))
    assert after_bad > 0 and after_good > 0 and (winners > 0).any()
    _compare(name, "mixed", shots, "osd_cs", order, monkeypatch, variant)
