"""Fixture loaders shared by the tests (data only; nothing here touches /root/reference)."""
import gzip
import json
import os

import numpy as np
from scipy.sparse import csc_matrix

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def circuit_text(name):
    with gzip.open(os.path.join(GOLD, "circuits", name + ".stim.gz"), "rb") as f:
        return f.read().decode()


def circuit_text_at_p(name, p_from, p_to):
    """The circuit the reference emits for ErrorModel(p_to, p_to, p_to, p_to), derived from the fixture made at p_from.
    With one rate on all four channels every noise argument is printed as the same '%.10f' literal (circuit.py:96-246),
    so the two texts differ by exactly that literal (tests/test_dem.py checks this on the six bb144 fixtures)."""
    old, new = "%.10f" % p_from, "%.10f" % p_to
    text = circuit_text(name)
    assert old in text
    return text.replace(old, new)


def circuit_index():
    return json.load(open(os.path.join(GOLD, "circuits", "index.json")))


def code(name):
    z = np.load(os.path.join(GOLD, "codes", name + ".npz"))
    out = {}
    for k in ("hz", "hx", "lz", "lx"):
        shp = tuple(int(x) for x in z[k + "_shape"])
        out[k] = np.unpackbits(z[k + "_bits"])[: shp[0] * shp[1]].reshape(shp)
    return out


def csc_from(z, prefix):
    idx = z[prefix + "_indices"]
    return csc_matrix((np.ones(len(idx), np.uint8), idx, z[prefix + "_indptr"]),
                      shape=tuple(int(x) for x in z[prefix + "_shape"]))


def windows_npz(name):
    return np.load(os.path.join(GOLD, "windows", name + ".npz"))


def dem_matrices(name):
    z = windows_npz(name)
    return csc_from(z, "H"), csc_from(z, "L"), z["priors"]


def window_set(name, W, F):
    """The reference's spacetime() output for (W, F) as a list of dicts, in the oracle's window format."""
    z = windows_npz(name)
    tag = "W%dF%d" % (W, F)
    nwin = int(z[tag + "_nwin"][0])
    hz_rows = None
    out = []
    for k in range(nwin):
        out.append({"H": csc_from(z, "%s_H%d" % (tag, k)), "L": csc_from(z, "%s_L%d" % (tag, k)),
                    "priors": z["%s_p%d" % (tag, k)],
                    "U": csc_from(z, "%s_U%d" % (tag, k)) if k < nwin - 1 else None})
    return out


def same_sparse(a, b):
    a = csc_matrix(a); a.sort_indices()
    b = csc_matrix(b); b.sort_indices()
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)


# ---- seeded synthetic windows with prescribed row and column weights (the GPU tests that need weights no fixture has) --------------
def _place(rng, rows, cdeg):
    """A 0/1 matrix with the row weights `rows` (heaviest first, dealt to shuffled row indices) and the column weights `cdeg`: every row
    takes the columns with the most free places, random among equals (the bipartite Havel-Hakimi rule: every edge is placed and no
    column is used twice in a row)."""
    left = cdeg.copy()
    H = np.zeros((len(rows), len(cdeg)), dtype=np.uint8)
    for i, w in zip(rng.permutation(len(rows)), rows):
        cols = np.lexsort((rng.random(len(cdeg)), -left))[:w]
        assert left[cols].min() >= 1
        H[i, cols] = 1
        left[cols] -= 1
    assert not left.any()
    return H


def synthetic_window(rows, cmin, cmax, seed):
    """A seeded random parity-check matrix (csc) with the row weights `rows` (heaviest first; the rows are shuffled) and its priors.
    Every row has exactly two faults of column weight 2 (as many such columns as rows); its other faults have weight cmin..cmax (about
    total / ((cmin + cmax) // 2) columns of equal weight, then seeded +1 / -1 moves that keep the sum and spread the weights over the
    whole range).  The two light faults keep min-sum's magnitudes from growing geometrically on a syndrome BP cannot meet (the all-ones
    one): a light fault passes on its prior plus ONE message, and every message a check sends is the minimum over edges that include a
    light fault, so the largest message grows by at most the largest prior per iteration."""
    rows = [int(w) for w in rows]
    rng = np.random.default_rng(seed)
    m = len(rows)
    assert rows == sorted(rows, reverse=True) and rows[-1] > 2 and 2 < cmin <= cmax <= m
    light = _place(rng, [2] * m, np.full(m, 2, dtype=np.int64))
    total = sum(rows) - 2 * m
    n = max(total // ((cmin + cmax) // 2), max(rows) - 2)
    cdeg = np.full(n, total // n, dtype=np.int64)
    cdeg[:total - cdeg.sum()] += 1
    assert cmin <= cdeg.min() and cdeg.max() <= cmax, (cdeg.min(), cdeg.max())
    for _ in range(2 * n * (cmax - cmin + 1)):
        a, b = rng.integers(0, n, size=2)
        if a != b and cdeg[a] < cmax and cdeg[b] > cmin:
            cdeg[a] += 1
            cdeg[b] -= 1
    assert cdeg.sum() == total and cdeg.min() >= cmin and cdeg.max() == cmax, (cdeg.min(), cdeg.max())
    H = np.concatenate([light, _place(rng, [w - 2 for w in rows], cdeg)], axis=1)
    H = H[:, rng.permutation(H.shape[1])]
    assert sorted(H.sum(axis=1).tolist(), reverse=True) == rows
    assert H.sum(axis=0).min() == 2 and H.sum(axis=0).max() == cmax
    # three to four faults per shot, spread over three decades: with near-equal priors the all-ones syndrome of an odd row weight is met
    # by the first iteration's hard decisions (every fault set) and nothing is left to iterate
    pri = np.minimum(0.08, 10.0 ** rng.uniform(-2.5, 0.5, size=H.shape[1]) * 8.0 / H.shape[1])
    return csc_matrix(H), pri


# ---- the CPU oracle over several processes (the oracle is single-threaded C; the larger parity tests slice the shots) ----------
def _oracle_procs():
    return max(1, min(32, len(os.sched_getaffinity(0))))


def _sw_worker(args):
    import oracle as orc
    wins, nz, det, prm, device_grid = args
    return orc.sliding_window_decode(wins, nz, det, orc.make_params(*prm), device_grid=device_grid)


def oracle_sliding_window_parallel(wins, nz, det, prm, device_grid=False):
    """orc.sliding_window_decode over shot slices in a fork pool; prm = the argument tuple of orc.make_params.
    Returns (predictions, summed stats)."""
    import multiprocessing as mp
    n = _oracle_procs()
    parts = [p for p in np.array_split(np.ascontiguousarray(det), min(n, max(1, len(det) // 2))) if len(p)]
    with mp.get_context("fork").Pool(min(n, len(parts))) as pool:
        res = pool.map(_sw_worker, [(wins, nz, p, prm, device_grid) for p in parts])
    stats = {k: sum(r[1][k] for r in res) for k in res[0][1]}
    return np.concatenate([r[0] for r in res], axis=0), stats


def _batch_worker(args):
    import oracle as orc
    H, pri, synd, prm, max_iter_grid = args
    g = orc.Graph(H, pri)
    if max_iter_grid is not None:
        g.device_grid(max_iter_grid)
    return g.decode_batch(synd, orc.make_params(*prm))


def oracle_decode_batch_parallel(H, pri, synd, prm, device_grid_max_iter=None):
    """Graph.decode_batch over shot slices in a fork pool (device_grid_max_iter: put the LLRs on the device's grid for that max_iter)."""
    import multiprocessing as mp
    n = _oracle_procs()
    parts = [p for p in np.array_split(np.ascontiguousarray(synd), min(n * 4, max(1, len(synd) // 8))) if len(p)]
    with mp.get_context("fork").Pool(min(n, len(parts))) as pool:
        res = pool.map(_batch_worker, [(H, pri, p, prm, device_grid_max_iter) for p in parts])
    return np.concatenate([r[0] for r in res], axis=0), np.concatenate([r[1] for r in res], axis=0)


def _osd_w_worker(args):
    import oracle as orc
    H, pri, synd, llr, method, order = args
    g = orc.Graph(H, pri)
    err = np.zeros((len(synd), g.n), np.uint8)
    st = np.zeros((len(synd), 3), np.int64)
    for b in range(len(synd)):
        err[b], s = g.osd_w(synd[b], llr[b].astype(np.float64), method, order, fixed=True)
        st[b] = s["pivots"], s["winner"], s["candidates"]
    return err, st


def oracle_osd_w_parallel(H, pri, synd, llr, method, order):
    """Graph.osd_w(.., fixed=True) -- higher-order OSD alone on given soft information, integer candidate costs -- shot by shot in a fork
    pool.  Returns (corrections [B, n], stats [B, 3] = pivots, 1 + index of the winning candidate (0: OSD-0 kept), candidates)."""
    import multiprocessing as mp
    synd, llr = np.ascontiguousarray(synd), np.ascontiguousarray(llr)
    n = min(12, _oracle_procs(), len(synd))
    if n <= 1:
        return _osd_w_worker((H, pri, synd, llr, method, order))
    parts = [p for p in np.array_split(np.arange(len(synd)), n) if len(p)]
    with mp.get_context("fork").Pool(len(parts)) as pool:
        res = pool.map(_osd_w_worker, [(H, pri, synd[p], llr[p], method, order) for p in parts])
    return np.concatenate([r[0] for r in res], axis=0), np.concatenate([r[1] for r in res], axis=0)


def _lsd_worker(args):
    import oracle as orc
    H, pri, synd, llr, method, order = args
    g = orc.Graph(H, pri)
    err = np.zeros((len(synd), g.n), np.uint8)
    st = np.zeros((len(synd), len(LSD_STATS)), np.int64)
    for b in range(len(synd)):
        err[b], s = g.lsd(synd[b], llr[b].astype(np.float64), method, order, fixed=True)
        st[b] = [int(s[k]) for k in LSD_STATS]
    return err, st


LSD_STATS = ("pivots", "added", "inconsistent", "rounds", "grown", "swept", "replaced", "clusters", "merges", "max_candidates")


def oracle_lsd_parallel(H, pri, synd, llr, method, order):
    """Graph.lsd(.., fixed=True) -- BP-LSD's post-processing alone on given soft information, integer candidate costs; method 'lsd_0' or
    order 0 is LSD-0 -- shot by shot in a fork pool.  Returns (corrections [B, n], stats [B, 10] in the order of LSD_STATS)."""
    import gc
    import multiprocessing as mp
    synd, llr = np.ascontiguousarray(synd), np.ascontiguousarray(llr)
    n = min(16, _oracle_procs(), len(synd))          # the children inherit the parent's open device: no more of them than a GPU machine lets hold one
    if n <= 1:
        return _lsd_worker((H, pri, synd, llr, method, order))
    parts = [np.arange(k, len(synd), n) for k in range(n)]             # strided: heavy shots often come in runs
    # what a failed test left behind (frames that hold device handles) must not be destroyed by a child's collector after the fork: the children
    # inherit it in the permanent generation, which their collector leaves alone
    gc.freeze()
    try:
        with mp.get_context("fork").Pool(n) as pool:
            res = pool.map(_lsd_worker, [(H, pri, synd[p], llr[p], method, order) for p in parts])
    finally:
        gc.unfreeze()
    err = np.zeros((len(synd), res[0][0].shape[1]), np.uint8)
    st = np.zeros((len(synd), len(LSD_STATS)), np.int64)
    for p, (e, s) in zip(parts, res):
        err[p], st[p] = e, s
    return err, st
