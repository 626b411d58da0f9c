"""The decoder at the two degree limits of its ABI: qd_graph_create takes any window of row weight <= 255 (QD_MAX_ROW_DEG) and column
weight <= 16 (QD_MAX_COL_DEG), and code that is selected by those weights runs on no fixture window (rows <= 78, columns <= 9):

  * qd_bp_minsum_kernel (bp_kernels.hip): qd_gather_dispatch's NCH = rec_words / 4 with rec_words = pad4(1 + column weight) -- weight 12..15
    falls into the last arm (NCH = 5 with bit_thr[15] = 0), weight 16 adds the lone r4.x group; sign mode 2 finds the sign words 1..7
    of a row through the 3-bit field ((rec >> 5) & 7) - 1 of the fault record; rows of 97..255 faults (4..8 sign words) take this
    kernel as their first choice, because no scatter kernel takes rows of more than 96;
  * the scatter kernels' certificate m2_limit = (2^23 - max|prior|) / max_cdeg - 1 at max_cdeg 12..16;
  * qd_bp_edge_kernel (bp_general.hip) with D = 16 on a small window, ell_w 192 and 256, serial prefixes over long rows,
    qd_bp_ps_lds_bytes' switches on the row weight;
  * the post-processors: pairs[64 * max_cdeg] of every OSD layout, osd_sr.hip's ELL columns at dl = 4 with all 16 entries used,
    lsd_kernels.hip off its ell_w = 64 fast path.

The windows are synthetic (helpers.synthetic_window: seeded, two weight-2 faults per row, the rest of weight cmin..cmax), of at most
128 checks and 4626 faults:

  name      rows                  heavy columns  what it is here for
  c12       96 x 36               7..12          rec_words 16 -> NCH = 5 with bit_thr[15] = 0; the fourth record chunk; m2_limit / 12
  c15       96 x 36               10..15         the same with 15 of the 16 record slots used
  c16       128 x 40              7..16          rec_words 20, r4.x; m2_limit / 16; K1g D = 16 without frec on a small nnz; pairs 64 x 16; dl = 4 full
  w96       72 x 96               3..6           the last row weight of three sign words; fewer than 1024 lanes: the gather kernel
  w97       72 x 97               3..6           four sign words, the last one with one real edge and three pads; no scatter kernel above 96
  w128      72 x 128              3..6           four full words
  w129      72 x 129              3..6           a fifth word with one real edge
  w255      72 x 255              3..6           eight words (w = 7, the largest the 3-bit field holds); edge position 254; ell_w 256
  w79_255   96 rows, 79..255      3..6           degree-sorted wavefronts whose lanes run past their degree in several words; a partial second
                                                 wavefront; the 512-thread instantiation (more than 2560 faults)
  w255_c16  64 x 255 + 64 x 100   7..16          both limits at once: sign mode 2 with NCH = 5

a. Flooding min-sum bit for bit, as in test_gpu_bp_sign_register.py: hard decisions, OSD-0 outputs, status words and exported posteriors
   of every path a window can take against each other and against the double-precision oracle on the device's LLR grid; 64 sampled
   syndromes and the all-ones syndrome, max_iter 1, 3 and 50; the one-message-per-edge kernel on the same grid on three windows.
   The scatter kernels' certificate has nothing to refuse on these windows (their two light faults per row keep every magnitude small), so
   c16 without its light faults adds shots that the oracle decodes on the coarse grid: the device must flag exactly those.
b. The other BP kernels and every post-processor on c16, w79_255 and w255_c16 against the oracle in the arithmetic
   orc.device_arithmetic names, compared the way tools/stress_parity.py compares.
c. One more than either limit is refused with QD_ECAPACITY."""
import functools

import numpy as np
import pytest

import helpers
import oracle as orc

pytestmark = pytest.mark.gpu

SWITCHES = ("QD_NO_SCATTER", "QD_BP_NO_FAST_START", "QD_SCATTER_M2_LIMIT", "QD_SCATTER_CPL1", "QD_SCATTER_WIDE_T704", "QD_OSDCS_OLD", "QD_GEN_STAGES")
SHOTS = 64
ONES_SHOTS = 4         # the all-ones syndrome is one syndrome: a few copies, so that more than one workgroup runs it
NLLR = 6               # posteriors are read back one shot at a time: the first NLLR shots that did not converge
WINDOWS = {            # name: (row weights, heaviest first; lightest and heaviest of the heavy columns; seed)
    "c12": ([36] * 96, 7, 12, 30012),
    "c15": ([36] * 96, 10, 15, 30015),
    "c16": ([40] * 128, 7, 16, 30016),
    "w96": ([96] * 72, 3, 6, 30096),
    "w97": ([97] * 72, 3, 6, 30097),
    "w128": ([128] * 72, 3, 6, 30128),
    "w129": ([129] * 72, 3, 6, 30129),
    "w255": ([255] * 72, 3, 6, 30255),
    "w79_255": (sorted((int(round(w)) for w in np.linspace(79, 255, 96)), reverse=True), 3, 6, 30079),
    "w255_c16": ([255] * 64 + [100] * 64, 7, 16, 30271),
}
SCATTER = ("c12", "c15", "c16")                          # a scatter kernel by default (bp_scatter_wide.hip: at most 128 checks); every other window: the gather kernel
THREADS = {name: 256 for name in WINDOWS}                # of qd_bp_minsum_kernel: max(m, n / 10) <= 256, <= 512
THREADS["w255"] = THREADS["w79_255"] = 512
EDGE_WINDOWS = ("c16", "w255", "w255_c16")
POST_WINDOWS = ("c16", "w79_255", "w255_c16")
SR, PANEL, LSD, OFFCHIP = "qd_osd0_sr_kernel", "qd_osdcs_kernel", "qd_lsd0_kernel", "qd_osd0_offchip_kernel"


@functools.lru_cache(maxsize=None)
def _matrix(which):
    rows, cmin, cmax, seed = WINDOWS[which]
    H, pri = helpers.synthetic_window(rows, cmin, cmax, seed)
    pri.setflags(write=False)
    return H, pri


@functools.lru_cache(maxsize=None)
def _window(which, synd):
    H, pri = _matrix(which)
    if synd == "ones":
        s = np.ones((ONES_SHOTS, H.shape[0]), dtype=np.uint8)
    else:
        s = np.ascontiguousarray(orc.sample_dem(H, H[:1], pri, seed=47, shot0=0, B=SHOTS)[0]).astype(np.uint8)
    s.setflags(write=False)
    return H, pri, s


@functools.lru_cache(maxsize=None)
def _reference(which, synd, max_iter):
    """The oracle in double precision on the device's grid, on the CPU: (OSD-0 outputs, flags, {shot: (hard decisions, posteriors)} of
    the first NLLR shots BP leaves unconverged).  Checked here, on the oracle alone: no shot leaves the fine grid or trips the exactness
    bound, every exported posterior fits a float exactly, and with max_iter > 1 some shot runs more than one iteration."""
    H, pri, s = _window(which, synd)
    g, form = orc.device_arithmetic(H, pri, "minimum_sum", "parallel", max_iter, 1.0)
    prm = orc.make_params("minimum_sum", "parallel", max_iter, "osd_0", 0, 1.0, form)
    ref, flags, grid = g.decode_batch(s, prm, return_grid=True)
    print("%s / %s / max_iter %d: oracle iterations min %d max %d, converged %d of %d" % (
        which, synd, max_iter, flags[:, 1].min(), flags[:, 1].max(), int(flags[:, 0].sum()), len(flags)))
    assert g.grid[0] >= 0 and (grid[:, 0] == g.grid[0]).all() and not grid[:, 1].any(), (which, synd, max_iter, grid)
    assert max_iter == 1 or int(flags[:, 1].max()) > 1, (which, synd, max_iter)
    soft = {}
    for b in np.flatnonzero(flags[:, 0] == 0)[:NLLR]:
        conv, dec, llr, it = g.bp(s[b], prm)
        assert not conv and it == flags[b, 1]
        # the device adds grid units in int32 and float: exact, and so comparable bit for bit, below 2^23 units
        assert float(np.abs(llr).max()) * 2.0 ** orc.grid_bits(pri, max_iter)[0] < 2.0 ** 23, (which, synd, max_iter, float(np.abs(llr).max()))
        soft[int(b)] = (dec, llr)
    return ref, flags, soft


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _graph(which):
    """The device graph of a window, seen to be the window the module's table describes."""
    from quits_amd.decoder.device import WindowGraph
    H, pri = _matrix(which)
    rows, _, cmax, _ = WINDOWS[which]
    wg = WindowGraph(H, pri)
    info = wg.info()
    assert (info["m"], info["max_row_weight"], info["max_col_weight"], info["bp_threads"]) == (len(rows), rows[0], cmax, THREADS[which]), (which, info)
    return wg


def _run(monkeypatch, which, synd, env, max_iter, **kw):
    import torch
    from quits_amd.decoder.device import BatchDecoder, unpack_bits
    s = _window(which, synd)[2]
    _env(monkeypatch, env)
    wg = _graph(which)
    dec = BatchDecoder(wg, max_iter=max_iter, osd_method="osd_0", **kw)
    det = torch.from_numpy(np.array(s)).cuda()
    out = {}
    bits, status = dec.decode(det, stage=1)
    out[1] = (unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy())
    failed = np.flatnonzero(((out[1][1] >> 16) & 1) == 0)[:NLLR]
    out["llr"] = {int(b): dec.failed_llr(int(b)).cpu().numpy() for b in failed}
    bits, status = dec.decode(det, stage=3)
    out[3] = (unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy())
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
    assert not ((status >> 14) & 3).any(), tag                                     # fine grid, exact: what _reference asserts of the oracle
    assert np.array_equal((status >> 16) & 1, flags[:, 0]), tag
    assert np.array_equal(status & 0x3FFF, flags[:, 1]), tag
    assert np.array_equal(bits, ref), tag
    assert sorted(out["llr"]) == sorted(soft), tag
    for b, (dec, llr) in soft.items():
        assert np.array_equal(out[1][0][b], dec), (tag, b)
        assert np.array_equal(out["llr"][b].astype(np.float64), llr), (tag, b)      # exact: the grid's posteriors fit a float


def _paths(monkeypatch, which, synd, max_iter):
    """Every path flooding min-sum can take on this window: identical to each other and to the oracle."""
    ref3 = _reference(which, synd, max_iter)
    outs, kernels = {}, {}
    outs["default"], info = _run(monkeypatch, which, synd, {}, max_iter)
    assert not info["edge_kernel"] and info["llr_grid_bits"] >= 0, info
    assert info["scatter_kernel"] == (which in SCATTER), (which, info)              # the window is on the path it is here for
    kernels["default"] = info
    if which in SCATTER:
        paths = [("gather", {"QD_NO_SCATTER": "1"}), ("recheck", {"QD_SCATTER_M2_LIMIT": "1"})]    # limit 1: every shot with a defect goes through the gather kernel's recheck pass
        if info["scatter_wide_kernel"]:
            paths.append(("generic", {"QD_BP_NO_FAST_START": "1"}))
        for tag, env in paths:
            outs[tag], kernels[tag] = _run(monkeypatch, which, synd, env, max_iter)
            assert kernels[tag]["scatter_kernel"] == (tag != "gather") and not kernels[tag]["edge_kernel"], (tag, kernels[tag])
            assert tag != "generic" or not kernels[tag]["bp_fast_start"], kernels[tag]
    for tag in outs:
        if tag != "default":
            _same(outs["default"], outs[tag], "default path against %s" % tag)
        _against_oracle(ref3, outs[tag], tag)
    st = outs["default"][1][1]
    run = st[(st >> 19) & 1 == 0]
    assert run.size and (run & 0x3FFF).min() >= 1 and (run & 0x3FFF).max() <= max_iter
    print("%s: %s" % (which, {tag: "K1sw" if i["scatter_wide_kernel"] else ("K1sw, one check per lane" if i["scatter_kernel"] else "K1") for tag, i in kernels.items()}))


@pytest.mark.parametrize("max_iter", [1, 3, 50])
@pytest.mark.parametrize("synd", ["sampled", "ones"])
@pytest.mark.parametrize("which", list(WINDOWS))
def test_flooding_min_sum_at_the_degree_limits(gpu, monkeypatch, which, synd, max_iter):
    """Every window of the module's table, with sampled syndromes and with the all-ones syndrome: the c* windows through the scatter
    kernel, the gather kernel and the scatter kernel's recheck pass, the w* windows through the gather kernel, which is their default."""
    _paths(monkeypatch, which, synd, max_iter)


@pytest.mark.parametrize("synd", ["sampled", "ones"])
@pytest.mark.parametrize("which", EDGE_WINDOWS)
def test_edge_kernel_on_the_grid_at_the_degree_limits(gpu, monkeypatch, which, synd):
    """edge_messages=True: flooding min-sum in the one-message-per-edge kernel on the same grid (D = 16 without fault records on c16 and
    w255_c16, ell_w 256 on the rows of 255).  _reference has checked that no shot leaves the fine grid, so the batch is comparable."""
    out, info = _run(monkeypatch, which, synd, {}, 3, edge_messages=True)
    assert info["edge_kernel"] and not info["scatter_kernel"] and info["llr_grid_bits"] >= 0, info
    _against_oracle(_reference(which, synd, 3), out, "edge kernel")


@functools.lru_cache(maxsize=None)
def _heavy_only(synd):
    """c16 without its weight-2 faults (128 x 442, rows of 38, columns of 7..16): nothing keeps the magnitudes from growing, so at max_iter 3
    some shots outgrow the fine grid's exactness bound and are decoded again on the coarse grid."""
    H, pri, _ = _window("c16", synd)
    keep = np.flatnonzero(np.asarray(H.sum(axis=0)).ravel() > 2)
    H, pri = H[:, keep].tocsc(), pri[keep]
    if synd == "ones":
        s = np.ones((ONES_SHOTS, H.shape[0]), dtype=np.uint8)
    else:
        s = np.ascontiguousarray(orc.sample_dem(H, H[:1], pri, seed=47, shot0=0, B=SHOTS)[0]).astype(np.uint8)
    g, form = orc.device_arithmetic(H, pri, "minimum_sum", "parallel", 3, 1.0)
    ref, flags, grid = g.decode_batch(s, orc.make_params("minimum_sum", "parallel", 3, "osd_0", 0, 1.0, form), return_grid=True)
    coarse = grid[:, 0] != g.grid[0]
    print("c16 without light faults / %s: oracle sends %d of %d shots to the coarse grid, %d inexact" % (synd, coarse.sum(), len(s), grid[:, 1].sum()))
    assert coarse.sum() >= 4 and not grid[:, 1].any(), (synd, coarse.sum(), grid[:, 1].sum())
    return H, pri, s, ref, flags, coarse


@pytest.mark.parametrize("synd", ["sampled", "ones"])
def test_scatter_certificate_at_column_weight_16(gpu, monkeypatch, synd):
    """The scatter kernel certifies a run by max|prior| + max_cdeg * (largest second minimum) < 2^23 (m2_limit in qd_decoder.hip) and hands
    every other shot to the gather kernel's recheck pass, which sends the shots that really outgrow the bound to the coarse grid.  At column
    weight 16 the shots the oracle decodes on the coarse grid must carry QD_STATUS_COARSE_GRID on the device too -- a certificate that
    forgets the column weight passes them on the fine grid -- and every output equals the oracle's, on every path."""
    import torch
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    H, pri, s, ref, flags, coarse = _heavy_only(synd)
    for tag, env in (("default", {}), ("gather", {"QD_NO_SCATTER": "1"}), ("recheck", {"QD_SCATTER_M2_LIMIT": "1"})):
        _env(monkeypatch, env)
        wg = WindowGraph(H, pri)
        assert wg.info()["max_col_weight"] == 16
        dec = BatchDecoder(wg, max_iter=3, osd_method="osd_0")
        assert dec.info()["scatter_kernel"] == (tag != "gather"), (tag, dec.info())
        bits, status = dec.decode(torch.from_numpy(s).cuda())
        err, st = unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy()
        assert np.array_equal((st >> 14) & 1, coarse.astype(int)), (tag, "coarse grid", np.flatnonzero(((st >> 14) & 1) != coarse))
        assert not ((st >> 15) & 1).any(), (tag, "inexact")
        assert np.array_equal((st >> 16) & 1, flags[:, 0]) and np.array_equal(st & 0x3FFF, flags[:, 1]), tag
        assert np.array_equal(err, ref), (tag, np.flatnonzero((err != ref).any(axis=1))[:5])


# ---- b. the other BP kernels and the post-processors -----------------------------------------------------------------------------------
POST_SHOTS = 48
CASES = {              # name: (bp_method, schedule, max_iter, ms_scaling_factor, osd_method, osd_order, off_chip, post-processing kernel)
    "ps_flooding_osd_cs10": ("product_sum", "parallel", 3, 1.0, "osd_cs", 10, False, PANEL),
    "ps_serial_osd_e4": ("product_sum", "serial", 2, 1.0, "osd_e", 4, False, PANEL),
    "ms_serial_lsd_cs2": ("minimum_sum", "serial", 8, 1.0, "lsd_cs", 2, False, LSD),            # max_iter 8: staged launches at the bounds 3 and 6
    "ms_alpha0_lsd_0": ("minimum_sum", "parallel", 3, 0.0, "lsd_0", 0, False, LSD),             # the float, off-grid gather kernel
    "ms_alpha0625_osd_cs2": ("minimum_sum", "parallel", 3, 0.625, "osd_cs", 2, False, PANEL),
    "ms_serial_lsd_e3": ("minimum_sum", "serial", 2, 0.625, "lsd_e", 3, False, LSD),
    "ms_alpha0625_osd_0": ("minimum_sum", "parallel", 3, 0.625, "osd_0", 0, False, SR),
    "ms_grid_off_chip_osd_0": ("minimum_sum", "parallel", 3, 1.0, "osd_0", 0, True, OFFCHIP),
    "ms_grid_osd_0_two_iterations": ("minimum_sum", "parallel", 2, 1.0, "osd_0", 0, False, SR),
}


@functools.lru_cache(maxsize=None)
def _post_syndromes(which):
    H, pri = _matrix(which)
    # (seed 61: on every window the oracle sends at least 16 of these shots to the post-processor after two iterations)
    s = np.ascontiguousarray(orc.sample_dem(H, H[:1], pri, seed=61, shot0=0, B=POST_SHOTS)[0]).astype(np.uint8)
    s[5] = np.random.default_rng(WINDOWS[which][3]).integers(0, 2, H.shape[0])       # arbitrary, possibly outside the column space
    s[11] = 0
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _post_reference(which, case):
    method, sched, max_iter, alpha, osd, order, off_chip, _ = CASES[case]
    H, pri = _matrix(which)
    go, form = orc.device_arithmetic(H, pri, method, sched, max_iter, alpha)
    ref, flags, grid = go.decode_batch(_post_syndromes(which), orc.make_params(method, sched, max_iter, osd, order, alpha, form), return_grid=True)
    print("%s / %s: oracle iterations max %d, converged %d of %d" % (which, case, flags[:, 1].max(), int(flags[:, 0].sum()), len(flags)))
    return ref, flags, grid, go.grid[0]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("which", POST_WINDOWS)
def test_other_kernels_and_post_processors_at_the_degree_limits(gpu, monkeypatch, which, case):
    """What tools/stress_parity.py compares -- decisions, the converged flag, iterations of non-zero syndromes, the post-processor's flag,
    its pivot count and inconsistent flag -- for every BP kernel but the ones of part a, each with one of the post-processors."""
    import torch
    from quits_amd.decoder.device import BatchDecoder, unpack_bits
    method, sched, max_iter, alpha, osd, order, off_chip, post = CASES[case]
    synd = _post_syndromes(which)
    ref, flags, grid, fine = _post_reference(which, case)
    if case == "ms_grid_osd_0_two_iterations":
        assert int((flags[:, 0] == 0).sum()) >= 16, (which, int((flags[:, 0] == 0).sum()))       # shots that reach the post-processor
    _env(monkeypatch, {})
    wg = _graph(which)
    dec = BatchDecoder(wg, bp_method=method, schedule=sched, max_iter=max_iter, osd_method=osd, osd_order=order, ms_scaling_factor=alpha, off_chip=off_chip)
    info = dec.info()
    flooding_ms = method == "minimum_sum" and sched == "parallel"
    on_grid = flooding_ms and alpha == 1.0
    assert info["post_kernel"] == post and info["edge_kernel"] == (off_chip or not flooding_ms), (which, case, info)
    assert info["scatter_kernel"] == (on_grid and not off_chip and which in SCATTER), (which, case, info)
    assert (info["llr_grid_bits"] >= 0) == (fine >= 0), (info, fine)
    bits, status = dec.decode(torch.from_numpy(np.array(synd)).cuda())
    err, st = unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy()
    tag = (which, case)
    exact = np.ones(len(synd), bool)
    if fine >= 0:                          # on the grid: the coarse-grid and inexact bits equal the oracle's account; an inexact shot is outside the contract
        assert np.array_equal((st >> 14) & 1, (grid[:, 0] != fine).astype(int)), ("coarse grid", tag)
        assert np.array_equal((st >> 15) & 1, grid[:, 1]), ("inexact flag", tag)
        exact = grid[:, 1] == 0
    assert np.array_equal(((st >> 16) & 1)[exact], flags[exact, 0]), ("converged", tag)
    nz = synd.any(axis=1) & exact
    assert np.array_equal((st & 0x3FFF)[nz], flags[nz, 1]), ("iterations", tag)
    assert np.array_equal(err[exact], ref[exact]), ("decisions", tag, np.flatnonzero((err != ref).any(axis=1) & exact)[:5])
    assert np.array_equal(((st >> 17) & 1)[exact], (1 - flags[:, 0])[exact]), ("osd flag", tag)
    if osd in ("osd_0", "lsd_0", "lsd_cs", "lsd_e") or order == 0:
        used = (((st >> 17) & 1) == 1) & exact
        assert np.array_equal(((st >> 20) & 0xFFF)[used], np.minimum(flags[used, 2], 4095)), ("pivots", tag)
        assert np.array_equal(((st >> 18) & 1)[used], (flags[used, 3] != 0).astype(int)), ("inconsistent", tag)


# ---- c. the limits themselves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cmax,message", [([256] + [40] * 71, 6, "row weight 256 outside 1..255"), ([40] * 72, 17, "column weight 17 outside 1..16")])
def test_one_past_a_limit_is_refused(gpu, rows, cmax, message):
    from quits_amd._lib import QdError
    from quits_amd.decoder.device import WindowGraph
    H, pri = helpers.synthetic_window(rows, cmax - 3, cmax, 31000 + cmax)
    with pytest.raises(QdError, match=message):
        WindowGraph(H, pri)
