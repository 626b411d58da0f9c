"""Off-chip windows: windows whose BP state does not fit the CU's LDS (qd_graph_create, include/quits_amd.h) decode in the
one-message-per-edge BP kernel -- flooding min-sum on the LLR grid with the exactness certificate and the coarse-grid redo pass --
and in qd_osd0_offchip_kernel (csrc/osd_offchip.hip).  The case that needs it: QLP [[1020,136]], 20 rounds, W = 5, F = 3, the
reference's standard window size (windows of 2250 x 30 900 / 31 500).

1. the same path forced (QD_FLAG_OFF_CHIP) on windows that fit, against the default kernels and the oracle;
2. a real off-chip window against the oracle;
3. the sliding-window call over the seven (5, 3) windows against the oracle's loop;
4. the OSD stage alone on crafted posteriors: every tier of the column order, every spilled Q plane;
5. the coarse-grid redo pass and the INEXACT flag;
6. a syndrome outside the column space;
7. what an off-chip window refuses, and what it does not.

Inputs are DEM-sampled with fixed seeds (the oracle's sampler); the oracle is orc.device_arithmetic's form for the options."""
import functools

import numpy as np
import pytest

import helpers
import oracle as orc

pytestmark = pytest.mark.gpu

BB72 = "bb72_custom_r6_p0.003"
HGP = "hgp225_cardinal_r3_p0.01"
QLP = "qlp1020_cardinal_r20_p0.003"
OFFCHIP_KERNEL = "qd_osd0_offchip_kernel"


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _unpack(bits, n):
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :n]


def _sample(H, pri, seed, B):
    return orc.sample_dem(H, H[:1], pri, seed=seed, shot0=0, B=B)[0]


def _window(which):
    """w1: BB72 W = 3 / F = 1 window 1 (108 x 1080); single: the BB72 history as one window (288 x 2592); hgp: the largest
    [[225,9]] HGP W = 3 window (324 x 3888, rows of 52 faults: two sign words and more in the gather kernel)."""
    if which == "single":
        H, L, pri = helpers.dem_matrices(BB72)
        return H, np.asarray(pri, dtype=np.float64)
    w = helpers.window_set(BB72 if which == "w1" else HGP, 3, 1)[1]
    return w["H"], np.asarray(w["priors"], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _qlp():
    """QLP [[1020,136]] r20 at p = 1e-3: circuit, DEM, and the reference's spacetime() windows for (W, F) = (5, 3)."""
    from quits_amd.decoder.base import detector_error_model_to_matrix, spacetime, window_count
    from quits_amd.dem import Circuit
    circ = Circuit(helpers.circuit_text_at_p(QLP, 0.003, 0.001))
    dem = detector_error_model_to_matrix(circ)
    cd = helpers.code("qlp1020")
    ncr, _, _ = window_count(20, 5, 3)
    checks, commits, priors, updates = spacetime(circ, cd["hz"], 5, 3, ncr)
    return circ, dem, cd, ncr, checks, commits, priors, updates


@functools.lru_cache(maxsize=None)
def _qlp_window0():
    checks, priors = _qlp()[4], _qlp()[6]
    return checks[0], np.asarray(priors[0], dtype=np.float64)


def _assert_oracle(H, pri, s, kw, got, certificate):
    """bits and status of `got` against the oracle in the arithmetic the device uses for the options `kw`."""
    method, schedule, max_iter = kw["bp_method"], kw["schedule"], kw["max_iter"]
    osd, order = kw.get("osd_method", "osd_0"), kw.get("osd_order", 0)
    g, form = orc.device_arithmetic(H, pri, method, schedule, max_iter, 1.0)
    ref, flags, grid = g.decode_batch(s, orc.make_params(method, schedule, max_iter, osd, order, 1.0, form), return_grid=True)
    bits, status = got
    assert np.array_equal((status >> 16) & 1, flags[:, 0]), "convergence flags differ"
    assert np.array_equal(status & 0x3FFF, flags[:, 1]), "iteration counts differ"
    assert np.array_equal((status >> 19) & 1, (s.sum(axis=1) == 0).astype(int)), "zero-syndrome flags differ"
    if osd != "osd_off":
        assert np.array_equal((status >> 17) & 1, 1 - flags[:, 0]), "post-processor flags differ"
        assert np.array_equal((status >> 20) & 0xFFF, np.minimum(flags[:, 2], 4095)), "pivot counts differ"
        assert np.array_equal((status >> 18) & 1, flags[:, 3]), "inconsistent flags differ"
    if certificate:
        assert g.grid[0] >= 0
        assert np.array_equal((status >> 14) & 1, (grid[:, 0] != g.grid[0]).astype(int)), "coarse-grid flags differ"
        assert np.array_equal((status >> 15) & 1, grid[:, 1]), "inexact flags differ"
    else:
        assert not ((status >> 14) & 3).any()
    bad = np.flatnonzero((_unpack(bits, H.shape[1]) != ref).any(axis=1))
    assert bad.size == 0, "output differs from the oracle on shots %s" % bad[:10]
    return flags, grid


OPTIONS = {
    "minsum_flooding_20": dict(bp_method="minimum_sum", schedule="parallel", max_iter=20, osd_method="osd_0"),
    "prodsum_serial_4": dict(bp_method="product_sum", schedule="serial", max_iter=4, osd_method="osd_0"),
}


# ---- 1. the off-chip path forced on windows that fit ---------------------------------------------------------------------------
@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("which", ["w1", "single", "hgp"])
def test_forced_off_chip_path_equals_default_and_oracle(gpu, which, opt):
    """QD_FLAG_OFF_CHIP on a window that fits: error bits and status bits 0..19 equal the default kernels', bits and status equal the
    oracle's, for a batch of 256 and one of 100 (not a multiple of the 64 shots of a wavefront); an empty batch is accepted."""
    import torch
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    H, pri = _window(which)
    kw = OPTIONS[opt]
    wg = WindowGraph(H, pri)
    assert wg.info()["bp_lds_bytes"] > 0, "the window should fit the CU"
    dflt, forced = BatchDecoder(wg, **kw), BatchDecoder(wg, off_chip=True, **kw)
    info = forced.info()
    assert info["edge_kernel"] and info["post_kernel"] == OFFCHIP_KERNEL, info
    assert dflt.info()["post_kernel"] != OFFCHIP_KERNEL
    minsum = kw["bp_method"] == "minimum_sum"
    assert (info["llr_grid_bits"] >= 0) == minsum
    seen_osd = 0
    for shots, seed in ((256, 311), (100, 312)):
        s = _sample(H, pri, seed, shots)
        a, b = _np(dflt.decode(_dev(s))), _np(forced.decode(_dev(s)))
        bad = np.flatnonzero((a[0] != b[0]).any(axis=1) | ((a[1] & 0xFFFFF) != (b[1] & 0xFFFFF)))
        assert bad.size == 0, "%d shots: forced path differs from the default kernels on shots %s" % (shots, bad[:10])
        flags, _ = _assert_oracle(H, pri, s, kw, b, certificate=minsum)
        seen_osd += int((1 - flags[:, 0]).sum())
    assert seen_osd >= 8, "the OSD kernel is hardly exercised (%d shots)" % seen_osd
    e, st = forced.decode(torch.empty((0, H.shape[0]), dtype=torch.uint8, device="cuda"))
    assert e.shape[0] == 0 and st.shape[0] == 0


# ---- 2. a real off-chip window -------------------------------------------------------------------------------------------------
def test_qlp_w5_window_decodes_and_equals_oracle(gpu):
    """Window 0 of QLP [[1020,136]] r20 (5, 3) is 2250 x 30 900: graph creation used to fail with QD_ECAPACITY.  48 shots, flooding
    min-sum 50 + OSD-0: bits and status equal the oracle's; at least 8 shots converge and at least 8 go through OSD."""
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    H, pri = _qlp_window0()
    assert H.shape == (2250, 30900)
    wg = WindowGraph(H, pri)
    gi = wg.info()
    assert gi["bp_lds_bytes"] == 0 and gi["bp_threads"] == 0, gi
    kw = dict(bp_method="minimum_sum", schedule="parallel", max_iter=50, osd_method="osd_0")
    dec = BatchDecoder(wg, **kw)
    info = dec.info()
    assert info["edge_kernel"] and info["post_kernel"] == OFFCHIP_KERNEL and info["llr_grid_bits"] >= 0, info
    s = _sample(H, pri, 1, 48)
    flags, grid = _assert_oracle(H, pri, s, kw, _np(dec.decode(_dev(s))), certificate=True)
    conv = int(flags[:, 0].sum())
    print("oracle: %d converged, %d OSD, %d coarse of 48" % (conv, 48 - conv, int((grid[:, 0] != info["llr_grid_bits"]).sum())))
    assert conv >= 8 and 48 - conv >= 8


# ---- 3. through the API --------------------------------------------------------------------------------------------------------
def _qlp_oracle_windows():
    circ, dem, cd, ncr, checks, commits, priors, updates = _qlp()
    nz = cd["hz"].shape[0]
    return [{"H": checks[k], "L": commits[k], "priors": priors[k], "U": updates[k] if k < ncr else None, "row0": 3 * k * nz}
            for k in range(len(checks))], nz


def test_qlp_w5_f3_sliding_window_equals_oracle_loop(gpu):
    """sliding_window_bposd_circuit_mem over the seven (5, 3) windows (six off-chip, the last one on-chip), min-sum flooding 50 +
    OSD-0, 32 shots: logical predictions equal the oracle's loop on the device's LLR grids."""
    from quits_amd.decoder import sliding_window_bposd_circuit_mem
    circ, (H, L, pri), cd = _qlp()[:3]
    wins, nz = _qlp_oracle_windows()
    assert [w["H"].shape for w in wins] == [(2250, 30900)] + [(2250, 31500)] * 5 + [(1800, 20520)]
    det = orc.sample_dem(H, L, pri, seed=44, shot0=0, B=32)[0]
    pred = sliding_window_bposd_circuit_mem(det, circ, cd["hz"], cd["lz"], 5, 3, max_iter=50, bp_method="minimum_sum",
                                            schedule="parallel", osd_method="osd_0")
    ref, stats = helpers.oracle_sliding_window_parallel(wins, nz, det, ("minimum_sum", "parallel", 50, "osd_0", 0, 1.0, orc.FORM_LDPC_F64),
                                                        device_grid=True)
    print("oracle:", stats)
    assert stats["bp_converged"] >= 32 and stats["osd_calls"] >= 32, stats
    assert pred.shape == (32, cd["lz"].shape[0]) and np.array_equal(pred, ref.astype(np.int64))


def test_qlp_w5_f3_wrapper_defaults_equal_float_mirror(gpu):
    """The wrapper's own defaults (product_sum, serial, osd_cs of order 0, max_iter 2) on 16 shots against the float-mirror oracle."""
    from quits_amd.decoder import sliding_window_bposd_circuit_mem
    circ, (H, L, pri), cd = _qlp()[:3]
    wins, nz = _qlp_oracle_windows()
    det = orc.sample_dem(H, L, pri, seed=45, shot0=0, B=16)[0]
    pred = sliding_window_bposd_circuit_mem(det, circ, cd["hz"], cd["lz"], 5, 3)
    ref, stats = helpers.oracle_sliding_window_parallel(wins, nz, det, ("product_sum", "serial", 2, "osd_cs", 0, 1.0, orc.FORM_LDPC_F32))
    print("oracle:", stats)
    assert stats["osd_calls"] >= 16, stats
    assert np.array_equal(pred, ref.astype(np.int64))


# ---- 4. the OSD stage alone ----------------------------------------------------------------------------------------------------
def test_offchip_osd_alone_every_tier_and_the_spill(gpu):
    """BatchDecoder.osd0 on the 2250 x 30 900 window (full row rank) with one uniformly random syndrome and posteriors ascending in
    the fault index, all equal (ties go by fault index: the same order), and descending.  The syndrome is one whose solution needs
    every one of the 2250 pivots -- 36 Q planes, most of them spilled to HBM -- and the ascending order completes the rank only at
    fault 27 626: more than 26 tiers of 1024 columns are drawn and eliminated.  Equal to Graph.osd0 in each case.  (Oracle: solutions of weight
    1098 / 1098 / 1125; 1.5 s for the three on one core.)"""
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    H, pri = _qlp_window0()
    m, n = H.shape
    dec = BatchDecoder(WindowGraph(H, pri), max_iter=1, osd_method="osd_0")
    assert dec.info()["post_kernel"] == OFFCHIP_KERNEL
    g = orc.Graph(H, pri)
    assert g.rank() == m
    synd = np.random.default_rng(0).integers(0, 2, size=(1, m), dtype=np.uint8)
    ramp = np.arange(n, dtype=np.float32) * np.float32(0.001) - np.float32(3.0)
    cases = {"ascending": ramp, "equal": np.full(n, 0.5, np.float32), "descending": ramp[::-1].copy()}
    llr = np.stack([cases[k] for k in cases])
    bits, status = _np(dec.osd0(_dev(np.repeat(synd, len(cases), axis=0)), _dev(llr)))
    err = _unpack(bits, n)
    for i, k in enumerate(cases):
        ref, st = g.osd0(synd[0], cases[k].astype(np.float64))
        assert not st["inconsistent"] and (st["pivots"] == m or k == "descending")
        assert (status[i] >> 17) & 1 and not (status[i] >> 18) & 1
        assert (status[i] >> 20) & 0xFFF == min(st["pivots"], 4095), (k, status[i] >> 20, st)
        assert np.array_equal(err[i], ref), "%s posteriors: OSD-0 solution differs from the oracle's" % k
        if k != "descending":
            assert int(np.flatnonzero(ref).max()) == 27626 and st["cols_examined"] > 26 * 1024


# ---- 5. the certificate --------------------------------------------------------------------------------------------------------
def _both_grids_trip_graph():
    """200 x 400, column weight 4, p = 0.02: at max_iter 30 every non-trivial shot outgrows both LLR grids (the recipe of the
    coarse-grid list test in test_gpu_batch_contract.py)."""
    from scipy.sparse import csc_matrix
    rng = np.random.default_rng(2024)
    m, n, w = 200, 400, 4
    rows = np.concatenate([rng.choice(m, size=w, replace=False) for _ in range(n)])
    H = csc_matrix((np.ones(n * w, np.uint8), (rows, np.repeat(np.arange(n), w))), shape=(m, n))
    return H, np.full(n, 0.02)


def test_forced_off_chip_path_coarse_grid_and_inexact_flags(gpu):
    """512 shots that leave the fine grid and the coarse one too (a check with a single fault sends an unbounded message): bits 14
    and 15 of the status equal the oracle's account (decode_batch(..., return_grid=True)), through the redo list and its
    min(batch, 4096) capacity; any shot the oracle certifies is identical to it (the next test has such shots)."""
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    H, pri = _both_grids_trip_graph()
    n = H.shape[1]
    s = _sample(H, pri, 77, 512)
    dec = BatchDecoder(WindowGraph(H, pri), max_iter=30, osd_method="osd_0", off_chip=True)
    info = dec.info()
    assert info["edge_kernel"] and info["post_kernel"] == OFFCHIP_KERNEL and info["llr_grid_bits"] > 10, info
    bits, status = _np(dec.decode(_dev(s)))
    g, form = orc.device_arithmetic(H, pri, "minimum_sum", "parallel", 30, 1.0)
    ref, flags, grid = g.decode_batch(s, orc.make_params("minimum_sum", "parallel", 30, "osd_0", 0, 1.0, form), return_grid=True)
    coarse, inexact = grid[:, 0] != g.grid[0], grid[:, 1] != 0
    print("oracle: %d coarse, %d inexact of 512; device: %d with bit 14, %d with bit 15" %
          (coarse.sum(), inexact.sum(), ((status >> 14) & 1).sum(), ((status >> 15) & 1).sum()))
    assert coarse.sum() >= 64 and inexact.sum() >= 64
    assert np.array_equal((status >> 14) & 1, coarse.astype(int)), "coarse-grid flags differ"
    assert np.array_equal((status >> 15) & 1, inexact.astype(int)), "inexact flags differ"
    exact = ~inexact
    assert np.array_equal(_unpack(bits, n)[exact], ref[exact])
    assert np.array_equal((status[exact] >> 16) & 1, flags[exact, 0]) and np.array_equal(status[exact] & 0x3FFF, flags[exact, 1])


def test_forced_off_chip_path_redo_pass_results(gpu):
    """max_iter = 0 (n iterations) on the 288 x 2592 window: the fine grid sits on the 2^-10 floor and the shots BP cannot finish
    can outgrow it; such a shot is decoded again on the rule's grid, which certifies it.  Which shots those are, and every result --
    the redo pass's included -- equal the oracle's.  (Shots 256..383 of seed 41: the oracle sends one of them, shot 308, to the coarse grid.)"""
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    H, pri = _window("single")
    s = orc.sample_dem(H, H[:1], pri, seed=41, shot0=256, B=128)[0]
    kw = dict(bp_method="minimum_sum", schedule="parallel", max_iter=0, osd_method="osd_0")
    dec = BatchDecoder(WindowGraph(H, pri), off_chip=True, **kw)
    info = dec.info()
    assert info["edge_kernel"] and info["post_kernel"] == OFFCHIP_KERNEL and info["llr_grid_bits"] == 10, info
    flags, grid = _assert_oracle(H, pri, s, kw, _np(dec.decode(_dev(s))), certificate=True)
    coarse = grid[:, 0] != info["llr_grid_bits"]
    print("oracle: %d of 128 shots on the coarse grid, %d inexact" % (coarse.sum(), (grid[:, 1] != 0).sum()))
    assert 1 <= coarse.sum() <= 64 and not grid[:, 1].any()


# ---- 6. a syndrome outside the column space ------------------------------------------------------------------------------------
def test_forced_off_chip_path_inconsistent_syndrome(gpu):
    """The 108 x 1080 window with row 0 appended again: a syndrome that disagrees on the two copies is outside the column space.
    Forced path = default path = oracle, bit 18 set."""
    from scipy.sparse import csr_matrix, vstack
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    H0, pri = _window("w1")
    H0 = csr_matrix(H0)
    H = vstack([H0, H0[0]]).tocsr()
    s = _sample(H, pri, 91, 64)
    assert np.array_equal(s[:, 0], s[:, -1])
    s[:, -1] ^= 1
    kw = dict(bp_method="minimum_sum", schedule="parallel", max_iter=8, osd_method="osd_0")
    wg = WindowGraph(H, pri)
    forced = BatchDecoder(wg, off_chip=True, **kw)
    assert forced.info()["post_kernel"] == OFFCHIP_KERNEL
    a, b = _np(BatchDecoder(wg, **kw).decode(_dev(s))), _np(forced.decode(_dev(s)))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1] & 0xFFFFF, b[1] & 0xFFFFF)
    _assert_oracle(H, pri, s, kw, b, certificate=True)
    assert ((b[1] >> 18) & 1).all() and ((b[1] >> 17) & 1).all()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_offchip_window_refuses_higher_order_and_lsd_only(gpu):
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    H, pri = _qlp_window0()
    wg = WindowGraph(H, pri)
    for kw in (dict(osd_method="osd_cs", osd_order=1), dict(osd_method="lsd_cs", osd_order=0)):
        with pytest.raises(NotImplementedError, match="2250 x 30900"):
            BatchDecoder(wg, max_iter=4, **kw)
    s = _sample(H, pri, 2, 8)
    for kw in (dict(osd_method="osd_cs", osd_order=0), dict(osd_method="osd_off")):
        dec = BatchDecoder(wg, max_iter=4, **kw)
        assert dec.info()["post_kernel"] == (OFFCHIP_KERNEL if kw["osd_method"] != "osd_off" else "none")
        full = dict(bp_method="minimum_sum", schedule="parallel", max_iter=4, **kw)
        _assert_oracle(H, pri, s, full, _np(dec.decode(_dev(s))), certificate=True)
