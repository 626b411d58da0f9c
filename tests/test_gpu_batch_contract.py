"""The batch contract of the decode calls (include/quits_amd.h, "decode"): what every production call depends on and the parity
tests only reach by accident.

A. Every kernel that reads a syndrome honours the detector slice (det_offset), the row strides and the carry (d_upd, upd_rows):
   the same decoder on a record with an odd offset, an odd stride, noise around the slice and a carry XORed in returns what it
   returns on the contiguous syndromes; that result equals the oracle's; and without the carry the result changes (the control).
B. One decoder over a fixed script of calls -- batch sizes around the wavefront, growth past the workspace, an empty batch,
   reserve / release, stages on their own and on two streams, batches that all / never converge, qd_osd0_batch in between --
   returns for every call what a fresh decoder returns.
C. The coarse-grid list holds min(batch, 4096) shots: what a batch that overflows it gets.
D. The byte and bit plumbing (qd_gf2_spmv_batch, qd_unpack_bits, qd_count_mismatch, qd_sample_dem, qd_sample_circuit) against
   numpy, the oracle's sampler and the frame mirror at the shapes and counters where such kernels go wrong."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle as orc

pytestmark = pytest.mark.gpu

BB72 = "bb72_custom_r6_p0.003"
SWITCHES = ("QD_NO_SCATTER", "QD_SCATTER_M2_LIMIT", "QD_SCATTER_CPL1", "QD_SCATTER_WIDE_T704", "QD_SCATTER_NATURAL_ROUNDS",
            "QD_SCATTER_BANKS_BY_SLOT", "QD_SCATTER_WALK_GREEDY", "QD_OSDCS_OLD", "QD_GEN_STAGES")


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _unpack(bits, n):
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :n]


def _set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _window(which):
    """(H, priors) of a committed window.  w1: the BB72 W = 3, F = 1 window 1 (108 x 1080; 36 carry rows in the real hand-off);
    single: the BB72 history as one window (288 x 2592); bb144: the headline matrix (1008 checks, rank 1002)."""
    if which == "w1":
        w = helpers.window_set(BB72, 3, 1)[1]
        return w["H"], np.asarray(w["priors"], dtype=np.float64)
    H, L, pri = helpers.dem_matrices(BB72 if which == "single" else "bb144_custom_r12_p0.003")
    return H, np.asarray(pri, dtype=np.float64)


def _sample(H, pri, seed, B):
    return orc.sample_dem(H, H[:1], pri, seed=seed, shot0=0, B=B)[0]


# ---- A. slice, strides, carry ----------------------------------------------------------------------------------------------
# (det_offset, carry rows): odd offsets -- every row of the record starts at another alignment, since the stride
# off + m + 3 is odd too -- with the hand-off's 36 rows, a single row, a carry over the whole window, and no carry at all
GEOMETRIES = ((1, 36), (1, 1), (1, "m"), (37, 36), (37, 1), (37, "m"), (37, None))


def _record(s, off, rows, rng):
    """Device inputs whose EFFECTIVE syndrome is s: rec[B, off + m + 3] with rec[:, off:off+m] = s ^ pad(u) and random 0/1 bytes
    around the slice; upd[B, rows + 5] with upd[:, :rows] = u and random 0/1 bytes beyond.  u is random; a one-row carry is
    all ones (a random one would leave half the shots without any carry and the control below could not ask for more than half)."""
    B, m = s.shape
    rec = rng.integers(0, 2, size=(B, off + m + 3), dtype=np.uint8)
    if rows is None:
        rec[:, off:off + m] = s
        return rec, None
    u = rng.integers(0, 2, size=(B, rows), dtype=np.uint8)
    if rows == 1:
        u[:] = 1
    upd = rng.integers(0, 2, size=(B, rows + 5), dtype=np.uint8)
    upd[:, :rows] = u
    sl = s.copy()
    sl[:, :rows] ^= u
    rec[:, off:off + m] = sl
    return rec, upd


def _three_way(call, s, rng, geometries=GEOMETRIES):
    """Legs 1 and 3.  call(det, det_offset, upd) -> (err_bits, status) as numpy.  Returns the contiguous result (for leg 2)."""
    m = s.shape[1]
    base = call(_dev(s), 0, None)
    for off, rows in geometries:
        rows = m if rows == "m" else rows
        rec, upd = _record(s, off, rows, rng)
        # (the wrapper takes the carry rows from the tensor's width: a view of the first `rows` columns keeps the row stride rows + 5)
        got = call(_dev(rec), off, None if upd is None else _dev(upd)[:, :rows])
        bad = np.flatnonzero((got[0] != base[0]).any(axis=1) | (got[1] != base[1]))
        assert bad.size == 0, "det_offset %d, carry rows %s: %d shots differ from the contiguous call, first %s" % (off, rows, bad.size, bad[:8])
        if upd is not None:                     # the control: the slice alone is s ^ pad(u)
            ctl = call(_dev(rec), off, None)
            differ = (ctl[0] != base[0]).any(axis=1) | (ctl[1] != base[1])
            assert differ.mean() > 0.5, "det_offset %d, carry rows %s: dropping the carry changes only %.2f of the shots" % (off, rows, differ.mean())
    return base


def _oracle_leg(H, pri, s, kw, base):
    """Leg 2: the contiguous result against the oracle in the form orc.device_arithmetic gives for these options."""
    method, schedule = kw.get("bp_method", "minimum_sum"), kw.get("schedule", "parallel")
    max_iter, alpha = kw.get("max_iter", 0), kw.get("ms_scaling_factor", 1.0)
    osd, order = kw.get("osd_method", "osd_0"), kw.get("osd_order", 0)
    edge = method != "minimum_sum" or schedule != "parallel" or kw.get("edge_messages", False)
    g, form = orc.device_arithmetic(H, pri, method, schedule, max_iter, alpha)
    if edge and form == orc.FORM_COMPRESSED_F32:
        form = orc.FORM_LDPC_F32                       # the edge kernel: ldpc's update order in float
    ref, flags, grid = g.decode_batch(s, orc.make_params(method, schedule, max_iter, osd, order, alpha, form), return_grid=True)
    bits, status = base
    assert np.array_equal((status >> 16) & 1, flags[:, 0]), "convergence flags differ"
    assert np.array_equal(status & 0x3FFF, flags[:, 1]), "iteration counts differ"
    if osd != "osd_off":
        assert np.array_equal((status >> 17) & 1, 1 - flags[:, 0]), "post-processor flags differ"
    if osd in ("osd_0", "lsd_0", "lsd_cs", "lsd_e") or order == 0:          # (the oracle reports no pivots for OSD-CS / OSD-E)
        assert np.array_equal((status >> 20) & 0xFFF, np.minimum(flags[:, 2], 4095)), "pivot counts differ"
        assert np.array_equal((status >> 18) & 1, flags[:, 3]), "inconsistent flags differ"
    if g.grid[0] >= 0 and not edge:
        assert np.array_equal((status >> 14) & 1, (grid[:, 0] != g.grid[0]).astype(int)), "coarse-grid flags differ"
        assert np.array_equal((status >> 15) & 1, grid[:, 1]), "inexact flags differ"
    bad = np.flatnonzero((_unpack(bits, H.shape[1]) != ref).any(axis=1))
    assert bad.size == 0, "output differs from the oracle on shots %s" % bad[:10]
    return flags, grid


MS = dict(max_iter=8, osd_method="osd_0")
# path -> (window, shots, seed, validation switches, decoder options, what info() must say, kind of non-vacuity condition)
PATHS = {
    "scatter_wide": ("w1", 256, 101, {}, MS, lambda i: i["scatter_wide_kernel"], "bp"),
    "scatter_one_check_per_lane": ("w1", 256, 102, {"QD_SCATTER_CPL1": "1"}, MS,
                                   lambda i: i["scatter_kernel"] and not i["scatter_wide_kernel"], "bp"),
    "gather_on_the_grid": ("w1", 256, 103, {"QD_NO_SCATTER": "1"}, MS,
                           lambda i: not i["scatter_kernel"] and not i["edge_kernel"] and i["llr_grid_bits"] >= 0, "bp"),
    # the existing tests' pairing: 40000 grid units on the 288 x 2592 window park most shots for the gather kernel's recheck launch
    "recheck_pass": ("single", 256, 104, {"QD_SCATTER_M2_LIMIT": "40000"}, dict(max_iter=30, osd_method="osd_0"),
                     lambda i: i["scatter_wide_kernel"], "bp"),
    "gather_float_llr_scaled": ("w1", 256, 105, {}, dict(max_iter=8, osd_method="osd_0", ms_scaling_factor=0.8125),
                                lambda i: i["llr_grid_bits"] == -1 and not i["scatter_kernel"] and not i["edge_kernel"], "bp"),
    "gather_float_llr_raw": ("w1", 256, 106, {}, dict(max_iter=8, osd_method="osd_0", raw_llr=True),
                             lambda i: i["llr_grid_bits"] == -1 and not i["scatter_kernel"] and not i["edge_kernel"], "bp"),
    "product_sum_lds": ("w1", 256, 107, {}, dict(bp_method="product_sum", schedule="parallel", max_iter=8, osd_method="osd_0"),
                        lambda i: i["edge_kernel"], "bp"),
    "edge_flooding": ("w1", 256, 108, {}, dict(max_iter=8, osd_method="osd_0", edge_messages=True), lambda i: i["edge_kernel"], "bp"),
    "edge_serial_one_launch": ("w1", 256, 109, {}, dict(bp_method="product_sum", schedule="serial", max_iter=3, osd_method="osd_0"),
                               lambda i: i["edge_kernel"], "bp"),
    # max_iter = 12: launches at the bounds 3, 6, 10, the survivors' syndromes carried in the second plane
    "edge_serial_staged_product_sum": ("w1", 256, 110, {}, dict(bp_method="product_sum", schedule="serial", max_iter=12, osd_method="osd_0"),
                                       lambda i: i["edge_kernel"], "bp"),
    "edge_serial_staged_minimum_sum": ("w1", 256, 111, {}, dict(bp_method="minimum_sum", schedule="serial", max_iter=12, osd_method="osd_0"),
                                       lambda i: i["edge_kernel"], "bp"),
    "osd0_many_pivot": ("w1", 256, 112, {}, dict(max_iter=4, osd_method="osd_0"), lambda i: i["post_kernel"] == "qd_osd0_sr_kernel", "post"),
    "osdcs_panel": ("w1", 256, 113, {}, dict(max_iter=4, osd_method="osd_cs", osd_order=2), lambda i: i["post_kernel"] == "qd_osdcs_kernel", "post"),
    "osdcs_row_form": ("w1", 256, 114, {"QD_OSDCS_OLD": "1"}, dict(max_iter=4, osd_method="osd_cs", osd_order=2),
                       lambda i: i["post_kernel"] == "qd_osd0_reg_kernel<row form>", "post"),
    "lsd0": ("w1", 256, 115, {}, dict(max_iter=4, osd_method="lsd_0"), lambda i: i["post_kernel"] == "qd_lsd0_kernel", "post"),
    "lsdcs_order1": ("w1", 256, 116, {}, dict(max_iter=4, osd_method="lsd_cs", osd_order=1), lambda i: i["post_kernel"] == "qd_lsd0_kernel", "post"),
}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_syndrome_slice_strides_and_carry(gpu, monkeypatch, path):
    """One syndrome reader per id (the table of the module docstring's part A): legs 1-3 on DEM-sampled syndromes of the window.
    BP paths run with OSD-0, post-processor paths with the default BP (the scatter kernel) cut short so that shots reach them.
    gather_float_llr_raw has no oracle form of its own (round-1 arithmetic, QD_FLAG_RAW_LLR); the same kernel is compared with
    the oracle under gather_float_llr_scaled."""
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    which, shots, seed, env, kw, info_ok, kind = PATHS[path]
    H, pri = _window(which)
    s = _sample(H, pri, seed, shots)
    _set_env(monkeypatch, env)
    dec = BatchDecoder(WindowGraph(H, pri), **kw)
    assert info_ok(dec.info()), (path, dec.info())
    base = _three_way(lambda det, off, upd: _np(dec.decode(det, off, upd)), s, np.random.default_rng(seed))
    status = base[1]
    conv = ((status >> 16) & 1).mean()
    print("%s: converged share %.3f, post-processed shots %d" % (path, conv, int(((status >> 17) & 1).sum())))
    if kind == "bp":
        assert 0 < conv < 1, conv
    else:
        assert ((status >> 17) & 1).sum() >= 10, "the post-processor is not exercised"
    if path != "gather_float_llr_raw":
        _oracle_leg(H, pri, s, kw, base)


def test_syndrome_slice_coarse_grid_pass(gpu, monkeypatch):
    """The coarse-grid launch (the gather kernel over redo_list): ldpc's max_iter = 0 on the 288 x 2592 window, the input of
    test_large_max_iter_keeps_a_fine_llr_grid -- the oracle puts 1 of these 400 shots on the coarse grid (22 do not converge)."""
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    H, L, pri = helpers.dem_matrices(BB72)
    s, _, _ = orc.sample_dem(H, L, pri, seed=41, shot0=0, B=400)
    _set_env(monkeypatch, {})
    kw = dict(max_iter=0, osd_method="osd_0")
    dec = BatchDecoder(WindowGraph(H, pri), **kw)
    assert dec.info()["scatter_kernel"] and dec.info()["llr_grid_bits"] == 10
    base = _three_way(lambda det, off, upd: _np(dec.decode(det, off, upd)), s, np.random.default_rng(41),
                      geometries=((1, 36), (37, "m"), (37, None)))
    flags, grid = _oracle_leg(H, pri, s, kw, base)
    print("coarse-grid shots by the oracle: %d, non-converged %d" % (int((grid[:, 0] != 10).sum()), int((1 - flags[:, 0]).sum())))
    assert (grid[:, 0] != 10).sum() >= 1, "no shot takes the coarse-grid pass"
    assert ((base[1] >> 14) & 1).sum() >= 1


def test_syndrome_slice_inconsistent_hand_over(gpu, monkeypatch):
    """OSD-0: the many-pivot kernel hands the shots whose syndrome is outside the column space to the register kernel, which reads
    the syndrome again.  BB144 headline matrix (rank 1002 of 1008).  Batch 1: the effective syndrome is random (mostly inconsistent)
    and the slice alone is not it; batch 2: the slice alone is random and the carry, over the whole window, turns it into a
    DEM-sampled, consistent syndrome.  Status bit 18 and the outputs follow the effective syndrome in both."""
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    H, pri = _window("bb144")
    m = H.shape[0]
    rng = np.random.default_rng(7)
    _set_env(monkeypatch, {})
    kw = dict(max_iter=8, osd_method="osd_0")
    dec = BatchDecoder(WindowGraph(H, pri), **kw)
    assert dec.info()["post_kernel"] == "qd_osd0_sr_kernel"
    inconsistent, shots = 0, 0
    for batch, s in enumerate(((rng.random((64, m)) < 0.15).astype(np.uint8), _sample(H, pri, 71, 64))):
        off, rows = (37, 36) if batch == 0 else (1, m)
        base = _three_way(lambda det, off_, upd: _np(dec.decode(det, off_, upd)), s, rng, geometries=((off, rows),))
        flags, _ = _oracle_leg(H, pri, s, kw, base)
        assert np.array_equal((base[1] >> 18) & 1, flags[:, 3])
        inconsistent += int(flags[:, 3].sum())
        shots += len(s)
        print("batch %d: %d of %d effective syndromes inconsistent" % (batch, int(flags[:, 3].sum()), len(s)))
    assert 0 < inconsistent < shots


@pytest.mark.parametrize("method,order", [("osd_0", 0), ("osd_cs", 2), ("lsd_0", 0)])
def test_syndrome_slice_osd_alone(gpu, monkeypatch, method, order):
    """qd_osd0_batch (the post-processor alone on caller-supplied posteriors) reads the same slice and carry: legs 1 and 3, and
    the contiguous result against the oracle's osd0 / osd_w / lsd0 on the effective syndromes."""
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    H, pri = _window("w1")
    n = H.shape[1]
    B = 24
    rng = np.random.default_rng(29)
    s = _sample(H, pri, 117, B)
    llr = (np.log((1 - pri) / pri)[None, :] + 2.0 * rng.normal(size=(B, n))).astype(np.float32)
    _set_env(monkeypatch, {})
    dec = BatchDecoder(WindowGraph(H, pri), max_iter=1, osd_method=method, osd_order=order)
    llr_d = _dev(llr)
    base = _three_way(lambda det, off, upd: _np(dec.osd0(det, llr_d, off, upd)), s, rng)
    err = _unpack(base[0], n)
    g = orc.Graph(H, pri)
    for b in range(B):
        if method == "osd_0":
            ref, st = g.osd0(s[b], llr[b].astype(np.float64), stop_early=True)
        elif method == "osd_cs":
            ref, st = g.osd_w(s[b], llr[b].astype(np.float64), method, order, fixed=True)
        else:
            ref, st = g.lsd0(s[b], llr[b].astype(np.float64))
        assert np.array_equal(err[b], ref), (method, b, st)
        if method != "osd_cs":
            assert ((base[1][b] >> 20) & 0xFFF) == min(st["pivots"], 4095) and bool(base[1][b] & (1 << 18)) == st["inconsistent"], (b, st)
    assert s.any(axis=1).sum() >= 10


@pytest.mark.parametrize("env", [{}, {"QD_NO_SCATTER": "1"}], ids=["scatter_wide", "gather"])
def test_syndrome_slice_three_sign_words(gpu, monkeypatch, env):
    """The QLP window (1350 x 18900, rows of up to 78 faults: three sign words; three checks per lane in the scatter kernel) with a
    carry of that code's 450 rows: legs 1 and 3 on 32 shots (the arithmetic is pinned by test_wide_scatter_kernel_and_gather_kernel_agree)."""
    from scipy.sparse import csc_matrix
    from quits_amd.decoder.device import BatchDecoder, DemSampler, WindowGraph
    w = helpers.window_set("qlp1020_cardinal_r20_p0.003", 3, 1)[1]
    H, pri = w["H"], np.asarray(w["priors"], dtype=np.float64) / 3.0
    assert H.shape == (1350, 18900)
    nz = helpers.code("qlp1020")["hz"].shape[0]
    assert nz == 450
    det, _ = DemSampler(H, csc_matrix(np.ones((1, H.shape[1]), dtype=np.uint8)), pri).sample(32, seed=5, shot0=1)
    s = det.cpu().numpy()
    _set_env(monkeypatch, env)
    dec = BatchDecoder(WindowGraph(H, pri), max_iter=30, osd_method="osd_0")
    assert dec.info()["scatter_wide_kernel"] == (not env) and dec.info()["scatter_kernel"] == (not env)
    base = _three_way(lambda d, off, upd: _np(dec.decode(d, off, upd)), s, np.random.default_rng(5), geometries=((1, nz), (37, nz)))
    conv = ((base[1] >> 16) & 1).mean()
    assert 0 < conv < 1, conv


# ---- B. one decoder, many calls --------------------------------------------------------------------------------------------
KINDS = {
    "scatter_wide_osd0": ({}, dict(max_iter=20, osd_method="osd_0")),
    "gather_osd0": ({"QD_NO_SCATTER": "1"}, dict(max_iter=20, osd_method="osd_0")),
    "scatter_wide_osdcs1": ({}, dict(max_iter=20, osd_method="osd_cs", osd_order=1)),
    "scatter_wide_lsd0": ({}, dict(max_iter=20, osd_method="lsd_0")),
    "scatter_wide_osd_off": ({}, dict(max_iter=20, osd_method="osd_off")),
    "serial_product_sum_osdcs1": ({}, dict(bp_method="product_sum", schedule="serial", max_iter=9, osd_method="osd_cs", osd_order=1,
                                           edge_messages=True)),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_one_decoder_many_calls(gpu, monkeypatch, kind):
    """The script below on ONE decoder (BB72 single window, slices of one sampled set); every call's (err_bits, status) equals a
    FRESH decoder's on the same rows, the first and the last call's equal the oracle's.  The two counter sets, the zeroing of the
    next call's counters behind a call's last stage, the workspace rebuilt on growth and the read-back of the failure count are
    what a stale value would come from."""
    import torch
    from quits_amd import _lib
    from quits_amd.decoder.device import BatchDecoder, DemSampler, WindowGraph
    env, kw = KINDS[kind]
    post = kw["osd_method"] != "osd_off"
    edge = kw.get("edge_messages", False)
    H, L, pri = helpers.dem_matrices(BB72)
    m, n = H.shape
    _set_env(monkeypatch, env)
    det, _ = DemSampler(H, L, pri).sample(6000, seed=2718)
    g = WindowGraph(H, pri)
    dec = BatchDecoder(g, **kw)
    info = dec.info()
    assert info["edge_kernel"] == edge and info["scatter_wide_kernel"] == (not edge and not env), info
    cache = {}

    def fresh(x, key):
        if key not in cache:
            cache[key] = _np(BatchDecoder(g, **kw).decode(x))
        return cache[key]

    def check(tag, x, key, out=None):
        got = _np(dec.decode(x) if out is None else out)
        exp = fresh(x, key)
        bad = np.flatnonzero((got[0] != exp[0]).any(axis=1) | (got[1] != exp[1]))
        assert bad.size == 0, "%s / %s: %d of %d shots differ from a fresh decoder's, first %s" % (kind, tag, bad.size, len(x), bad[:8])
        return got

    def rows(a, k):
        return det[a:a + k]

    # batch sizes around the wavefront, growth past the workspace (cap 300 -> 5000: everything freed and rebuilt), smaller again
    a, first = 0, None
    for k in (1, 63, 64, 65, 300, 5000, 7, 300):
        got = check("B = %d" % k, rows(a, k), (a, k))
        first = got if first is None else first
        a += k
    assert a == 5800
    _oracle_leg(H, pri, det[:1].cpu().numpy(), kw, first)
    # an empty batch: QD_OK whatever the pointers, no buffer touched, the next call unaffected
    b0, s0 = dec.decode(rows(0, 0))
    assert b0.shape == (0, g.words) and s0.shape == (0,)
    keep_bits = torch.full((4, g.words), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    keep_st = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = C.c_void_p(0)
    for stage in (1, 2, 3):
        assert dec._L.qd_decode_stage(dec._h, C.c_void_p(det.data_ptr()), det.stride(0), 0, null, 0, 0, 0, C.c_void_p(keep_bits.data_ptr()),
                                      C.c_void_p(keep_st.data_ptr()), stage, sp) == 0
        assert dec._L.qd_decode_stage(dec._h, null, 0, 0, null, 0, 0, 0, null, null, stage, sp) == 0
    if post:
        e0, t0 = dec.osd0(rows(0, 0), torch.empty((0, n), dtype=torch.float32, device="cuda"))
        assert e0.shape == (0, g.words) and t0.shape == (0,)
        assert dec._L.qd_osd0_batch(dec._h, C.c_void_p(det.data_ptr()), det.stride(0), 0, null, 0, 0, 0, null, C.c_void_p(keep_bits.data_ptr()),
                                    C.c_void_p(keep_st.data_ptr()), sp) == 0
    torch.cuda.synchronize()
    assert bool((keep_bits == 0x5A5A5A5A).all()) and bool((keep_st == -7).all())
    check("after B = 0", rows(100, 64), (100, 64))
    # reserve / release between calls
    dec.reserve(8192)
    check("after reserve", rows(200, 300), (200, 300))
    dec.release_workspace()
    # (stage 2 for a batch the workspace does not hold -- here: none at all -- is refused: it would walk lists of another size)
    with pytest.raises(_lib.QdError):
        dec.decode(rows(300, 65), stage=2)
    check("after release", rows(300, 65), (300, 65))
    # stage 1, then stage 3 on other rows: the outputs are those of the stage-3 rows
    dec.decode(rows(0, 300), stage=1)
    check("stage 1, stage 3 on other rows", rows(1000, 300), (1000, 300), out=dec.decode(rows(1000, 300), stage=3))
    # stage 1 on a side stream, an event, stage 2 on the current stream with the same arguments
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    for head_start in (False, True):
        x = rows(1500 + 400 * head_start, 300)
        bits = torch.empty((300, g.words), dtype=torch.int32, device="cuda")
        st = torch.empty((300,), dtype=torch.int32, device="cuda")
        side.wait_stream(cur)
        dec.decode(x, err_bits=bits, status=st, stage=1, stream=side)
        if head_start:
            dec.post_head_start(side)
        ev = torch.cuda.Event()
        ev.record(side)
        cur.wait_event(ev)
        dec.decode(x, err_bits=bits, status=st, stage=2)
        side.wait_stream(cur)
        check("two streams%s" % (", post_head_start" if head_start else ""), x, (1500 + 400 * head_start, 300), out=(bits, st))
    # every shot converges (zero syndromes and weight-1 errors), none does (random syndromes), and back
    Hd = np.asarray(H.todense(), dtype=np.uint8)
    easy = _dev(np.concatenate([np.zeros((16, m), np.uint8), Hd[:, 0:2400:10].T]))
    hard = (torch.rand((300, m), device="cuda") < 0.25).to(torch.uint8)
    for rep, (x, key) in enumerate(((easy, "easy"), (hard, "hard"), (easy, "easy"), (hard, "hard"))):
        got = check("all converge / none converges, call %d" % rep, x, key)
        conv = (got[1] >> 16) & 1
        assert conv.all() if key == "easy" else not conv.any(), (kind, key, conv.mean())
    # qd_osd0_batch between two decode() calls
    if post:
        x = rows(600, 48)
        rng = np.random.default_rng(5)
        llr = _dev((np.log((1 - pri) / pri)[None, :] + 2.0 * rng.normal(size=(48, n))).astype(np.float32))
        got, exp = _np(dec.osd0(x, llr)), _np(BatchDecoder(g, **kw).osd0(x, llr))
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (kind, "osd0 between decodes")
        check("after osd0", rows(700, 300), (700, 300))
    # the edge kernel's workspace cut to ~ 256-shot chunks between two calls
    if edge:
        dec.set_workspace_limit(int(0.02 * 2**30))
        check("after set_workspace_limit", rows(2500, 1500), (2500, 1500))
    last = check("last call", rows(5500, 300), (5500, 300))
    _oracle_leg(H, pri, det[5500:5800].cpu().numpy(), kw, last)


# ---- C. the coarse-grid list's capacity -------------------------------------------------------------------------------------
def _both_grids_trip_graph():
    """200 x 400, column weight 4, p = 0.02: at max_iter 30 every non-trivial shot outgrows both LLR grids."""
    from scipy.sparse import csc_matrix
    rng = np.random.default_rng(2024)
    m, n, w = 200, 400, 4
    rows = np.concatenate([rng.choice(m, size=w, replace=False) for _ in range(n)])
    H = csc_matrix((np.ones(n * w, np.uint8), (rows, np.repeat(np.arange(n), w))), shape=(m, n))
    return H, np.full(n, 0.02)


def test_coarse_grid_list_capacity(gpu, monkeypatch):
    """Off the 2^-10 floor the coarse-grid list holds min(batch, 4096) shots; a shot that finds it full keeps its fine-grid result
    and gets QD_STATUS_INEXACT without QD_STATUS_COARSE_GRID (quits_amd.h).  5000 shots that all leave the fine grid: every shot the
    oracle flags inexact carries bit 15, exactly 4096 carry bit 14, and no shot outside the oracle's inexact set differs from it."""
    from quits_amd.decoder.device import BatchDecoder, WindowGraph
    H, pri = _both_grids_trip_graph()
    n = H.shape[1]
    shots = 5000
    s = _sample(H, pri, 77, shots)
    _set_env(monkeypatch, {})
    dec = BatchDecoder(WindowGraph(H, pri), max_iter=30, osd_method="osd_0")
    assert dec.info()["llr_grid_bits"] > 10, dec.info()
    bits, status = _np(dec.decode(_dev(s)))
    g, form = orc.device_arithmetic(H, pri, "minimum_sum", "parallel", 30, 1.0)
    ref, flags, grid = g.decode_batch(s, orc.make_params("minimum_sum", "parallel", 30, "osd_0", 0, 1.0, form), return_grid=True)
    coarse, inexact = grid[:, 0] != g.grid[0], grid[:, 1] != 0
    print("oracle: %d coarse, %d inexact of %d; device: %d with bit 14, %d with bit 15" %
          (coarse.sum(), inexact.sum(), shots, ((status >> 14) & 1).sum(), ((status >> 15) & 1).sum()))
    assert coarse.sum() > 4096, "the batch does not overflow the list"
    assert ((status >> 15) & 1)[inexact].all(), "a shot the oracle flags inexact lacks QD_STATUS_INEXACT"
    assert ((status >> 14) & 1).sum() == 4096
    exact = ~inexact
    assert np.array_equal(_unpack(bits, n)[exact], ref[exact])
    assert np.array_equal((status[exact] >> 16) & 1, flags[exact, 0]) and np.array_equal(status[exact] & 0x3FFF, flags[exact, 1])
    # the shots without bit 14 that left the fine grid are the overflow: fine-grid result, flagged inexact
    over = coarse & (((status >> 14) & 1) == 0)
    assert over.sum() == coarse.sum() - 4096 and ((status >> 15) & 1)[over].all()


# ---- D. the plumbing kernels against numpy ----------------------------------------------------------------------------------
def _pack(e):
    """uint8 [B, k] -> int32 [B, ceil(k / 32)] words, bit (j & 31) of word (j >> 5) = e[:, j]."""
    B, k = e.shape
    pad = np.zeros((B, (-k) % 32), np.uint8)
    return np.packbits(np.concatenate([e, pad], axis=1), axis=1, bitorder="little").view(np.int32)


@pytest.mark.parametrize("nrows", [1, 31, 32, 33, 511, 512, 513, 1500])
def test_gf2_xor_apply_against_numpy(gpu, nrows):
    """qd_gf2_spmv_batch in its two forms (by set column for up to 512 rows, by row beyond): dense product mod 2 in numpy.  The error
    rows are wider than ncols and carry set bits beyond it (faults of the window that are not committed), sit in a wider tensor,
    and the output is a column slice of a wider tensor whose neighbours must stay as they were."""
    import torch
    from scipy.sparse import csr_matrix
    from quits_amd.decoder.device import GF2Matrix
    rng = np.random.default_rng(nrows)
    for ncols in (1, 31, 32, 33, 1000):
        for density in (0.0, 0.3 if ncols < 100 else 0.02):
            A = (rng.random((nrows, ncols)) < density).astype(np.uint8)
            M = GF2Matrix(csr_matrix(A))
            words = (ncols + 31) // 32 + 1                               # one word more than the matrix has columns for
            for B in (1, 3, 4, 5, 257):
                for zero_errors in (False, True):
                    e = (rng.random((B, 32 * words)) < 0.4).astype(np.uint8)
                    if zero_errors:
                        e[:, :ncols] = 0                                 # (the bits beyond ncols stay set)
                    wide = np.full((B, words + 2), -1, np.int32)
                    wide[:, :words] = _pack(e)
                    err = _dev(wide)[:, :words]
                    assert err.stride(0) == words + 2
                    want = (e[:, :ncols].astype(np.int64) @ A.T.astype(np.int64)) % 2
                    for accumulate in (False, True):
                        old = rng.integers(0, 2 if accumulate else 256, size=(B, nrows + 7), dtype=np.uint8)
                        buf = _dev(old)
                        out = buf[:, 3:3 + nrows]
                        M.xor_apply(err, out, accumulate=accumulate)
                        got = buf.cpu().numpy()
                        exp = old.copy()
                        exp[:, 3:3 + nrows] = (old[:, 3:3 + nrows] ^ want) if accumulate else want
                        assert np.array_equal(got, exp), (nrows, ncols, density, B, zero_errors, accumulate)


@pytest.mark.parametrize("nbits", [1, 31, 32, 33, 1080])
def test_unpack_bits_against_numpy(gpu, nbits):
    from quits_amd.decoder.device import unpack_bits
    rng = np.random.default_rng(nbits)
    words = (nbits + 31) // 32
    for B in (1, 5, 257):
        wide = rng.integers(-2**31, 2**31, size=(B, words + 3), dtype=np.int64).astype(np.int32)
        bits = _dev(wide)[:, :words]
        assert bits.stride(0) == words + 3
        got = unpack_bits(bits, nbits).cpu().numpy()
        assert got.shape == (B, nbits) and np.array_equal(got, _unpack(wide[:, :words], nbits))


@pytest.mark.parametrize("k", [1, 12, 136])
def test_count_mismatch_against_numpy(gpu, k):
    from quits_amd.decoder.device import count_mismatch
    rng = np.random.default_rng(k)
    for B in (1, 63, 64, 65, 255, 256, 257, 100000):
        obs = rng.integers(0, 2, size=(B, k), dtype=np.uint8)
        assert int(count_mismatch(_dev(obs), _dev(obs)).item()) == 0
        for b in (B - 1, 0):                       # one bit of the last shot, one of the first
            pred = obs.copy()
            pred[b, k - 1 if b else 0] ^= 1
            assert int(count_mismatch(_dev(pred), _dev(obs)).item()) == 1, (k, B, b)
        pred = obs ^ (rng.random((B, k)) < 0.5 / k).astype(np.uint8)
        want = int((pred != obs).any(axis=1).sum())
        assert int(count_mismatch(_dev(pred), _dev(obs)).item()) == want, (k, B)
        # non-contiguous views (the wrapper makes them contiguous): columns of a wider tensor, every other row
        wp, wo = rng.integers(0, 2, size=(B, k + 3), dtype=np.uint8), rng.integers(0, 2, size=(B, k + 3), dtype=np.uint8)
        wp[:, 2:2 + k], wo[:, 2:2 + k] = pred, obs
        assert int(count_mismatch(_dev(wp)[:, 2:2 + k], _dev(wo)[:, 2:2 + k]).item()) == want, (k, B, "column slice")
        want2 = int((pred[::2] != obs[::2]).any(axis=1).sum())
        assert int(count_mismatch(_dev(pred)[::2], _dev(obs)[::2]).item()) == want2, (k, B, "row step")


@pytest.mark.parametrize("shot0", [2**32 - 3, 2**40 + 5])
def test_dem_sampler_counter_words_and_edge_priors(gpu, shot0):
    """qd_sample_dem against orc.sample_dem bit for bit where the Philox counter and key have high words: a seed with two non-zero
    halves, batches that cross the low counter word's wrap (shot0 = 2^32 - 3) or sit beyond it (2^40 + 5), a partial last
    Philox group (n = 1, 3, 5), priors of exactly 0 (never), 1 (always), 2^-33 (threshold 0: never) and 0.5, and an observable
    matrix with an empty column."""
    from scipy.sparse import csc_matrix
    from quits_amd.decoder.device import DemSampler
    seed = (0x9E3779B9 << 32) | 0x7F4A7C15
    special = np.array([1.0, 0.5, 0.0, 2.0**-33, 0.3])
    rng = np.random.default_rng(3)
    B = 64
    fired = 0
    for m in (1, 33):
        for n in (1, 3, 5):
            for rot in range(5):
                pri = np.roll(special, rot)[:n].copy()
                Hd = (rng.random((m, n)) < 0.6).astype(np.uint8)
                Hd[0, :] = 1                                       # every fault shows in detector 0
                Ld = (rng.random((3, n)) < 0.6).astype(np.uint8)
                Ld[:, n - 1] = 0                                   # a fault that flips no observable
                H, L = csc_matrix(Hd), csc_matrix(Ld)
                det, obs = DemSampler(H, L, pri).sample(B, seed=seed, shot0=shot0)
                s_ref, o_ref, nf = orc.sample_dem(H, L, pri, seed=seed, shot0=shot0, B=B)
                assert np.array_equal(det.cpu().numpy(), s_ref), (m, n, rot)
                assert np.array_equal(obs.cpu().numpy(), o_ref), (m, n, rot)
                assert (nf >= (pri == 1.0).sum()).all() and (nf <= (pri >= 0.3).sum()).all(), (m, n, rot)
                fired += int(nf.sum())
    assert fired > 0
    # a real window across the same counters, and its composition from the two sides of the wrap
    H, L, pri = helpers.dem_matrices(BB72)
    smp = DemSampler(H, L, pri)
    det, obs = smp.sample(40, seed=seed, shot0=shot0)
    s_ref, o_ref, _ = orc.sample_dem(H, L, pri, seed=seed, shot0=shot0, B=40)
    assert np.array_equal(det.cpu().numpy(), s_ref) and np.array_equal(obs.cpu().numpy(), o_ref) and s_ref.any()
    d2, o2 = smp.sample(37, seed=seed, shot0=shot0 + 3)
    assert np.array_equal(d2.cpu().numpy(), s_ref[3:]) and np.array_equal(o2.cpu().numpy(), o_ref[3:])


def test_circuit_sampler_across_the_counter_wrap(gpu):
    """test_device_equals_mirror with shot0 = 2^32 - 100: the batch crosses into the high counter word."""
    import frame_mirror as fm
    from quits_amd.decoder.device import CircuitSampler
    seed = (0x9E3779B9 << 32) | 0x7F4A7C15
    text = helpers.circuit_text(BB72)
    B, shot0 = 4133, 2**32 - 100
    det, obs = CircuitSampler(text).sample(B, seed=seed, shot0=shot0)
    rdet, robs = fm.sample(text, seed, shot0, B)
    d = det.cpu().numpy()
    assert np.array_equal(d, rdet), "%d of %d detector bytes differ" % (int((d != rdet).sum()), d.size)
    assert np.array_equal(obs.cpu().numpy(), robs)
    assert rdet[:100].any() and rdet[100:].any()
