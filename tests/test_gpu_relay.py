"""Relay-BP on the device (csrc/bp_relay.hip, qd_decoder_create_relay) against its definition, quits_amd.relay.relay_mirror: error bits, the
iteration field, CONVERGED and the leg bits, bit for bit.  Shots are drawn from the (scaled) priors with a numpy generator, so the mirror
sees the same bytes; the scale of every window was chosen with the mirror so that shots solved in leg 0, shots solved in a later leg and
unsolved shots all occur (asserted: no path is vacuously green).  Budgets: pre_iter 20, 4 sets of 15, at most 96 shots."""
import functools

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import helpers
import test_graph_layout as tgl
from quits_amd import _lib
from quits_amd.relay import RelayConfig, relay_gammas, relay_mirror

pytestmark = pytest.mark.gpu

NAME = "bb72_custom_r6_p0.003"
SMALL = dict(pre_iter=20, num_sets=4, set_max_iter=15)
B = 96
# window -> (prior scale, sign mode of the layout, record chunks, threads): mirror counts (leg 0 / later / unsolved) at this scale, default_rng(1), 96 shots
WINDOWS = {
    "bb72_whole": (1.0, 1, 2, 512),                 # 63 / 25 / 8     (rows of up to 35 faults: signs 32.. in the state's meta word)
    "bb72_W3_window0": (1.5, 1, 2, 256),            # 42 / 32 / 22
    "96x720_rows_of_28": (2.0, 0, 2, 256),          # 74 / 10 / 12    (no fixture window has rows of at most 32 faults: sign mode 0 is synthetic)
    "70x300_rows_to_40": (2.0, 1, None, 256),       # 68 / 10 / 11 (7 zero syndromes)
    "rows_of_255": (1.0, 2, None, 512),             # 44 / 23 / 25 (4 zero syndromes)
    "column_of_weight_16": (2.0, 1, 5, 256),        # 52 / 15 / 29
}


@functools.lru_cache(maxsize=None)
def window(name):
    if name == "bb72_whole":
        H, _, pri = helpers.dem_matrices(NAME)
    elif name == "bb72_W3_window0":
        w = helpers.window_set(NAME, 3, 1)[0]
        H, pri = w["H"], w["priors"]
    elif name == "96x720_rows_of_28":
        H, pri = helpers.synthetic_window([28] * 96, 3, 6, 40028)
    else:
        H, pri = tgl._syn(name)
        if isinstance(H, tuple):
            rp, ci, n = H
            H = csr_matrix((np.ones(len(ci), np.uint8), ci, rp), shape=(len(rp) - 1, n))
    H = csr_matrix(H)
    H.sort_indices()
    pri = np.minimum(np.asarray(pri, dtype=np.float64) * WINDOWS[name][0], 0.4)
    pri.setflags(write=False)
    return H, pri


@functools.lru_cache(maxsize=None)
def shots(name, count=B, seed=1):
    H, pri = window(name)
    e = (np.random.default_rng(seed).random((count, H.shape[1])) < pri).astype(np.uint8)
    s = (csr_matrix(e) @ H.T).toarray().astype(np.uint8) & 1
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def mirror(name, stop_nconv=1, alpha=1.0):
    H, pri = window(name)
    return relay_mirror(H, pri, shots(name), RelayConfig(stop_nconv=stop_nconv, **SMALL), ms_scaling_factor=alpha, marginals=True)


def device_decode(H, pri, syn, cfg, gammas=None, alpha=1.0, osd_method="osd_off", **kw):
    import torch
    from quits_amd.decoder.device import RelayBatchDecoder, WindowGraph, unpack_bits
    wg = WindowGraph(H, pri)
    dec = RelayBatchDecoder(wg, cfg, osd_method=osd_method, ms_scaling_factor=alpha, gammas=gammas)
    bits, st = dec.decode(torch.from_numpy(np.array(syn, dtype=np.uint8)).cuda(), **kw)
    torch.cuda.synchronize()
    return unpack_bits(bits, wg.n).cpu().numpy(), st.cpu().numpy(), dec


def assert_same(err, st, ref, what=""):
    r_err, r_solved, r_it, r_leg, _ = ref[:5]
    print("%s: %d shots, %d solved in leg 0, %d later, %d unsolved; iterations mean %.1f max %d" % (
        what, len(r_it), int((r_solved & (r_leg == 0)).sum()), int((r_solved & (r_leg > 0)).sum()), int((~r_solved).sum()), r_it.mean(), r_it.max()))
    assert np.array_equal(st & _lib.STATUS_ITER_MASK, r_it), what
    assert np.array_equal((st & _lib.STATUS_CONVERGED) != 0, r_solved), what
    assert np.array_equal((st & _lib.STATUS_RELAY_LEG_MASK) >> _lib.STATUS_RELAY_LEG_SHIFT, r_leg), what
    assert np.array_equal(err, r_err), what
    assert not (st & (_lib.STATUS_COARSE_GRID | _lib.STATUS_INEXACT | _lib.STATUS_OSD)).any()


def assert_all_outcomes(ref, syn):
    _, solved, _, leg, _ = ref[:5]
    nz = syn.any(axis=1)
    assert (solved & (leg == 0) & nz).sum() >= 4 and (solved & (leg > 0)).sum() >= 4 and (~solved).sum() >= 4


def test_every_sign_mode_has_a_window():
    assert {v[1] for v in WINDOWS.values()} == {0, 1, 2}


@pytest.mark.parametrize("name", list(WINDOWS))
def test_bit_exact_against_the_mirror(gpu, name):
    from quits_amd.decoder.device import WindowGraph
    H, pri = window(name)
    _, sign_mode, chunks, threads = WINDOWS[name]
    info = WindowGraph(H, pri).info()
    assert info["bp_threads"] == threads
    rdeg = (info["max_row_weight"] + 3) & ~3
    assert (0 if rdeg <= 32 else (1 if rdeg <= 44 else 2)) == sign_mode
    if chunks:
        assert (1 + info["max_col_weight"] + 3) // 4 == chunks
    ref = mirror(name)
    assert_all_outcomes(ref, shots(name))
    err, st, dec = device_decode(H, pri, shots(name), RelayConfig(**SMALL))
    assert dec.info()["llr_grid_bits"] == -1
    zero = ~shots(name).any(axis=1)
    assert np.array_equal((st & _lib.STATUS_ZERO) != 0, zero)
    assert_same(err, st, ref, name)


@pytest.mark.parametrize("stop_nconv,alpha", [(3, 1.0), (1, 0.625), (1, 0.0)])
def test_more_candidates_and_scaled_messages(gpu, stop_nconv, alpha):
    H, pri = window("bb72_whole")
    ref = mirror("bb72_whole", stop_nconv, alpha)
    if stop_nconv > 1:
        assert (ref[4] > 1).sum() >= 4 and (ref[3][ref[1]] > 0).sum() >= 4          # several candidates; a later one was the lighter
    err, st, _ = device_decode(H, pri, shots("bb72_whole"), RelayConfig(stop_nconv=stop_nconv, **SMALL), alpha=alpha)
    assert_same(err, st, ref, "stop_nconv %d alpha %g" % (stop_nconv, alpha))


def test_negative_zero_messages(gpu):
    """A table that holds exactly -0.0 and negative strengths, on equal priors: every message is then a small multiple of one float, with
    gamma = 0 or -0.5 marginals and "posterior minus own message" pass through zero exactly, and fault->check messages equal to 0 occur by
    the thousand (the mirror counts them: 70 783 on these shots, and check->fault messages -0 with them); shots are solved in every leg.
    A fault->check message of -0 itself could not be made: x - y is -0 only for x = -0, a sum is -0 only if every term is, and
    Lam_j = a_j + gamma_j M_j = -0 needs a_j = -0 -- a prior of exactly 1/2 under gamma_j > 1 -- together with gamma_j M_j = -0, which
    needs M_j = -0, i.e. an earlier Lam_j = -0: the first Lam_j is a_j + gamma_j (+0) = +0, so there is none."""
    H, _ = window("bb72_W3_window0")
    n = H.shape[1]
    pri = np.full(n, 1.0 / 17.0)                          # L0 = log 16
    cfg = RelayConfig(pre_iter=6, num_sets=3, set_max_iter=10, gamma0=0.0)
    gam = np.full((3, n), -0.5, dtype=np.float32)
    gam[0, ::2] = -0.0
    gam[1, ::3] = -0.0
    gam[2, 1::2] = -0.5
    e = (np.random.default_rng(5).random((64, n)) < 0.006).astype(np.uint8)
    syn = (csr_matrix(e) @ H.T).toarray().astype(np.uint8) & 1
    trace = {}
    ref = relay_mirror(H, pri, syn, cfg, gammas=gam, trace=trace)
    print("fault->check messages equal to +-0 in the mirror's run: %d, to -0: %d" % (trace["nu_zero"], trace["nu_neg_zero"]))
    assert trace["nu_zero"] >= 1 and (ref[1] & (ref[3] > 0)).sum() >= 4
    err, st, _ = device_decode(H, pri, syn, cfg, gammas=gam)
    assert_same(err, st, ref, "negative zero")


@pytest.mark.parametrize("name", list(WINDOWS))
def test_one_leg_without_memory_is_the_float_min_sum_kernel(gpu, name):
    """The two kernels built on csrc/bp_gather_common.h against each other: every sign mode, 2 and 5 record chunks."""
    import torch
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    H, pri = window(name)
    syn = shots(name)
    err, st, _ = device_decode(H, pri, syn, RelayConfig(pre_iter=30, num_sets=0, gamma0=0.0))
    wg = WindowGraph(H, pri)
    old = BatchDecoder(wg, raw_llr=True, osd_method="osd_off", max_iter=30)
    bits, st0 = old.decode(torch.from_numpy(np.array(syn, dtype=np.uint8)).cuda())
    st0 = st0.cpu().numpy()
    assert np.array_equal(err, unpack_bits(bits, wg.n).cpu().numpy())
    assert np.array_equal(st & (_lib.STATUS_ITER_MASK | _lib.STATUS_CONVERGED), st0 & (_lib.STATUS_ITER_MASK | _lib.STATUS_CONVERGED))
    conv = (st0 & _lib.STATUS_CONVERGED) != 0
    assert conv.sum() >= 4 and (~conv).sum() >= 4


def test_unsolved_shots_go_to_the_post_processor(gpu):
    import torch
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    H, pri = window("bb72_whole")
    syn = shots("bb72_whole")
    ref = mirror("bb72_whole")
    r_err, r_solved, r_it, r_leg, _, r_marg = ref
    err, st, _ = device_decode(H, pri, syn, RelayConfig(**SMALL), osd_method="osd_0")
    off, st_off, _ = device_decode(H, pri, syn, RelayConfig(**SMALL))
    assert np.array_equal(((st & _lib.STATUS_OSD) != 0), ~r_solved)
    assert np.array_equal(err[r_solved], off[r_solved]) and np.array_equal(st[r_solved], st_off[r_solved])
    un = np.flatnonzero(~r_solved)
    assert ((csr_matrix(err[un]) @ H.T).toarray() & 1 == syn[un]).all()
    wg = WindowGraph(H, pri)
    post = BatchDecoder(wg, osd_method="osd_0", max_iter=1)
    bits, _ = post.osd0(torch.from_numpy(np.array(syn[un], dtype=np.uint8)).cuda(), torch.from_numpy(np.ascontiguousarray(r_marg[un])).cuda())
    assert np.array_equal(err[un], unpack_bits(bits, wg.n).cpu().numpy())
    assert np.array_equal(st[un] & _lib.STATUS_ITER_MASK, r_it[un])


def test_batch_contract(gpu):
    import torch
    from quits_amd.decoder.device import RelayBatchDecoder, WindowGraph, unpack_bits
    H, pri = window("bb72_W3_window0")
    m, n = H.shape
    syn = shots("bb72_W3_window0")
    cfg = RelayConfig(**SMALL)
    wg = WindowGraph(H, pri)
    dec = RelayBatchDecoder(wg, cfg, osd_method="osd_0")
    # B = 0
    bits, st = dec.decode(torch.empty((0, m), dtype=torch.uint8, device="cuda"))
    assert bits.shape == (0, wg.words) and st.shape == (0,)
    # a slice of a wider array with an offset, and a carry on the first rows
    rng = np.random.default_rng(3)
    wide = rng.integers(0, 2, size=(B, m + 11), dtype=np.uint8)
    upd = rng.integers(0, 2, size=(B, 40), dtype=np.uint8)
    eff = syn.copy()
    wide[:, 7:7 + m] = eff
    wide[:, 7:7 + 40] ^= upd
    d_wide, d_upd = torch.from_numpy(wide).cuda(), torch.from_numpy(upd).cuda()
    bits1, st1 = dec.decode(d_wide, det_offset=7, upd=d_upd)
    bits2, st2 = dec.decode(torch.from_numpy(np.array(syn, dtype=np.uint8)).cuda())
    assert torch.equal(bits1, bits2) and torch.equal(st1, st2)
    # twice on one decoder; stages 1 + 2 = stage 3
    bits3, st3 = dec.decode(d_wide, det_offset=7, upd=d_upd)
    assert torch.equal(bits1, bits3) and torch.equal(st1, st3)
    b4, s4 = dec.decode(d_wide, det_offset=7, upd=d_upd, stage=1)
    dec.decode(d_wide, det_offset=7, upd=d_upd, err_bits=b4, status=s4, stage=2)
    assert torch.equal(bits1, b4) and torch.equal(st1, s4)
    ref = mirror("bb72_W3_window0")
    solved = ref[1]
    assert np.array_equal(unpack_bits(bits1, n).cpu().numpy()[solved], ref[0][solved])
    assert np.array_equal(((st1.cpu().numpy() & _lib.STATUS_OSD) != 0), ~solved)


def test_refusals(gpu):
    import ctypes as C
    from quits_amd.decoder.device import RelayBatchDecoder, WindowGraph
    H, pri = window("bb72_W3_window0")
    wg = WindowGraph(H, pri)
    L = wg._L
    rp = _lib.QdRelayParams(20, 0, 15, 1, 0.125, 0)
    for bp, sched in ((0, 0), (1, 1)):
        prm = _lib.QdParams(bp, sched, 0, 0, 0, 0, 1.0)
        h = C.c_void_p()
        assert L.qd_decoder_create_relay(wg._h, C.byref(prm), C.byref(rp), C.c_void_p(0), C.byref(h)) == -1 and not h.value
    prm = _lib.QdParams(1, 0, 0, 0, 0, 0, 1.0)
    big = _lib.QdRelayParams(8000, 1, 8384, 1, 0.125, 0)                      # 16384 iterations
    g0 = np.zeros(wg.n, dtype=np.float32)
    h = C.c_void_p()
    assert L.qd_decoder_create_relay(wg._h, C.byref(prm), C.byref(big), g0.ctypes.data_as(C.c_void_p), C.byref(h)) == -1
    with pytest.raises(ValueError):
        RelayConfig(pre_iter=8000, num_sets=1, set_max_iter=8384)
    (rp_, ci, n), p = tgl._syn("4100x9000_columns_of_3")
    off = WindowGraph(csr_matrix((np.ones(len(ci), np.uint8), ci, rp_), shape=(len(rp_) - 1, n)), p)
    assert off.info()["bp_lds_bytes"] == 0
    with pytest.raises(_lib.QdError) as exc:
        RelayBatchDecoder(off, RelayConfig(**SMALL))
    assert exc.value.code == -4 and "LDS" in str(exc.value)


def _host_sliding_window(det, wins, nz, cfg):
    """The reference's window loop (sliding_window.py:162-186) on the host with relay_mirror as the inner decoder, whole batch at once:
    acc += L_k e, carry = U_k e over the committed columns."""
    acc = np.zeros((det.shape[0], wins[0]["L"].shape[0]), dtype=np.uint8)
    carry = np.zeros((det.shape[0], nz), dtype=np.uint8)
    for k, w in enumerate(wins):
        H = csr_matrix(w["H"])
        s = det[:, k * nz:k * nz + H.shape[0]].astype(np.uint8)
        s[:, :nz] ^= carry
        e = relay_mirror(H, w["priors"], s, cfg)[0]
        nc = w["L"].shape[1]
        acc ^= (csr_matrix(e[:, :nc]) @ csr_matrix(w["L"]).T).toarray().astype(np.uint8) & 1
        if w["U"] is not None:
            carry = (csr_matrix(e[:, :nc]) @ csr_matrix(w["U"]).T).toarray().astype(np.uint8) & 1
    return acc.astype(np.int64)


def test_sliding_window_equals_the_host_loop_over_the_mirror(gpu):
    from quits_amd.decoder import RelayBpDecoder, sliding_window_circuit_mem, sliding_window_relaybp_circuit_mem
    from quits_amd.decoder.device import DemSampler
    from quits_amd.dem import Circuit, dem_to_text
    from quits_amd.samples import PackedSamples
    H, L, pri = helpers.dem_matrices(NAME)
    cd = helpers.code("bb72")
    hz, lz = cd["hz"], cd["lz"]
    cfg = RelayConfig(**SMALL)
    det = DemSampler(H, L, pri).sample(64, seed=11)[0].cpu().numpy().astype(bool)
    circ = Circuit(helpers.circuit_text(NAME))
    ref = _host_sliding_window(det, helpers.window_set(NAME, 3, 1), hz.shape[0], cfg)
    pred = sliding_window_relaybp_circuit_mem(det, circ, hz, lz, 3, 1, relay=cfg)
    assert pred.dtype == np.int64 and ref.any() and np.array_equal(pred, ref)
    assert np.array_equal(sliding_window_relaybp_circuit_mem(PackedSamples.pack(det), circ, hz, lz, 3, 1, relay=cfg), ref)
    assert np.array_equal(sliding_window_relaybp_circuit_mem(det, dem_to_text(circ.detector_error_model()), hz, lz, 3, 1, relay=cfg), ref)
    opts = dict(SMALL)
    assert np.array_equal(sliding_window_circuit_mem(det, circ, hz, lz, 3, 1, RelayBpDecoder, RelayBpDecoder, dict(opts), dict(opts),
                                                     "channel_probs", "channel_probs", "decode", "decode"), ref)
    with pytest.raises(TypeError):
        sliding_window_circuit_mem(det, circ, hz, lz, 3, 1, RelayBpDecoder, RelayBpDecoder, dict(opts, max_iter=5), dict(opts),
                                   "channel_probs", "channel_probs", "decode", "decode")
    # the plug-in class by itself, one syndrome per call
    w0 = helpers.window_set(NAME, 3, 1)[0]
    one = RelayBpDecoder(w0["H"], channel_probs=w0["priors"], **SMALL)
    s = det[:4, :w0["H"].shape[0]].astype(np.uint8)
    m0 = relay_mirror(csr_matrix(w0["H"]), w0["priors"], s, cfg)
    for b in range(4):
        assert np.array_equal(one.decode(s[b]), m0[0][b]) and one.converge == bool(m0[1][b]) and one.iter == m0[2][b]


def test_memory_experiment_equals_sample_decode_compare(gpu):
    from quits_amd.decoder import sliding_window_relaybp_circuit_mem
    from quits_amd.decoder.device import CircuitSampler
    from quits_amd.dem import Circuit
    from quits_amd.simulation import get_circuit_mem_pL, get_relay_mem_pL
    cd = helpers.code("bb72")
    hz, lz = cd["hz"], cd["lz"]
    circ = Circuit(helpers.circuit_text(NAME))
    cfg = RelayConfig(**SMALL)
    res = get_relay_mem_pL(circ, hz, lz, 3, 1, 4096, relay=cfg, seed=5, batch=2048)
    det, obs = CircuitSampler(circ).sample(4096, seed=5)
    pred = sliding_window_relaybp_circuit_mem(det.cpu().numpy().astype(bool), circ, hz, lz, 3, 1, relay=cfg)
    fail = np.flatnonzero((pred != obs.cpu().numpy()).any(axis=1))
    assert res.shots == 4096 and res.errors == len(fail) and len(fail) >= 1 and np.array_equal(res.failing_shots, fail)
    assert res.flagged["post"] == (0, 0)
    # the factored loop still serves the BP-OSD entry point: the same shots through its decoder
    kw = dict(max_iter=20, bp_method="minimum_sum", schedule="parallel", osd_method="osd_0")
    old = get_circuit_mem_pL(circ, hz, lz, 3, 1, 4096, seed=5, batch=2048, **kw)
    from quits_amd.decoder import sliding_window_bposd_circuit_mem
    pred0 = sliding_window_bposd_circuit_mem(det.cpu().numpy().astype(bool), circ, hz, lz, 3, 1, **kw)
    assert (old.shots, old.errors) == (4096, int((pred0 != obs.cpu().numpy()).any(axis=1).sum()))
