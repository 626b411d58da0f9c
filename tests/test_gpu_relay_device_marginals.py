"""Relay-BP with the marginals M_j in a device-memory workspace (csrc/bp_relay_device.hip: the MD = true form of qd_bp_relay_kernel) against the
definition, quits_amd.relay.relay_mirror, and against the LDS form -- error bits, iteration counts, CONVERGED and the leg bits, bit for bit.
The form is what lets QLP [[1020,136]] W = 3 / F = 1 (1350 x 18 900, rows of up to 78 faults: 190 KB of LDS with the marginals, 115 KB without)
decode at all; on the windows of tests/test_gpu_relay.py it is forced (marginals="device") and must change nothing.  Windows, shots and cached
mirrors are that file's where they exist."""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import helpers
import test_graph_layout as tgl
import test_gpu_relay as tgr
from quits_amd import _lib
from quits_amd.relay import RelayConfig, relay_mirror

pytestmark = pytest.mark.gpu

QLP = "qlp1020_cardinal_r20_p0.003"
SMALL = tgr.SMALL
LDS_LIMIT = 160 * 1024


@functools.lru_cache(maxsize=None)
def qlp_window(k):
    """Window k of QLP W = 3 / F = 1 with the priors scaled by 0.33 (capped at 0.4): at the fixture's p = 0.003 no shot of 16 is solved."""
    w = helpers.window_set(QLP, 3, 1)[k]
    H = csr_matrix(w["H"])
    H.sort_indices()
    pri = np.minimum(np.asarray(w["priors"], dtype=np.float64) * 0.33, 0.4)
    pri.setflags(write=False)
    return H, pri


@functools.lru_cache(maxsize=None)
def qlp_shots(k):
    H, pri = qlp_window(k)
    e = (np.random.default_rng(1).random((16, H.shape[1])) < pri).astype(np.uint8)
    s = (csr_matrix(e) @ H.T).toarray().astype(np.uint8) & 1
    s.setflags(write=False)
    return s


def decode(H, pri, syn, cfg, marginals, alpha=1.0, osd_method="osd_off", stage=3):
    import torch
    from quits_amd.decoder.device import RelayBatchDecoder, WindowGraph, unpack_bits
    wg = WindowGraph(H, pri)
    dec = RelayBatchDecoder(wg, cfg, osd_method=osd_method, ms_scaling_factor=alpha, marginals=marginals)
    bits, st = dec.decode(torch.from_numpy(np.array(syn, dtype=np.uint8)).cuda(), stage=stage)
    torch.cuda.synchronize()
    return unpack_bits(bits, wg.n).cpu().numpy(), st.cpu().numpy(), dec


def test_qlp_window_takes_the_device_form(gpu):
    """Fails on the parent: QdError -4, the relay state (about 190 KB) does not fit the CU's LDS."""
    from quits_amd.decoder.device import RelayBatchDecoder, WindowGraph
    H, pri = qlp_window(0)
    assert H.shape == (1350, 18300) and H.nnz == 79200
    wg = WindowGraph(H, pri)
    gi = wg.info()
    assert gi["max_row_weight"] == 78 and gi["max_col_weight"] == 9
    info = RelayBatchDecoder(wg, RelayConfig(**SMALL)).info()
    print("QLP window 0: relay_marginals %s, relay_lds_bytes %d (min-sum layout %d)" % (info["relay_marginals"], info["relay_lds_bytes"], gi["bp_lds_bytes"]))
    assert info["relay_marginals"] == "device" and gi["bp_lds_bytes"] < info["relay_lds_bytes"] <= LDS_LIMIT
    assert info["bp_kernel"] == "qd_bp_relay_kernel" and info["llr_grid_bits"] == -1


@pytest.mark.parametrize("k", [0, 1])
def test_bit_exact_on_qlp(gpu, k):
    H, pri = qlp_window(k)
    assert H.shape == (1350, (18300, 18900)[k])
    syn = qlp_shots(k)
    ref = relay_mirror(H, pri, syn, RelayConfig(**SMALL))
    _, solved, _, leg, _ = ref[:5]
    assert (solved & (leg == 0) & syn.any(axis=1)).sum() >= 1 and (solved & (leg > 0)).sum() >= 1 and (~solved).sum() >= 1
    err, st, dec = decode(H, pri, syn, RelayConfig(**SMALL), "auto")
    assert dec.info()["relay_marginals"] == "device"
    tgr.assert_same(err, st, ref, "QLP window %d" % k)


@pytest.mark.parametrize("name", list(tgr.WINDOWS))
def test_forced_form_on_the_six_windows(gpu, name):
    """Sign modes 0, 1, 2, record chunks 2 and 5, 256 and 512 threads: the forced device form = the mirror = the LDS form."""
    H, pri = tgr.window(name)
    syn = tgr.shots(name)
    ref = tgr.mirror(name)
    tgr.assert_all_outcomes(ref, syn)
    err, st, dec = decode(H, pri, syn, RelayConfig(**SMALL), "device")
    err0, st0, dec0 = decode(H, pri, syn, RelayConfig(**SMALL), "lds")
    i1, i0 = dec.info(), dec0.info()
    assert (i1["relay_marginals"], i0["relay_marginals"]) == ("device", "lds") and i1["relay_lds_bytes"] < i0["relay_lds_bytes"] <= LDS_LIMIT
    assert np.array_equal(st, st0) and np.array_equal(err, err0)
    assert np.array_equal((st & _lib.STATUS_ZERO) != 0, ~syn.any(axis=1))
    tgr.assert_same(err, st, ref, name)


@pytest.mark.parametrize("stop_nconv,alpha", [(3, 1.0), (1, 0.0)])
def test_forced_form_more_candidates_and_running_scale(gpu, stop_nconv, alpha):
    H, pri = tgr.window("bb72_whole")
    syn = tgr.shots("bb72_whole")
    ref = tgr.mirror("bb72_whole", stop_nconv, alpha)
    if stop_nconv > 1:
        assert (ref[4] > 1).sum() >= 4 and (ref[3][ref[1]] > 0).sum() >= 4          # several candidates; a later one was the lighter
    cfg = RelayConfig(stop_nconv=stop_nconv, **SMALL)
    err, st, _ = decode(H, pri, syn, cfg, "device", alpha=alpha)
    err0, st0, _ = decode(H, pri, syn, cfg, "lds", alpha=alpha)
    assert np.array_equal(st, st0) and np.array_equal(err, err0)
    tgr.assert_same(err, st, ref, "stop_nconv %d alpha %g" % (stop_nconv, alpha))


def test_unsolved_shots_reach_the_post_processor(gpu):
    import torch
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    name = "bb72_W3_window0"
    H, pri = tgr.window(name)
    syn = tgr.shots(name)
    r_err, r_solved, r_it, r_leg, _, r_marg = tgr.mirror(name)
    un = np.flatnonzero(~r_solved)
    assert len(un) >= 4
    err, st, _ = decode(H, pri, syn, RelayConfig(**SMALL), "device", osd_method="osd_0")
    err0, st0, _ = decode(H, pri, syn, RelayConfig(**SMALL), "lds", osd_method="osd_0")
    assert np.array_equal(st, st0) and np.array_equal(err, err0)
    assert np.array_equal((st & _lib.STATUS_OSD) != 0, ~r_solved)
    assert ((csr_matrix(err[un]) @ H.T).toarray() & 1 == syn[un]).all()
    # the marginals the kernel parked (rows of the posterior workspace, read back after the BP stage) are the mirror's, float for float ...
    _, st1, dec1 = decode(H, pri, syn, RelayConfig(**SMALL), "device", osd_method="osd_0", stage=1)
    assert np.array_equal((st1 & _lib.STATUS_CONVERGED) != 0, r_solved)
    for b in un:
        parked = dec1.failed_llr(int(b)).cpu().numpy()
        assert np.array_equal(parked.view(np.uint32), np.ascontiguousarray(r_marg[b], dtype=np.float32).view(np.uint32)), b
    # ... and the post-processor's answer on the mirror's marginals is the decoder's (where tests/test_gpu_relay.py inspects them)
    wg = WindowGraph(H, pri)
    post = BatchDecoder(wg, osd_method="osd_0", max_iter=1)
    bits, _ = post.osd0(torch.from_numpy(np.array(syn[un], dtype=np.uint8)).cuda(), torch.from_numpy(np.ascontiguousarray(r_marg[un])).cuda())
    assert np.array_equal(err[un], unpack_bits(bits, wg.n).cpu().numpy())
    assert np.array_equal(st[un] & _lib.STATUS_ITER_MASK, r_it[un])


def test_batch_contract(gpu):
    """One device-form decoder, calls of 5, 96, 7 and 96 (rows reversed) shots: the workspace grows once, rows are reused by other shots --
    zero-syndrome shots, which never touch their row, land where shots that ran BP were and the other way round -- and every call equals
    the mirror for its rows."""
    import torch
    from quits_amd.decoder.device import RelayBatchDecoder, WindowGraph, unpack_bits
    name = "70x300_rows_to_40"
    H, pri = tgr.window(name)
    syn = np.array(tgr.shots(name))
    ref = tgr.mirror(name)
    zero = ~syn.any(axis=1)
    assert 1 <= zero.sum() < len(syn) and zero[::-1].tolist() != zero.tolist()
    wg = WindowGraph(H, pri)
    dec = RelayBatchDecoder(wg, RelayConfig(**SMALL), marginals="device")
    assert dec.info()["relay_marginals"] == "device"
    for rows in (np.arange(5), np.arange(tgr.B), np.arange(7), np.arange(tgr.B)[::-1]):
        bits, st = dec.decode(torch.from_numpy(np.ascontiguousarray(syn[rows])).cuda())
        torch.cuda.synchronize()
        st = st.cpu().numpy()
        assert np.array_equal((st & _lib.STATUS_ZERO) != 0, zero[rows])
        tgr.assert_same(unpack_bits(bits, wg.n).cpu().numpy(), st, tuple(np.asarray(r)[rows] for r in ref[:5]), "%d rows from %d" % (len(rows), rows[0]))
    # released and reserved again: the next call sizes the workspace anew
    dec.release_workspace()
    bits, st = dec.decode(torch.from_numpy(np.ascontiguousarray(syn[:7])).cuda())
    tgr.assert_same(unpack_bits(bits, wg.n).cpu().numpy(), st.cpu().numpy(), tuple(np.asarray(r)[:7] for r in ref[:5]), "after release")


def test_refusals(gpu):
    from quits_amd.decoder.device import RelayBatchDecoder, WindowGraph
    H, pri = qlp_window(0)
    wg = WindowGraph(H, pri)
    info = RelayBatchDecoder(wg, RelayConfig(**SMALL)).info()
    n_pad = (wg.n + 63) // 64 * 64
    lds_form = info["relay_lds_bytes"] + (((n_pad + 1) * 4 + 15) & ~15)          # the same layout with the marginals in front of the candidate
    assert lds_form > LDS_LIMIT
    with pytest.raises(_lib.QdError) as exc:
        RelayBatchDecoder(wg, RelayConfig(**SMALL), marginals="lds")
    print(exc.value)
    assert exc.value.code == -4 and str(lds_form) in str(exc.value) and str(info["relay_lds_bytes"]) in str(exc.value)
    with pytest.raises(ValueError):
        RelayBatchDecoder(wg, RelayConfig(**SMALL), marginals="registers")
    # flag bits of qd_relay_params.reserved: the one that exists is taken, every other is QD_EINVAL
    small = WindowGraph(*tgr.window("bb72_W3_window0"))
    L = small._L
    prm = _lib.QdParams(1, 0, 0, 0, 0, 0, 1.0)
    for flags, rc in ((_lib.RELAY_FLAG_MARGINALS_DEVICE, 0), (2, -1), (_lib.RELAY_FLAG_MARGINALS_DEVICE | 2, -1), (1 << 30, -1), (-2147483648, -1)):
        rp = _lib.QdRelayParams(20, 0, 15, 1, 0.125, flags)
        h = C.c_void_p()
        assert L.qd_decoder_create_relay(small._h, C.byref(prm), C.byref(rp), C.c_void_p(0), C.byref(h)) == rc, flags
        assert bool(h.value) == (rc == 0)
        if h.value:
            arr = (C.c_int32 * 4)()
            assert L.qd_decoder_relay_info(h, arr) == 0 and arr[0] == 2 and 0 < arr[1] < arr[2] <= arr[3] == LDS_LIMIT
            L.qd_decoder_destroy(h)
    # an off-chip window: even the gather layout does not fit, whatever the form
    (rp_, ci, n), p = tgl._syn("4100x9000_columns_of_3")
    off = WindowGraph(csr_matrix((np.ones(len(ci), np.uint8), ci, rp_), shape=(len(rp_) - 1, n)), p)
    assert off.info()["bp_lds_bytes"] == 0
    for mode in ("auto", "lds", "device"):
        with pytest.raises(_lib.QdError) as exc:
            RelayBatchDecoder(off, RelayConfig(**SMALL), marginals=mode)
        assert exc.value.code == -4 and "LDS" in str(exc.value)


def test_sliding_window_on_qlp_equals_the_host_loop_over_the_mirror(gpu):
    """QLP W = 3 / F = 1 through the entry point (priors as the circuit has them: the entry point takes none): 20 windows, the
    full-size ones in the device-marginal form by the automatic choice, a plan whose workspace estimate counts their rows."""
    from quits_amd.decoder import sliding_window_relaybp_circuit_mem
    from quits_amd.decoder.plan import build_circuit_plan, workspace_bytes_per_shot
    from quits_amd.decoder.relaybp import RelayBpDecoder, relay_options
    from quits_amd.dem import Circuit
    H, _, pri = helpers.dem_matrices(QLP)
    cd = helpers.code("qlp1020")
    hz, lz = cd["hz"], cd["lz"]
    cfg = RelayConfig(pre_iter=12, num_sets=2, set_max_iter=8)
    e = (np.random.default_rng(7).random((4, H.shape[1])) < pri).astype(np.uint8)
    det = ((csr_matrix(e) @ csr_matrix(H).T).toarray() & 1).astype(bool)
    circ = Circuit(helpers.circuit_text(QLP))
    wins = helpers.window_set(QLP, 3, 1)
    ref = tgr._host_sliding_window(det, wins, hz.shape[0], cfg)
    pred = sliding_window_relaybp_circuit_mem(det, circ, hz, lz, 3, 1, relay=cfg)
    assert pred.dtype == np.int64 and ref.any() and np.array_equal(pred, ref)
    opts = relay_options(cfg)
    plan = build_circuit_plan(circ, hz, 3, 1, 20, dict(opts), dict(opts), RelayBpDecoder, RelayBpDecoder)
    decs = plan.decoders()
    forms = [d.info()["relay_marginals"] for d in decs]
    print("QLP W = 3 / F = 1 plan: %d windows, %d decoders, forms %s" % (len(plan.windows), len(decs), forms))
    # the windows of 1350 x 18 300 / 18 900 cannot keep their marginals in LDS; a smaller closing window may
    assert len(plan.windows) == 20 and all(f == "device" for d, f in zip(decs, forms) if d.graph.n >= 18300) and forms.count("device") >= 2
    assert workspace_bytes_per_shot(decs) == sum((8 if f == "device" else 4) * ((d.graph.n + 63) // 64 * 64) + 64 for d, f in zip(decs, forms))
