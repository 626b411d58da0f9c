"""Relay-BP on the host (quits_amd/relay.py): the configuration, the table of memory strengths and the float32 mirror that every GPU test of
the kernel compares against.  No GPU."""
import dataclasses

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import helpers
from quits_amd.relay import RelayConfig, candidate_weights, prior_llr32, relay_gammas, relay_mirror

NAME = "bb72_custom_r6_p0.003"
SMALL = dict(pre_iter=20, num_sets=4, set_max_iter=15)


@pytest.fixture(scope="module")
def window():
    w = helpers.window_set(NAME, 3, 1)[0]
    H = csr_matrix(w["H"])
    H.sort_indices()
    pri = np.minimum(w["priors"] * 1.5, 0.4)
    e = (np.random.default_rng(1).random((96, H.shape[1])) < pri).astype(np.uint8)
    syn = (csr_matrix(e) @ H.T).toarray().astype(np.uint8) & 1
    return H, pri, syn


def test_config_defaults_and_validation():
    c = RelayConfig()
    assert dataclasses.astuple(c) == (80, 60, 60, 0.125, -0.24, 0.66, 1, 0) and c.total_iter == 3680
    with pytest.raises(dataclasses.FrozenInstanceError):
        c.pre_iter = 3
    for bad in (dict(pre_iter=0), dict(set_max_iter=0), dict(num_sets=-1), dict(num_sets=1024), dict(stop_nconv=0),
                dict(gamma_min=0.5, gamma_max=0.25), dict(gamma0=float("nan")), dict(gamma0=1.5), dict(gamma_min=-1.5),
                dict(gamma_max=float("inf")), dict(pre_iter=16384, num_sets=0), dict(pre_iter=84, num_sets=163, set_max_iter=100)):
        with pytest.raises(ValueError):
            RelayConfig(**bad)
    with pytest.raises(TypeError):
        RelayConfig(pre_iter=2.5)
    assert RelayConfig(pre_iter=83, num_sets=163, set_max_iter=100).total_iter == 16383
    assert RelayConfig(gamma_min=0.3, gamma_max=0.3, gamma0=-1.25).gamma0 == -1.25


def test_gammas_are_pinned_bounded_and_differ_by_row():
    cfg = RelayConfig(num_sets=3)
    g = relay_gammas(1001, cfg)
    assert g.dtype == np.float32 and g.shape == (3, 1001)
    assert np.array_equal(g, relay_gammas(1001, cfg)) and np.array_equal(g[:, :9], relay_gammas(9, cfg))
    # Philox4x32-10, key (0, 0), counter (j >> 2, r, 0, 3), word j & 3, mapped onto [-0.24, 0.66]
    # (0.03239431, 0.51716244, -0.10382277, 0.45715812 and 0.46921375, 0.3054146, 0.31837034, 0.2555362, as float32 bit patterns)
    assert g[0, :4].view(np.uint32).tolist() == [0x3D04AFE6, 0x3F0464C2, 0xBDD4A108, 0x3EEA10A1]
    assert g[1, 4:8].view(np.uint32).tolist() == [0x3EF03CC9, 0x3E9C5F4D, 0x3EA30170, 0x3E82D5A4]
    assert g.min() >= np.float32(-0.24) and g.max() <= np.float32(0.66) and g.min() < -0.2 and g.max() > 0.6
    assert not np.array_equal(g[0], g[1]) and not np.array_equal(g[1], g[2])
    assert not np.array_equal(g, relay_gammas(1001, RelayConfig(num_sets=3, seed=1)))
    narrow = relay_gammas(64, RelayConfig(num_sets=2, gamma_min=0.25, gamma_max=0.25))
    assert np.array_equal(narrow, np.full((2, 64), 0.25, dtype=np.float32))
    assert relay_gammas(5, RelayConfig(num_sets=0)).shape == (0, 5)


def _plain_min_sum(H, pri, syn, max_iter):
    """Flooding min-sum in float32, one message per edge, written without the mirror's machinery."""
    Hd = H.toarray().astype(bool)
    llr0 = np.log((1.0 - pri) / pri).astype(np.float32)
    out, its = np.zeros((len(syn), H.shape[1]), np.uint8), np.zeros(len(syn), np.int32)
    for b, s in enumerate(syn):
        if not s.any():
            continue
        mu = np.zeros(Hd.shape, np.float32)
        for t in range(1, max_iter + 1):
            P = llr0.copy()
            for i in range(Hd.shape[0]):                              # ascending detector order
                P = np.where(Hd[i], P + mu[i], P)
            nu = np.where(Hd, P[None, :] - mu, np.float32(np.inf)).astype(np.float32)
            new = np.zeros_like(mu)
            for i in range(Hd.shape[0]):
                cols = np.flatnonzero(Hd[i])
                for j in cols:
                    others = cols[cols != j]
                    mag = np.abs(nu[i, others]).min() if len(others) else np.finfo(np.float32).max
                    new[i, j] = -mag if (int(s[i]) + int((nu[i, others] <= 0).sum())) & 1 else mag
            mu = new
            M = llr0.copy()
            for i in range(Hd.shape[0]):
                M = np.where(Hd[i], M + mu[i], M)
            out[b], its[b] = (M <= 0), t
            if np.array_equal((Hd[:, M <= 0].sum(axis=1) & 1).astype(np.uint8), s):
                break
    return out, its


def test_without_memory_the_mirror_is_plain_min_sum():
    H, pri = helpers.synthetic_window([12] * 24, 3, 5, 5)
    H = csr_matrix(H)
    e = (np.random.default_rng(2).random((16, H.shape[1])) < pri).astype(np.uint8)      # the mirror: 13 solved, 2 unsolved, 1 zero syndrome
    syn = (csr_matrix(e) @ H.T).toarray().astype(np.uint8) & 1
    ref, its = _plain_min_sum(H, pri, syn, 8)
    err, solved, it, leg, ncand = relay_mirror(H, pri, syn, RelayConfig(pre_iter=8, num_sets=0, gamma0=0.0))
    assert np.array_equal(err, ref) and np.array_equal(it, its) and not leg.any()
    assert (solved & syn.any(axis=1)).sum() >= 3 and (~solved).sum() >= 1
    assert np.array_equal(solved, ((csr_matrix(err) @ H.T).toarray() & 1 == syn).all(axis=1))


def test_more_candidates_are_never_heavier_and_solved_rows_meet_the_syndrome(window):
    H, pri, syn = window
    one = relay_mirror(H, pri, syn, RelayConfig(stop_nconv=1, **SMALL))
    three = relay_mirror(H, pri, syn, RelayConfig(stop_nconv=3, **SMALL))
    first = relay_mirror(H, pri, syn, RelayConfig(stop_nconv=1, **SMALL), marginals=True)
    w = candidate_weights(prior_llr32(pri))
    assert np.array_equal(one[1], three[1])                          # the first candidate is the same one: solved by the same shots ...
    later = three[1] & (three[3] != one[3])
    assert (three[4] > 1).sum() >= 4 and later.sum() >= 1
    assert np.array_equal(three[0][~later], one[0][~later])          # ... and where no later candidate won, it is the answer
    assert ((three[0].astype(np.int64) * w).sum(axis=1) <= (one[0].astype(np.int64) * w).sum(axis=1))[one[1]].all()
    assert ((three[0][later].astype(np.int64) * w).sum(axis=1) < (one[0][later].astype(np.int64) * w).sum(axis=1)).all()
    for res in (one, three):
        err, solved, it, leg, ncand = res
        assert ((csr_matrix(err[solved]) @ H.T).toarray() & 1 == syn[solved]).all()
        assert (solved & (leg == 0)).sum() >= 4 and (solved & (leg > 0)).sum() >= 4 and (~solved).sum() >= 4
        assert (it[~solved] == 80).all() and (leg[~solved] == 4).all() and (ncand[~solved] == 0).all() and (ncand[solved] >= 1).all()
    assert np.array_equal(first[0][~first[1]], (first[5][~first[1]] <= 0).astype(np.uint8))


def test_the_generic_functions_never_loop_on_the_host(monkeypatch):
    from quits_amd.decoder import (RelayBpDecoder, sliding_window_circuit_mem, sliding_window_phenom_mem, sliding_window_relaybp_circuit_mem,
                                   sliding_window_relaybp_phenom_mem)
    from quits_amd.dem import Circuit
    from quits_amd.simulation import get_relay_mem_pL
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)         # (what a machine without a GPU reports)
    cd = helpers.code("bb72")
    hz, lz = cd["hz"], cd["lz"]
    circ = Circuit(helpers.circuit_text(NAME))
    det = np.zeros((3, 8 * hz.shape[0]), dtype=bool)
    opts = dict(SMALL)
    with pytest.raises(RuntimeError, match="no HIP device"):
        sliding_window_circuit_mem(det, circ, hz, lz, 3, 1, RelayBpDecoder, RelayBpDecoder, dict(opts), dict(opts), "channel_probs",
                                   "channel_probs", "decode", "decode")
    with pytest.raises(RuntimeError, match="no HIP device"):
        sliding_window_phenom_mem(det, hz, lz, 3, 1, RelayBpDecoder, RelayBpDecoder, dict(opts, error_rate=0.01), dict(opts, error_rate=0.01),
                                  "decode", "decode")
    with pytest.raises(RuntimeError, match="no HIP device"):
        sliding_window_relaybp_circuit_mem(det, circ, hz, lz, 3, 1, relay=RelayConfig(**SMALL))
    with pytest.raises(RuntimeError, match="no HIP device"):
        sliding_window_relaybp_phenom_mem(det, hz, lz, 3, 1, 0.01, relay=RelayConfig(**SMALL))
    with pytest.raises(RuntimeError, match="no HIP device"):
        get_relay_mem_pL(circ, hz, lz, 3, 1, 64, relay=RelayConfig(**SMALL))
    # unknown or mismatched keywords: refused before anything touches the device
    with pytest.raises(TypeError):
        sliding_window_relaybp_circuit_mem(det, circ, hz, lz, 3, 1, relay=dict(SMALL))
    with pytest.raises(TypeError):
        sliding_window_circuit_mem(det, circ, hz, lz, 3, 1, RelayBpDecoder, RelayBpDecoder, dict(opts, max_iter=4), dict(opts), "channel_probs",
                                   "channel_probs", "decode", "decode")
    with pytest.raises(ValueError):
        sliding_window_circuit_mem(det, circ, hz, lz, 3, 1, RelayBpDecoder, RelayBpDecoder, dict(opts, pre_iter=0), dict(opts), "channel_probs",
                                   "channel_probs", "decode", "decode")


def test_library_exports_the_relay_entry_point():
    from quits_amd import _lib
    L = _lib.load()
    assert L.qd_version() >= 112 and _lib.require_relay(L) is L and "qd_decoder_create_relay" in _lib.EXPORTS
