"""Biased noise on the MI355X: Y_ERROR, PAULI_CHANNEL_1 and PAULI_CHANNEL_2 in qd_sample_circuit / CircuitSampler, bit for bit
against the CPU mirror (tests/frame_mirror_channels.py), the component map without the mirror, composition of shot ranges, the
DEM extractor's approximate-disjoint conversion against circuit samples, and one decode from circuit text to predictions."""
import numpy as np
import pytest

import channel_circuits as cc_
import frame_mirror_channels as fmc
import helpers
from test_frame_sampler import dem_marginals

SEED = (0x9E3779B9 << 32) | 0x7F4A7C15          # both halves non-zero
BB72 = "bb72_custom_r6_p0.003"


def _sampler(text):
    from quits_amd.decoder.device import CircuitSampler
    return CircuitSampler(text)


@pytest.fixture(scope="module")
def biased_text():
    return cc_.biased(helpers.circuit_text(BB72))


@pytest.fixture(scope="module")
def biased_samples(gpu, biased_text):
    """2^17 shots of the biased bb72 circuit, drawn once for the tests that need many."""
    det, obs = _sampler(biased_text).sample(1 << 17, seed=SEED + 1)
    return det, obs


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["synthetic", "bb72_biased"])
def test_device_equals_mirror(gpu, biased_text, case):
    if case == "synthetic":
        text, B, shot0 = cc_.SYNTHETIC, 197, 2 ** 32 - 100       # the high shot word changes inside the batch
    else:
        text, B, shot0 = biased_text, 1000, 1000003
    s = _sampler(text)
    det, obs = s.sample(B, seed=SEED, shot0=shot0)
    rdet, robs = fmc.sample(text, SEED, shot0, B)
    assert rdet.any() and robs.any()                             # not a vacuous comparison
    if case == "bb72_biased":
        assert s.m == 288
    assert det.shape == rdet.shape and obs.shape == robs.shape
    d = det.cpu().numpy()
    assert np.array_equal(d, rdet), "%d of %d detector bytes differ" % (int((d != rdet).sum()), d.size)
    assert np.array_equal(obs.cpu().numpy(), robs)


def _xbits(pauli):
    return int(pauli in (1, 2))


def _zbits(pauli):
    return int(pauli >= 2)


def _both_bases(noise_line, nq):
    """The noise between a reset and a measurement of qubits 0 .. nq - 1 in the Z basis (detectors show the X bits) and in the X basis
    (the Z bits); returns uint8 [256, nq] each."""
    qs = " ".join(str(q) for q in range(nq))
    dets = "".join("DETECTOR rec[-%d]\n" % (nq - q) for q in range(nq))
    out = []
    for r, m in (("R", "M"), ("RX", "MX")):
        det, _ = _sampler("%s %s\n%s\n%s %s\n%s" % (r, qs, noise_line, m, qs, dets)).sample(256, seed=SEED + 3)
        out.append(det.cpu().numpy())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(1, 16))
def test_component_map_two_qubit(gpu, k):
    args = ["0"] * 15
    args[k - 1] = "1.0"
    x, z = _both_bases("PAULI_CHANNEL_2(%s) 0 1" % ", ".join(args), 2)
    a, b = k >> 2, k & 3
    assert np.array_equal(x, np.tile(np.uint8([_xbits(a), _xbits(b)]), (256, 1))), (k, x[:4])
    assert np.array_equal(z, np.tile(np.uint8([_zbits(a), _zbits(b)]), (256, 1))), (k, z[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("line,pauli", [("PAULI_CHANNEL_1(1.0, 0, 0) 0", 1), ("PAULI_CHANNEL_1(0, 1.0, 0) 0", 2),
                                        ("PAULI_CHANNEL_1(0, 0, 1.0) 0", 3), ("Y_ERROR(1.0) 0", 2)])
def test_component_map_one_qubit(gpu, line, pauli):
    # p = 1.0 clamps to the threshold 2^32 - 1: the one draw r = 2^32 - 1 in 2^32 would not fire (1 in 1.7e7 for the 256 shots here)
    x, z = _both_bases(line, 1)
    assert np.array_equal(x, np.full((256, 1), _xbits(pauli), np.uint8))
    assert np.array_equal(z, np.full((256, 1), _zbits(pauli), np.uint8))


@pytest.mark.gpu
def test_split_identity(gpu, biased_text):
    import torch
    s = _sampler(biased_text)
    B, B1 = 5000, 1733
    det, obs = s.sample(B, seed=SEED)
    d1, o1 = s.sample(B1, seed=SEED)
    d2, o2 = s.sample(B - B1, seed=SEED, shot0=B1)
    assert bool(det.any())
    assert torch.equal(det, torch.cat([d1, d2])) and torch.equal(obs, torch.cat([o1, o2]))


@pytest.mark.gpu
def test_extractor_marginals_on_biased_circuit_samples(gpu, biased_text, biased_samples):
    """Every detector's and observable's flip rate over 2^17 circuit-sampled shots against the rate the approximate-disjoint DEM
    predicts: within 5 sigma each.  The approximation's bias is of relative order p = 3e-3, a quarter of a sigma (1 % relative) here;
    tests/test_frame_channels.py runs the same check on the mirror alone."""
    import torch
    from quits_amd.dem import Circuit
    det, obs = biased_samples
    B = det.shape[0]
    rd = det.sum(dim=0, dtype=torch.int64).cpu().numpy() / B
    ro = obs.sum(dim=0, dtype=torch.int64).cpu().numpy() / B
    pd, po = dem_marginals(Circuit(biased_text, approximate_disjoint_errors=True))
    report = []
    for kind, rate, pred in (("detector", rd, pd), ("observable", ro, po)):
        z = (rate - pred) / np.sqrt(np.maximum(pred * (1 - pred), 1e-12) / B)
        print("%s: largest |z| %.2f" % (kind, np.abs(z).max()))
        bad = np.flatnonzero(np.abs(z) > 5.0)
        report += ["%s %d: rate %.6f, DEM %.6f, z %.1f" % (kind, i, rate[i], pred[i], z[i]) for i in bad[:20]]
    assert not report, "; ".join(report)


@pytest.mark.gpu
def test_end_to_end_decode(gpu, biased_text, biased_samples):
    """Circuit text -> samples -> predictions, with circuit-level priors (on request) and with phenomenological ones."""
    from quits_amd.decoder import sliding_window_bposd_circuit_mem, sliding_window_bposd_phenom_mem
    from quits_amd.decoder.sliding_window import plan_cache_clear
    from quits_amd.dem import Circuit
    cd = helpers.code("bb72")
    N = 1 << 14
    det = biased_samples[0][:N].cpu().numpy()
    obs = biased_samples[1][:N].cpu().numpy()
    kw = dict(max_iter=20, osd_order=0, bp_method="minimum_sum", schedule="parallel", osd_method="osd_0")
    plan_cache_clear()
    pred = sliding_window_bposd_circuit_mem(det, Circuit(biased_text, approximate_disjoint_errors=True), cd["hz"], cd["lz"], 3, 1, **kw)
    phen = sliding_window_bposd_phenom_mem(det, cd["hz"], cd["lz"], 3, 1, eff_error_rate_per_fault=0.003, **kw)
    k = cd["lz"].shape[0]
    assert pred.dtype == np.int64 and pred.shape == (N, k) and phen.dtype == np.int64 and phen.shape == (N, k)
    fails = int((pred != obs).any(axis=1).sum())
    trivial = int(obs.any(axis=1).sum())
    print("circuit-level decode fails on %d of %d shots, phenomenological on %d, predicting no flip on %d"
          % (fails, N, int((phen != obs).any(axis=1).sum()), trivial))
    assert trivial > 0 and fails < trivial
    # the flagged call has populated the plan cache; the plain text must still be refused, not served that plan
    with pytest.raises(NotImplementedError):
        sliding_window_bposd_circuit_mem(det[:64], biased_text, cd["hz"], cd["lz"], 3, 1, **kw)
    with pytest.raises(NotImplementedError):
        sliding_window_bposd_circuit_mem(det[:64], Circuit(biased_text), cd["hz"], cd["lz"], 3, 1, **kw)


@pytest.mark.gpu
def test_public_surface_accepts_channels(gpu, biased_text):
    from quits_amd.dem import Circuit
    from quits_amd.simulation import get_circuit_mem_result
    d1, o1 = get_circuit_mem_result(biased_text, 777, seed=9)
    d2, o2 = get_circuit_mem_result(Circuit(biased_text), 777, seed=9)          # sampling needs no flag
    assert d1.dtype == np.bool_ and d1.shape == (777, 288) and o1.shape == (777, 12) and d1.any()
    assert np.array_equal(d1, d2) and np.array_equal(o1, o2)
    info = _sampler(biased_text).info()
    assert info["sites"] == 7704 and info["detectors"] == 288
