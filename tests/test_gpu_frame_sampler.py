"""Circuit-level frame sampler on the MI355X (qd_sample_circuit / CircuitSampler): bit for bit against the CPU mirror
(tests/frame_mirror.py), composition of shot ranges, and -- on 2^20 circuit-sampled shots -- the DEM extractor's probabilities
(dem.py), the headline decode and the published anchors, none of which could tell the sampler's and the decoder's priors apart
while both came from the same DEM."""
import os
import sys

import numpy as np
import pytest

import frame_mirror as fm
import helpers
from test_frame_sampler import SPLIT_CIRCUIT, dem_marginals, zero_noise

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import published_anchor as pa  # noqa: E402

SEED = (0x9E3779B9 << 32) | 0x7F4A7C15          # both halves non-zero
FIXTURES = sorted(helpers.circuit_index())
BIG = 1 << 20


def _sampler(text):
    from quits_amd.decoder.device import CircuitSampler
    return CircuitSampler(text)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES + ["split_circuit"])
def test_device_equals_mirror(gpu, name):
    text = SPLIT_CIRCUIT if name == "split_circuit" else helpers.circuit_text(name)
    B = 320 if name.startswith("qlp") else 4133
    shot0 = 1000003
    det, obs = _sampler(text).sample(B, seed=SEED, shot0=shot0)
    rdet, robs = fm.sample(text, SEED, shot0, B)
    assert det.shape == rdet.shape and obs.shape == robs.shape
    d = det.cpu().numpy()
    assert np.array_equal(d, rdet), "%d of %d detector bytes differ" % (int((d != rdet).sum()), d.size)
    assert np.array_equal(obs.cpu().numpy(), robs)
    if name != "split_circuit":
        assert rdet.any()                                   # not a vacuous comparison


@pytest.mark.gpu
def test_split_identity(gpu):
    import torch
    s = _sampler(helpers.circuit_text("bb72_custom_r6_p0.003"))
    B, B1 = 5000, 1733
    det, obs = s.sample(B, seed=SEED)
    d1, o1 = s.sample(B1, seed=SEED)
    d2, o2 = s.sample(B - B1, seed=SEED, shot0=B1)
    assert torch.equal(det, torch.cat([d1, d2])) and torch.equal(obs, torch.cat([o1, o2]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_noise_free_is_zero(gpu, name):
    det, obs = _sampler(zero_noise(helpers.circuit_text(name))).sample(1000, seed=SEED, shot0=5)
    assert not bool(det.any()) and not bool(obs.any())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bb144_custom_r12_p0.003", "hgp225_cardinal_r15_p0.001"])
def test_extractor_marginals_on_circuit_samples(gpu, name):
    """Every detector's and observable's flip rate over 2^20 circuit-sampled shots against the rate the DEM extractor's
    mechanisms predict: within 5 sigma each, and the chi-square over the detectors not rejected at 1e-3."""
    import torch
    from scipy.stats import chi2 as chi2_dist
    text = helpers.circuit_text(name)
    det, obs = _sampler(text).sample(BIG, seed=SEED + 1)
    rd = det.sum(dim=0, dtype=torch.int64).cpu().numpy() / BIG
    ro = obs.sum(dim=0, dtype=torch.int64).cpu().numpy() / BIG
    pd, po = dem_marginals(text)
    report = []
    for kind, rate, pred in (("detector", rd, pd), ("observable", ro, po)):
        z = (rate - pred) / np.sqrt(np.maximum(pred * (1 - pred), 1e-12) / BIG)
        bad = np.flatnonzero(np.abs(z) > 5.0)
        report += ["%s %d: rate %.6f, DEM %.6f, z %.1f" % (kind, i, rate[i], pred[i], z[i]) for i in bad[:20]]
    chi2 = float((((rd - pd) ** 2) / (pd * (1 - pd) / BIG)).sum())
    pval = float(chi2_dist.sf(chi2, len(pd)))
    assert not report and pval > 1e-3, "chi2 %.1f over %d detectors (p = %.2e); %s" % (chi2, len(pd), pval, "; ".join(report))


def _headline_failures(text, det, obs):
    """minimum_sum, parallel, max_iter=50, OSD-0 on the whole history as one window: number of shots whose prediction misses."""
    import torch
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.decoder.device import BatchDecoder, GF2Matrix, WindowGraph
    from quits_amd.dem import Circuit
    H, L, pri = detector_error_model_to_matrix(Circuit(text).detector_error_model())
    dec = BatchDecoder(WindowGraph(H, pri), "minimum_sum", "parallel", 50, "osd_0")
    Lm = GF2Matrix(L)
    fails = 0
    step = 1 << 17
    for b in range(0, det.shape[0], step):
        bits, _ = dec.decode(det[b:b + step])
        pred = torch.empty((bits.shape[0], L.shape[0]), dtype=torch.uint8, device=det.device)
        Lm.xor_apply(bits, pred, False)
        fails += int((pred != obs[b:b + step]).any(dim=1).sum())
    return fails


@pytest.mark.gpu
def test_headline_ler_circuit_vs_dem_samples(gpu):
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.decoder.device import DemSampler
    from quits_amd.dem import Circuit
    text = helpers.circuit_text("bb144_custom_r12_p0.003")
    det, obs = _sampler(text).sample(BIG, seed=SEED + 2)
    fc = _headline_failures(text, det, obs)
    H, L, pri = detector_error_model_to_matrix(Circuit(text).detector_error_model())
    det, obs = DemSampler(H, L, pri).sample(BIG, seed=SEED + 2)
    fd = _headline_failures(text, det, obs)
    pc, pd = fc / BIG, fd / BIG
    sigma = np.sqrt((pc * (1 - pc) + pd * (1 - pd)) / BIG)
    assert fc > 0 and fd > 0
    assert abs(pc - pd) <= 3 * sigma, "circuit-sampled pL %.6f (%d) vs DEM-sampled %.6f (%d), 3 sigma = %.6f" % (pc, fc, pd, fd, 3 * sigma)


@pytest.mark.gpu
@pytest.mark.parametrize("case", pa.CASES, ids=[c[0] for c in pa.CASES])
def test_published_anchor_on_circuit_samples(gpu, case):
    cid, cell, _, _, _, p, _, _, kind, kw, k_pub, n_pub = case
    det, obs = _sampler(pa.circuit_for(case)).sample(1 << 15, seed=3)
    pred = pa.device_decode(case, det)
    pl = float((pred != obs.cpu().numpy()).any(axis=1).mean())
    lo, hi = pa.clopper_pearson(k_pub, n_pub)
    assert lo <= pl <= hi, "%s (%s): pL %.5f on circuit samples outside [%.5f, %.5f] of the published %d / %d" % (
        cid, cell, pl, lo, hi, k_pub, n_pub)


@pytest.mark.gpu
def test_get_circuit_mem_result_matches_dem_path_types(gpu):
    from quits_amd.dem import Circuit
    from quits_amd.simulation import get_circuit_mem_result, get_stim_mem_result
    circ = Circuit(helpers.circuit_text("bb72_custom_r6_p0.003"))
    d1, o1 = get_circuit_mem_result(circ, 777, seed=9)
    d2, o2 = get_stim_mem_result(circ, 777, seed=9)
    assert (d1.dtype, d1.shape, o1.dtype, o1.shape) == (d2.dtype, d2.shape, o2.dtype, o2.shape)
    d3, o3 = get_circuit_mem_result(str(circ), 777, seed=9)
    assert np.array_equal(d1, d3) and np.array_equal(o1, o3)


@pytest.mark.gpu
def test_info_and_argument_checks(gpu):
    import torch
    from quits_amd import _lib
    s = _sampler(helpers.circuit_text("bb144_custom_r12_p0.003"))
    info = s.info()
    assert info["qubits"] == 288 and info["sites"] == 28368 and info["lds_bytes"] == s.compiled.lds_bytes
    L = _lib.load()
    det = torch.empty((64, s.m - 1), dtype=torch.uint8, device="cuda")
    obs = torch.empty((64, s.nobs), dtype=torch.uint8, device="cuda")
    assert L.qd_sample_circuit(s._h, 1, 0, 64, det.data_ptr(), det.stride(0), obs.data_ptr(), obs.stride(0), None) == -1
    assert b"stride" in L.qd_last_error()
    bad = s.compiled.program.copy()
    bad[2] = 10 ** 6                                              # a qubit far out of range: refused before anything reaches the GPU
    import ctypes as C
    h = C.c_void_p()
    thr = s.compiled.thresholds
    rc = L.qd_circuit_create(bad.ctypes.data_as(C.c_void_p), len(bad), s.compiled.nq, s.compiled.nmeas, s.compiled.ndet, s.compiled.nobs,
                             thr.ctypes.data_as(C.c_void_p), len(thr), s.compiled.ring, 0, C.byref(h))
    assert rc == -1 and b"out of range" in L.qd_last_error()
