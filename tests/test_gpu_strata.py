"""The stratified DEM sampler on the device (qd_sample_dem_strata) against its numpy specification (quits_amd.strata.sample_mirror), bit for
bit, and the stratified experiment (get_stratified_pL) against the mirror's shots and against the direct experiment (get_fault_spectrum).
Run on the GPU box with `pytest -m gpu -s` to see the figures of the last test (profiles/stratified_sampler_gputests.txt holds a run's)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import helpers
from quits_amd import strata

pytestmark = pytest.mark.gpu

BB72 = "bb72_custom_r6_p0.003"
MINSUM = dict(bp_method="minimum_sum", schedule="parallel", max_iter=20, osd_method="osd_0", osd_order=0)


def _unpack(words, n):
    """int32 [B, words] -> bool [B, n]."""
    w = np.ascontiguousarray(words)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :n].astype(bool)


def _pack(bits, words):
    """bool [B, n] -> int32 [B, words], padding bits zero."""
    pad = np.zeros((bits.shape[0], 32 * words), np.uint8)
    pad[:, :bits.shape[1]] = bits
    return np.packbits(pad, axis=1, bitorder="little").view("<i4").reshape(bits.shape[0], words)


def _toy(n, seed):
    """A seeded model of n faults on 7 detectors and 2 observables; priors from 0.01 to 0.3 and one fault that never fires."""
    from scipy.sparse import csc_matrix
    rng = np.random.default_rng(seed)
    H = (rng.random((7, n)) < 0.4).astype(np.uint8)
    L = (rng.random((2, n)) < 0.3).astype(np.uint8)
    pri = 10.0 ** rng.uniform(-2.0, math.log10(0.3), size=n)
    pri[n // 2] = 0.0
    return csc_matrix(H), csc_matrix(L), pri


@functools.lru_cache(maxsize=None)
def _bb72():
    H, L, pri = helpers.dem_matrices(BB72)
    return H, L, np.asarray(pri, np.float64)


def _equal_to_mirror(got, H, L, pri, ks, seed, shots):
    det, obs, fb = (t.cpu().numpy() for t in got)
    n = H.shape[1]
    mdet, mobs, E = strata.sample_mirror(H, L, pri, ks, seed, shots)
    assert fb.shape == (E.shape[0], (n + 31) // 32)
    assert np.array_equal(fb, _pack(E, fb.shape[1])), "fault words differ from the mirror (rows %s)" % np.flatnonzero((_unpack(fb, n) != E).any(axis=1))[:8]
    assert np.array_equal(det, mdet) and np.array_equal(obs, mobs)
    return E


@pytest.mark.parametrize("n", [10, 31, 33, 64, 65, 66])
def test_device_equals_mirror_on_small_models(gpu, n):
    """Word boundaries, whole and partial Philox groups, n not a multiple of 4; 70 rows = one full wavefront and a partial one; every count
    from 0 to the number of faults that can fire, k = n - 1 among them (one prior is 0), rows repeated and out of order."""
    from quits_amd.decoder.device import StratifiedDemSampler
    H, L, pri = _toy(n, 100 + n)
    kmax = n - 1
    smp = StratifiedDemSampler(H, L, pri, kmax)
    assert smp.info() == {"faults": n, "kmax": kmax, "table_bytes": 4 * n * (kmax + 1), "device": smp.Ht.device}
    assert abs(smp.pmf.sum() + smp.tail - 1.0) < 1e-12
    ks = np.arange(70) % (kmax + 1)
    E = _equal_to_mirror(smp.sample_faults(ks, 77), H, L, pri, ks, 77, 70)
    assert np.array_equal(E.sum(axis=1), ks) and not E[:, n // 2].any()
    shots = np.array([5, 3, 5, 2 ** 40 + 1, 0, 3, 69, 5])
    _equal_to_mirror(smp.sample_shots_faults(shots, ks[shots % 70], 77), H, L, pri, ks[shots % 70], 77, shots)
    _equal_to_mirror(smp.sample_faults(3, 78, shot0=9, shots=5), H, L, pri, 3, 78, np.arange(9, 14))
    assert smp.sample_faults(np.zeros(0, np.int64), 1)[2].shape == (0, (n + 31) // 32)
    with pytest.raises(ValueError):
        smp.sample_faults([n], 1)                      # more than can fire
    with pytest.raises(ValueError):
        smp.sample_faults([-1], 1)


def test_every_fault_of_a_toy_model(gpu):
    """k = n: the whole row is forced, whatever the thresholds say."""
    from scipy.sparse import csc_matrix
    from quits_amd.decoder.device import StratifiedDemSampler
    rng = np.random.default_rng(4)
    H, L = csc_matrix((rng.random((5, 10)) < 0.5).astype(np.uint8)), csc_matrix((rng.random((1, 10)) < 0.5).astype(np.uint8))
    pri = rng.uniform(0.01, 0.4, size=10)
    smp = StratifiedDemSampler(H, L, pri, 10)
    ks = np.array([10, 0, 10, 9, 1, 10])
    E = _equal_to_mirror(smp.sample_faults(ks, 3), H, L, pri, ks, 3, 6)
    assert E[ks == 10].all() and np.array_equal(E.sum(axis=1), ks)


@pytest.mark.parametrize("B", [100, 256])
def test_device_equals_mirror_on_bb72_with_mixed_strata(gpu, B):
    """288 x 2592, strata 0, 1, 2, 7, 40 and kmax = 255 side by side in every wavefront; then shots beyond 2^33 and a list with repeats."""
    from quits_amd.decoder.device import StratifiedDemSampler
    H, L, pri = _bb72()
    smp = StratifiedDemSampler(H, L, pri, 255)
    ks = np.array([0, 1, 2, 7, 40, 255])[np.random.default_rng(B).integers(0, 6, size=B)]
    ks[:6] = [255, 0, 40, 1, 7, 2]
    E = _equal_to_mirror(smp.sample_faults(ks, 2026), H, L, pri, ks, 2026, B)
    assert np.array_equal(E.sum(axis=1), ks)
    if B == 100:
        s0 = 2 ** 33 + 5
        far = _equal_to_mirror(smp.sample_faults(ks, 2026, shot0=s0), H, L, pri, ks, 2026, s0 + np.arange(B))
        assert not np.array_equal(far, E)
        shots = np.array([3, 3, 99, 0, 2 ** 33 + 7, 3, 50, 0])
        kk = np.array([7, 7, 2, 40, 40, 1, 255, 40])
        again = _equal_to_mirror(smp.sample_shots_faults(shots, kk, 2026), H, L, pri, kk, 2026, shots)
        assert np.array_equal(again[0], again[1]) and np.array_equal(again[3], again[7]) and not np.array_equal(again[0], again[5])
        assert np.array_equal(again[4], far[2])                      # shot 2^33 + 7 with 40 faults, drawn in a range and from a list


def test_outputs_into_column_slices_and_refused_arguments(gpu):
    """Rows that are column slices of wider arrays: the bytes and words outside the slice keep their values.  Then the refusals that need
    real handles: strides too small, a table for another model."""
    import torch
    from quits_amd import _lib
    from quits_amd.decoder.device import StratifiedDemSampler
    H, L, pri = _toy(66, 9)
    smp = StratifiedDemSampler(H, L, pri, 20)
    Lb = smp._L
    B, m, nobs, words = 70, 7, 2, 3
    ks = np.arange(B) % 21
    k = torch.from_numpy(ks.astype(np.int32)).cuda()
    det = torch.full((B, m + 13), 0xAB, dtype=torch.uint8, device="cuda")
    obs = torch.full((B, nobs + 5), 0xCD, dtype=torch.uint8, device="cuda")
    fb = torch.full((B, words + 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dv, ov, fv = det[:, 5:5 + m], obs[:, 2:2 + nobs], fb[:, 1:1 + words]
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(strata_h, det_stride, obs_stride, fault_stride):
        return Lb.qd_sample_dem_strata(strata_h, smp.Ht._h, smp.Lt._h, C.c_uint64(31), 4, None, C.c_void_p(k.data_ptr()), B, C.c_void_p(dv.data_ptr()),
                                       det_stride, C.c_void_p(ov.data_ptr()), obs_stride, C.c_void_p(fv.data_ptr()), fault_stride, sp)
    assert call(smp._h, det.stride(0), obs.stride(0), fb.stride(0)) == 0
    torch.cuda.synchronize()
    _equal_to_mirror((dv, ov, fv.contiguous()), H, L, pri, ks, 31, 4 + np.arange(B))
    keep = torch.ones_like(det, dtype=torch.bool)
    keep[:, 5:5 + m] = False
    assert bool((det[keep] == 0xAB).all())
    keep = torch.ones_like(obs, dtype=torch.bool)
    keep[:, 2:2 + nobs] = False
    assert bool((obs[keep] == 0xCD).all())
    assert bool((fb[:, 0] == 0x5A5A5A5A).all()) and bool((fb[:, 1 + words:] == 0x5A5A5A5A).all())
    err = lambda: Lb.qd_last_error().decode()
    assert call(smp._h, m - 1, obs.stride(0), fb.stride(0)) == -1 and "strides" in err()
    assert call(smp._h, det.stride(0), nobs - 1, fb.stride(0)) == -1 and "strides" in err()
    assert call(smp._h, det.stride(0), obs.stride(0), 2) == -1 and "fault rows hold 64 bits" in err()
    other = StratifiedDemSampler(*_toy(65, 9), 20)
    assert call(other._h, det.stride(0), obs.stride(0), fb.stride(0)) == -1 and "65 faults" in err()


def test_every_row_holds_its_count(gpu):
    """2^14 BB72 rows with counts from 0 to 255, the popcount taken on the device."""
    import torch
    from quits_amd.decoder.device import StratifiedDemSampler
    H, L, pri = _bb72()
    smp = StratifiedDemSampler(H, L, pri, 255)
    ks = np.random.default_rng(8).integers(0, 256, size=1 << 14)
    det, obs, fb = smp.sample_faults(ks, 12345)
    by = fb.contiguous().view(torch.uint8)
    pop = sum(((by >> i) & 1).sum(dim=1, dtype=torch.int64) for i in range(8))
    assert torch.equal(pop.cpu(), torch.from_numpy(ks.astype(np.int64)))
    assert not bool(det[torch.from_numpy(ks == 0).cuda()].any())


def _circuit_model():
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.dem import Circuit
    circ = Circuit(helpers.circuit_text(BB72))
    H, L, pri = detector_error_model_to_matrix(circ.detector_error_model())
    return circ, helpers.code("bb72"), H, L, np.asarray(pri, np.float64)


def test_driver_counts_the_failures_of_the_mirrors_shots(gpu):
    """get_stratified_pL, strata 0, 2 and 14 of 2^12 shots each: the failures of a stratum are those of the MIRROR's shots decoded by
    sliding_window_bposd_circuit_mem, exactly; stratum 0 never fails; the result does not depend on the batch; the lightest residual is
    what its (k, shot) says."""
    from scipy.sparse import csr_matrix
    from quits_amd.decoder import sliding_window_bposd_circuit_mem, sliding_window_corrections
    from quits_amd.simulation import get_stratified_pL, replay_strata_faults
    circ, cd, H, L, pri = _circuit_model()
    N = 1 << 12
    args = (circ, cd["hz"], cd["lz"], 3, 1, {0: N, 2: N, 14: N, 9: 0})
    r = get_stratified_pL(*args, seed=6, batch=1024, **MINSUM)
    assert r.shots_by_faults.sum() == 3 * N and all(r.shots_by_faults[k] == N for k in (0, 2, 14))
    for k in (0, 2, 14):
        det, obs, E = strata.sample_mirror(H, L, pri, k, 6, N)
        pred = sliding_window_bposd_circuit_mem(det, circ, cd["hz"], cd["lz"], 3, 1, **MINSUM)
        fails = int((pred != obs.astype(np.int64)).any(axis=1).sum())
        print("stratum %d: %d failures of %d" % (k, fails, N))
        assert r.errors_by_faults[k] == fails
    assert r.errors_by_faults[0] == 0 and r.errors_by_faults[14] > 0 and r.errors_by_faults.sum() == sum(r.errors_by_faults[k] for k in (2, 14))
    pmf, tail = strata.fault_count_pmf(pri, 255)
    assert np.array_equal(r.pmf, pmf) and r.tail == tail
    want = strata.estimate(r.shots_by_faults, r.errors_by_faults, pmf, tail)
    assert (r.pL, r.sigma, r.unsampled_mass) == want and r.unsampled_mass == pytest.approx(1.0 - pmf[[0, 2, 14]].sum(), abs=1e-12)
    other = get_stratified_pL(*args, seed=6, batch=4096, **MINSUM)
    assert np.array_equal(other.errors_by_faults, r.errors_by_faults) and other.lightest == r.lightest
    assert np.array_equal(other.residual_weight_hist, r.residual_weight_hist)
    assert r.residual_shots == 0 and r.residual_weight_hist.sum() == r.errors_by_faults.sum()
    w, k, s = r.lightest
    assert k in (2, 14) and 0 < w and r.residual_weight_hist[:w].sum() == 0 and r.residual_weight_hist[min(w, 255)] >= 1
    Es = replay_strata_faults(circ, k, [s], 6)
    assert Es.shape == (1, H.shape[1]) and Es.sum() == k
    assert np.array_equal(Es, strata.sample_faults_mirror(pri, k, 6, np.array([s])))
    det = np.asarray((csr_matrix(H) @ Es.T.astype(np.int64)).T % 2).astype(np.uint8)
    pred, packed = sliding_window_corrections(det, circ, cd["hz"], cd["lz"], 3, 1, **MINSUM)
    resid = Es[0].astype(np.uint8) ^ np.asarray(packed)[0]
    assert resid.sum() == w
    assert not ((csr_matrix(H) @ resid.astype(np.int64)) % 2).any() and ((csr_matrix(L) @ resid.astype(np.int64)) % 2).any()


def test_same_law_through_the_decoder(gpu):
    """The direct experiment (2^18 independent-fault shots, binned by |E|) and stratified runs measure the same f(k): at k = 13, 14, 15 (the
    mean fault count is 14.0; each direct stratum must hold >= 100 failures) |f_direct - f_strat| <= 4 sqrt(sum of the two binomial variances),
    and pL over the strata 0 .. 60, 2^12 shots each, agrees with the direct pL within 4 combined sigma + the unsampled mass.  Seeds are fixed:
    the test is deterministic, and a 4 sigma miss (probability 6e-5 for one stratum) is a finding.  Measured on an MI355X: 0.8, 2.0 and 1.4
    combined sigma at k = 13, 14, 15, and 2.7 for pL -- the strata of one seed share their random words, so these are not independent draws
    and `sigma` understates the spread of the sum (StratifiedResult.sigma_max bounds it)."""
    from quits_amd.simulation import get_fault_spectrum, get_stratified_pL
    circ, cd, H, L, pri = _circuit_model()
    a = (circ, cd["hz"], cd["lz"], 3, 1)
    direct = get_fault_spectrum(*a, 1 << 18, seed=21, **MINSUM)
    near = get_stratified_pL(*a, {13: 1 << 14, 14: 1 << 14, 15: 1 << 14}, seed=22, **MINSUM)
    fd, fs = direct.failure_fraction(), near.failure_fraction()
    for k in (13, 14, 15):
        nd, ns = int(direct.shots_by_faults[k]), int(near.shots_by_faults[k])
        bound = 4.0 * math.sqrt(fd[k] * (1.0 - fd[k]) / nd + fs[k] * (1.0 - fs[k]) / ns)
        print("k = %d: direct %d / %d = %.5f, stratified %d / %d = %.5f, difference %.5f, bound %.5f"
              % (k, direct.errors_by_faults[k], nd, fd[k], near.errors_by_faults[k], ns, fs[k], abs(fd[k] - fs[k]), bound))
        assert ns == 1 << 14 and direct.errors_by_faults[k] >= 100
        assert abs(fd[k] - fs[k]) <= bound
        assert abs(nd / direct.shots - near.pmf[k]) <= 5.0 * math.sqrt(near.pmf[k] / direct.shots)       # the pmf weighs the strata as the direct run fills them
    wide = get_stratified_pL(*a, {k: 1 << 12 for k in range(61)}, seed=23, **MINSUM)
    sd = math.sqrt(direct.pL * (1.0 - direct.pL) / direct.shots)
    bound = 4.0 * math.sqrt(sd * sd + wide.sigma ** 2) + wide.unsampled_mass
    print("pL: direct %.6f +- %.6f (%d shots), stratified %.6f +- %.6f (61 strata of 4096), unsampled mass %.3e, difference %.6f, bound %.6f"
          % (direct.pL, sd, direct.shots, wide.pL, wide.sigma, wide.unsampled_mass, abs(direct.pL - wide.pL), bound))
    assert wide.unsampled_mass < 1e-12 and wide.errors_by_faults[0] == 0
    assert abs(direct.pL - wide.pL) <= bound
