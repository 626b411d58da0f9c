"""Stratified DEM sampling on the host (quits_amd/strata.py): the threshold table against exact arithmetic, the fault-count pmf, the numpy
mirror that specifies qd_sample_dem_strata, the estimator's algebra, the refusals, and the new exports' argument checks.  No GPU."""
import ctypes
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import helpers
from quits_amd import strata

BB72 = "bb72_custom_r6_p0.003"
TWO32 = 1 << 32


def _odds(priors):
    return [Fraction(p) / (1 - Fraction(p)) for p in priors]


def _esym(w, kmax):
    """e_0 .. e_kmax of the list w, exactly."""
    e = [Fraction(1)] + [Fraction(0)] * kmax
    for x in w:
        for r in range(kmax, 0, -1):
            e[r] += x * e[r - 1]
    return e


def _exact_q(priors, kmax):
    """{(j, r): q[j][r]} for every state with e_r(w_{j..}) > 0, from the definition."""
    w = _odds(priors)
    n = len(w)
    suffix = [_esym(w[j:], kmax) for j in range(n + 1)]
    return {(j, r): w[j] * suffix[j + 1][r - 1] / suffix[j][r] for j in range(n) for r in range(1, kmax + 1) if suffix[j][r] > 0}


def test_thresholds_against_exact_arithmetic():
    """n = 10, mixed priors, kmax = 10: every reachable threshold within one unit of floor(q 2^32) (the recursion's rounding is far below a
    unit; the unit covers a q 2^32 that sits on an integer), q = 1 where inclusion is forced, the sentinel elsewhere, column 0 zero."""
    pri = [0.3, 1e-9, 0.0, 0.011, 0.009, 0.0123, 0.0101, 0.02, 0.008, 0.013]
    thr = strata.strata_thresholds(pri, 10)
    assert thr.dtype == np.uint32 and thr.shape == (10, 11) and not thr[:, 0].any()
    exact = _exact_q(pri, 10)
    assert len(exact) > 40
    for (j, r), q in exact.items():
        want = min(q.numerator * TWO32 // q.denominator, TWO32 - 1)
        assert abs(int(thr[j, r]) - want) <= 1, (j, r, int(thr[j, r]), want)
    for j in range(10):
        for r in range(1, 11):
            if (j, r) not in exact:
                assert thr[j, r] == strata.UNREACHABLE
    # no prior 0 behind j = 3: n - j = r is a reachable state there and its q is 1
    for j in range(3, 10):
        assert exact[(j, 10 - j)] == 1 and thr[j, 10 - j] == TWO32 - 1
    # the rows do not depend on how many columns the table has
    assert np.array_equal(strata.strata_thresholds(pri, 4), thr[:, :5])


def _log_domain_q(pri, kmax):
    """q[j][r] from log e_r(w_{j..}) by logaddexp: an independent float route (relative error about n 2^-52 in every e)."""
    w = np.asarray(pri, np.float64)
    lw = np.log(w / (1.0 - w), where=w > 0, out=np.full(w.shape, -np.inf))
    n = len(w)
    le = np.full(kmax + 1, -np.inf)
    le[0] = 0.0
    q = np.full((n, kmax + 1), np.nan)
    with np.errstate(invalid="ignore"):
        for j in range(n - 1, -1, -1):
            new = le.copy()
            new[1:] = np.logaddexp(le[1:], lw[j] + le[:-1])
            q[j, 1:] = np.exp(lw[j] + le[:-1] - new[1:])
            le = new
    return q, np.isfinite(q)


@pytest.mark.parametrize("which", ["bb72", "spread"])
def test_no_reachable_state_is_lost_at_kmax_255(which):
    """2592 faults, kmax = 255: the recursion raises no invalid operation, division by zero or overflow, and every reachable state's threshold
    agrees with the log-domain route to 1e-9 relative (4.3 units of 2^-32) + 1.  Again with priors from 1e-12 to 0.4."""
    pri = np.asarray(helpers.dem_matrices(BB72)[2], np.float64)
    if which == "spread":
        pri = 10.0 ** np.random.default_rng(11).uniform(-12.0, math.log10(0.4), size=pri.shape[0])
    with np.errstate(invalid="raise", divide="raise", over="raise"):
        thr = strata.strata_thresholds(pri, 255)
    n = pri.shape[0]
    q, ok = _log_domain_q(pri, 255)
    j, r = np.meshgrid(np.arange(n), np.arange(256), indexing="ij")
    reach = (r >= 1) & (r <= n - j)
    assert np.array_equal(ok & (r >= 1), reach)                       # all priors positive: reachable = enough faults left
    want = np.minimum(np.floor(q[reach] * 4294967296.0), 4294967295.0)
    assert np.abs(thr[reach].astype(np.float64) - want).max() <= 1e-9 * 4294967296.0 + 1.0
    assert not thr[~reach].any()
    assert (thr[n - 255 + np.arange(255), 255 - np.arange(255)] == 0xFFFFFFFF).all()      # n - j = r


def test_fault_count_pmf():
    pri = [0.3, 1e-9, 0.0, 0.011, 0.009, 0.0123, 0.0101, 0.02, 0.008, 0.013, 0.25, 0.04]
    e = _esym(_odds(pri), 12)
    none = Fraction(1)
    for p in pri:
        none *= 1 - Fraction(p)
    for kmax in (12, 5, 0):
        pmf, tail = strata.fault_count_pmf(pri, kmax)
        assert pmf.dtype == np.float64 and pmf.shape == (kmax + 1,)
        for k in range(kmax + 1):
            want = float(none * e[k])
            assert abs(pmf[k] - want) <= 1e-12 * want, (kmax, k)
        want = float(none * sum(e[kmax + 1:], Fraction(0)))
        assert abs(tail - want) <= 1e-12 * want
    pri = np.asarray(helpers.dem_matrices(BB72)[2], np.float64)
    pmf, tail = strata.fault_count_pmf(pri, 255)
    assert abs(pmf.sum() + tail - 1.0) <= 1e-10 and abs((np.arange(256) * pmf).sum() - pri.sum()) <= 1e-10
    assert 0.0 <= tail < 1e-100


def test_mirror_philox_is_the_test_suites():
    import frame_mirror
    rng = np.random.default_rng(3)
    c = rng.integers(0, TWO32, size=(4, 33), dtype=np.uint64)
    for a, b in zip(strata.philox4x32_10(c[0], c[1], c[2], c[3], 0x243F6A88, 0x85A308D3), frame_mirror.philox(c[0], c[1], c[2], c[3], 0x243F6A88, 0x85A308D3)):
        assert np.array_equal(a, b)


def test_mirror_rows():
    """Exactly k faults per row, det = H E and obs = L E, rows a function of (seed, shot, k) alone, k = 0 and k = n."""
    H, L, pri = helpers.dem_matrices(BB72)
    n = H.shape[1]
    ks = np.array([0, 1, 2, 7, 40] * 8)
    det, obs, E = strata.sample_mirror(H, L, pri, ks, 9, 40)
    assert E.shape == (40, n) and E.dtype == bool and det.dtype == np.uint8 and det.shape == (40, H.shape[0]) and obs.shape == (40, L.shape[0])
    assert np.array_equal(E.sum(axis=1), ks)
    Hd, Ld = np.asarray(H.todense()).astype(np.int64), np.asarray(L.todense()).astype(np.int64)
    assert np.array_equal(det, (E.astype(np.int64) @ Hd.T) % 2) and np.array_equal(obs, (E.astype(np.int64) @ Ld.T) % 2)
    assert not det[ks == 0].any() and not obs[ks == 0].any()
    # split batches, a shuffled shot list, repeats
    a = strata.sample_faults_mirror(pri, ks[:13], 9, np.arange(13))
    b = strata.sample_faults_mirror(pri, ks[13:], 9, np.arange(13, 40))
    assert np.array_equal(np.concatenate([a, b]), E)
    order = np.random.default_rng(1).permutation(40)
    order = np.concatenate([order, order[:5]])
    assert np.array_equal(strata.sample_faults_mirror(pri, ks[order], 9, order), E[order])
    assert not np.array_equal(strata.sample_faults_mirror(pri, ks, 10, 40), E)              # the seed matters
    assert not np.array_equal(strata.sample_faults_mirror(pri, 7, 9, np.arange(40) + (1 << 32))[ks == 7], E[ks == 7])     # ... and the shot's high word
    # a tiny model: k = n takes every fault, whatever the priors
    tiny = [0.2, 0.01, 0.4, 0.05, 0.3]
    Et = strata.sample_faults_mirror(tiny, [5, 0, 5, 4], 2, 4)
    assert Et[0].all() and Et[2].all() and not Et[1].any() and Et[3].sum() == 4


def test_mirror_draws_the_exact_conditional_law():
    """n = 8, k = 3, 2^16 shots: each of the 56 subsets within 5 binomial sigma of N prod w_j / e_3(w); the least likely expects >= 200."""
    pri = [0.10, 0.17, 0.12, 0.15, 0.11, 0.16, 0.13, 0.14]
    N = 1 << 16
    E = strata.sample_faults_mirror(pri, 3, 2026, N)
    assert (E.sum(axis=1) == 3).all()
    w = _odds(pri)
    e3 = _esym(w, 3)[3]
    codes = (E.astype(np.int64) << np.arange(8)).sum(axis=1)
    counts = np.bincount(codes, minlength=256)
    seen = 0
    for S in itertools.combinations(range(8), 3):
        prob = float(w[S[0]] * w[S[1]] * w[S[2]] / e3)
        assert N * prob >= 200
        got = int(counts[sum(1 << i for i in S)])
        assert abs(got - N * prob) <= 5.0 * math.sqrt(N * prob * (1.0 - prob)), (S, got, N * prob)
        seen += got
    assert seen == N


def test_estimator_algebra():
    from quits_amd.simulation import StratifiedResult
    pmf = np.array([0.5, 0.25, 0.125, 0.0625])
    shots = np.zeros(256, np.int64)
    errors = np.zeros(256, np.int64)
    shots[:3] = [100, 400, 0]
    errors[:3] = [0, 100, 0]
    shots[3], errors[3] = 50, 25
    r = StratifiedResult.from_counts(shots, errors, np.concatenate([pmf, np.zeros(252)]), 0.0625)
    assert r.pL == pytest.approx(0.25 * 0.25 + 0.0625 * 0.5, rel=1e-15)
    assert r.sigma == pytest.approx(math.sqrt(0.25 ** 2 * 0.25 * 0.75 / 400 + 0.0625 ** 2 * 0.25 / 50), rel=1e-14)
    assert r.unsampled_mass == pytest.approx(0.125 + 0.0625, rel=1e-15)
    assert r.sigma_max == pytest.approx(0.25 * math.sqrt(0.25 * 0.75 / 400) + 0.0625 * math.sqrt(0.25 / 50), rel=1e-14) and r.sigma_max >= r.sigma
    f = r.failure_fraction()
    assert f[0] == 0.0 and f[1] == 0.25 and f[3] == 0.5 and np.isnan(f[2]) and np.isnan(f[4:]).all()
    assert r.lightest is None and r.residual_weight_hist.shape == (256,)
    assert strata.estimate(shots[:4], errors[:4], pmf, 0.0625) == (r.pL, r.sigma, r.unsampled_mass)
    with pytest.raises(ValueError):
        strata.estimate([1, 2], [2, 0], [0.5, 0.5], 0.0)              # more errors than shots
    with pytest.raises(ValueError):
        strata.estimate([1, 2, 3], [0, 0, 0], [0.5, 0.5], 0.0)        # shots in a stratum the pmf does not cover


def test_refusals():
    from quits_amd.simulation import _strata_plan
    for fn in (strata.strata_thresholds, strata.fault_count_pmf):
        with pytest.raises(ValueError, match="priors"):
            fn([0.1, 1.0], 2)
        with pytest.raises(ValueError, match="priors"):
            fn([0.1, -1e-9], 2)
        with pytest.raises(ValueError, match="priors"):
            fn([0.1, float("nan")], 2)
        with pytest.raises(ValueError, match="kmax"):
            fn([0.1, 0.2], 256)
        with pytest.raises(ValueError, match="kmax"):
            fn([0.1, 0.2], -1)
    pri = [0.1, 0.0, 0.2, 0.3]
    assert strata.check_ks(3, 2, pri, 3).tolist() == [3, 3] and strata.check_ks([0, 3], 2, pri, 3).dtype == np.int32
    with pytest.raises(ValueError, match="p > 0"):
        strata.check_ks(4, 1, pri, 4)                                 # four faults, three that can fire
    with pytest.raises(ValueError):
        strata.check_ks([1, 3], 2, pri, 2)                            # beyond the table
    with pytest.raises(ValueError):
        strata.check_ks([-1], 1, pri, 3)
    with pytest.raises(ValueError):
        strata.check_ks([1, 2], 3, pri, 3)                            # one count per shot
    with pytest.raises(ValueError):
        strata.check_ks([1.5], 1, pri, 3)
    with pytest.raises(ValueError, match="p > 0"):
        strata.sample_faults_mirror(pri, 4, 1, 2)
    assert _strata_plan({14: 8, 0: 4, 2: 0}) == [(0, 4), (14, 8)]
    with pytest.raises(ValueError):
        _strata_plan({256: 1})
    with pytest.raises(ValueError):
        _strata_plan({3: -1})


def test_exports_check_their_arguments_without_a_gpu():
    from quits_amd import _lib
    L = _lib.load()
    assert L.qd_version() >= 111 and _lib.require_strata(L) is L
    for name in ("qd_strata_create", "qd_strata_destroy", "qd_strata_info", "qd_sample_dem_strata"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    err = lambda: L.qd_last_error().decode()
    thr = np.zeros((3, 3), np.uint32)
    thr[:, 1:] = 7
    tp = thr.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p()
    # create(n, kmax, thresholds, device, &out): every call below is refused before a device is touched
    assert L.qd_strata_create(3, 2, tp, 0, None) == -1 and "out is null" in err()
    assert L.qd_strata_create(0, 2, tp, 0, ctypes.byref(h)) == -1 and "at least one fault" in err()
    assert L.qd_strata_create(3, -1, tp, 0, ctypes.byref(h)) == -1 and "kmax" in err()
    assert L.qd_strata_create(3, 256, tp, 0, ctypes.byref(h)) == -1 and "kmax" in err()
    assert L.qd_strata_create(3, 2, None, 0, ctypes.byref(h)) == -1 and "null thresholds" in err()
    thr[1, 0] = 5
    assert L.qd_strata_create(3, 2, tp, 0, ctypes.byref(h)) == -1 and "column 0" in err() and "thresholds[1][0]" in err()
    assert not h.value
    assert L.qd_strata_info(None, None) == -1 and "null" in err()
    L.qd_strata_destroy(None)
    # sample(strata, Ht, Lt, seed, shot0, d_shots, d_k, B, d_det, det_stride, d_obs, obs_stride, d_fault_bits, fault_stride_words, stream)
    buf = ctypes.create_string_buffer(64)          # never dereferenced: every call below is refused, or has no shots
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.qd_sample_dem_strata(None, None, None, 1, 0, None, None, 0, None, 0, None, 0, None, 0, None) == 0          # B = 0: nothing to do
    assert L.qd_sample_dem_strata(p, p, p, 1, 0, None, p, -1, p, 9, p, 9, p, 9, None) == -1 and "shot count" in err()
    assert L.qd_sample_dem_strata(p, p, p, 1, -1, None, p, 1, p, 9, p, 9, p, 9, None) == -1 and "negative shot0" in err()
    assert L.qd_sample_dem_strata(p, p, p, 1, 0, None, None, 1, p, 9, p, 9, p, 9, None) == -1 and "d_k" in err()
    assert L.qd_sample_dem_strata(None, p, p, 1, 0, None, p, 1, p, 9, p, 9, p, 9, None) == -1 and "null" in err()
    assert L.qd_sample_dem_strata(p, None, p, 1, 0, None, p, 1, p, 9, p, 9, p, 9, None) == -1 and "null" in err()
    assert L.qd_sample_dem_strata(p, p, None, 1, 0, None, p, 1, p, 9, p, 9, p, 9, None) == -1 and "null" in err()
    assert L.qd_sample_dem_strata(p, p, p, 1, 0, None, p, 1, None, 9, p, 9, p, 9, None) == -1 and "null" in err()
    assert L.qd_sample_dem_strata(p, p, p, 1, 0, None, p, 1, p, 9, None, 9, p, 9, None) == -1 and "null" in err()
    assert L.qd_sample_dem_strata(p, p, p, 1, 0, None, p, 1, p, 9, p, 9, None, 9, None) == -1 and "null" in err()


def test_kernel_compiles_without_scratch(tmp_path):
    """One kernel, in the library's source list, no scratch (its arrays of four Philox words and thresholds stay in registers), no static LDS,
    no preprocessor fork."""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cs = os.path.join(root, "quits_amd", "csrc")
    mk = open(os.path.join(cs, "Makefile")).read()
    assert re.search(r"^SRC := .*\bstrata_sampler\.hip\b", mk, re.M)
    flags = [f for f in re.search(r"^FLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split() if f != "-shared"]
    out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o",
                          str(tmp_path / "strata.o"), os.path.join(cs, "strata_sampler.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out.stderr)]
    assert len(names) == 1 and "qd_sample_strata_kernel" in names[0], names
    assert scratch == [0] and lds == [0]
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", open(os.path.join(cs, "strata_sampler.hip")).read(), re.M)
