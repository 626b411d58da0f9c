"""Circuit-level frame sampler, host side: the compile step (quits_amd/frame.py) and the CPU mirror (tests/frame_mirror.py) that
specifies the device kernel.  No GPU needed."""
import re

import numpy as np
import pytest

import dem_forward
import frame_mirror as fm
import helpers
from quits_amd import frame
from quits_amd.dem import Circuit
from quits_amd.stim_text import flatten

ALL_FIXTURES = sorted(helpers.circuit_index())


def zero_noise(text):
    return re.sub(r"(X_ERROR|Z_ERROR|DEPOLARIZE1|DEPOLARIZE2)\([^)]*\)", r"\1(0)", text)


def dem_marginals(text):
    """Per-detector and per-observable flip rates the circuit's DEM predicts: (1 - prod_j (1 - 2 p_j)) / 2 over its mechanisms."""
    dem = Circuit(text).detector_error_model()
    ld = np.zeros(dem.num_detectors)
    lo = np.zeros(dem.num_observables)
    for p, dets, obs in dem.errors:
        f = np.log(abs(1.0 - 2.0 * p))
        for d in dets:
            ld[d] += f
        for o in obs:
            lo[o] += f
    return (1.0 - np.exp(ld)) / 2.0, (1.0 - np.exp(lo)) / 2.0


@pytest.mark.parametrize("name,sites,lookback,nq", [("bb144_custom_r12_p0.003", 28368, 288, 288),
                                                     ("qlp1020_cardinal_r20_p0.003", 474420, 1920, None)])
def test_compile_counts(name, sites, lookback, nq):
    cc = frame.compile_circuit(helpers.circuit_text(name))
    assert cc.nsites == sites and cc.lookback == lookback
    if nq is not None:
        assert cc.nq == nq
    assert cc.lds_bytes == 8 * (2 * cc.nq + cc.ring + cc.nobs) <= frame.LDS_BUDGET      # QLP-1020 r20 fits


@pytest.mark.parametrize("name", ["bb144_custom_r12_p0.003", "hgp225_cardinal_r15_p0.001", "bb72_custom_r2_xbasis_mixed"])
def test_sites_start_on_multiples_of_4(name):
    cc = frame.compile_circuit(helpers.circuit_text(name))
    ops = flatten(helpers.circuit_text(name))[0]
    sizes = [len(op.targets) // (2 if op.name == "DEPOLARIZE2" else 1) for op in ops
             if op.name in ("X_ERROR", "Z_ERROR", "DEPOLARIZE1", "DEPOLARIZE2")]
    first = cc.first_sites
    assert len(first) == len(sizes) and first[0] == 0 and np.all(first % 4 == 0)
    nxt = first[:-1] + np.asarray(sizes[:-1])
    assert np.array_equal(first[1:], (nxt + 3) // 4 * 4)          # the next multiple of 4 after the previous instruction
    assert cc.site_span == first[-1] + sizes[-1] and cc.nsites == sum(sizes)


def test_thresholds_match_oracle():
    import oracle as orc
    L = orc.lib()
    text = helpers.circuit_text("bb72_custom_r2_xbasis_mixed")          # four distinct channel rates
    cc = frame.compile_circuit(text)
    ps = sorted({op.arg for op in flatten(text)[0] if op.name in ("X_ERROR", "Z_ERROR", "DEPOLARIZE1", "DEPOLARIZE2")})
    assert len(ps) > 1
    assert sorted(int(t) for t in cc.thresholds) == sorted(int(L.oq_prob_threshold(p)) for p in ps)
    for p in ps + [0.0, 1e-9, 0.5, 1.0]:
        assert frame.prob_threshold(p) == int(L.oq_prob_threshold(p)) == fm.threshold(p)


SPLIT_CIRCUIT = """R 0 1 2 3
X_ERROR(0.25) 0 0 2
H 0 1 0 2
CX 0 1 1 2 2 3 0 3
DEPOLARIZE2(0.3) 0 1 1 2
M 3
MR 1 1
DEPOLARIZE1(0.2) 3 3
MX 0
DETECTOR rec[-1] rec[-2]
DETECTOR rec[-3]
OBSERVABLE_INCLUDE(0) rec[-4]
"""


def _parts(cc):
    out, pc, p = [], 0, cc.program
    while pc < len(p):
        op, n = int(p[pc]), int(p[pc + 1])
        out.append((op, [int(x) for x in p[pc + 2:pc + frame._length(op, n)]]))
        pc += frame._length(op, n)
    return out


def test_repeated_qubits_are_split():
    cc = frame.compile_circuit(SPLIT_CIRCUIT)
    parts = _parts(cc)
    gates = [(op, a) for op, a in parts if op in (frame.OP_H, frame.OP_CX, frame.OP_MR)]
    assert gates == [(frame.OP_H, [0, 1]), (frame.OP_H, [0, 2]),
                     (frame.OP_CX, [0, 1]), (frame.OP_CX, [1, 2]), (frame.OP_CX, [2, 3]), (frame.OP_CX, [0, 3]),
                     (frame.OP_MR, [1, 1 % cc.ring]), (frame.OP_MR, [1, 2 % cc.ring])]
    # noise instructions are not split: a repeated target is two independent sites
    noise = [(op, a) for op, a in parts if op in (frame.OP_XERR, frame.OP_DEP1, frame.OP_DEP2)]
    assert [(op, a[1], a[2:]) for op, a in noise] == [(frame.OP_XERR, 0, [0, 0, 2]), (frame.OP_DEP2, 4, [0, 1, 1, 2]),
                                                      (frame.OP_DEP1, 8, [3, 3])]
    # the split program computes what the sequential semantics does: all lanes of a part touch distinct qubits
    for op, a in gates:
        qs = a if op == frame.OP_H else (a if op == frame.OP_CX else a[0::2])
        assert len(set(qs)) == len(qs)


def test_cx_control_equal_target_refused():
    with pytest.raises(ValueError):
        frame.compile_circuit("R 0 1\nCX 0 1 1 1\nM 0\nDETECTOR rec[-1]\n")


def test_lds_budget_refusal():
    n = 5000
    qs = " ".join(str(q) for q in range(n))
    text = "R %s\nX_ERROR(0.01) %s\nM %s\nDETECTOR rec[-1]\n" % (qs, qs, qs)
    with pytest.raises(NotImplementedError, match=r"%d qubits.*5000-measurement ring.*budget is %d B" % (n, frame.LDS_BUDGET)):
        frame.compile_circuit(text)
    frame.compile_circuit(text, lds_budget=1 << 20)             # the same circuit under a larger budget compiles


def test_mirror_philox_matches_oracle():
    """The mirror's vectorised Philox (uint64 arithmetic, many counters per call) against the oracle's C function."""
    import oracle as orc
    L = orc.lib()
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64)
    for k0, k1 in ((0, 0), (0xDEADBEEF, 0x12345678), (0xFFFFFFFF, 1)):
        got = np.stack(fm.philox(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], k0, k1), axis=1).astype(np.uint32)
        for row, c in zip(got, ctr):
            out = np.zeros(4, np.uint32)
            L.oq_philox(*(int(x) for x in c), k0, k1, out)
            assert np.array_equal(row, out)


@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_mirror_noise_free_is_zero(name):
    text = zero_noise(helpers.circuit_text(name))
    B = 70 if name.startswith("qlp") else 200
    det, obs = fm.sample(text, seed=(5 << 40) | 99, shot0=3, B=B)
    assert not det.any() and not obs.any()
    cc = frame.compile_circuit(text)
    assert list(cc.thresholds) == [0]


@pytest.mark.parametrize("name", ["bb72_custom_r6_p0.003", "bb72_custom_r2_xbasis_mixed"])
def test_mirror_forced_components_match_forward_propagation(name):
    text = helpers.circuit_text(name)
    parsed = flatten(text)
    total = dem_forward.forward_detector_sets(text, 0, 1, parsed)[3]
    comps = np.unique(np.concatenate([np.random.default_rng(11).choice(total, 700, replace=False), [0, total - 1]]))
    det, _ = fm.run(text, len(comps), fm.forced_noise(comps), parsed)
    # one forward pass over the span of the sample, then its columns
    lo, hi = int(comps[0]), int(comps[-1]) + 1
    ndet, dflip, ncomp, _ = dem_forward.forward_detector_sets(text, lo, hi, parsed)
    bits = np.unpackbits(dflip.view(np.uint8), axis=1, bitorder="little")[:, :ncomp]     # [ndet, components lo..hi)
    expect = bits[:, comps - lo].T
    assert det.shape == expect.shape and np.array_equal(det, expect)
    assert det.any(axis=1).mean() > 0.5                         # the sample is not dominated by silent components


def test_mirror_marginals_match_dem():
    name = "bb72_custom_r6_p0.003"
    text = helpers.circuit_text(name)
    B = 4096
    det, obs = fm.sample(text, seed=2026, shot0=0, B=B)
    pd, po = dem_marginals(text)
    for rate, pred in ((det.mean(axis=0), pd), (obs.mean(axis=0), po)):
        sigma = np.sqrt(np.maximum(pred * (1 - pred), 1e-12) / B)
        z = (rate - pred) / sigma
        assert np.abs(z).max() < 5.0, (np.argmax(np.abs(z)), z.max(), z.min())
    chi2 = float((((det.mean(axis=0) - pd) ** 2) / (pd * (1 - pd) / B)).sum())
    from scipy.stats import chi2 as chi2_dist
    assert chi2_dist.sf(chi2, len(pd)) > 1e-3


def test_mirror_streams_compose():
    text = helpers.circuit_text("bb72_custom_r2_xbasis_mixed")
    seed = (0xA5A5 << 32) | 0x1234
    d, o = fm.sample(text, seed, 10, 150)
    d1, o1 = fm.sample(text, seed, 10, 61)
    d2, o2 = fm.sample(text, seed, 71, 89)
    assert np.array_equal(d, np.concatenate([d1, d2])) and np.array_equal(o, np.concatenate([o1, o2]))


def test_abi_refuses_bad_programs_before_touching_a_device():
    """qd_circuit_create checks every index the kernel will use, and the LDS budget, on the host (no GPU needed)."""
    import ctypes as C
    from quits_amd import _lib
    L = _lib.load()
    cc = frame.compile_circuit(helpers.circuit_text("bb72_custom_r6_p0.003"))
    thr = cc.thresholds

    def create(prog, ring=cc.ring, nq=cc.nq):
        h = C.c_void_p()
        rc = L.qd_circuit_create(prog.ctypes.data_as(C.c_void_p), len(prog), nq, cc.nmeas, cc.ndet, cc.nobs,
                                 thr.ctypes.data_as(C.c_void_p), len(thr), ring, 0, C.byref(h))
        return rc, L.qd_last_error()
    bad = cc.program.copy()
    assert bad[0] == frame.OP_R
    bad[2] = cc.nq                                               # first reset target one past the last qubit
    rc, msg = create(bad)
    assert rc == -1 and b"qubit out of range" in msg
    assert b"runs past the end" in create(cc.program[:-1])[1]
    assert create(cc.program, ring=8000)[0] == -4                # 8 (2 nq + ring + nobs) > 64 KiB
