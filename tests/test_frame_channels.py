"""Biased noise (Y_ERROR, PAULI_CHANNEL_1, PAULI_CHANNEL_2), host side: the parser's `channels` keyword, the compile step, the CPU
mirror that specifies the kernel (tests/frame_mirror_channels.py), the DEM extractor's opt-in conversion and the C ABI's
checks.  No GPU needed."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import channel_circuits as cc_
import frame_mirror as fm
import frame_mirror_channels as fmc
import helpers
from quits_amd import frame
from quits_amd.dem import Circuit, circuit_to_dem, dem_struct_cache_clear, dem_struct_cache_info
from quits_amd.stim_text import CircuitSyntaxError, flatten
from test_frame_sampler import dem_marginals

ALL_FIXTURES = sorted(helpers.circuit_index())
BB72 = "bb72_custom_r6_p0.003"
P15 = ", ".join(["0.01"] * 15)


# ---------------------------------------------------------------------------------------------------------------- parser

def test_parser_accepts_the_three_instructions():
    ops, nm, nd, no = flatten("R 0 1 2\nPAULI_CHANNEL_1(0.1, 0.2, 0.3) 0 2\nPAULI_CHANNEL_2(%s) 0 1 2 0\nY_ERROR(0.25) 1\nM 0\n" % P15,
                              channels=True)
    pc1, pc2, ye = ops[1], ops[2], ops[3]
    assert (pc1.name, pc1.args, pc1.targets) == ("PAULI_CHANNEL_1", (0.1, 0.2, 0.3), (0, 2))
    assert pc1.arg == (0.1 + 0.2) + 0.3
    assert (pc2.name, pc2.args, pc2.targets) == ("PAULI_CHANNEL_2", (0.01,) * 15, (0, 1, 2, 0))
    assert abs(pc2.arg - 0.15) < 1e-15
    assert (ye.name, ye.arg, ye.args, ye.targets) == ("Y_ERROR", 0.25, (0.25,), (1,))
    assert ops[0].args == () and ops[4].args == ()              # everything else keeps an empty list
    assert nm == 1


def test_op_keeps_its_three_argument_construction():
    from quits_amd.stim_text import Op
    assert Op("H", 0.0, (1,)).args == ()


@pytest.mark.parametrize("line", ["PAULI_CHANNEL_1(0.1, 0.2) 0", "PAULI_CHANNEL_1(0.1, 0.2, 0.3, 0.1) 0", "PAULI_CHANNEL_2(0.1, 0.2, 0.3) 0 1",
                                  "Y_ERROR(0.1, 0.2) 0", "Y_ERROR 0", "PAULI_CHANNEL_2(%s) 0 1 2" % P15])
def test_parser_argument_and_target_counts(line):
    with pytest.raises(CircuitSyntaxError):
        flatten(line + "\n", channels=True)


@pytest.mark.parametrize("line", ["PAULI_CHANNEL_1(0.1, -0.2, 0.3) 0", "PAULI_CHANNEL_1(0.5, 0.4, 0.2) 0", "Y_ERROR(-0.5) 0", "Y_ERROR(1.5) 0",
                                  "PAULI_CHANNEL_2(%s) 0 1" % ", ".join(["0.07"] * 15)])
def test_parser_probability_errors(line):
    with pytest.raises(ValueError) as e:
        flatten(line + "\n", channels=True)
    assert not isinstance(e.value, CircuitSyntaxError)
    flatten("PAULI_CHANNEL_1(0.5, 0.25, 0.25) 0\nPAULI_CHANNEL_1(0.5, 0.5, 1e-10) 0\n", channels=True)      # a sum of 1, and 1 within 1e-9


@pytest.mark.parametrize("line", ["PAULI_CHANNEL_1(0.1, 0.2, 0.3) 0", "PAULI_CHANNEL_2(%s) 0 1" % P15, "Y_ERROR(0.1) 0"])
def test_parser_default_still_refuses(line):
    with pytest.raises(NotImplementedError):
        flatten(line + "\n")
    with pytest.raises(NotImplementedError):
        flatten("R 0\nM(0.01) 0\n", channels=True)              # measurement noise stays out of scope in both modes


# --------------------------------------------------------------------------------------------------------------- compile

def _instructions(cc):
    out, pc, p = [], 0, cc.program
    while pc < len(p):
        op, n = int(p[pc]), int(p[pc + 1])
        out.append((op, n, [int(x) for x in p[pc + 2:pc + frame._length(op, n)]]))
        pc += frame._length(op, n)
    assert pc == len(p)
    return out


def test_opcode_numbers_do_not_move():
    assert (frame.OP_R, frame.OP_DEP2, frame.OP_OBS) == (0, 9, 12)
    assert (frame.OP_YERR, frame.OP_PC1, frame.OP_PC2) == (13, 14, 15)


@pytest.mark.parametrize("text", [cc_.SYNTHETIC, cc_.biased(helpers.circuit_text(BB72))], ids=["synthetic", "bb72_biased"])
def test_sites_start_on_multiples_of_4(text):
    cc = frame.compile_circuit(text)
    ops = flatten(text, channels=True)[0]
    sizes = [len(op.targets) // (2 if op.name in ("DEPOLARIZE2", "PAULI_CHANNEL_2") else 1) for op in ops
             if op.name in ("X_ERROR", "Z_ERROR", "Y_ERROR", "DEPOLARIZE1", "DEPOLARIZE2", "PAULI_CHANNEL_1", "PAULI_CHANNEL_2")]
    first = cc.first_sites
    assert len(first) == len(sizes) and first[0] == 0 and np.all(first % 4 == 0)
    assert np.array_equal(first[1:], (first[:-1] + np.asarray(sizes[:-1]) + 3) // 4 * 4)
    assert cc.site_span == first[-1] + sizes[-1] and cc.nsites == sum(sizes)


def test_synthetic_program_layout():
    cc = frame.compile_circuit(cc_.SYNTHETIC)
    noise = [(op, n, a[1]) for op, n, a in _instructions(cc) if op >= frame.OP_XERR and op not in (frame.OP_DET, frame.OP_FLUSH, frame.OP_OBS)]
    assert noise == [(frame.OP_YERR, 5, 0), (frame.OP_PC1, 6, 8), (frame.OP_PC2, 7, 16), (frame.OP_XERR, 2, 24), (frame.OP_YERR, 2, 28),
                     (frame.OP_DEP2, 2, 32), (frame.OP_PC1, 2, 36)]
    assert cc.nsites == 26 and cc.site_span == 38


def test_channel_pair_on_one_qubit_refused():
    with pytest.raises(ValueError):
        frame.compile_circuit("R 0 1\nPAULI_CHANNEL_2(%s) 0 1 1 1\nM 0\nDETECTOR rec[-1]\n" % P15)


def test_tables_are_cumulative_and_deduplicated():
    text = cc_.biased(helpers.circuit_text("bb72_custom_r2_xbasis_mixed"))         # several distinct rates
    cc = frame.compile_circuit(text)
    ops = flatten(text, channels=True)[0]
    scalars = {frame.prob_threshold(op.arg) for op in ops if op.name in ("X_ERROR", "Z_ERROR")}
    t1 = {tuple(fmc.channel_thresholds(op.args)) for op in ops if op.name == "PAULI_CHANNEL_1"}
    t2 = {tuple(fmc.channel_thresholds(op.args)) for op in ops if op.name == "PAULI_CHANNEL_2"}
    assert len(t1) >= 1 and len(t2) >= 1 and len(t1) + len(t2) > 2
    assert len(cc.thresholds) == len(scalars) + 3 * len(t1) + 15 * len(t2)          # every table stored once
    thr = [int(x) for x in cc.thresholds]
    chan = [(op, a) for op, n, a in _instructions(cc) if op in (frame.OP_PC1, frame.OP_PC2)]
    want = [op for op in ops if op.name in ("PAULI_CHANNEL_1", "PAULI_CHANNEL_2")]
    assert len(chan) == len(want)
    for (code, a), op in zip(chan, want):
        K = 3 if code == frame.OP_PC1 else 15
        tab = thr[a[0]:a[0] + K]
        assert len(tab) == K and tab == fmc.channel_thresholds(op.args) == list(frame.channel_thresholds(op.args))
        assert all(x <= y for x, y in zip(tab, tab[1:]))
        assert tab[-1] == frame.prob_threshold(sum_left_to_right(op.args))


def sum_left_to_right(args):
    acc = 0.0
    for p in args:
        acc += p
    return acc


def test_zero_components_repeat_the_previous_threshold():
    tab = frame.channel_thresholds([0.25 * w for w in cc_.W2])
    for k in (3, 8, 13):                                         # W2's zero weights
        assert tab[k] == tab[k - 1]
    assert frame.channel_thresholds((0.5, 0.25, 0.25))[-1] == 2 ** 32 - 1          # p = 1 clamps


# sha1(program bytes | thresholds bytes), noise sites, site span of every golden circuit as the compile step produced them before the
# channel opcodes existed: a circuit without the new instructions must compile to the same words
_BEFORE = {
    "bb144_custom_r12_p0.001": ("e2d0700519e89be02c91bc2e188664baf3089d05", 28368, 28368),
    "bb144_custom_r12_p0.002": ("ed4e2bd0b91e2fc52663e31b3d98f3e4e0f88b75", 28368, 28368),
    "bb144_custom_r12_p0.003": ("3d03edff2ec1da0bcb53e0b83c3a4ac2409c3b51", 28368, 28368),
    "bb144_custom_r12_p0.004": ("23960ac11d4026588eeb23ff2dfc403b67a815c6", 28368, 28368),
    "bb144_custom_r12_p0.005": ("2329385dc878a1bbac71f4d39f05a90adee3a810", 28368, 28368),
    "bb144_custom_r12_p0.006": ("3de488aeab90c287898d70514deef3a283177924", 28368, 28368),
    "bb72_custom_r0_p0.003": ("9a7dafae7f2b40e0e3c5e4e55a44ce5984b8b94f", 1224, 1224),
    "bb72_custom_r2_alldet_p0.003": ("dc67a7cd8460eea984df24f0c153354c033d08c5", 2232, 2232),
    "bb72_custom_r2_xbasis_mixed": ("76012e1a80022be552a0ed4a80a9a8fb8c831c59", 3384, 3384),
    "bb72_custom_r6_p0.003": ("edac7bdc698931af4ce90108901e7b03fbf2daec", 7704, 7704),
    "bb90_custom_r15_p0.001": ("914b2f09de1d42bd5fbe26aa5df636b8367664ab", 21780, 22326),
    "bpc_cardinal_r10_p0.0005": ("85ce931453d75b1151f71485a988e88db42fa980", 17010, 17298),
    "hgp225_cardinal_r15_p0.001": ("471acb3d31dbb30dbe51136f1c029abea037d650", 57321, 57977),
    "hgp225_cardinal_r3_p0.01": ("1d535dc8ef036d17d716377bd788c2dce2551536", 14661, 14825),
    "hgprep3_zxcoloration_r3_p0.001": ("7aed4f3fe78381e21cb5ef243cd9ee45a604cefe", 1530, 1779),
    "qlp1020_cardinal_r20_p0.003": ("4db2c579dfabaa6fc9b8eda825058950e7aa1b8a", 474420, 475092),
}


@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_old_circuits_compile_to_the_same_program(name):
    cc = frame.compile_circuit(helpers.circuit_text(name))
    assert cc.program.dtype == np.int32 and cc.thresholds.dtype == np.uint32
    digest = hashlib.sha1(cc.program.tobytes() + b"|" + cc.thresholds.tobytes()).hexdigest()
    assert (digest, cc.nsites, cc.site_span) == _BEFORE[name]


# ---------------------------------------------------------------------------------------------------------------- mirror

@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_mirror_equals_the_old_mirror_on_old_circuits(name):
    text = helpers.circuit_text(name)
    B = 70 if name.startswith("qlp") else 200
    seed, shot0 = (5 << 40) | 99, 2 ** 32 - 30
    d0, o0 = fm.sample(text, seed, shot0, B)
    d1, o1 = fmc.sample(text, seed, shot0, B)
    assert d0.any()
    assert np.array_equal(d0, d1) and np.array_equal(o0, o1)


def test_mirror_uniform_channels_have_depolarizing_marginals():
    """PAULI_CHANNEL_1(p/3 x 3) / PAULI_CHANNEL_2(p/15 x 15) IS the depolarizing channel: the mirror's samples of the rewritten circuit
    against the exact DEM of the original (no approximation involved), 5 sigma per detector and observable."""
    text = helpers.circuit_text(BB72)
    B = 4096
    det, obs = fmc.sample(cc_.uniform(text), seed=2027, shot0=0, B=B)
    pd, po = dem_marginals(text)
    for rate, pred in ((det.mean(axis=0), pd), (obs.mean(axis=0), po)):
        z = (rate - pred) / np.sqrt(np.maximum(pred * (1 - pred), 1e-12) / B)
        assert np.abs(z).max() < 5.0, (int(np.argmax(np.abs(z))), z.max(), z.min())


def test_mirror_streams_compose():
    text = cc_.SYNTHETIC
    seed = (0xA5A5 << 32) | 0x1234
    d, o = fmc.sample(text, seed, 10, 150)
    d1, o1 = fmc.sample(text, seed, 10, 61)
    d2, o2 = fmc.sample(text, seed, 71, 89)
    assert d.any() and o.any()
    assert np.array_equal(d, np.concatenate([d1, d2])) and np.array_equal(o, np.concatenate([o1, o2]))


def test_mirror_component_frequencies():
    """2^18 shots of one PAULI_CHANNEL_2 site (15 distinct probabilities, three of them 0) and one PAULI_CHANNEL_1 site: every component's
    count within 5 sigma of B (T_k - T_{k-1}) / 2^32, sigma = sqrt(B q (1 - q)); zero-probability components never drawn; and the
    frame bits are the ones the component map prescribes."""
    B = 1 << 18
    p2 = [0.6 * w for w in cc_.W2]
    p1 = (0.02, 0.3, 0.11)
    text = ("R 0 1 2\nPAULI_CHANNEL_2(%s) 0 1\nPAULI_CHANNEL_1(%s) 2\nM 0 1 2\nDETECTOR rec[-3]\nDETECTOR rec[-2]\nDETECTOR rec[-1]\n"
            % (", ".join(repr(x) for x in p2), ", ".join(repr(x) for x in p1)))
    det, _, drawn = fmc.sample(text, seed=(77 << 32) | 5, shot0=0, B=B, components=True)
    assert [(nm, s, c.shape) for nm, s, c in drawn] == [("PAULI_CHANNEL_2", 0, (1, B)), ("PAULI_CHANNEL_1", 4, (1, B))]
    for (nm, _, comp), probs in zip(drawn, (p2, p1)):
        K = len(probs)
        tab = [0] + fmc.channel_thresholds(probs)
        counts = np.bincount(comp[0].astype(np.int64), minlength=K + 1)
        assert counts.sum() == B and len(counts) == K + 1
        for k in range(1, K + 1):
            q = (tab[k] - tab[k - 1]) / 2.0 ** 32
            assert abs(q - probs[k - 1]) < 2.0 ** -31               # the thresholds realise the stated probabilities
            if probs[k - 1] == 0.0:
                assert counts[k] == 0, (nm, k)
            else:
                sigma = np.sqrt(B * q * (1 - q))
                print("%s component %2d: %6d drawn, %9.1f expected, %+.2f sigma" % (nm, k, counts[k], B * q, (counts[k] - B * q) / sigma))
                assert abs(counts[k] - B * q) < 5 * sigma, (nm, k, counts[k], B * q, sigma)
        q0 = 1.0 - tab[K] / 2.0 ** 32
        assert abs(counts[0] - B * q0) < 5 * np.sqrt(B * q0 * (1 - q0))
    # Z-basis measurements see the X bits: Pauli 1 = X and 2 = Y flip, 3 = Z does not
    v = drawn[0][2][0].astype(np.int64)
    k1 = drawn[1][2][0].astype(np.int64)
    flips = lambda pauli: ((pauli == 1) | (pauli == 2)).astype(np.uint8)      # noqa: E731
    assert np.array_equal(det[:, 0], flips(v >> 2)) and np.array_equal(det[:, 1], flips(v & 3)) and np.array_equal(det[:, 2], flips(k1))


# ------------------------------------------------------------------------------------------------------------------- DEM

ONE_QUBIT = "R 0\nPAULI_CHANNEL_1(0.1, 0.2, 0.3) 0\nM 0\nDETECTOR rec[-1]\n"


def test_dem_one_qubit_channel():
    dem = circuit_to_dem(ONE_QUBIT, approximate_disjoint_errors=True)
    assert len(dem.errors) == 1
    p, dets, obs = dem.errors[0]
    assert (dets, obs) == ((0,), ()) and abs(p - (0.1 * 0.8 + 0.2 * 0.9)) < 1e-15
    with pytest.raises(NotImplementedError):
        circuit_to_dem(ONE_QUBIT)
    with pytest.raises(NotImplementedError):
        circuit_to_dem(ONE_QUBIT, approximate_disjoint_errors=False)
    with pytest.raises(NotImplementedError):
        Circuit(ONE_QUBIT).detector_error_model()
    assert Circuit(ONE_QUBIT, approximate_disjoint_errors=True).detector_error_model().errors == dem.errors
    assert Circuit(ONE_QUBIT).detector_error_model(approximate_disjoint_errors=True).errors == dem.errors
    c = Circuit(ONE_QUBIT, approximate_disjoint_errors=True)
    assert str(c) == ONE_QUBIT and c.num_detectors == 1
    with pytest.raises(NotImplementedError):
        c.detector_error_model(approximate_disjoint_errors=False)      # the argument overrides the instance's setting


def test_dem_threshold():
    assert circuit_to_dem(ONE_QUBIT, approximate_disjoint_errors=0.3).errors == circuit_to_dem(ONE_QUBIT, True).errors
    with pytest.raises(ValueError):
        circuit_to_dem(ONE_QUBIT, approximate_disjoint_errors=0.25)     # the Z component, 0.3, is above it
    with pytest.raises(ValueError):
        Circuit(ONE_QUBIT, approximate_disjoint_errors=0.25).detector_error_model()
    with pytest.raises(ValueError):
        circuit_to_dem(ONE_QUBIT, approximate_disjoint_errors=1.5)


def test_dem_y_error_is_exact_and_needs_no_flag():
    d = circuit_to_dem("R 0\nRX 1\nY_ERROR(0.125) 0 1\nM 0\nMX 1\nDETECTOR rec[-2]\nDETECTOR rec[-1]\n")
    assert d.errors == [(0.125, (0,), ()), (0.125, (1,), ())]
    d = circuit_to_dem("R 0\nH 0\nCX 0 1\nY_ERROR(0.25) 0\nCX 0 1\nH 0\nM 0 1\nDETECTOR rec[-2]\nDETECTOR rec[-1]\n".replace("R 0", "R 0 1"))
    assert d.errors == [(0.25, (0, 1), ())]                      # Y on the control: X spreads to the target, Z is seen as X after H


def test_dem_of_the_independent_equivalent_rewrite_equals_the_original():
    text = helpers.circuit_text(BB72)
    ref = circuit_to_dem(text)
    got = circuit_to_dem(cc_.independent_equivalent(text), approximate_disjoint_errors=True)
    assert (got.num_detectors, got.num_observables, got.num_errors) == (ref.num_detectors, ref.num_observables, ref.num_errors)
    assert [(d, o) for _, d, o in got.errors] == [(d, o) for _, d, o in ref.errors]          # the same rows in the same order
    pg, pr = np.array([e[0] for e in got.errors]), np.array([e[0] for e in ref.errors])
    rel = np.abs(pg - pr) / pr
    print("largest relative difference %.3g over %d mechanisms" % (rel.max(), len(pr)))
    assert rel.max() <= 1e-12


def test_dem_structure_cache_does_not_replay_channels():
    """Two channel circuits of one structure and different probabilities: the second must get its own priors, not the first one's
    replayed, and both must equal what the pass gives with the cache off."""
    base = helpers.circuit_text("bb72_custom_r0_p0.003")
    a, b = cc_.biased(base), cc_.biased(base, scale=2.5)
    dem_struct_cache_clear()
    da = circuit_to_dem(a, True)
    db = circuit_to_dem(b, True)
    assert dem_struct_cache_info()["size"] == 0                  # neither went through the cache
    assert [(d, o) for _, d, o in da.errors] == [(d, o) for _, d, o in db.errors]
    pa, pb = np.array([e[0] for e in da.errors]), np.array([e[0] for e in db.errors])
    # the channel terms of b are 2.5 times a's, the X_ERROR terms are the same: every prior grows or stays, most grow a lot
    assert np.all(pb >= pa) and np.mean(pb > 2.0 * pa) > 0.5
    # and the order of the two calls does not matter, bit for bit
    assert circuit_to_dem(b, True).errors == db.errors and circuit_to_dem(a, True).errors == da.errors
    # the small case in closed form, second circuit after the first
    assert abs(circuit_to_dem(ONE_QUBIT, True).errors[0][0] - 0.26) < 1e-15
    other = ONE_QUBIT.replace("0.1, 0.2, 0.3", "0.3, 0.05, 0.6")
    assert abs(circuit_to_dem(other, True).errors[0][0] - (0.3 * 0.95 + 0.05 * 0.7)) < 1e-15
    # Y_ERROR has one probability per instruction and does go through the replay
    y = "R 0\nY_ERROR(%s) 0\nM 0\nDETECTOR rec[-1]\n"
    assert circuit_to_dem(y % "0.125").errors == [(0.125, (0,), ())]
    assert circuit_to_dem(y % "0.375").errors == [(0.375, (0,), ())]
    assert dem_struct_cache_info()["hits"] >= 1


def test_plan_key_carries_the_setting():
    from quits_amd.decoder.plan_cache import _circuit_fingerprint
    text = cc_.biased(helpers.circuit_text("bb72_custom_r0_p0.003"))
    plain, flagged = _circuit_fingerprint(text), _circuit_fingerprint(Circuit(text, approximate_disjoint_errors=True))
    assert plain == _circuit_fingerprint(Circuit(text)) == hashlib.sha1(text.encode()).hexdigest()
    assert flagged != plain and flagged == _circuit_fingerprint(Circuit(text, approximate_disjoint_errors=1.0))
    assert _circuit_fingerprint(Circuit(text, approximate_disjoint_errors=0.5)) not in (plain, flagged)


def test_mirror_marginals_match_the_approximate_dem():
    """The reference alone: the mirror's samples of the biased bb72 circuit against the marginals of the approximate-disjoint DEM, at a
    size the mirror can afford.  The approximation's bias is of relative order p = 3e-3 against a sigma of 6 % relative here."""
    text = cc_.biased(helpers.circuit_text(BB72))
    B = 8192
    det, obs = fmc.sample(text, seed=2026, shot0=0, B=B)
    pd, po = dem_marginals(Circuit(text, approximate_disjoint_errors=True))
    for rate, pred in ((det.mean(axis=0), pd), (obs.mean(axis=0), po)):
        z = (rate - pred) / np.sqrt(np.maximum(pred * (1 - pred), 1e-12) / B)
        assert np.abs(z).max() < 5.0, (int(np.argmax(np.abs(z))), z.max(), z.min())


# ------------------------------------------------------------------------------------------------------------------- ABI

def test_abi_checks_the_channel_opcodes_before_touching_a_device():
    from quits_amd import _lib
    L = _lib.load()
    cc = frame.compile_circuit(cc_.biased(helpers.circuit_text(BB72)))

    def create(prog, thr=cc.thresholds, nq=cc.nq):
        prog = np.ascontiguousarray(prog, np.int32)
        thr = np.ascontiguousarray(thr, np.uint32)
        h = C.c_void_p()
        rc = L.qd_circuit_create(prog.ctypes.data_as(C.c_void_p), len(prog), nq, cc.nmeas, cc.ndet, cc.nobs,
                                 thr.ctypes.data_as(C.c_void_p), len(thr), cc.ring, 0, C.byref(h))
        msg = L.qd_last_error()
        if rc == 0:
            L.qd_circuit_destroy(h)
        return rc, msg
    ins, pc = {}, 0
    while pc < len(cc.program):
        op, n = int(cc.program[pc]), int(cc.program[pc + 1])
        ins.setdefault(op, pc)
        pc += frame._length(op, n)
    p1, p2 = ins[frame.OP_PC1], ins[frame.OP_PC2]
    # the compiled program passes every check; without a device the call then stops at hipSetDevice (-3), never at a check (-1)
    rc, msg = create(cc.program)
    assert rc in (0, -3), (rc, msg)
    if rc == -3:
        assert b"hipSetDevice" in msg
    nthr = len(cc.thresholds)
    for pc, K in ((p1, 3), (p2, 15)):
        bad = cc.program.copy()
        bad[pc + 2] = nthr - K + 1                               # the table's last entry is one past the thresholds
        rc, msg = create(bad)
        assert rc == -1 and b"runs past the end of the thresholds" in msg, (rc, msg)
        bad[pc + 2] = nthr - K                                   # the last place it fits: not a range error any more
        rc, msg = create(bad)
        assert rc == 0 or (b"runs past" not in msg and b"out of range" not in msg), (rc, msg)   # (created, on a GPU: the message is the last failure's)
    thr = cc.thresholds.copy()
    t0 = int(cc.program[p2 + 2])
    thr[t0 + 7] = thr[t0 + 6] - 1
    rc, msg = create(cc.program, thr=thr)
    assert rc == -1 and b"non-decreasing" in msg
    bad = cc.program.copy()
    bad[p2 + 5] = cc.nq                                          # second qubit of the first pair
    rc, msg = create(bad)
    assert rc == -1 and b"qubit out of range" in msg
    bad = cc.program.copy()
    bad[p2 + 5] = bad[p2 + 4]
    rc, msg = create(bad)
    assert rc == -1 and b"must differ" in msg
    bad = cc.program.copy()
    bad[p1 + 3] += 2
    assert b"multiple of 4" in create(bad)[1]
    assert create(cc.program[:p2 + 6])[0] == -1                  # PAULI_CHANNEL_2 cut inside its pairs: width check
    rc, msg = create(np.asarray([16, 0], np.int32))
    assert rc == -1 and b"unknown opcode" in msg


# ---------------------------------------------------------------------------------------------------------------- kernel

def test_both_sampler_kernels_use_no_scratch(tmp_path):
    """The frame sampler has two instantiations, without and with the channel opcodes; neither may spill to scratch."""
    from test_api import _resource_usage
    kern = [(n, sc) for n, sc in _resource_usage(tmp_path, "frame_sampler.hip") if "qd_frame_sample_kernel" in n]
    assert len(kern) == 2, kern
    assert all(sc == 0 for _, sc in kern), kern
