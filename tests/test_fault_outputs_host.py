"""Fault-level outputs, the host side: where the windows' committed columns lie (base.commit_ranges), the arithmetic of a
FaultSpectrumResult, `predict`'s new arguments, and the new exports' place in the binding."""
import numpy as np
import pytest

import helpers
from quits_amd.decoder.base import commit_ranges, detector_error_model_to_matrix, spacetime, window_count
from quits_amd.dem import Circuit

CASES = [("bb72_custom_r6_p0.003", "bb72", 6), ("bb144_custom_r12_p0.003", "bb144", 12), ("hgp225_cardinal_r3_p0.01", "hgp225", 3)]


@pytest.mark.parametrize("name,code,R", CASES)
def test_commit_ranges_partition_the_faults(name, code, R):
    """For every (W, F) of the fixture: range k starts where range k - 1 ends, is as wide as spacetime's observable matrix k, the last
    window commits all its columns, and together the ranges are [0, n).  The committed columns of window k are the model's own columns
    col0 .. col0 + ncommit - 1: L_k is that slice of the observable matrix."""
    z = helpers.windows_npz(name)
    circ = Circuit(helpers.circuit_text(name))
    hz = helpers.code(code)["hz"]
    H, L, _ = detector_error_model_to_matrix(circ)
    n = H.shape[1]
    tags = sorted({k.split("_")[0] for k in z.files if k.startswith("W")})
    assert tags
    for tag in tags:
        W, F = int(tag[1:tag.index("F")]), int(tag[tag.index("F") + 1:])
        ncr = window_count(R, W, F)[0]
        checks, commits, priors, updates = spacetime(circ, hz, W, F, ncr)
        ranges = commit_ranges(commits)
        assert len(ranges) == ncr + 1
        at = 0
        for k, (col0, ncommit) in enumerate(ranges):
            assert col0 == at and ncommit == commits[k].shape[1] and 0 < ncommit <= checks[k].shape[1]
            assert helpers.same_sparse(commits[k], L[:, col0:col0 + ncommit])
            at += ncommit
        assert at == n
        assert ranges[-1][1] == checks[-1].shape[1]
        assert ranges == commit_ranges([helpers.csc_from(z, "%s_L%d" % (tag, k)) for k in range(ncr + 1)])


def test_commit_ranges_of_the_issue_fixtures():
    """BB72 r6 (3, 1) commits 324, 360, 360, 360, 360, 828 columns; HGP r3 (3, 1) 1188, 1296, 2925 (offsets 1188 and 2484: off the word grid)."""
    got = [nc for _, nc in commit_ranges([w["L"] for w in helpers.window_set("bb72_custom_r6_p0.003", 3, 1)])]
    assert got == [324, 360, 360, 360, 360, 828]
    hgp = commit_ranges([w["L"] for w in helpers.window_set("hgp225_cardinal_r3_p0.01", 3, 1)])
    assert hgp == [(0, 1188), (1188, 1296), (2484, 2925)] and 1188 % 32 and 2484 % 32
    assert commit_ranges([]) == []


def test_fault_spectrum_result_arithmetic():
    from quits_amd.simulation import FaultSpectrumResult
    hist = np.zeros((3, 256), np.int64)
    hist[0, [0, 3, 4, 255]] = [10, 6, 4, 1]
    hist[1, [3, 4, 255]] = [1, 2, 1]
    hist[2, [6, 9]] = [2, 1]
    r = FaultSpectrumResult.from_counts(hist, [21, 4, 2, 1], (6, (1 << 32) + 5), seed=3, batch=64)
    assert (r.shots, r.errors, r.residual_shots, r.failing_residual_shots) == (21, 4, 2, 1)
    assert r.pL == 4 / 21 and r.lightest == (6, (1 << 32) + 5) and r.seed == 3
    assert r.shots_by_faults.shape == r.errors_by_faults.shape == r.residual_weight_hist.shape == (256,)
    assert r.shots_by_faults.sum() == r.shots and r.errors_by_faults.sum() == r.errors
    assert r.residual_weight_hist.sum() == r.errors - r.failing_residual_shots
    f = r.failure_fraction()
    assert f.shape == (256,) and f[0] == 0.0 and f[3] == 1 / 6 and f[4] == 0.5 and f[255] == 1.0
    assert np.isnan(f[1]) and np.isnan(f[254]) and np.isnan(f).sum() == 252
    empty = FaultSpectrumResult.from_counts(np.zeros((3, 256), np.int64), [0, 0, 0, 0], None)
    assert empty.shots == 0 and np.isnan(empty.pL) and empty.lightest is None and np.isnan(empty.failure_fraction()).all()
    hist[2, 9] = 2                                   # a residual more than there are failing shots with a zero residual
    with pytest.raises(ValueError, match="disagree"):
        FaultSpectrumResult.from_counts(hist, [21, 4, 2, 1], None)


def test_predict_takes_corrections_arguments_and_does_not_need_them():
    from quits_amd.__main__ import _parser
    base = ["predict", "--dem", "m.dem", "--in", "s.b8", "--in_format", "b8", "--out", "p.01", "--out_format", "01"]
    a = _parser().parse_args(base)
    assert a.corrections_out is None and a.corrections_format == "b8"
    a = _parser().parse_args(base + ["--corrections_out", "c.hits", "--corrections_format", "hits"])
    assert a.corrections_out == "c.hits" and a.corrections_format == "hits"
    assert _parser().parse_args(base + ["--corrections_out", "c.b8"]).corrections_format == "b8"
    with pytest.raises(SystemExit):
        _parser().parse_args(base + ["--corrections_out", "c", "--corrections_format", "dets"])


def test_new_names_are_exported_and_bound():
    import inspect
    import quits_amd.decoder as d
    from quits_amd import _lib, simulation
    for name in ("sliding_window_corrections", "decode_dem_corrections"):
        assert name in d.__all__ and callable(getattr(d, name))
    sig = inspect.signature(d.sliding_window_corrections)
    assert list(sig.parameters) == ["zcheck_samples", "circuit", "hz", "lz", "W", "F", "max_iter", "osd_order", "bp_method", "schedule",
                                    "osd_method", "lsd_method", "lsd_order"]
    assert list(inspect.signature(d.decode_dem_corrections).parameters) == list(inspect.signature(d.decode_dem).parameters)
    ref = inspect.signature(simulation.get_circuit_mem_pL).parameters
    sig = inspect.signature(simulation.get_fault_spectrum).parameters
    five = ["max_iter", "osd_order", "bp_method", "schedule", "osd_method"]
    assert list(sig)[:11] == list(ref)[:11] == ["circuit", "hz", "lz", "W", "F", "num_trials"] + five
    assert [sig[k].default for k in five] == [ref[k].default for k in five]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("seed", "batch", "shard"))
    for name in ("qd_sample_dem_faults", "qd_commit_bits", "qd_fault_stats_batch"):
        assert name in _lib.EXPORTS
    L = _lib.load()
    assert L.qd_version() >= 110 and _lib.require_faults(L) is L


def test_commit_bits_and_fault_stats_refuse_bad_arguments_without_a_gpu():
    """Argument validation comes before any launch: QD_EINVAL with text; empty calls are accepted whatever the pointers."""
    import ctypes as C
    from quits_amd import _lib
    L = _lib.load()
    null, one = C.c_void_p(0), C.c_void_p(64)
    assert L.qd_commit_bits(null, 0, 0, 0, null, 0, 0, null) == 0
    assert L.qd_commit_bits(one, 1, 0, 5, one, 1, 7, null) == 0                  # nbits = 0: a no-op
    assert L.qd_commit_bits(one, 1, 33, 5, one, 4, 0, null) == -1 and b"err_stride_words" in L.qd_last_error()
    assert L.qd_commit_bits(one, 2, 33, 5, one, 2, 32, null) == -1 and b"out_stride_words" in L.qd_last_error()
    assert L.qd_commit_bits(one, 2, -1, 5, one, 2, 0, null) == -1
    assert L.qd_commit_bits(one, 2, 8, 5, one, 2, -3, null) == -1
    assert L.qd_commit_bits(null, 2, 8, 5, one, 2, 0, null) == -1 and b"null" in L.qd_last_error()
    assert L.qd_fault_stats_batch(null, null, 0, 0, null, 0, 0, null, 0, 0, null, null, null, null) == 0
    assert L.qd_fault_stats_batch(one, one, 1, 33, one, 4, 4, one, 8, 0, one, one, one, null) == -1 and b"stride_words" in L.qd_last_error()
    assert L.qd_fault_stats_batch(one, one, 2, 33, one, 3, 4, one, 8, 0, one, one, one, null) == -1 and b"res_stride" in L.qd_last_error()
    assert L.qd_fault_stats_batch(one, one, 2, 33, one, 4, 4, one, 8, 1 << 40, one, one, one, null) == -1 and b"2^40" in L.qd_last_error()
    assert L.qd_fault_stats_batch(one, one, 2, 33, one, 4, 4, null, 8, 0, one, one, one, null) == -1 and b"null" in L.qd_last_error()
    assert L.qd_sample_dem_faults(null, null, null, 0, 0, null, 0, null, 0, null, 0, null, 0, null) == 0
    assert L.qd_sample_dem_faults(null, null, null, 0, 0, null, -1, null, 0, null, 0, null, 0, null) == -1
    assert L.qd_sample_dem_faults(null, null, null, 0, 0, null, 4, one, 8, one, 8, null, 0, null) == -1 and b"fault" in L.qd_last_error()
