"""Soft outputs on the host: quits_amd/soft.py, the definition the kernels of csrc/soft.hip must equal, and what the public calls do on a
machine without a GPU."""
import math
import os

import numpy as np
import pytest

import helpers
from quits_amd import soft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fields_and_bins():
    assert soft.FIELDS == ("weight", "faults", "events", "iters", "post", "tail")
    assert soft.BINS == 1024


def test_fault_weights():
    w = soft.fault_weights([0.5, 1.0 / (1.0 + math.e), 1e-300, 0.003, 0.9])
    assert w.dtype == np.int32
    assert w[0] == 0
    assert w[1] == 65536
    # the clip: 2^16 log(1e300) = 45 270 665 is still inside +-(2^31 - 1), and so is every normal float64 prior (log below 709 nat); the
    # definition clips where (1 - p) / p leaves the float64 range, from the subnormal priors on
    assert w[2] == int(np.rint(math.log(1e300) * 65536.0)) == 45270665
    assert soft.fault_weights([5e-324])[0] == 2 ** 31 - 1
    assert w[3] == int(np.rint(math.log(0.997 / 0.003) * 65536.0))
    assert w[4] == int(np.rint(math.log((1.0 - 0.9) / 0.9) * 65536.0)) < 0
    assert soft.fault_weights([]).shape == (0,)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            soft.fault_weights([0.1, bad])


def test_bin_of():
    for shift in (0, 1, 5, 15, 40):
        for k in (1, 2, 7, 1023):
            assert soft.bin_of(k * 2 ** shift - 1, shift) == k - 1
            assert soft.bin_of(k * 2 ** shift, shift) == k
        assert soft.bin_of(0, shift) == 0
        assert soft.bin_of(-1, shift) == 0
        assert soft.bin_of(-2 ** 62, shift) == 0
        assert soft.bin_of(1023 * 2 ** shift, shift) == 1023
        assert soft.bin_of(1024 * 2 ** shift - 1, shift) == 1023
        assert soft.bin_of(1024 * 2 ** shift, shift) == 1023
        assert soft.bin_of(2 ** 62, shift) == 1023
    v = np.array([-5, 0, 3, 4, 4095, 4096, 10 ** 9])
    assert soft.bin_of(v, 2).tolist() == [0, 0, 0, 1, 1023, 1023, 1023]
    assert soft.bin_of(v, 2).dtype == np.int64


def test_selection_curve_eight_bins():
    hist = np.array([[10, 0, 5, 5, 0, 20, 0, 10],
                     [0, 0, 1, 0, 0, 4, 0, 5]])
    kept, errors, pL, sigma = soft.selection_curve(hist)
    assert kept.dtype == np.int64 and errors.dtype == np.int64
    assert kept.tolist() == [10, 10, 15, 20, 20, 40, 40, 50]
    assert errors.tolist() == [0, 0, 1, 1, 1, 5, 5, 10]
    assert (kept[-1], errors[-1]) == (hist[0].sum(), hist[1].sum())
    assert pL.tolist() == [0.0, 0.0, 1 / 15, 0.05, 0.05, 0.125, 0.125, 0.2]
    assert sigma[-1] == math.sqrt(0.2 * 0.8 / 50) and sigma[0] == 0.0
    kept, errors, pL, sigma = soft.selection_curve(np.array([[0, 0, 3], [0, 0, 1]]))
    assert np.isnan(pL[:2]).all() and np.isnan(sigma[:2]).all() and pL[2] == 1 / 3
    with pytest.raises(ValueError):
        soft.selection_curve(np.zeros((3, 8), int))


def test_soft_mirror_three_windows_five_shots():
    OSD, CONV, INEXACT, ZERO = 1 << 17, 1 << 16, 1 << 15, 1 << 19
    weights = np.array([10, -3, 2 ** 31 - 1, 7, -(2 ** 31 - 1), 1], dtype=np.int64)
    corr = np.array([[0, 0, 0, 0, 0, 0],
                     [1, 1, 0, 0, 0, 0],
                     [0, 0, 1, 1, 0, 0],
                     [1, 1, 1, 1, 1, 1],
                     [0, 0, 0, 0, 1, 0]], dtype=np.uint8)
    det = np.array([[0, 0, 0, 0],
                    [1, 0, 0xFE, 0xFF],
                    [1, 1, 1, 1],
                    [2, 4, 8, 16],
                    [3, 0, 0, 0]], dtype=np.uint8)
    st0 = np.array([ZERO | CONV, 5 | CONV, 20 | OSD | (7 << 20), 0x3FFF | OSD | (0xFFF << 20), 3 | CONV | INEXACT], dtype=np.int64)
    st0 = st0.astype(np.uint32).view(np.int32)               # (0xFFF << 20 sets the sign bit of the int32 word)
    st1 = np.array([1 | CONV, 20 | OSD | (1 << 20), 2 | CONV, 20 | OSD | (100 << 20), 0x7FFFF & ~0x3FFF & ~OSD], dtype=np.int32)
    st2a = np.array([4 | CONV, 4 | CONV], dtype=np.int32)     # window 2 arrives in two pieces, as the single-stream driver's chunks do
    st2b = np.array([20 | OSD | (3 << 20), 6 | CONV, 20 | OSD], dtype=np.int32)
    got = soft.soft_mirror(corr, det, [(0, st0), (1, st1), (2, st2a), (2, st2b)], weights)
    want = np.array([[0, 0, 0, 0 + 1 + 4, 0, 0],
                     [7, 2, 2, 5 + 20 + 4, 1, 1],
                     [2 ** 31 - 1 + 7, 2, 4, 20 + 2 + 20, 2, 7 + 3],
                     [10 - 3 + 7 + 1, 6, 0, 0x3FFF + 20 + 6, 2, 0xFFF + 100],
                     [-(2 ** 31 - 1), 1, 1, 3 + 0 + 20, 1, 0]], dtype=np.int64)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    # the order of the windows does not matter, the order inside a window does
    again = soft.soft_mirror(corr, det, [(2, st2a), (1, st1), (2, st2b), (0, st0)], weights)
    assert np.array_equal(again, want)
    with pytest.raises(ValueError):
        soft.soft_mirror(corr, det, [(0, st0), (1, st1[:4])], weights)
    with pytest.raises(ValueError):
        soft.soft_mirror(corr, det, [(0, st0)], weights[:5])


def test_histogram_matches_bin_of():
    rec = np.array([[100, 3, 2, 40, 0, 0], [-7, 0, 0, 1, 0, 0], [5000, 9, 8, 60, 3, 12285]], dtype=np.int64)
    shifts = [2, 0, 0, 1, 0, 4]
    h = soft.histogram(rec, shifts, fail=[False, False, True])
    assert h.shape == (6, 2, 1024) and (h[:, 0].sum(axis=1) == 3).all() and (h[:, 1].sum(axis=1) == 1).all()
    assert h[0, 0, 25] == 1 and h[0, 0, 0] == 1 and h[0, 0, 1023] == 1 and h[0, 1, 1023] == 1
    assert h[5, 1, 12285 >> 4] == 1
    assert soft.histogram(rec, shifts)[:, 1].sum() == 0


def test_default_shifts_depend_on_their_arguments_alone():
    pri = np.full(2592, 0.003)
    w = soft.fault_weights(pri)
    a = soft.default_shifts(w, pri, 648, 6, 20)
    b = soft.default_shifts(w.copy(), pri.copy(), 648, 6, 20)
    assert a.dtype == np.int32 and a.shape == (6,) and np.array_equal(a, b)
    expect = 4.0 * float(np.sum(pri * w))
    assert (int(math.ceil(expect)) >> int(a[0])) <= 1023 and (a[0] == 0 or (int(math.ceil(expect)) >> int(a[0] - 1)) > 1023)
    assert a[1] == 2 and a[2] == 0           # 2592 faults: bins of 4; 648 detectors fit as they are
    assert a[3] == 0 and a[4] == 0           # 120 iterations
    assert a[5] == 5                         # 6 * 4095 = 24570 -> bins of 32
    assert soft.default_shifts(w, pri, 648, 6, 16383)[3] == 7
    assert soft.default_shifts(w, pri, 5000, 6, 20)[2] == 3
    with pytest.raises(ValueError):
        soft.default_shifts(w, pri[:5], 648, 6, 20)


def test_post_selection_result_reads_the_curve():
    from quits_amd.simulation import PostSelectionResult
    rec = np.zeros((100, 6), dtype=np.int64)
    rec[:, 2] = np.arange(100)               # events 0 .. 99, the ten largest fail
    fail = np.arange(100) >= 90
    shifts = [0, 0, 1, 0, 0, 0]
    counts = np.zeros(12, dtype=np.int64)
    counts[0], counts[1] = 100, 10
    res = PostSelectionResult.from_counts(counts, shifts, soft.histogram(rec, shifts, fail))
    assert (res.shots, res.errors, res.pL) == (100, 10, 0.1)
    edge, kept, errors, pL, sigma = res.curve("events")
    assert edge[0] == 1 and edge[1] == 3 and (kept[-1], errors[-1]) == (100, 10)
    assert kept[0] == 2 and kept[44] == 90 and errors[44] == 0 and errors[45] == 2
    at = res.at_rejection("events", 0.1)
    assert at == {"threshold": 89, "kept": 90, "errors": 0, "pL": 0.0, "sigma": 0.0, "rejected": 0.1}
    assert res.at_rejection("events", 0.0)["kept"] == 100
    assert res.at_rejection("events", 0.095)["kept"] == 90          # whole bins: at least the fraction asked for
    assert res.at_rejection("post", 0.5)["threshold"] is None       # every shot sits in bin 0: nothing can be kept
    assert res.at_rejection(2, 1.0)["kept"] == 0
    with pytest.raises(ValueError):
        res.curve("nonsense")
    bad = soft.histogram(rec, shifts, fail)
    bad[3, 0, 0] -= 1
    with pytest.raises(ValueError):
        PostSelectionResult.from_counts(counts, shifts, bad)


def test_no_device_is_an_error_not_a_fallback(monkeypatch):
    import torch
    from quits_amd.decoder import decode_dem_soft_outputs, sliding_window_soft_outputs
    from quits_amd.simulation import get_postselected_pL
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)         # (what a machine without a GPU reports)
    cd = helpers.code("bb72")
    text = helpers.circuit_text("bb72_custom_r6_p0.003")
    with pytest.raises(RuntimeError, match="no HIP device"):
        get_postselected_pL(text, cd["hz"], cd["lz"], 3, 1, 1000)
    with pytest.raises(RuntimeError, match="no HIP device"):
        sliding_window_soft_outputs(np.zeros((4, 8 * 36), np.uint8), text, cd["hz"], cd["lz"], 3, 1)
    with pytest.raises(RuntimeError, match="no HIP device"):
        decode_dem_soft_outputs(text, np.zeros((4, 288), np.uint8))


def test_symbols_declared_exported_and_gated():
    from quits_amd import _lib
    with open(os.path.join(ROOT, "include", "quits_amd.h")) as fh:
        header = fh.read()
    for name in ("qd_soft_fold", "qd_soft_weigh", "qd_soft_tally"):
        assert "int %s(" % name in header
        assert name in _lib.EXPORTS
    assert "#define QD_SOFT_FIELDS 6" in header and "#define QD_SOFT_BINS 1024" in header
    assert (_lib.SOFT_FIELDS, _lib.SOFT_BINS) == (len(soft.FIELDS), soft.BINS)
    L = _lib.load()
    assert L.qd_version() >= 116 and _lib.require_soft(L) is L


def test_bad_arguments_and_empty_batches_need_no_device():
    """B = 0 is accepted whatever else is passed; bad arguments are QD_EINVAL with a message, before any device call."""
    import ctypes as C
    from quits_amd import _lib
    L = _lib.require_soft(_lib.load())
    sh = (C.c_int32 * 6)(0, 0, 0, 0, 0, 0)
    assert L.qd_soft_fold(None, 0, None, 6, None) == 0
    assert L.qd_soft_weigh(None, 0, 0, None, None, 0, 0, 0, None, 6, None) == 0
    assert L.qd_soft_tally(None, 6, 0, sh, None, None, None) == 0
    assert L.qd_soft_fold(None, -1, None, 6, None) == -1 and b"negative" in L.qd_last_error()
    assert L.qd_soft_fold(64, 5, 64, 5, None) == -1 and b"soft_stride" in L.qd_last_error()
    assert L.qd_soft_fold(None, 5, 64, 6, None) == -1 and b"null" in L.qd_last_error()
    assert L.qd_soft_weigh(64, 1, 33, 64, 64, 4, 4, 5, 64, 6, None) == -1 and b"stride_words" in L.qd_last_error()
    assert L.qd_soft_weigh(64, 2, 33, 64, 64, 3, 4, 5, 64, 6, None) == -1 and b"det_stride" in L.qd_last_error()
    assert L.qd_soft_weigh(64, 2, -1, 64, 64, 4, 4, 5, 64, 6, None) == -1 and b"negative" in L.qd_last_error()
    assert L.qd_soft_weigh(None, 2, 33, 64, 64, 4, 4, 5, 64, 6, None) == -1 and b"null" in L.qd_last_error()
    assert L.qd_soft_weigh(64, 2, 33, 64, 64, 4, 4, 5, 64, 3, None) == -1 and b"soft_stride" in L.qd_last_error()
    assert L.qd_soft_tally(64, 6, 5, None, None, 64, None) == -1 and b"shifts" in L.qd_last_error()
    assert L.qd_soft_tally(64, 6, 5, (C.c_int32 * 6)(0, 0, 63, 0, 0, 0), None, 64, None) == -1 and b"shift" in L.qd_last_error()
    assert L.qd_soft_tally(64, 6, 5, (C.c_int32 * 6)(0, -1, 0, 0, 0, 0), None, 64, None) == -1 and b"shift" in L.qd_last_error()
    assert L.qd_soft_tally(None, 6, 5, sh, None, 64, None) == -1 and b"null" in L.qd_last_error()
    assert L.qd_soft_tally(64, 4, 5, sh, None, 64, None) == -1 and b"soft_stride" in L.qd_last_error()
