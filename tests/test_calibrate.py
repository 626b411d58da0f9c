"""Fitting a model's priors to detector samples, host side (quits_amd/calibrate.py): the fit on exact moments, the numpy mirror of the counting
kernels against a per-shot loop, the jackknife on the oracle's sample stream, the .dem round trip, clipping and unidentified columns, the
kernels' resource usage, the library's argument checks and the command line through the mirror.  No GPU."""
import ctypes
import json

import numpy as np
import pytest
from scipy.sparse import csc_matrix

import helpers
from quits_amd import calibrate as qc
from quits_amd.dem import Circuit

_MODELS = {}


def model(name):
    """(H, L, priors) of a fixture circuit, computed once."""
    if name not in _MODELS:
        from quits_amd.decoder.base import detector_error_model_to_matrix
        H, L, p = detector_error_model_to_matrix(Circuit(helpers.circuit_text(name)).detector_error_model())
        _MODELS[name] = (csc_matrix(H), csc_matrix(L), np.asarray(p, dtype=np.float64))
    return _MODELS[name]


def from_columns(cols, ndet, nobs=2):
    """(H, L) with the given detector lists as columns; column j flips observable j % nobs."""
    rows = np.array([d for c in cols for d in c])
    at = np.repeat(np.arange(len(cols)), [len(c) for c in cols])
    H = csc_matrix((np.ones(len(rows), np.uint8), (rows, at)), shape=(ndet, len(cols)))
    L = csc_matrix((np.ones(len(cols), np.uint8), (np.arange(len(cols)) % nobs, np.arange(len(cols)))), shape=(nobs, len(cols)))
    return H, L


def crafted_12():
    """12 detectors; a nested chain {0} < {0, 1} < {0, 1, 2}."""
    return from_columns([[0], [0, 1], [0, 1, 2], [3, 4], [5, 6, 7, 8], [9, 10, 11], [2, 9], [4]], 12)


CRAFTED_70 = [[0], [0, 1], [0, 1, 2],                                           # a chain, weights 1 .. 3
              [10, 11], [10, 11, 12, 13], list(range(10, 17)),                  # a second one through weights 2, 4, 7
              list(range(20, 25)), list(range(25, 31)), list(range(31, 39)), list(range(40, 49)), list(range(50, 60)),     # 5, 6, 8, 9, 10
              [0, 69], [63, 64], [3, 64, 65], [67], [5, 30, 45, 55, 62, 63, 64, 66, 69]]


def crafted_70():
    """70 detectors: columns of every weight 1 .. 10, two nested chains, a column on detectors 0 and 69, columns across detector 64, detector
    68 in no column."""
    assert sorted(set(len(c) for c in CRAFTED_70)) == list(range(1, 11)) and all(68 not in c for c in CRAFTED_70)
    return from_columns(CRAFTED_70, 70)


def exact_moments(H, priors, table):
    """z[ptr[j] + t - 1] = the product of 1 - 2 p over the columns with an odd overlap with the detectors t selects of column j.  The columns
    that meet e_j are grouped by what they share with it (a mask a over e_j): the overlap with t is odd iff |a & t| is."""
    Hd = csc_matrix(H).toarray().astype(np.int64)
    lam = -np.log1p(-2.0 * priors)
    z = np.zeros(table.total)
    odd = {}
    for j in range(table.n):
        d = table.detectors(j)
        s = len(d)
        if s not in odd:
            t = np.arange(1 << s)
            odd[s] = np.array([[bin(x & y).count("1") & 1 for y in t] for x in t[1:]], dtype=np.float64)
        shared = (1 << np.arange(s)) @ Hd[d]
        near = np.flatnonzero(shared)
        z[table.ptr[j]:table.ptr[j + 1]] = np.exp(-(odd[s] @ np.bincount(shared[near], weights=lam[near], minlength=1 << s)))
    return z


def brute_counts(samples, table):
    out = np.zeros(table.total, np.int64)
    for shot in np.asarray(samples):
        for j in range(table.n):
            d = table.detectors(j)
            for t in range(1, 1 << len(d)):
                out[table.ptr[j] + t - 1] += sum(int(shot[d[i]]) & 1 for i in range(len(d)) if (t >> i) & 1) & 1
    return out


def z_conditions(res, priors):
    """The jackknife's z = (raw - p) / stderr against Student's t with 15 degrees of freedom: rms sqrt(15 / 13) = 1.07, P(|t| > 3) = 0.9 %."""
    z = (res.raw - priors) / res.stderr
    rms, share, top, mean = float(np.sqrt((z ** 2).mean())), float((np.abs(z) > 3).mean()), float(np.abs(z).max()), float(z.mean())
    print("rms z %.3f  |z| > 3: %.2f %%  max |z| %.2f  mean z %+.3f  median rel err %.2f %%" %
          (rms, 100 * share, top, mean, 100 * float(np.median(np.abs(res.raw / priors - 1)))))
    assert 0.9 <= rms <= 1.25
    assert share <= 0.02
    assert top <= 6.5
    assert abs(mean) <= 0.1
    assert len(res.clipped) == 0 and len(res.unidentified) == 0


@pytest.mark.parametrize("name,shape,top,most", [("bb72_custom_r6_p0.003", (288, 2592), 6, None), ("bb72_custom_r2_alldet_p0.003", (216, 5400), 9, 227)])
def test_exact_moments_give_back_the_priors(name, shape, top, most):
    H, L, p = model(name)
    table = qc.hyperedge_table(H, L)
    assert H.shape == shape and table.weight.max() == top and table.weight.min() >= 1
    if most is not None:
        assert np.diff(table.sup_ptr).max() == most
    z = exact_moments(H, p, table)
    raw, unid = qc.fit_moments(z, table, p)
    assert not unid.any()
    assert np.abs(raw / p - 1).max() <= 1e-9
    # ... and through real-valued counts of a nominal N
    N = 1 << 20
    res = qc.fit_priors((1.0 - z) * (N / 2.0), [N], table, p, min_prior=0.0)
    assert np.abs(res.raw / p - 1).max() <= 1e-9 and np.array_equal(res.priors, res.raw) and np.isnan(res.stderr).all()


def test_superset_lists():
    H, L = crafted_12()
    t = qc.hyperedge_table(H, L)
    assert [list(t.supersets(j)) for j in range(t.n)] == [[1, 2], [2], [], [], [], [], [], [3]]
    assert list(t.ptr) == [0, 1, 4, 11, 14, 29, 36, 39, 40] and t.total == 40
    assert list(t.detectors(6)) == [2, 9]
    with pytest.raises(NotImplementedError, match=r"column 1 has weight 11"):
        qc.hyperedge_table(*from_columns([[0], list(range(11))], 12))
    with pytest.raises(ValueError, match="same detectors"):
        qc.hyperedge_table(*from_columns([[0, 1], [2], [1, 0]], 3))
    with pytest.raises(ValueError, match="flips no detector"):
        qc.hyperedge_table(csc_matrix(np.array([[1, 0], [0, 0]], np.uint8)))


def test_mirror_equals_a_per_shot_loop():
    H, L = crafted_12()
    table = qc.hyperedge_table(H, L)
    rng = np.random.default_rng(5)
    samples = rng.random((50, 12)) < 0.4
    counts, shots = qc.parity_counts_mirror(samples, table, blocks=4)
    assert list(shots) == [12, 13, 12, 13] and counts.shape == (4, 40)
    edges = qc.block_edges(50, 4)
    for k in range(4):
        assert np.array_equal(counts[k], brute_counts(samples[edges[k]:edges[k + 1]], table))
    # the low bit counts; more blocks than shots are capped
    c2, s2 = qc.parity_counts_mirror(samples.astype(np.uint8) + 2, table, blocks=4)
    assert np.array_equal(c2, counts)
    c3, s3 = qc.parity_counts_mirror(samples[:3], table, blocks=16)
    assert list(s3) == [1, 1, 1] and np.array_equal(c3.sum(axis=0), brute_counts(samples[:3], table))
    # the planes: 130 shots, pad bits zero
    planes = qc.bit_planes_mirror(rng.random((130, 12)) < 0.5)
    assert planes.shape == (12, 3) and planes.dtype == np.uint64 and not (planes[:, 2] >> np.uint64(2)).any()


def test_jackknife_on_the_oracle_stream():
    """bb72_custom_r6_p0.003, oracle.sample_dem seed 1, shots 0 .. 2^18 - 1, 16 blocks.  A numpy prototype of the definition measured rms z
    1.08, 0.77 % beyond 3, max 4.78, mean -0.03."""
    import oracle as orc
    H, L, p = model("bb72_custom_r6_p0.003")
    det = orc.sample_dem(H, L, p, 1, 0, 1 << 18)[0]
    res = qc.estimate_priors_mirror((H, L, p), det, blocks=16)
    assert res.shots == 1 << 18 and res.counts.shape == (16, res.table.total) and list(res.block_shots) == [1 << 14] * 16
    z_conditions(res, p)


def test_round_trip_through_dem_text():
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.dem import parse_dem
    H, L, p = model("bb72_custom_r6_p0.003")
    table = qc.hyperedge_table(H, L)
    rng = np.random.default_rng(11)
    fitted = p * np.exp(rng.uniform(-1, 1, len(p)))
    res = qc.fit_priors((1.0 - exact_moments(H, fitted, table)) * 512.0, [1024], table, p, min_prior=0.0)
    H2, L2, p2 = detector_error_model_to_matrix(parse_dem(res.dem_text()))
    assert helpers.same_sparse(H, H2) and helpers.same_sparse(L, L2)
    assert np.array_equal(p2, res.priors)
    H3, L3, p3 = res.matrices()
    assert helpers.same_sparse(H, H3) and helpers.same_sparse(L, L3) and np.array_equal(p3, res.priors)
    assert not np.array_equal(detector_error_model_to_matrix(parse_dem(res.dem_text(digits=6)))[2], res.priors)


def test_clipping_and_unidentified_columns():
    H, L = from_columns([[0], [1], [1, 2], [2], [3]], 4)
    model_p = np.array([0.01, 0.02, 0.03, 0.04, 0.05])
    det = np.zeros((64, 4), np.uint8)
    det[::2, 1] = 1                                      # detector 1 fires in exactly half of the shots: its moment is 0
    det[:5, 2] = 1
    det[60:, 3] = 1
    res = qc.estimate_priors_mirror((H, L, model_p), det, blocks=16)
    assert list(res.clipped) == [0] and res.raw[0] == 0.0 and res.priors[0] == 0.5 / 64
    assert list(res.unidentified) == [1, 2, 3]           # {1}, {1, 2} and, below an unidentified superset, {2}
    assert np.array_equal(res.priors[[1, 2, 3]], model_p[[1, 2, 3]])
    assert res.priors[4] == res.raw[4] and abs(res.raw[4] - 4 / 64) < 1e-12
    wide = qc.estimate_priors_mirror((H, L, model_p), det, blocks=16, min_prior=0.1)
    assert list(wide.clipped) == [0, 4] and wide.priors[0] == 0.1 and wide.priors[4] == 0.1
    with pytest.raises(ValueError, match="no shots"):
        qc.estimate_priors_mirror((H, L, model_p), det[:0])
    with pytest.raises(ValueError, match="detectors"):
        qc.estimate_priors_mirror((H, L, model_p), det[:, :3])


def test_unidentified_supersets_pass_on_their_model_lambda():
    """{0, 1} is unidentified (a zero moment on its own mask 3 only); {0} below it subtracts the model's lambda of {0, 1}."""
    H, L = from_columns([[0], [0, 1]], 2)
    table = qc.hyperedge_table(H, L)
    p = np.array([0.05, 0.1])
    z = exact_moments(H, p, table)
    z[table.ptr[1] + 2] = 0.0
    raw, unid = qc.fit_moments(z, table, p)
    assert list(unid) == [True, True]                    # ({0} has a proper superset with a bad moment)
    z = exact_moments(H, p, table)
    raw, unid = qc.fit_moments(z, table, np.array([0.2, 0.3]))
    assert not unid.any() and np.abs(raw / p - 1).max() < 1e-12          # the model's priors never enter an identified fit


def test_new_kernels_use_no_scratch(tmp_path):
    from test_api import _resource_usage
    kern = _resource_usage(tmp_path, "calibrate.hip")
    assert sorted(n for n, _ in kern) == sorted(n for n, _ in kern if "qd_bit_planes_kernel" in n or "qd_parity_counts_kernel" in n) and len(kern) == 2
    assert all(sc == 0 for _, sc in kern), kern


def test_library_refuses_bad_tables_before_any_launch():
    from quits_amd import _lib
    L = _lib.require_calibrate(_lib.load())
    h = ctypes.c_void_p()

    def create(ndet, cols):
        cp = np.zeros(len(cols) + 1, np.int64)
        cp[1:] = np.cumsum([len(c) for c in cols])
        cd = np.array([d for c in cols for d in c] + [0], np.int32)
        return L.qd_calib_create(ndet, len(cols), cp.ctypes.data, cd.ctypes.data, 0, ctypes.byref(h))

    assert create(12, [[0], list(range(11))]) == _lib.QD_ECAPACITY and b"column 1 has weight 11" in L.qd_last_error() and not h
    assert create(4, [[0], [1, 4]]) == -1 and b"detector 4 is outside 0 .. 3" in L.qd_last_error()
    assert create(4, [[0], [2, 1]]) == -1 and b"do not ascend" in L.qd_last_error()
    assert create(4, [[0], []]) == -1 and b"empty" in L.qd_last_error()
    assert L.qd_calib_create(4, 1, None, None, 0, ctypes.byref(h)) == -1 and b"null" in L.qd_last_error()
    assert L.qd_calib_create(-1, 0, None, None, 0, ctypes.byref(h)) == -1 and b"negative" in L.qd_last_error()
    assert L.qd_parity_counts(None, None, 0, 0, None, None) == -1 and b"null column table" in L.qd_last_error()
    assert L.qd_bit_planes(None, 4, 4, -1, None, 1, None) == -1 and b"negative" in L.qd_last_error()
    assert L.qd_bit_planes(None, 3, 4, 1, None, 1, None) == -1 and b"in_stride" in L.qd_last_error()
    assert L.qd_bit_planes(None, 4, 4, 65, None, 1, None) == -1 and b"plane_stride" in L.qd_last_error()
    assert L.qd_bit_planes(None, 4, 4, 64, None, 1, None) == -1 and b"null" in L.qd_last_error()
    assert L.qd_bit_planes(None, 4, 4, 0, None, 0, None) == 0


def test_command_line_through_the_mirror(tmp_path, capsys):
    from quits_amd.__main__ import main
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.dem import DetectorErrorModel, dem_to_text, parse_dem
    from quits_amd.samples import write_shots
    H, L = crafted_12()
    p = np.linspace(0.02, 0.09, H.shape[1])
    table = qc.hyperedge_table(H, L)
    dem = DetectorErrorModel([(float(p[j]), tuple(int(d) for d in table.detectors(j)), (j % 2,)) for j in range(table.n)], 12, 2)
    (tmp_path / "m.dem").write_text(dem_to_text(dem))
    rng = np.random.default_rng(3)
    det = ((rng.random((4096, table.n)) < p).astype(np.int64) @ H.T.toarray() & 1).astype(np.uint8)
    write_shots(str(tmp_path / "s.b8"), np.concatenate([det, np.zeros((4096, 2), np.uint8)], axis=1), "b8")
    rc = main(["calibrate", "--dem", str(tmp_path / "m.dem"), "--in", str(tmp_path / "s.b8"), "--in_format", "b8", "--in_includes_appended_observables",
               "--out", str(tmp_path / "f.dem"), "--stderr_out", str(tmp_path / "f.txt"), "--blocks", "8", "--mirror"])
    assert rc == 0
    out = json.loads(capsys.readouterr().out)
    assert out["shots"] == 4096 and out["columns"] == 8 and out["clipped"] == 0 and out["unidentified"] == 0 and out["max_rel_stderr"] < 1.0
    ref = qc.estimate_priors_mirror((H, L, p), det, blocks=8)
    H2, L2, p2 = detector_error_model_to_matrix(parse_dem((tmp_path / "f.dem").read_text()))
    assert helpers.same_sparse(H, H2) and helpers.same_sparse(L, L2) and np.array_equal(p2, ref.priors)
    assert np.abs(ref.raw - p).max() < 0.03
    lines = (tmp_path / "f.txt").read_text().split("\n")[:-1]
    assert len(lines) == 8 and all(ln.endswith(" ok") for ln in lines) and float(lines[3].split()[1]) == ref.stderr[3]
    assert main(["calibrate", "--dem", str(tmp_path / "m.dem"), "--in", str(tmp_path / "missing.b8"), "--in_format", "b8", "--out", str(tmp_path / "g.dem"),
                 "--mirror"]) == 1
