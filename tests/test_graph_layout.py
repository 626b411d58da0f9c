"""The host-only layout of a window graph (quits_amd/csrc/graph_layout.hip) under the address and undefined-behaviour sanitizers: a stand-alone
program (tests/layout_check.cpp) lays out one window per run and checks the invariants the kernels rely on -- slot orders, LDS carve-ups,
adjacency and fault records, the per-edge records, the scatter walk and wave map.  No GPU and nothing loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILERS = ["g++"] + [c for c in ("/opt/rocm/llvm/bin/clang++",) if shutil.which(c)]     # g++ always: without it the build below fails, it does not skip


def golden(name, first_of=None):
    if first_of:
        w = helpers.window_set(name, *first_of)[0]
        return w["H"], w["priors"]
    H, _, pri = helpers.dem_matrices(name)
    return H, pri


def synthetic(m, n, weights, seed, heavy_column=0, off_chip_columns=0):
    """A window of the given row weights in which every fault sits on a check (fault j on check j mod m, the rest drawn)."""
    rng = np.random.default_rng(seed)
    if off_chip_columns:                                 # by columns: every fault on `off_chip_columns` distinct checks
        rows = [set() for _ in range(m)]
        for j in range(n):
            for i in rng.choice(m, off_chip_columns, replace=False):
                rows[int(i)].add(j)
    else:
        rows = [set(range(i, n, m)) if weights[i] > 1 else set() for i in range(m)]
        for i in range(m):
            if weights[i] == 1:                          # a check of one fault: its share of the faults goes to the next check
                rows[i].add(i)
                rows[i + 1].update(range(i + m, n, m))
        for i in range(m):
            while len(rows[i]) < weights[i]:
                rows[i].add(int(rng.integers(n)))
    if heavy_column:                                     # fault 7 on exactly that many checks
        for r in rows:
            r.discard(7)
        for i in rng.choice(m, heavy_column, replace=False):
            rows[int(i)].add(7)
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col_idx = np.concatenate([sorted(r) for r in rows]).astype(np.int32)
    return (row_ptr, col_idx, n), rng.uniform(1e-3, 1e-2, n)


# row weights, lightest and heaviest of the columns beside the two weight-2 faults of every row, seed (helpers.synthetic_window)
LIMITS = {"rows_of_255": ([255] * 72, 3, 6, 30255), "column_of_weight_16": ([40] * 128, 7, 16, 30016),
          "rows_of_255_columns_of_16": ([255] * 64 + [100] * 64, 7, 16, 30271),
          "row_of_256": ([256] + [40] * 71, 3, 6, 31006), "column_of_weight_17": ([40] * 72, 14, 17, 31017)}
REFUSED = {"row_of_256": "row weight 256 outside 1..255", "column_of_weight_17": "column weight 17 outside 1..16"}


def _syn(name):
    rng = np.random.default_rng(7)
    if name == "70x300_rows_to_40":
        return synthetic(70, 300, rng.integers(6, 41, 70), 1)
    if name == "600x6000_row_of_70":
        return synthetic(600, 6000, np.concatenate([[70], rng.integers(10, 15, 599)]), 2)
    if name == "row_of_one_fault":
        return synthetic(40, 120, np.concatenate([rng.integers(3, 7, 5), [1], rng.integers(3, 7, 34)]), 3)
    if name == "column_of_weight_12":
        return synthetic(64, 200, rng.integers(4, 9, 64), 4, heavy_column=12)
    if name in LIMITS:                                   # the windows of tests/test_gpu_graph_limits.py at the limits of the ABI, and one past each
        return helpers.synthetic_window(*LIMITS[name])
    assert name == "4100x9000_columns_of_3"
    return synthetic(4100, 9000, None, 5, off_chip_columns=3)


# window -> (how to make it, what layout_check's summary line must say: the branch the window is here for)
WINDOWS = {
    "hgp225_cardinal_r3_p0.01": (lambda: golden("hgp225_cardinal_r3_p0.01"), {"off_chip": 0}),
    "bb72_custom_r6_p0.003": (lambda: golden("bb72_custom_r6_p0.003"), {"off_chip": 0, "sc_ok": 1, "wide_cpl": 2}),
    "bb144_custom_r12_p0.003": (lambda: golden("bb144_custom_r12_p0.003"), {"sc_ok": 1, "wide_threads": 512, "wide_cpl": 2}),
    "qlp1020_cardinal_r20_p0.003_W3F1_0": (lambda: golden("qlp1020_cardinal_r20_p0.003", (3, 1)), {"sc_ok": 1, "wide_threads": 512, "wide_cpl": 3, "sign_mode": 2}),
    "70x300_rows_to_40": (lambda: _syn("70x300_rows_to_40"), {"sign_mode": 1, "off_chip": 0}),
    "600x6000_row_of_70": (lambda: _syn("600x6000_row_of_70"), {"sign_mode": 2, "sc_ok": 1, "wide_cpl": 3}),
    "row_of_one_fault": (lambda: _syn("row_of_one_fault"), {"min_rdeg": 1, "sc_ok": 0}),
    "column_of_weight_12": (lambda: _syn("column_of_weight_12"), {"frec": 0, "unroll": 16}),
    "rows_of_255": (lambda: _syn("rows_of_255"), {"sign_mode": 2, "sc_ok": 0, "threads": 512, "off_chip": 0}),
    "column_of_weight_16": (lambda: _syn("column_of_weight_16"), {"sign_mode": 1, "sc_ok": 1, "frec": 0, "unroll": 16, "off_chip": 0}),
    "rows_of_255_columns_of_16": (lambda: _syn("rows_of_255_columns_of_16"), {"sign_mode": 2, "sc_ok": 0, "frec": 0, "unroll": 16, "off_chip": 0}),
    "4100x9000_columns_of_3": (lambda: _syn("4100x9000_columns_of_3"), {"off_chip": 1, "threads": 0, "sc_ok": 0}),
    # one check per lane without any switch: the accumulators leave no room for twice the workgroups (tests/test_gpu_bp_one_check_per_lane.py decodes them)
    "hgp225_cardinal_r3_p0.01_W2F1_0": (lambda: golden("hgp225_cardinal_r3_p0.01", (2, 1)), {"sc_ok": 1, "threads": 256, "wide_threads": 256, "wide_cpl": 1}),
    "410x5056_one_check_per_lane": (lambda: helpers.synthetic_window([36] * 410, 3, 4, 41001), {"sc_ok": 1, "threads": 512, "wide_threads": 512, "wide_cpl": 1}),
    "800x10933_one_check_per_lane": (lambda: helpers.synthetic_window([40] * 800, 3, 4, 41002), {"sc_ok": 1, "threads": 1024, "wide_threads": 1024, "wide_cpl": 1}),
}
SWITCHES = {"QD_SCATTER_BANKS_BY_SLOT": {"sc_ok": 1}, "QD_SCATTER_WALK_GREEDY": {"sc_ok": 1}, "QD_SCATTER_NATURAL_ROUNDS": {"wide_cpl": 2},
            "QD_SCATTER_CPL1": {"sc_ok": 1, "wide_threads": 512, "wide_cpl": 1}}


def write_window(path, H, priors):
    """int32 m, n, nnz, row_ptr, col_idx, double priors: what layout_check reads."""
    if isinstance(H, tuple):
        row_ptr, col_idx, n = H
        m = len(row_ptr) - 1
    else:
        R = H.tocsr()
        R.sort_indices()
        (m, n), row_ptr, col_idx = R.shape, R.indptr, R.indices
    with open(path, "wb") as f:
        np.array([m, n, len(col_idx)], np.int32).tofile(f)
        np.asarray(row_ptr, np.int32).tofile(f)
        np.asarray(col_idx, np.int32).tofile(f)
        np.asarray(priors, np.float64).tofile(f)


@pytest.fixture(scope="module", params=COMPILERS, ids=[os.path.basename(c) for c in COMPILERS])
def layout_check(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layout_check") / "layout_check")
    cmd = [request.param, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
           os.path.join(ROOT, "quits_amd", "csrc", "graph_layout.hip"), os.path.join(ROOT, "tests", "layout_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def window_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("windows")
    files = {}
    for name, (make, _) in WINDOWS.items():
        files[name] = str(d / (name + ".bin"))
        write_window(files[name], *make())
    return files


def run(exe, window, expect, env=None):
    out = subprocess.run([exe, window], capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout, out.stderr[-3000:])     # a failed invariant and a sanitizer report both land here
    said = {k: v for k, v in (kv.split("=") for kv in out.stdout.split())}
    for k, v in expect.items():
        assert said[k] == str(v), (k, v, out.stdout)
    return said


@pytest.mark.parametrize("name", list(WINDOWS))
def test_layout_invariants(layout_check, window_files, name):
    run(layout_check, window_files[name], WINDOWS[name][1])


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_layout_invariants_under_the_validation_switches(layout_check, window_files, switch):
    name = "bb72_custom_r6_p0.003"
    plain = run(layout_check, window_files[name], WINDOWS[name][1])
    said = run(layout_check, window_files[name], SWITCHES[switch], env={switch: "1"})
    if switch in ("QD_SCATTER_BANKS_BY_SLOT", "QD_SCATTER_WALK_GREEDY"):       # the switch was read: the older bank assignment / walk costs more LDS cycles in the model
        assert int(said["walk"].split("/")[0]) > int(plain["walk"].split("/")[0]), (plain, said)


@pytest.mark.parametrize("name", list(REFUSED))
def test_one_past_a_limit_is_refused(layout_check, tmp_path, name):
    """A row of 256 faults, a column of weight 17: qd_host_graph answers QD_ECAPACITY with the limit in the message, and the program exits with its refusal status."""
    window = str(tmp_path / (name + ".bin"))
    write_window(window, *_syn(name))
    out = subprocess.run([layout_check, window], capture_output=True, text=True)
    assert out.returncode == 3 and out.stderr.strip() == REFUSED[name] and not out.stdout, (out.returncode, out.stdout, out.stderr[-3000:])
