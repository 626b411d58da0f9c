"""The search for light undetectable logical faults, host side: the numpy mirror (quits_amd.search.search_mirror) against level sizes frozen
from a separate prototype of the same definition, the witness contract, the stop rules, the limits and the command line.  No GPU."""
import json

import numpy as np
import pytest
from scipy.sparse import csc_matrix

import helpers
from quits_amd import search as ls
from quits_amd.dem import Circuit

# (circuit, shape of H, keywords, outcome, weight, logical masks, completed level sizes): frozen values
ROWS = {
    "rep3": ("hgprep3_zxcoloration_r3_p0.001", (45, 234), dict(max_event_set=4, max_fault_degree=4), "found", 3, 2, [234, 840, 2504]),
    "bb72_r0": ("bb72_custom_r0_p0.003", (72, 432), dict(max_event_set=4, max_fault_degree=4), "found", 6, 45, [360, 2381, 3117, 3389, 4062, 7715]),
    "bb72_r0_no_increase": ("bb72_custom_r0_p0.003", (72, 432), dict(max_event_set=4, max_fault_degree=4, no_increase=True), "space", None, 0,
                            [360, 173, 66, 66, 6]),
    "bb72_r2_xbasis": ("bb72_custom_r2_xbasis_mixed", (144, 1152), dict(max_event_set=4, max_fault_degree=4), "found", 6, 42,
                       [936, 8598, 22002, 38084, 48870, 65468]),
    "bb72_r6": ("bb72_custom_r6_p0.003", (288, 2592), dict(max_event_set=3, max_fault_degree=6), "space", None, 0,
                [1836, 3966, 5646, 6654, 6798, 6078, 4494, 2046, 354]),
    "bb72_r2_alldet": ("bb72_custom_r2_alldet_p0.003", (216, 5400), dict(max_event_set=3, max_fault_degree=9), "space", None, 0,
                       [1008, 3084, 8422, 11873, 9143, 5575, 4003, 1771, 640, 191, 20]),
    "hgp225_r3": ("hgp225_cardinal_r3_p0.01", (540, 5409), dict(max_event_set=3, max_fault_degree=6), "space", None, 0, [2304, 4177, 5151, 4617, 2355, 476]),
    "bb72_r0_cap_36890": ("bb72_custom_r0_p0.003", (72, 432), dict(max_event_set=6, max_fault_degree=6, max_states=36890), "capacity", None, 0,
                          [432, 3860, 32598]),
    "bb72_r0_cap_36889": ("bb72_custom_r0_p0.003", (72, 432), dict(max_event_set=6, max_fault_degree=6, max_states=36889), "capacity", None, 0, [432, 3860]),
}

_MATRICES = {}


def matrices(name):
    """(H, L) of a fixture circuit, computed once."""
    if name not in _MATRICES:
        from quits_amd.decoder.base import detector_error_model_to_matrix
        H, L, _ = detector_error_model_to_matrix(Circuit(helpers.circuit_text(name)).detector_error_model())
        _MATRICES[name] = (csc_matrix(H), csc_matrix(L))
    return _MATRICES[name]


def check_row(res, row, H, L):
    """A result against a frozen row: every deterministic field, and the contract of every witness."""
    _, shape, kw, outcome, weight, nmasks, sizes = row
    assert H.shape == shape
    assert res.outcome == outcome and res.weight == weight
    assert res.level_sizes == sizes and res.levels_completed == len(sizes) and res.total_states == sum(sizes)
    assert len(res.logical_masks) == nmasks and res.logical_masks == sorted(set(res.logical_masks)) and all(m != 0 for m in res.logical_masks)
    assert len(res.witnesses) == min(nmasks, 16)
    for e, mask in zip(res.witnesses, res.logical_masks):
        ls.check_witness(H, L, e, mask, res.observables, res.weight, res.max_fault_degree)
    assert (res.max_event_set, res.max_fault_degree, res.no_increase) == (kw["max_event_set"], kw["max_fault_degree"], kw.get("no_increase", False))
    if "max_states" in kw:
        assert res.max_states == kw["max_states"]


@pytest.mark.parametrize("key", list(ROWS))
def test_mirror_reproduces_the_frozen_levels(key):
    row = ROWS[key]
    H, L = matrices(row[0])
    check_row(ls.search_mirror(H, L, **row[2]), row, H, L)


def test_max_weight_stops_the_search():
    H, L = matrices("bb72_custom_r0_p0.003")
    res = ls.search_mirror(H, L, max_event_set=4, max_fault_degree=4, max_weight=3)
    assert (res.outcome, res.weight, res.levels_completed, res.level_sizes, res.logical_masks, res.witnesses) == ("weight", None, 3, [360, 2381, 3117], [], [])
    assert res.max_weight == 3
    # found comes before the weight rule at the same level
    res = ls.search_mirror(H, L, max_event_set=4, max_fault_degree=4, max_weight=6)
    assert res.outcome == "found" and res.weight == 6


def test_a_fault_without_detectors_is_a_weight_one_logical():
    H = csc_matrix(np.array([[1, 0, 1], [1, 0, 1]], np.uint8))           # faults 0 and 2 flip both detectors, fault 1 none
    L = csc_matrix(np.array([[0, 1, 1]], np.uint8))
    res = ls.search_mirror(H, L)
    assert (res.outcome, res.weight, res.level_sizes, res.logical_masks) == ("found", 1, [3], [1])
    assert [w.tolist() for w in res.witnesses] == [[1]]
    ls.check_witness(H, L, res.witnesses[0], 1, res.observables, 1, res.max_fault_degree)
    # with a zero mask the same fault is ignored: the logical is then faults 0 and 2 together
    res = ls.search_mirror(H, csc_matrix(np.array([[0, 0, 1]], np.uint8)))
    assert (res.outcome, res.weight, res.level_sizes, res.logical_masks) == ("found", 2, [2, 1], [1])
    assert [w.tolist() for w in res.witnesses] == [[0, 2]]


def test_limits_raise_value_errors():
    H, L = matrices("hgprep3_zxcoloration_r3_p0.001")
    with pytest.raises(ValueError, match="max_event_set"):
        ls.search_mirror(H, L, max_event_set=9)
    with pytest.raises(ValueError, match="max_fault_degree"):
        ls.search_mirror(H, L, max_fault_degree=17)
    with pytest.raises(ValueError, match="max_event_set"):
        ls.find_undetectable_logical_errors((H, L), max_event_set=0)           # checked before the device is looked for
    wide = csc_matrix(np.ones((65, H.shape[1]), np.uint8))
    with pytest.raises(ValueError, match="pass a selection"):
        ls.search_mirror(H, wide)
    assert ls.search_mirror(H, wide, observables=list(range(64)), max_weight=1).outcome == "weight"
    with pytest.raises(ValueError, match="at most 64"):
        ls.search_mirror(H, wide, observables=list(range(65)))
    tall = csc_matrix((np.ones(2, np.uint8), ([0, 65535], [0, 1])), shape=(65536, 2))
    with pytest.raises(ValueError, match="65535"):
        ls.search_mirror(tall, csc_matrix(np.ones((1, 2), np.uint8)))
    with pytest.raises(ValueError, match="one column per fault"):
        ls.search_mirror(H, L[:, :-1])


def test_a_selection_searches_one_mask_bit():
    name = "hgprep3_zxcoloration_r3_p0.001"
    H, L = matrices(name)
    assert L.shape[0] > 1
    res = ls.search_mirror(H, L, max_event_set=4, max_fault_degree=4, observables=[0])
    assert res.observables == [0] and res.outcome == "found" and res.logical_masks == [1]
    for e in res.witnesses:
        ls.check_witness(H, L, e, 1, [0], res.weight, 4)
    m = ls.prepare(H, L, 4, 4, observables=[0])
    assert int(m.fault_obs.max()) == 1
    # every input form gives the same matrices
    text = helpers.circuit_text(name)
    a, b = ls._matrices(text), ls._matrices(Circuit(text))
    assert helpers.same_sparse(a[0], H) and helpers.same_sparse(b[0], H) and helpers.same_sparse(a[1], L)


def test_memory_statement_and_default_max_states():
    assert ls.search_memory_bytes(1000, 4096, 2048) == 32 * 1000 + 4 * 4096 + 40 * 2048 + 4 * ls.FOUND_CAP
    free = 200 << 30
    n = ls.default_max_states(free)
    assert ls.search_memory_bytes(n) <= free // 2 < ls.search_memory_bytes(n + 1)
    assert ls.default_max_states(1 << 62) == 0xFFFFFFFE - ls.DEFAULT_STAGE                 # pool and staging indices share 32 bits
    with pytest.raises(RuntimeError, match="free bytes"):
        ls.default_max_states(1 << 20)
    t = ls.default_table_size(36889, 4096)
    assert t & (t - 1) == 0 and t >= 2 * (36889 + 4096) > t // 2


def test_library_exports_the_search():
    from quits_amd import _lib
    L = _lib.load()
    assert L.qd_version() >= 115 and _lib.require_search(L) is L
    from quits_amd import simulation
    assert simulation.find_undetectable_logical_errors is ls.find_undetectable_logical_errors


def test_command_line_prints_the_result_as_json(tmp_path, capsys):
    from quits_amd.__main__ import main
    row = ROWS["rep3"]
    path = tmp_path / "c.stim"
    path.write_text(helpers.circuit_text(row[0]))
    assert main(["search", "--circuit", str(path), "--max_event_set", "4", "--max_fault_degree", "4", "--mirror"]) == 0
    out = json.loads(capsys.readouterr().out)
    assert (out["outcome"], out["weight"], out["level_sizes"], out["total_states"]) == ("found", 3, [234, 840, 2504], 3578)
    assert len(out["logical_masks"]) == 2 and len(out["witnesses"]) == 2
    H, L = matrices(row[0])
    for e, mask in zip(out["witnesses"], out["logical_masks"]):
        ls.check_witness(H, L, e, mask, out["observables"], 3, 4)
    assert main(["search", "--circuit", str(path), "--max_event_set", "9", "--mirror"]) == 1


def test_search_kernels_use_no_scratch(tmp_path):
    """The symmetric difference of the expansion kernel stays in registers (two 64-bit words, no indexed register array)."""
    from test_api import _resource_usage
    kern = dict(_resource_usage(tmp_path, "logical_search.hip"))
    names = [n for n in kern if "qd_search_" in n]
    assert len(names) == 3 and any("expand" in n for n in names), names
    assert all(kern[n] == 0 for n in names), kern
