"""The search for light undetectable logical faults on the device (csrc/logical_search.hip) against the frozen level sizes of
tests/test_search.py: every deterministic field of the result, the witness contract, the exact capacity boundary, repeated runs, a frontier
split into several chunks and a visited table almost full."""
import pytest

from quits_amd import search as ls
from test_search import ROWS, check_row, matrices

pytestmark = pytest.mark.gpu


ROOMY = 1 << 18         # states: more than any row of the table holds (183 958), so a row that sets no max_states never meets the limit


def run(key, **extra):
    """A row of the table on the device.  Rows that set no max_states get ROOMY instead of the default (half of the free device memory,
    which test_default_max_states_is_half_of_the_free_memory covers): allocating and clearing that much takes seconds per case."""
    row = ROWS[key]
    H, L = matrices(row[0])
    opts = {**row[2], **extra}
    opts.setdefault("max_states", ROOMY)
    return ls.find_undetectable_logical_errors((H, L), **opts), row, H, L


@pytest.mark.parametrize("key", list(ROWS))
def test_device_reproduces_the_frozen_levels(key):
    res, row, H, L = run(key)
    check_row(res, row, H, L)
    assert len(res.candidates) == len(row[6]) and all(c >= s for c, s in zip(res.candidates, row[6]))


def test_default_max_states_is_half_of_the_free_memory():
    import torch
    row = ROWS["rep3"]
    H, L = matrices(row[0])
    free = torch.cuda.mem_get_info()[0]
    res = ls.find_undetectable_logical_errors((H, L), **row[2])
    check_row(res, row, H, L)
    assert ls.search_memory_bytes(res.max_states) <= free // 2 and res.max_states > ROOMY
    with pytest.raises(RuntimeError, match="allocation failed"):             # raised by the allocation, before any launch
        ls.find_undetectable_logical_errors((H, L), **row[2], max_states=ROOMY, table_size=1 << 40)       # a table of 4 TiB


def test_capacity_leaves_a_working_device():
    """36 890 states hold three levels, 36 889 only two; after the overflow the next search runs as if nothing had happened."""
    res, row, H, L = run("bb72_r0_cap_36890")
    assert (res.outcome, res.levels_completed, res.total_states) == ("capacity", 3, 36890)
    res, row, H, L = run("bb72_r0_cap_36889")
    assert (res.outcome, res.levels_completed, res.level_sizes) == ("capacity", 2, [432, 3860])
    res, row, H, L = run("rep3")
    check_row(res, row, H, L)


def deterministic(res):
    return (res.outcome, res.weight, res.levels_completed, res.level_sizes, res.total_states, res.logical_masks, res.candidates)


def test_a_second_run_gives_the_same_deterministic_fields():
    first, row, H, L = run("bb72_r0")
    again, _, _, _ = run("bb72_r0")
    assert deterministic(first) == deterministic(again)
    # the same search object, reset: the driver's loop on it
    import time
    m = ls.prepare(H, L, 4, 4)
    eng = ls.LogicalSearcher(m, 1 << 16)
    try:
        a = ls._drive(eng, m, None, 1 << 16, 16, time.perf_counter())
        eng.reset()
        b = ls._drive(eng, m, None, 1 << 16, 16, time.perf_counter())
    finally:
        eng.close()
    assert deterministic(a) == deterministic(b) == deterministic(first)
    for e, mask in zip(b.witnesses, b.logical_masks):
        ls.check_witness(H, L, e, mask, b.observables, b.weight, 4)


def test_a_frontier_in_several_chunks_gives_the_same_levels():
    """64 states a chunk: the level of 11 873 states is expanded in 186 chunks, so duplicates of one level meet across chunks."""
    res, row, H, L = run("bb72_r2_alldet", chunk_states=64)
    check_row(res, row, H, L)


def test_a_table_almost_full_gives_the_same_levels():
    """3 578 states in 4 096 slots, the smallest power of two that holds them: long probe chains."""
    total = sum(ROWS["rep3"][6])
    size = 1 << (total - 1).bit_length()
    assert size == 4096 and size // 2 < total
    res, row, H, L = run("rep3", table_size=size, max_states=total)
    assert res.max_states == total
    check_row(res, row, H, L)
    with pytest.raises(RuntimeError, match="visited table is full"):
        run("rep3", table_size=size // 2, max_states=total)


def test_a_selection_and_a_weight_one_logical_on_the_device():
    import numpy as np
    from scipy.sparse import csc_matrix
    H, L = matrices(ROWS["rep3"][0])
    res = ls.find_undetectable_logical_errors((H, L), max_event_set=4, max_fault_degree=4, observables=[0], max_states=ROOMY)
    ref = ls.search_mirror(H, L, max_event_set=4, max_fault_degree=4, observables=[0])
    assert deterministic(res)[:6] == deterministic(ref)[:6] and res.logical_masks == [1]
    for e in res.witnesses:
        ls.check_witness(H, L, e, 1, [0], res.weight, 4)
    H1 = csc_matrix(np.array([[1, 0, 1], [1, 0, 1]], np.uint8))
    L1 = csc_matrix(np.array([[0, 1, 1]], np.uint8))
    res = ls.find_undetectable_logical_errors((H1, L1), max_states=ROOMY)
    assert (res.outcome, res.weight, res.level_sizes, res.logical_masks, [w.tolist() for w in res.witnesses]) == ("found", 1, [3], [1], [[1]])
