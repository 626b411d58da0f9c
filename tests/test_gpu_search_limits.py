"""The logical-fault search on the device (csrc/logical_search.hip) at the limits of its state record, on the crafted models of
tests/test_search_limits.py: event sets of 5 to 8 detectors, faults of up to 16, detector 65534, mask bit 63, level 1 seeded in several
chunks, a visited table exactly full, and a level of 65 536 and of 65 537 undetectable states.  The numpy mirror is the reference (the CPU
file pins it record by record); everything is compared exactly, and the states themselves are recovered from the device's parent chains."""
import numpy as np
import pytest
from scipy.sparse import csc_matrix

from quits_amd import search as ls
from test_search_limits import FROZEN, MODELS, found_list, reference, sixty_five_observables, state_of

pytestmark = pytest.mark.gpu

ROOMY = 1 << 18


def deterministic(res):
    return (res.outcome, res.weight, res.levels_completed, res.level_sizes, res.total_states, res.logical_masks)


def check_against_mirror(res, ref_res, H, L):
    """Every deterministic field equal, every witness under its contract, and no fewer candidates looked up than states kept."""
    assert deterministic(res) == deterministic(ref_res)
    assert len(res.witnesses) == len(ref_res.witnesses) == min(16, len(res.logical_masks))
    for e, mask in zip(res.witnesses, res.logical_masks):
        ls.check_witness(H, L, e, mask, res.observables, res.weight, res.max_fault_degree)
    assert len(res.candidates) == len(res.level_sizes) and all(c >= s for c, s in zip(res.candidates, res.level_sizes))


@pytest.mark.parametrize("name", list(MODELS))
def test_device_gives_every_deterministic_field_of_the_mirror(name):
    ref = reference(name)
    res = ls.find_undetectable_logical_errors((ref.H, ref.L), max_states=ROOMY, **ref.opts)
    assert (res.outcome, res.weight, res.level_sizes) == FROZEN[name]
    check_against_mirror(res, ref.res, ref.H, ref.L)


def device_levels(ref, max_states=ROOMY, **config):
    """Drive a LogicalSearcher by hand through the levels the mirror completed; per level the list of (S, o) of its pool records, each
    recovered on the host from the record's parent chain.  Asserts the chain lengths and that every fault of a chain is admitted."""
    levels = []
    eng = ls.LogicalSearcher(ref.m, max_states, **config)
    try:
        for level in range(1, len(ref.res.level_sizes) + 1):
            new = eng.start() if level == 1 else eng.step()
            lo, hi = eng._frontier
            assert new == hi - lo and lo == ref.bounds[level - 1], "level %d: %r new states from pool index %d" % (level, new, lo)
            chains = [eng.chain(idx) for idx in range(lo, hi)]
            assert all(len(c) == level for c in chains), "a chain of level %d has another length" % level
            assert all(1 <= len(ref.dets[j]) <= ref.m.D for c in chains for j in c), "a fault of a chain is not admitted"
            levels.append([state_of(ref, c) for c in chains])
            found = sorted(mask for mask, _ in eng.found())
            assert found == (ref.res.logical_masks if level == ref.res.weight else [])
        assert eng.counters()["pool"] == ref.res.total_states
    finally:
        eng.close()
    return levels


def check_levels(ref, levels):
    """The device's states of every level are the mirror's: the same set, and none of them twice in a level or in two levels."""
    assert [len(lv) for lv in levels] == ref.res.level_sizes
    for level, (got, want) in enumerate(zip(levels, ref.levels), start=1):
        assert len(set(got)) == len(got), "level %d holds a state twice" % level
        extra, missing = set(got) - want, want - set(got)
        assert not extra and not missing, "level %d: %d states the mirror lacks %r, %d it alone has %r" % (
            level, len(extra), sorted(extra)[:3], len(missing), sorted(missing)[:3])
    assert len(set().union(*map(set, levels))) == ref.res.total_states, "a state belongs to two levels"


@pytest.mark.parametrize("name", list(MODELS))
def test_device_states_are_the_mirror_states(name):
    ref = reference(name)
    check_levels(ref, device_levels(ref))


def _full_table(ref):
    total = ref.res.total_states
    size = 1 << (total - 1).bit_length()
    assert size // 2 < total <= size
    return dict(max_states=total, table_size=size)


STRESS = {
    "chunks": lambda ref: dict(stage_states=ref.m.max_row, chunk_states=1),         # k8: 50 seeds in chunks of 24; one frontier state a launch
    "full_table": _full_table,                                                      # k8: 2212 states in 4096 slots and a pool of 2212
    "both": lambda ref: dict(stage_states=ref.m.max_row, chunk_states=1, **_full_table(ref)),
}


# (on k5 the chunked seeding has a duplicate to remove: the copy of fault 0 arrives two chunks after fault 0 itself)
@pytest.mark.parametrize("name,how", [("k8", "chunks"), ("k8", "full_table"), ("k8", "both"), ("k5", "chunks")])
def test_stressed_configurations_give_the_same_states(name, how):
    ref = reference(name)
    config = STRESS[how](ref)
    if "stage_states" in config:
        assert len(ls.level_one(ref.m)) > 2 * config["stage_states"] and config["stage_states"] == ref.m.max_row > 16
    check_levels(ref, device_levels(ref, **config))


def test_found_list_at_its_capacity_and_one_beyond():
    H, L = found_list(ls.FOUND_CAP)
    res = ls.find_undetectable_logical_errors((H, L), max_states=ROOMY, keep=2)
    assert (res.outcome, res.weight, res.level_sizes, res.total_states) == ("found", 1, [ls.FOUND_CAP + 1], ls.FOUND_CAP + 1)
    assert res.logical_masks == list(range(1, ls.FOUND_CAP + 1))
    assert [w.tolist() for w in res.witnesses] == [[1], [2]]
    for e, mask in zip(res.witnesses, res.logical_masks):
        ls.check_witness(H, L, e, mask, res.observables, 1, res.max_fault_degree)
    H, L = found_list(ls.FOUND_CAP + 1)
    with pytest.raises(RuntimeError, match="more than 65536 undetectable logical states"):
        ls.find_undetectable_logical_errors((H, L), max_states=ROOMY, keep=2)
    # the overflow leaves a working device
    ref = reference("line")
    res = ls.find_undetectable_logical_errors((ref.H, ref.L), max_states=ROOMY, **ref.opts)
    assert (res.outcome, res.weight, res.logical_masks, [w.tolist() for w in res.witnesses]) == ("found", 10, [1 << 63], [list(range(10))])
    check_against_mirror(res, ref.res, ref.H, ref.L)


def test_refusals_come_before_any_launch():
    ref = reference("k8")
    with pytest.raises(ValueError, match="exceeds the 24 staged candidates"):
        ls.LogicalSearcher(ref.m, ROOMY, stage_states=ref.m.max_row, chunk_states=2)
    tall = csc_matrix((np.ones(2, np.uint8), ([0, 65535], [0, 1])), shape=(65536, 2))
    with pytest.raises(ValueError, match="65536 detectors"):
        ls.find_undetectable_logical_errors((tall, csc_matrix(np.ones((1, 2), np.uint8))), max_states=ROOMY)
    H, L, rows = sixty_five_observables()
    opts = MODELS["k7"][1]
    with pytest.raises(ValueError, match="pass a selection"):
        ls.find_undetectable_logical_errors((H, L), max_states=ROOMY, **opts)
    res = ls.find_undetectable_logical_errors((H, L), max_states=ROOMY, observables=rows, **opts)
    assert res.observables == rows
    check_against_mirror(res, ls.search_mirror(H, L, observables=rows, **opts), H, L)
