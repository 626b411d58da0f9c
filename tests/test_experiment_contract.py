"""What every experiment driver of quits_amd.simulation does before it touches the device: the argument checks come first and are
ValueErrors, a missing device is a RuntimeError and never a fallback.  And the table behind _lib's require_* functions.  No GPU needed."""
import numpy as np
import pytest

import helpers

NAME = "bb72_custom_r6_p0.003"
W = 3

# every public driver as (name, positional arguments after F, keywords)
DRIVERS = [
    ("get_circuit_mem_pL", (64,), {}),
    ("get_relay_mem_pL", (64,), {}),
    ("get_postselected_pL", (64,), {}),
    ("get_fault_spectrum", (64,), {}),
    ("get_stratified_pL", ({2: 10},), {}),
    ("shrink_fault_sets", (np.zeros((1, 40), dtype=bool),), {}),
    ("get_minimal_failures", (64,), {}),
    ("get_relay_minimal_failures", (64,), {}),
]

REQUIRE_NAMES = ["require_bitpack", "require_calibrate", "require_distance", "require_experiment", "require_faults", "require_relay",
                 "require_relay_forms", "require_search", "require_shrink", "require_soft", "require_strata"]


@pytest.fixture
def no_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)         # (what a machine without a GPU reports)


@pytest.fixture(scope="module")
def case():
    cd = helpers.code("bb72")
    return helpers.circuit_text(NAME), cd["hz"], cd["lz"]


def call(case, name, F, args, kw):
    from quits_amd import simulation
    text, hz, lz = case
    return getattr(simulation, name)(text, hz, lz, W, F, *args, **kw)


@pytest.mark.parametrize("name,args,kw", DRIVERS, ids=[d[0] for d in DRIVERS])
def test_F_zero_is_refused_before_the_device_is_asked_for(no_gpu, case, name, args, kw):
    with pytest.raises(ValueError, match="Input parameter F cannot be zero."):
        call(case, name, 0, args, kw)


@pytest.mark.parametrize("name", ["get_circuit_mem_pL", "get_postselected_pL"])
def test_a_bad_sampler_name_is_refused_before_the_device_is_asked_for(no_gpu, case, name):
    with pytest.raises(ValueError, match="sampler must be 'circuit' or 'dem'"):
        call(case, name, 1, (64,), {"sampler": "x"})


def test_the_drivers_own_argument_checks_come_before_the_device(no_gpu, case):
    with pytest.raises(ValueError, match="stratum 300"):
        call(case, "get_stratified_pL", 1, ({300: 10},), {})
    with pytest.raises(ValueError, match="max_parents and keep_sets must not be negative"):
        call(case, "get_minimal_failures", 1, (64,), {"max_parents": -1})


@pytest.mark.parametrize("name,args,kw", DRIVERS, ids=[d[0] for d in DRIVERS])
def test_no_device_is_an_error_for_every_driver(no_gpu, case, name, args, kw):
    with pytest.raises(RuntimeError, match="no HIP device"):
        call(case, name, 1, args, kw)


def test_no_device_is_an_error_for_the_replays(no_gpu, case):
    from quits_amd.simulation import replay_faults, replay_shots, replay_strata_faults
    text = case[0]
    with pytest.raises(RuntimeError, match="no HIP device"):
        replay_shots(text, [1, 2], 0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        replay_shots(text, [1, 2], 0, "dem")
    with pytest.raises(RuntimeError, match="no HIP device"):
        replay_faults(text, [1, 2], 0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        replay_strata_faults(text, 2, [1, 2], 0)


def test_replay_shots_refuses_a_bad_sampler_name_before_the_device_is_asked_for(no_gpu, case):
    from quits_amd.simulation import replay_shots
    with pytest.raises(ValueError, match="sampler must be 'circuit' or 'dem'"):
        replay_shots(case[0], [1], 0, "x")


def test_require_functions_come_from_one_table_and_keep_their_behaviour():
    from quits_amd import _lib
    assert sorted(n for n in dir(_lib) if n.startswith("require_") and n != "require_gpu") == REQUIRE_NAMES
    L = _lib.load()

    class Old:
        def qd_version(self):
            return 97
    for name in REQUIRE_NAMES:
        require = getattr(_lib, name)
        assert require(L) is L, name
        with pytest.raises(RuntimeError, match=r"is version 97; .* >= 1\d\d -- rebuild it") as exc:
            require(Old())
        assert _lib.LIB_PATH in str(exc.value), name
    # today's texts, word for word, for the oldest and the newest group
    with pytest.raises(RuntimeError) as exc:
        _lib.require_experiment(Old())
    assert str(exc.value) == "quits_amd: %s is version 97; the device-resident memory experiment needs >= 108 -- rebuild it" % _lib.LIB_PATH
    with pytest.raises(RuntimeError) as exc:
        _lib.require_calibrate(Old())
    assert str(exc.value) == "quits_amd: %s is version 97; fitting priors needs >= 118 -- rebuild it" % _lib.LIB_PATH
