"""The fault-set shrinker on the device (qd_shrink_begin / qd_shrink_step, decoder.device.FaultShrinker) against its numpy definition
(quits_amd.shrink.shrink_mirror) under scripted verdicts, bit for bit and round by round; then get_minimal_failures end to end: against
get_fault_spectrum, against the public decode call on every final set and its children, against the mirror driven by that call."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers
from quits_amd import shrink

pytestmark = pytest.mark.gpu

BB72 = "bb72_custom_r6_p0.003"
MINSUM = dict(bp_method="minimum_sum", schedule="parallel", max_iter=20, osd_method="osd_0", osd_order=0)
SEED, SHOTS = 11, 1 << 12


def _toy(n, seed):
    """A seeded model of n faults on 7 detectors and 2 observables."""
    from scipy.sparse import csc_matrix
    rng = np.random.default_rng(seed)
    return csc_matrix((rng.random((7, n)) < 0.4).astype(np.uint8)), csc_matrix((rng.random((2, n)) < 0.3).astype(np.uint8))


def _wide():
    """2100 faults (33 words: more than one per lane) on 70 detectors (rows longer than a wavefront) and 2 observables; fault 5 flips 16
    detectors, fault 7 nothing at all."""
    from scipy.sparse import csc_matrix
    rng = np.random.default_rng(2100)
    H = (rng.random((70, 2100)) < 0.05).astype(np.uint8)
    L = (rng.random((2, 2100)) < 0.3).astype(np.uint8)
    H[:, 5] = 0
    H[rng.choice(70, 16, replace=False), 5] = 1
    H[:, 7] = 0
    L[:, 7] = 0
    return csc_matrix(H), csc_matrix(L)


def _parents(n, seed):
    """70 parents (a full wavefront's worth of rows and a partial one): random sets of a few densities, the empty set, a singleton, the full
    set, and one with members in the last word only."""
    rng = np.random.default_rng(seed)
    E = rng.random((70, n)) < rng.choice([0.02, 0.1, 0.3], size=70)[:, None] * min(1.0, 40.0 / n)
    E[3] = False
    E[10] = False
    E[10, n // 2] = True
    E[20] = True
    E[30] = False
    E[30, [(n - 1) // 32 * 32, n - 1]] = True
    return E


def _monotone(n):
    T = np.flatnonzero(np.random.default_rng(n).random(n) < 0.6)
    return lambda rows: np.asarray(rows, bool)[:, T].sum(axis=1) >= 2


def _mod3(rows):
    rows = np.asarray(rows, bool)
    return (rows * np.arange(rows.shape[1])[None, :]).sum(axis=1) % 3 != 0


def _drive(H, L, E, fails):
    """The device walk of parents E under the predicate, checked against the mirror every round and at the end."""
    import torch
    from quits_amd.decoder.device import FaultShrinker
    n = H.shape[1]
    Hd, Ld = np.asarray(H.todense()).astype(np.float32), np.asarray(L.todense()).astype(np.float32)
    seen = []

    def recording(rows):
        seen.append(np.array(rows, bool))
        return fails(rows)
    want, log = shrink.shrink_mirror(E, recording, rounds=True)
    shr = FaultShrinker(H, L)
    packed = torch.from_numpy(shrink.pack_sets(E)).cuda()
    before = packed.clone()
    shr.begin(packed)
    for r, (par, flt) in enumerate(log):
        assert not shr.done and shr.live == par.size, "round %d: %d live rows, the mirror has %d" % (r, shr.live, par.size)
        det, obs, fault, parent = (t.cpu().numpy() for t in shr.trials())
        assert np.array_equal(parent, par) and np.array_equal(fault, flt), "round %d" % r
        T = seen[r]
        assert np.array_equal(det, ((T.astype(np.float32) @ Hd.T) % 2).astype(np.uint8)), "detector rows of round %d" % r
        assert np.array_equal(obs, ((T.astype(np.float32) @ Ld.T) % 2).astype(np.uint8)), "observable rows of round %d" % r
        v = fails(T)
        if r % 2:                                                   # both forms of the verdicts: a bool sequence, Tally.add's mask
            pad = np.zeros((par.size + 63) // 64 * 64, np.uint8)
            pad[:par.size] = v
            shr.commit(torch.from_numpy(np.packbits(pad, bitorder="little").view("<i8").copy()).cuda())
        else:
            shr.commit(v)
    assert shr.done and shr.rounds == len(log)
    assert torch.equal(packed, before), "begin() must copy the caller's sets"
    got = shr.result()
    S = shrink.unpack_sets(got.sets, n)
    assert np.array_equal(S, want.sets)
    for name in ("fails", "minimal", "start_weight", "weight", "trials"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert np.array_equal(shr.kept_det.cpu().numpy(), ((S.astype(np.float32) @ Hd.T) % 2).astype(np.uint8)), "kept H S"
    assert np.array_equal(shr.kept_obs.cpu().numpy(), ((S.astype(np.float32) @ Ld.T) % 2).astype(np.uint8)), "kept L S"
    assert (got.trials <= shrink.trial_bound(got.start_weight)).all()
    return got


@pytest.mark.parametrize("predicate", ["monotone", "mod3"])
@pytest.mark.parametrize("n", [10, 31, 32, 33, 64, 65, 66])
def test_device_equals_mirror_on_small_models(gpu, n, predicate):
    """Word boundaries on 7 detectors; every round's parents, faults and rows, then sets, flags, weights and trial counts."""
    H, L = _toy(n, 300 + n)
    got = _drive(H, L, _parents(n, n), _monotone(n) if predicate == "monotone" else _mod3)
    assert got.start_weight[3] == 0 and got.start_weight[10] == 1 and got.start_weight[20] == n and got.fails.any() and not got.fails.all()


@pytest.mark.parametrize("predicate", ["monotone", "mod3"])
def test_device_equals_mirror_on_a_wide_model(gpu, predicate):
    """n = 2100, m = 70, a column of weight 16 and an empty one; the full set (its members sum to a multiple of 3) and the full set without
    fault 1 (they do not) walk for thousands of rounds on their own."""
    H, L = _wide()
    assert H[:, 5].sum() == 16 and H[:, 7].sum() == 0
    E = _parents(2100, 1)
    E[21] = True
    E[21, 1] = False
    E[40, [5, 7, 900]] = True
    got = _drive(H, L, E, _monotone(2100) if predicate == "monotone" else _mod3)
    assert got.start_weight[20] == 2100 and got.start_weight[21] == 2099 and got.fails[21] and got.minimal[21] and got.trials[21] > 2100


def test_rows_as_column_slices_and_refused_arguments(gpu):
    """Every array a column slice of a wider one: the bytes and words outside keep their values, inside is what contiguous arrays get.  Then
    the refusals: strides too small, the live list compacted in place, more live rows than parents."""
    import torch
    from quits_amd.decoder.device import FaultShrinker
    n, m, k, words, P = 66, 7, 2, 3, 70
    H, L = _toy(n, 9)
    E = _parents(n, 2)
    ref = FaultShrinker(H, L)
    ref.begin(shrink.pack_sets(E))
    v0 = _mod3(E)
    ref_first = [t.clone() for t in ref.trials()]
    ref.commit(v0)
    A1 = ref.live
    Lb = ref._L
    dev = "cuda"
    sets = torch.full((P, words + 3), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    hs = torch.full((P, m + 4), 0x11, dtype=torch.uint8, device=dev)
    ls = torch.full((P, k + 6), 0x22, dtype=torch.uint8, device=dev)
    det = torch.full((P, m + 13), 0xAB, dtype=torch.uint8, device=dev)
    obs = torch.full((P, k + 5), 0xCD, dtype=torch.uint8, device=dev)
    sv, hv, lv, dv, ov = sets[:, 1:1 + words], hs[:, 2:2 + m], ls[:, 3:3 + k], det[:, 5:5 + m], obs[:, 2:2 + k]
    sv.copy_(torch.from_numpy(shrink.pack_sets(E)).cuda())
    ref.H.xor_apply(sv, hv, accumulate=False)
    ref.L.xor_apply(sv, lv, accumulate=False)
    state = torch.zeros((P, 8), dtype=torch.int32, device=dev)
    live = [torch.full((P,), -7, dtype=torch.int32, device=dev) for _ in range(2)]
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    fault = torch.empty((P,), dtype=torch.int32, device=dev)
    parent = torch.empty((P,), dtype=torch.int32, device=dev)
    pad = np.zeros(128, np.uint8)
    pad[:P] = v0
    mask = torch.from_numpy(np.packbits(pad, bitorder="little").view("<i8").copy()).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def begin(set_stride=sets.stride(0), hs_stride=hs.stride(0), ls_stride=ls.stride(0), det_stride=det.stride(0), obs_stride=obs.stride(0)):
        return Lb.qd_shrink_begin(ref.Ht._h, ref.Lt._h, p(sv), set_stride, P, p(state), p(live[0]), p(count), p(hv), hs_stride, p(lv), ls_stride,
                                  p(dv), det_stride, p(ov), obs_stride, p(fault), p(parent), sp)

    def step(A=P, nxt=1, det_stride=det.stride(0), obs_stride=obs.stride(0)):
        return Lb.qd_shrink_step(ref.Ht._h, ref.Lt._h, p(sv), sets.stride(0), P, p(state), p(live[0]), A, p(mask), p(live[nxt]), p(count), p(hv),
                                 hs.stride(0), p(lv), ls.stride(0), p(dv), det_stride, p(ov), obs_stride, p(fault), p(parent), sp)
    err = lambda: Lb.qd_last_error().decode()
    assert begin(set_stride=words - 1) == -1 and "set_stride_words" in err()
    assert begin(hs_stride=m - 1) == -1 and "detector row strides" in err()
    assert begin(det_stride=m - 1) == -1 and "detector row strides" in err()
    assert begin(ls_stride=k - 1) == -1 and "observable row strides" in err()
    assert begin(obs_stride=k - 1) == -1 and "observable row strides" in err()
    assert begin() == 0
    assert int(count.cpu()[0]) == P
    assert torch.equal(dv, ref_first[0]) and torch.equal(ov, ref_first[1]) and torch.equal(fault, ref_first[2]) and torch.equal(parent, ref_first[3])
    assert step(nxt=0) == -1 and "out of place" in err()
    assert step(A=P + 1) == -1 and "live rows" in err()
    assert step(det_stride=m - 1) == -1 and "detector row strides" in err()
    assert step(obs_stride=k - 1) == -1 and "observable row strides" in err()
    assert step() == 0
    assert int(count.cpu()[0]) == A1
    now = ref.trials()
    assert torch.equal(dv[:A1], now[0]) and torch.equal(ov[:A1], now[1]) and torch.equal(fault[:A1], now[2]) and torch.equal(parent[:A1], now[3])
    assert torch.equal(live[1][:A1], now[3]) and torch.equal(sv, ref.sets) and torch.equal(hv, ref.kept_det) and torch.equal(lv, ref.kept_obs)
    assert torch.equal(state, ref.state)
    for wide, lo, width, fill in ((det, 5, m, 0xAB), (obs, 2, k, 0xCD), (hs, 2, m, 0x11), (ls, 3, k, 0x22)):
        keep = torch.ones_like(wide, dtype=torch.bool)
        keep[:, lo:lo + width] = False
        assert bool((wide[keep] == fill).all())
    assert bool((sets[:, 0] == 0x5A5A5A5A).all()) and bool((sets[:, 1 + words:] == 0x5A5A5A5A).all())


# ---- end to end on the [[72,12,6]] code's 6-round circuit ---------------------------------------------------------------------------------
def _circuit_model():
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.dem import Circuit
    circ = Circuit(helpers.circuit_text(BB72))
    H, L, pri = detector_error_model_to_matrix(circ.detector_error_model())
    return circ, helpers.code("bb72"), H, L


@functools.lru_cache(maxsize=None)
def _run():
    """One run for the tests below: 2^12 DEM shots, W = 3, F = 1, min-sum 20 + OSD-0, every final set kept."""
    from quits_amd.simulation import get_minimal_failures
    circ, cd, H, L = _circuit_model()
    return get_minimal_failures(circ, cd["hz"], cd["lz"], 3, 1, SHOTS, seed=SEED, keep_sets=1 << 16, **MINSUM)


def _public_fails(decode):
    """rows bool [A, n] -> bool [A]: the definition's `fails` through a public sliding-window call on the host's detector bits."""
    from scipy.sparse import csr_matrix
    circ, cd, H, L = _circuit_model()
    Hs, Ls = csr_matrix(H).astype(np.int64), csr_matrix(L).astype(np.int64)

    def fails(rows):
        R = csr_matrix(np.asarray(rows, dtype=np.int64))
        det = np.asarray((R @ Hs.T).todense() % 2).astype(np.uint8)
        obs = np.asarray((R @ Ls.T).todense() % 2).astype(np.int64)
        if det.shape[0] == 0:
            return np.zeros(0, bool)
        return (np.asarray(decode(det, circ, cd["hz"], cd["lz"], 3, 1)) != obs).any(axis=1)
    return fails


def _bposd_fails():
    from quits_amd.decoder import sliding_window_bposd_circuit_mem
    return _public_fails(lambda det, *a: sliding_window_bposd_circuit_mem(det, *a, **MINSUM))


def _minimal_by(fails, sets):
    """Every set fails and none of its one-fault-removed children does, all rows in one call of `fails`."""
    rows, owner = [], []
    for i, s in enumerate(sets):
        members = np.flatnonzero(s)
        block = np.repeat(s[None, :], members.size + 1, axis=0)
        block[np.arange(1, members.size + 1), members] = False
        rows.append(block)
        owner += [(i, True)] + [(i, False)] * members.size
    v = fails(np.concatenate(rows))
    is_parent = np.array([o[1] for o in owner])
    assert v[is_parent].all(), "final sets that do not fail: %s" % [o[0] for o, x in zip(owner, v) if o[1] and not x][:8]
    assert not v[~is_parent].any(), "final sets with a failing child: %s" % sorted({o[0] for o, x in zip(owner, v) if not o[1] and x})[:8]
    return v.shape[0]


def test_shrinks_the_failures_of_the_fault_spectrum(gpu):
    """Same seed, same shots: `errors` is get_fault_spectrum's, every failing shot is a parent, every parent ends minimal, no set grows and
    the total shrinks (mean |E| = 14 on a distance-6 code: a run in which nothing shrinks is a finding)."""
    from quits_amd.simulation import get_fault_spectrum
    circ, cd, H, L = _circuit_model()
    r = _run()
    spec = get_fault_spectrum(circ, cd["hz"], cd["lz"], 3, 1, SHOTS, seed=SEED, **MINSUM)
    print("shots %d, errors %d, parents %d, rounds %d, decodes %d, start weights %.1f -> %.2f mean, lightest %s, lightest residual %s, %.2f s %s"
          % (r.shots, r.errors, r.parents, r.rounds, r.decodes, r.start_weights.mean(), r.weights.mean(), r.lightest, r.lightest_residual, r.seconds, r.timing))
    assert r.shots == spec.shots == SHOTS and r.errors == spec.errors and r.parents == r.errors > 100 and r.parents_truncated == 0
    assert np.array_equal(r.start_weight_hist, spec.errors_by_faults)
    assert r.minimal.all() and r.minimal.shape == (r.parents,)
    assert (r.weights <= r.start_weights).all() and r.weights.sum() < r.start_weights.sum()
    assert (r.trials <= shrink.trial_bound(r.start_weights)).all() and r.trials.sum() == r.decodes and r.rounds == r.trials.max()
    assert r.weight_hist.sum() == r.parents and np.array_equal(r.weight_hist, np.bincount(r.weights, minlength=256))
    assert np.array_equal(r.set_weights, np.sort(r.weights)) and r.lightest == (r.set_weights[0], r.set_shots[0])
    assert np.array_equal(np.sort(r.set_shots), r.parent_shots) and np.array_equal(r.parent_shots, np.sort(r.parent_shots))
    assert np.array_equal(shrink.unpack_sets(r.sets, H.shape[1]).sum(axis=1), r.set_weights)


def test_final_sets_are_one_minimal_for_the_public_decoder(gpu):
    """Independent of the shrinker's own decodes: every final set, with its children, through sliding_window_bposd_circuit_mem in one call."""
    circ, cd, H, L = _circuit_model()
    r = _run()
    rows = _minimal_by(_bposd_fails(), shrink.unpack_sets(r.sets, H.shape[1]))
    print("%d final sets and children decoded" % rows)


def test_first_parents_equal_the_mirror(gpu):
    """The first 64 parents: shrink_mirror on their replayed fault sets, driven by the public call, ends on the same sets after the same trials."""
    from quits_amd.simulation import replay_faults
    circ, cd, H, L = _circuit_model()
    r = _run()
    first = r.parent_shots[:64]
    E = replay_faults(circ, first, SEED)
    assert np.array_equal(E.sum(axis=1), r.start_weights[:64])
    want = shrink.shrink_mirror(E, _bposd_fails())
    at = {int(s): i for i, s in enumerate(r.set_shots)}
    got = shrink.unpack_sets(r.sets[[at[int(s)] for s in first]], H.shape[1])
    assert want.fails.all() and want.minimal.all()
    assert np.array_equal(got, want.sets) and np.array_equal(r.trials[:64], want.trials) and np.array_equal(r.weights[:64], want.weight)


def test_result_does_not_depend_on_the_batch(gpu):
    from quits_amd.simulation import get_minimal_failures
    circ, cd, H, L = _circuit_model()
    r = _run()
    o = get_minimal_failures(circ, cd["hz"], cd["lz"], 3, 1, SHOTS, seed=SEED, keep_sets=1 << 16, batch=192, **MINSUM)
    assert o.batch == 192 and o.batch != r.batch
    assert (o.shots, o.errors, o.parents, o.rounds, o.decodes, o.lightest, o.lightest_residual) == (r.shots, r.errors, r.parents, r.rounds, r.decodes, r.lightest, r.lightest_residual)
    for name in ("sets", "set_shots", "set_weights", "parent_shots", "weights", "trials", "minimal", "residual_weight_hist", "weight_hist"):
        assert np.array_equal(getattr(o, name), getattr(r, name)), name


def test_lightest_set_and_lightest_residual_replay(gpu):
    """The lightest set is a subset of its shot's sampled faults; the lightest residual, recomputed through sliding_window_corrections from its
    set, has the stated weight, no syndrome and a logical effect."""
    from scipy.sparse import csr_matrix
    from quits_amd.decoder import sliding_window_corrections
    from quits_amd.simulation import replay_faults
    circ, cd, H, L = _circuit_model()
    r = _run()
    n = H.shape[1]
    w, shot = r.lightest
    S = shrink.unpack_sets(r.sets[:1], n)[0]
    assert S.sum() == w == r.weights.min() and not (S & ~replay_faults(circ, [shot], SEED)[0]).any()
    rw, rshot = r.lightest_residual
    assert r.residual_weight_hist[:rw].sum() == 0 and r.residual_weight_hist[min(rw, 255)] >= 1 and r.residual_weight_hist.sum() <= r.parents
    S = shrink.unpack_sets(r.sets[np.flatnonzero(r.set_shots == rshot)], n)[0]
    det = np.asarray((csr_matrix(H) @ S.astype(np.int64)) % 2).astype(np.uint8).reshape(1, -1)
    pred, packed = sliding_window_corrections(det, circ, cd["hz"], cd["lz"], 3, 1, **MINSUM)
    resid = S.astype(np.uint8) ^ np.asarray(packed)[0]
    assert resid.sum() == rw
    assert not ((csr_matrix(H) @ resid.astype(np.int64)) % 2).any() and ((csr_matrix(L) @ resid.astype(np.int64)) % 2).any()


def test_public_shrink_of_given_sets(gpu):
    """shrink_fault_sets on the first parents as bool rows and as packed words: get_minimal_failures's sets; a set that does not fail stays."""
    from quits_amd.simulation import replay_faults, shrink_fault_sets
    circ, cd, H, L = _circuit_model()
    r = _run()
    E = replay_faults(circ, r.parent_shots[:16], SEED)
    E = np.concatenate([E, np.zeros((1, E.shape[1]), bool)])
    a = shrink_fault_sets(circ, cd["hz"], cd["lz"], 3, 1, E, **MINSUM)
    b = shrink_fault_sets(circ, cd["hz"], cd["lz"], 3, 1, shrink.pack_sets(E), **MINSUM)
    assert a.sets.dtype == np.bool_ and b.sets.dtype == np.int32 and np.array_equal(shrink.unpack_sets(b.sets, E.shape[1]), a.sets)
    assert a.fails[:16].all() and a.minimal[:16].all() and not a.fails[16] and not a.minimal[16] and a.trials[16] == 1
    assert np.array_equal(a.weight[:16], r.weights[:16]) and np.array_equal(a.trials[:16], r.trials[:16]) and np.array_equal(a.start_weight[:16], r.start_weights[:16])


def test_stratified_parents(gpu):
    """shots_per_weight: the failures of get_stratified_pL's rows are the parents."""
    from quits_amd.simulation import get_minimal_failures, get_stratified_pL, replay_strata_faults
    circ, cd, H, L = _circuit_model()
    a = (circ, cd["hz"], cd["lz"], 3, 1)
    r = get_minimal_failures(*a, 0, seed=SEED, shots_per_weight={14: SHOTS}, keep_sets=1 << 16, **MINSUM)
    s = get_stratified_pL(*a, {14: SHOTS}, seed=SEED, **MINSUM)
    assert r.shots == SHOTS and r.errors == s.errors_by_faults[14] > 0 and r.parents == r.errors
    assert r.minimal.all() and (r.start_weights == 14).all() and (r.parent_strata == 14).all() and r.weights.sum() < r.start_weights.sum()
    S = shrink.unpack_sets(r.sets[:8], H.shape[1])
    E = replay_strata_faults(circ, 14, r.set_shots[:8], SEED)
    assert not (S & ~E).any() and np.array_equal(S.sum(axis=1), r.set_weights[:8])
    _minimal_by(_bposd_fails(), S)
    z = get_minimal_failures(*a, 0, seed=SEED, shots_per_weight={0: 64}, **MINSUM)          # no fault, no failure, no parent: nothing to shrink
    assert (z.shots, z.errors, z.parents, z.rounds, z.decodes, z.lightest, z.lightest_residual) == (64, 0, 0, 0, 0, None, None)
    assert z.sets.shape == (0, (H.shape[1] + 31) // 32) and z.weight_hist.sum() == 0


def test_relay_bp(gpu):
    """get_relay_minimal_failures, a short Relay-BP configuration without a post-processor: the same 1-minimality through the public Relay-BP call."""
    from quits_amd.decoder.relaybp import sliding_window_relaybp_circuit_mem
    from quits_amd.relay import RelayConfig
    from quits_amd.simulation import get_relay_minimal_failures
    circ, cd, H, L = _circuit_model()
    cfg = RelayConfig(pre_iter=20, num_sets=3, set_max_iter=20)
    r = get_relay_minimal_failures(circ, cd["hz"], cd["lz"], 3, 1, 512, relay=cfg, osd_method="osd_off", seed=SEED, keep_sets=1 << 16)
    print("Relay-BP: %d errors of %d, start weights %.1f -> %.2f mean, lightest %s, %d rounds" % (r.errors, r.shots, r.start_weights.mean() if r.parents else 0,
                                                                                                 r.weights.mean() if r.parents else 0, r.lightest, r.rounds))
    assert r.shots == 512 and r.parents == r.errors > 0 and r.minimal.all() and (r.weights <= r.start_weights).all()
    fails = _public_fails(lambda det, *a: sliding_window_relaybp_circuit_mem(det, *a, relay=cfg, osd_method="osd_off"))
    _minimal_by(fails, shrink.unpack_sets(r.sets, H.shape[1]))
