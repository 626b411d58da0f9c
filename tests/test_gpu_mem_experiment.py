"""The device-resident memory experiment on the MI355X: get_circuit_mem_pL against the reference-shaped flow (samples to the host,
sliding_window_bposd_circuit_mem, numpy), its independence of the batch size, shards, the early stop, qd_tally_batch and
qd_shot_flags_fold against numpy, list sampling of both samplers against contiguous sampling and the CPU mirrors, the replay round trip.

Shape throughout: bb72_custom_r6_p0.003, W = 3 / F = 1 (six windows), minimum_sum / parallel / max_iter = 20 / osd_0.  The CPU oracle's
loop on 6000 DEM-sampled shots of it gives 720 failing shots and 10 719 post-processed window decodes, so the floors asserted below
(>= 100 failing shots, >= 100 post-processed shots) are far from the edge; an input that misses them fails the test."""
import numpy as np
import pytest

import channel_circuits as cc_
import frame_mirror as fm
import frame_mirror_channels as fmc
import helpers

NAME = "bb72_custom_r6_p0.003"
W, F, R = 3, 1, 6
KW = dict(max_iter=20, osd_order=0, bp_method="minimum_sum", schedule="parallel", osd_method="osd_0")
N, SEED = 6000, 11
FLOOR = 100
BIG_SEED = (0x9E3779B9 << 32) | 0x7F4A7C15          # both halves non-zero


def _run(text, cd, **kw):
    from quits_amd.simulation import get_circuit_mem_pL
    return get_circuit_mem_pL(text, cd["hz"], cd["lz"], W, F, kw.pop("num_trials", N), **KW, seed=kw.pop("seed", SEED), **kw)


def _same(a, b):
    return (a.shots == b.shots and a.errors == b.errors and np.array_equal(a.per_observable_errors, b.per_observable_errors)
            and a.flagged == b.flagged and np.array_equal(a.failing_shots, b.failing_shots) and a.failures_truncated == b.failures_truncated)


@pytest.fixture(scope="module")
def text():
    return helpers.circuit_text(NAME)


@pytest.fixture(scope="module")
def cd():
    return helpers.code("bb72")


@pytest.fixture(scope="module")
def full(gpu, text, cd):
    """The experiment every comparison shares: 6000 circuit-sampled shots in three batches, the last one partial, every failure kept."""
    r = _run(text, cd, batch=2048, keep_failures=N)
    print("full run: %d shots, %d errors, flagged %s, %.0f shots/s" % (r.shots, r.errors, r.flagged, r.shots_per_s))
    assert r.errors >= FLOOR and r.flagged["post"][0] >= FLOOR
    return r


def _reference_flow(text, cd, det, obs):
    """What the reference's users do with host arrays: decode, compare with numpy."""
    from quits_amd.decoder import sliding_window_bposd_circuit_mem
    pred = sliding_window_bposd_circuit_mem(det, text, cd["hz"], cd["lz"], W, F, **KW)
    miss = pred.astype(bool) != obs.astype(bool)
    return miss.any(axis=1), miss.sum(axis=0)


def _post_counts(text, cd, det_dev, fail):
    """Shots some window of which the post-processor decoded, and the failing ones among them: from plan.decode's status words, by torch."""
    import torch
    from quits_amd.decoder.sliding_window import build_circuit_plan
    from quits_amd.dem import Circuit
    opts = {k: KW[k] for k in ("bp_method", "max_iter", "schedule", "osd_method", "osd_order")}
    plan = build_circuit_plan(Circuit(text), cd["hz"], W, F, R, dict(opts), dict(opts))
    stats = []
    plan.decode(det_dev, stats)
    post = torch.zeros((det_dev.shape[0],), dtype=torch.bool, device=det_dev.device)
    at = [0] * len(plan.windows)
    for k, st in stats:
        post[at[k]:at[k] + st.shape[0]] |= ((st >> 17) & 1).bool()
        at[k] += st.shape[0]
    post = post.cpu().numpy()
    return int(post.sum()), int((post & fail).sum())


@pytest.mark.gpu
def test_equals_the_reference_shaped_flow(gpu, text, cd, full):
    import torch
    from quits_amd.simulation import get_circuit_mem_result
    det, obs = get_circuit_mem_result(text, N, seed=SEED)
    fail, per_obs = _reference_flow(text, cd, det, obs)
    print("reference flow: %d failing shots, per observable %s" % (int(fail.sum()), per_obs.tolist()))
    assert int(fail.sum()) >= FLOOR
    assert full.shots == N and full.errors == int(fail.sum())
    assert np.array_equal(full.per_observable_errors, per_obs)
    assert np.array_equal(full.failing_shots, np.flatnonzero(fail)) and not full.failures_truncated
    assert full.failing_shots.dtype == np.int64
    post = _post_counts(text, cd, torch.from_numpy(det.view(np.uint8)).to("cuda"), fail)
    assert post[0] >= FLOOR and full.flagged["post"] == post
    assert full.pL == full.errors / N and (full.seed, full.sampler, full.batch) == (SEED, "circuit", 2048)


@pytest.mark.gpu
def test_equals_the_reference_shaped_flow_dem_sampler(gpu, text, cd):
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.decoder.device import DemSampler
    from quits_amd.dem import Circuit
    H, L, pri = detector_error_model_to_matrix(Circuit(text).detector_error_model())
    det_dev, obs_dev = DemSampler(H, L, pri).sample(N, seed=SEED)
    det, obs = det_dev.cpu().numpy(), obs_dev.cpu().numpy()
    fail, per_obs = _reference_flow(text, cd, det, obs)
    r = _run(text, cd, batch=2048, keep_failures=N, sampler="dem")
    print("dem sampler: %d failing shots (reference flow %d), flagged %s" % (r.errors, int(fail.sum()), r.flagged))
    assert int(fail.sum()) >= FLOOR
    assert r.shots == N and r.errors == int(fail.sum()) and np.array_equal(r.per_observable_errors, per_obs)
    assert np.array_equal(r.failing_shots, np.flatnonzero(fail)) and r.sampler == "dem"
    post = _post_counts(text, cd, det_dev, fail)
    assert post[0] >= FLOOR and r.flagged["post"] == post


@pytest.mark.gpu
@pytest.mark.parametrize("batch,rounded", [(1000, 1024), (4096, 4096), (6000, 6016)])
def test_result_does_not_depend_on_the_batch(gpu, text, cd, full, batch, rounded):
    r = _run(text, cd, batch=batch, keep_failures=N)
    assert r.batch == rounded and _same(r, full)


@pytest.mark.gpu
def test_two_stream_driver_gives_the_same(gpu, text, cd, full, monkeypatch):
    """A batch of three plan chunks (chunks of 1024 shots) goes through the two-stream driver, whose status words arrive as views of one
    table: same tallies, same failing shots."""
    from quits_amd.decoder import pipeline
    from quits_amd.decoder import sliding_window as sw
    calls = []
    impl = pipeline.decode_pipelined
    monkeypatch.setattr(pipeline, "decode_pipelined", lambda plan, det, stats, ready=None: calls.append(det.shape[0]) or impl(plan, det, stats, ready))
    monkeypatch.setenv("QD_CHUNK_SHOTS", "1024")
    sw.plan_cache_clear()                                  # the cached plan has the default chunk
    try:
        r = _run(text, cd, batch=3072, keep_failures=N)
    finally:
        sw.plan_cache_clear()
    assert calls == [3072, N - 3072]
    assert _same(r, full)


@pytest.mark.gpu
def test_shards_add_up(gpu, text, cd, full):
    parts = [_run(text, cd, batch=1024, keep_failures=N, shard=(r, 3)) for r in range(3)]
    assert [p.shots for p in parts] == [2000, 2000, 2000]
    assert sum(p.errors for p in parts) == full.errors
    assert np.array_equal(sum(p.per_observable_errors for p in parts), full.per_observable_errors)
    for name in full.flagged:
        assert tuple(sum(p.flagged[name][j] for p in parts) for j in (0, 1)) == full.flagged[name]
    assert np.array_equal(np.concatenate([p.failing_shots for p in parts]), full.failing_shots)       # global indices, rank after rank
    assert all(p.errors > 0 for p in parts)


@pytest.mark.gpu
def test_early_stop_follows_the_documented_rule(gpu, text, cd, full):
    """max_errors = 200, batches of 1024: batch i >= 2 is issued iff fewer than 200 of the shots of batches 0 .. i - 2 failed."""
    limit, step = 200, 1024
    fails = full.failing_shots
    nb = -(-N // step)
    issued = nb
    for i in range(2, nb):
        if int((fails < (i - 1) * step).sum()) >= limit:
            issued = i
            break
    shots = min(N, issued * step)
    assert 2 * step < shots < N, shots                      # the stop is exercised, and not by the two batches that are always issued
    r = _run(text, cd, batch=step, max_errors=limit, keep_failures=N)
    print("early stop: %d shots, %d errors" % (r.shots, r.errors))
    assert r.shots == shots and r.errors == int((fails < shots).sum()) and r.errors >= limit
    assert np.array_equal(r.failing_shots, fails[fails < shots])
    few = _run(text, cd, batch=step, max_errors=limit, keep_failures=16)
    assert np.array_equal(few.failing_shots, fails[:16]) and few.failures_truncated and few.errors == r.errors
    none = _run(text, cd, batch=step, keep_failures=0)
    assert none.errors == full.errors and none.failing_shots.shape == (0,) and not none.failures_truncated


def _tally_reference(pred, obs, flags):
    miss = ((pred ^ obs) & 1).astype(bool)
    fail = miss.any(axis=1)
    head = [pred.shape[0], int(fail.sum())]
    for j in range(4):
        bit = ((flags >> j) & 1).astype(bool) if flags is not None else np.zeros(pred.shape[0], bool)
        head += [int(bit.sum()), int((bit & fail).sum())]
    words = np.zeros((pred.shape[0] + 63) // 64, dtype=np.uint64)
    for b in np.flatnonzero(fail):
        words[b >> 6] |= np.uint64(1) << np.uint64(b & 63)
    return np.array(head + miss.sum(axis=0).tolist(), dtype=np.int64), words


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 12, 136])
def test_tally_against_numpy(gpu, k):
    """Crafted inputs: bytes with high bits set (only the low bit counts), row strides > k (column slices of wider arrays), with and
    without flags, two calls accumulating, the fail mask's words and its zero bits past B; 300 000 rows are 1172 pieces of 256 for the
    bounded grid of 1024 workgroups, so the first 148 of them take a second stride and the others one (k = 12 only)."""
    import torch
    from quits_amd.decoder.device import Tally
    rng = np.random.default_rng(1000 + k)
    for B in [0, 1, 63, 64, 65, 1000] + ([300000] if k == 12 else []):
        wide_p = rng.integers(0, 256, (B, k + 5), dtype=np.uint8)
        wide_o = wide_p[:, :k + 3].copy()                                     # its own array: rows of k + 3 bytes
        wide_o[:, :k] = wide_p[:, 2:2 + k] ^ (rng.random((B, k)) < 0.1)       # one low bit in ten differs
        wide_o[:, :k] ^= (rng.integers(0, 128, (B, k), dtype=np.uint8) << 1)  # ... and the high bits at random
        flags = rng.integers(0, 16, (B,), dtype=np.uint8)
        dp, do, df = torch.from_numpy(wide_p).cuda(), torch.from_numpy(wide_o).cuda(), torch.from_numpy(flags).cuda()
        pred, obs = dp[:, 2:2 + k], do[:, :k]
        assert B == 0 or (pred.stride(0) == k + 5 and obs.stride(0) == k + 3)
        ref, words = _tally_reference(wide_p[:, 2:2 + k], wide_o[:, :k], flags)
        ref_nf, _ = _tally_reference(wide_p[:, 2:2 + k], wide_o[:, :k], None)
        nw = (B + 63) // 64
        mask = torch.full((nw + 2,), -1, dtype=torch.int64, device="cuda")
        t = Tally(k)
        t.add(pred, obs, df, mask)
        got = t.counts()
        assert got.dtype == np.int64 and got.shape == (10 + k,)
        assert np.array_equal(got, ref), (B, got[:10], ref[:10])
        m = mask.cpu().numpy().view(np.uint64)
        assert np.array_equal(m[:nw], words) and (m[nw:] == np.uint64(2 ** 64 - 1)).all()     # written up to ceil(B / 64) words, no further
        t.add(pred, obs)                                                   # no flags, no mask: accumulates
        assert np.array_equal(t.counts(), ref + ref_nf)
        if B >= 63:
            assert ref[1] > 0 and ref[10:].sum() >= ref[1]


@pytest.mark.gpu
def test_shot_flags_fold_against_numpy(gpu):
    import torch
    from quits_amd import _lib
    from quits_amd.decoder.device import shot_flags_fold
    rng = np.random.default_rng(5)
    for B in (0, 1, 255, 256, 1000):
        flags = torch.zeros((B,), dtype=torch.uint8, device="cuda")
        want = np.zeros(B, dtype=np.uint8)
        for call in range(2):                                              # the fold ORs over calls (one per window)
            st = (rng.integers(0, 64, (B,), dtype=np.int64) << 14 | rng.integers(0, 1 << 14, (B,), dtype=np.int64)).astype(np.int32)
            shot_flags_fold(torch.from_numpy(st).cuda(), flags)
            want |= (((st & _lib.STATUS_OSD) != 0) * 1 + ((st & _lib.STATUS_INCONSISTENT) != 0) * 2 + ((st & _lib.STATUS_INEXACT) != 0) * 4
                     + ((st & _lib.STATUS_COARSE_GRID) != 0) * 8).astype(np.uint8)
            assert np.array_equal(flags.cpu().numpy(), want)
            assert call or B < 255 or len(set(want.tolist())) == 16         # every combination of the four bits occurs


def _indices(B, span, rng):
    idx = rng.integers(0, span, (B,), dtype=np.int64)                      # unsorted
    if B >= 2:
        idx[B // 2] = idx[0]                                               # with a repeat
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["circuit", "dem", "circuit_channels"])
def test_list_sampling_equals_rows_of_a_contiguous_sample(gpu, text, which):
    import torch
    from quits_amd.simulation import _as_circuit, _make_sampler
    if which == "circuit_channels":
        s = _make_sampler(_as_circuit(cc_.biased(text)), "circuit")
        assert s.info()["detectors"] == 288
    else:
        s = _make_sampler(_as_circuit(text), which)
    shot0, span = 1000003, 2000
    det, obs = s.sample(span, BIG_SEED, shot0)
    assert bool(det.any()) and bool(obs.any())
    rng = np.random.default_rng(3)
    for B in (0, 1, 65, 300):
        idx = _indices(B, span, rng)
        d, o = s.sample_shots(torch.from_numpy(idx + shot0).cuda() if B == 65 else (idx + shot0).tolist(), BIG_SEED)
        assert d.shape == (B, s.m) and o.shape == (B, s.nobs) and d.dtype == torch.uint8
        at = torch.from_numpy(idx).cuda()
        assert torch.equal(d, det[at]) and torch.equal(o, obs[at])
    with pytest.raises(ValueError):
        s.sample_shots([3, -1], BIG_SEED)


@pytest.mark.gpu
def test_list_sampling_beyond_2_to_32_equals_the_cpu_mirrors(gpu, text):
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.decoder.device import CircuitSampler, DemSampler
    from quits_amd.dem import Circuit
    import oracle as orc
    base = 2 ** 32 + 5
    order = np.array([5, 0, 7, 2, 2, 6, 1, 4, 3], dtype=np.int64)
    idx = (base + order).tolist()
    det, obs = CircuitSampler(text).sample_shots(idx, BIG_SEED)
    rdet, robs = fm.sample(text, BIG_SEED, base, 8)
    assert rdet.any()
    assert np.array_equal(det.cpu().numpy(), rdet[order]) and np.array_equal(obs.cpu().numpy(), robs[order])
    biased = cc_.biased(text)
    det, obs = CircuitSampler(biased).sample_shots(idx, BIG_SEED)
    rdet, robs = fmc.sample(biased, BIG_SEED, base, 8)
    assert rdet.any()
    assert np.array_equal(det.cpu().numpy(), rdet[order]) and np.array_equal(obs.cpu().numpy(), robs[order])
    H, L, pri = detector_error_model_to_matrix(Circuit(text).detector_error_model())
    det, obs = DemSampler(H, L, pri).sample_shots(idx, BIG_SEED)
    rdet, robs, _ = orc.sample_dem(H, L, pri, BIG_SEED, base, 8)
    assert rdet.any()
    assert np.array_equal(det.cpu().numpy(), rdet[order]) and np.array_equal(obs.cpu().numpy(), robs[order])


@pytest.mark.gpu
def test_replay_round_trip(gpu, text, cd, full):
    """The failing shots, regenerated from their indices and decoded through the public call, all fail again; 64 others do not."""
    from quits_amd.decoder import sliding_window_bposd_circuit_mem
    from quits_amd.simulation import replay_shots
    det, obs = replay_shots(text, full.failing_shots, SEED)
    assert det.dtype == np.bool_ and det.shape == (full.errors, 288) and obs.shape == (full.errors, 12)
    pred = sliding_window_bposd_circuit_mem(det, text, cd["hz"], cd["lz"], W, F, **KW)
    assert (pred.astype(bool) != obs).any(axis=1).all()
    good = np.setdiff1d(np.arange(N), full.failing_shots)[::-1][:64]          # descending: any order will do
    det, obs = replay_shots(text, good, SEED)
    pred = sliding_window_bposd_circuit_mem(det, text, cd["hz"], cd["lz"], W, F, **KW)
    assert not (pred.astype(bool) != obs).any()


def test_experiment_kernels_use_no_scratch(tmp_path):
    from test_api import _resource_usage
    kern = [(n, sc) for n, sc in _resource_usage(tmp_path, "experiment.hip") if "qd_" in n]
    assert sorted(n.split("qd_")[1][:10] for n, _ in kern) == ["shot_flags", "tally_kern"], kern
    assert all(sc == 0 for _, sc in kern), kern
