"""The device-resident memory experiment (quits_amd.simulation.get_circuit_mem_pL), the parts that need no GPU: how the shots are cut
into batches, the early-stop rule as arithmetic, the result's arithmetic, the public signature, the C ABI's new names."""
import inspect
import os
import re

import numpy as np
import pytest

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["qd_shot_flags_fold", "qd_tally_batch", "qd_sample_circuit_shots", "qd_sample_dem_shots"]


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("N", [0, 1, 63, 64, 6000])
def test_experiment_batches_tile_the_shots_once(N, world):
    from quits_amd.simulation import experiment_batches
    for batch in (1, 64, 100, 1000, 1024, 4096, 6000, 10 ** 6):
        step = (batch + 63) // 64 * 64
        cover = np.zeros(N, dtype=np.int64)
        edge = 0
        for rank in range(world):
            bs = experiment_batches(N, batch, rank, world)
            assert all(n > 0 for _, n in bs)
            assert all(n == step for _, n in bs[:-1])                  # every batch but a rank's last: the rounded size, a multiple of 64
            assert all(n <= step for _, n in bs)
            for (s0, n), nxt in zip(bs, bs[1:] + [None]):
                assert s0 == edge                                          # in order, no gap: inside a rank and from one rank to the next
                cover[s0:s0 + n] += 1
                edge = s0 + n
                assert nxt is None or nxt[0] == edge
        assert edge == N and (cover == 1).all()
    assert experiment_batches(6000, 2048) == [(0, 2048), (2048, 2048), (4096, 1904)]
    assert experiment_batches(6000, 1000, 1, 3) == [(2000, 1024), (3024, 976)]
    with pytest.raises(ValueError):
        experiment_batches(10, 0)


def test_early_stop_rule_as_arithmetic():
    from quits_amd.simulation import experiment_batches, shots_before_stop
    bs = experiment_batches(6000, 1024)
    assert len(bs) == 6
    fails = np.arange(0, 6000, 8)                                          # 128 failing shots per full batch
    assert shots_before_stop(bs, fails, 10 ** 9) == 6
    assert shots_before_stop(bs, fails, 1) == 2                            # the first two batches are always issued
    assert shots_before_stop(bs, fails, 128) == 2 and shots_before_stop(bs, fails, 129) == 3
    assert shots_before_stop(bs, fails, 256) == 3 and shots_before_stop(bs, fails, 257) == 4
    assert shots_before_stop(bs, fails, 512) == 5 and shots_before_stop(bs, fails, 513) == 6
    assert shots_before_stop(bs[:1], fails, 1) == 1 and shots_before_stop([], fails, 1) == 0
    # a rank's slice counts its own failures only
    bs1 = experiment_batches(6000, 1024, 1, 2)
    assert bs1[0][0] == 3000 and shots_before_stop(bs1, fails, 129) == 3


def test_decoder_keywords_are_the_sliding_window_call_s():
    from quits_amd.decoder import sliding_window_bposd_circuit_mem
    from quits_amd.simulation import get_circuit_mem_pL, replay_shots
    ref = inspect.signature(sliding_window_bposd_circuit_mem).parameters
    sig = inspect.signature(get_circuit_mem_pL).parameters
    names = list(sig)
    assert names[:6] == ["circuit", "hz", "lz", "W", "F", "num_trials"]
    dec = [n for n in ref if n not in ("zcheck_samples", "circuit", "hz", "lz", "W", "F", "tqdm_on")]
    assert dec == ["max_iter", "osd_order", "bp_method", "schedule", "osd_method"]
    assert names[6:11] == dec
    for n in dec:
        assert sig[n].default == ref[n].default and sig[n].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
    extra = names[11:]
    assert extra == ["seed", "sampler", "batch", "max_errors", "keep_failures", "shard", "distributed"]
    assert all(sig[n].kind == inspect.Parameter.KEYWORD_ONLY for n in extra)
    assert [sig[n].default for n in extra] == [0, "circuit", None, None, 4096, None, False]
    assert list(inspect.signature(replay_shots).parameters) == ["circuit", "shot_indices", "seed", "sampler"]


def test_result_arithmetic():
    from quits_amd.simulation import MemExperimentResult
    counts = np.array([6000, 720, 3000, 700, 5, 5, 0, 0, 40, 12] + [300 + i for i in range(12)], dtype=np.int64)
    r = MemExperimentResult.from_counts(counts, failing_shots=[3, 9, 4000], failures_truncated=True, seed=11, sampler="dem", batch=2048, seconds=0.5)
    assert (r.shots, r.errors) == (6000, 720) and r.pL == pytest.approx(0.12)
    assert r.sigma == pytest.approx(np.sqrt(0.12 * 0.88 / 6000))
    assert r.per_observable_errors.dtype == np.int64 and r.per_observable_errors.tolist() == [300 + i for i in range(12)]
    assert r.flagged == {"post": (3000, 700), "inconsistent": (5, 5), "inexact": (0, 0), "coarse": (40, 12)}
    assert r.failing_shots.dtype == np.int64 and r.failing_shots.tolist() == [3, 9, 4000] and r.failures_truncated
    assert (r.seed, r.sampler, r.batch) == (11, "dem", 2048) and r.shots_per_s == pytest.approx(12000.0)
    empty = MemExperimentResult.from_counts(np.zeros(10 + 12, np.int64))
    assert empty.shots == 0 and np.isnan(empty.pL) and empty.failing_shots.shape == (0,) and empty.shots_per_s == 0.0


def test_fail_mask_words_to_indices():
    from quits_amd.simulation import _mask_to_indices
    words = np.zeros(5, dtype=np.uint64)
    words[0] = (1 << 0) | (1 << 63)
    words[3] = 1 << 7
    idx, more = _mask_to_indices(words, 1000, 10)
    assert idx.tolist() == [1000, 1063, 1000 + 3 * 64 + 7] and not more and idx.dtype == np.int64
    idx, more = _mask_to_indices(words, 2 ** 40, 2)
    assert idx.tolist() == [2 ** 40, 2 ** 40 + 63] and more
    idx, more = _mask_to_indices(np.zeros(0, np.uint64), 0, 4)
    assert idx.shape == (0,) and not more


def test_header_and_binding_hold_the_new_entry_points():
    from quits_amd import _lib
    text = open(os.path.join(ROOT, "include", "quits_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.EXPORTS
    for macro, value in (("QD_SHOT_POST", 1), ("QD_SHOT_INCONSISTENT", 2), ("QD_SHOT_INEXACT", 4), ("QD_SHOT_COARSE", 8), ("QD_TALLY_HEAD", 10)):
        assert re.search(r"#define %s %d\b" % (macro, value), code), macro
    assert (_lib.SHOT_POST, _lib.SHOT_INCONSISTENT, _lib.SHOT_INEXACT, _lib.SHOT_COARSE, _lib.TALLY_HEAD) == (1, 2, 4, 8, 10)
    L = _lib.load()
    assert L.qd_version() >= 108 and all(hasattr(L, n) for n in NEW_EXPORTS)
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)


def test_argument_checks_need_no_gpu():
    """B = 0 is QD_OK whatever the pointers; null pointers and bad sizes are QD_EINVAL with a message; nothing is launched."""
    from quits_amd import _lib
    L = _lib.load()
    assert L.qd_shot_flags_fold(None, 0, None, None) == 0
    assert L.qd_tally_batch(None, 0, None, 0, 12, 0, None, None, None, None) == 0
    assert L.qd_sample_circuit_shots(None, 1, None, 0, None, 0, None, 0, None) == 0
    assert L.qd_sample_dem_shots(None, None, None, 1, None, 0, None, 0, None, 0, None) == 0
    assert L.qd_shot_flags_fold(None, 5, None, None) == -1 and b"null" in L.qd_last_error()
    assert L.qd_tally_batch(None, 12, None, 12, 12, 5, None, None, None, None) == -1 and b"null" in L.qd_last_error()
    assert L.qd_tally_batch(64, 12, 64, 12, 0, 5, None, 64, None, None) == -1 and b"observables" in L.qd_last_error()
    assert L.qd_tally_batch(64, 11, 64, 12, 12, 5, None, 64, None, None) == -1 and b"stride" in L.qd_last_error()
    assert L.qd_sample_circuit_shots(None, 1, None, 5, None, 0, None, 0, None) == -1 and b"null circuit" in L.qd_last_error()
    assert L.qd_sample_dem_shots(None, None, None, 1, None, 5, None, 0, None, 0, None) == -1 and b"null" in L.qd_last_error()


def test_no_device_is_an_error_not_a_fallback(monkeypatch):
    import torch
    from quits_amd.simulation import get_circuit_mem_pL, replay_shots
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)         # (what a machine without a GPU reports)
    cd = helpers.code("bb72")
    text = helpers.circuit_text("bb72_custom_r6_p0.003")
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
        get_circuit_mem_pL(text, cd["hz"], cd["lz"], 3, 1, 1000)
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
        replay_shots(text, [1, 2, 3], 0)


REDUCE_WORKER = r"""
import json, sys
sys.path.insert(0, %(root)r)
import numpy as np
from quits_amd import parallel
from quits_amd.simulation import MemExperimentResult
rank, world, _ = parallel.env_rank_world()
dist = parallel.init_distributed("gloo")
counts = np.arange(22, dtype=np.int64) * (rank + 1)
counts[0] = (1 << 40) + rank                                             # beyond 2^32: the collective carries int64
total = parallel.reduce_vector(dist, counts)
r = MemExperimentResult.from_counts(total)
if rank == 0:
    print(json.dumps({"total": total.tolist(), "shots": r.shots, "errors": r.errors}))
dist.barrier(); dist.destroy_process_group()
"""


def test_counts_are_summed_over_ranks_in_one_vector(tmp_path):
    """distributed=True sums the whole counter vector with one all-reduce (parallel.reduce_vector): two gloo ranks here."""
    import json
    import subprocess
    import sys
    from quits_amd import parallel
    assert parallel.reduce_vector(None, [1, 2, 3]).tolist() == [1, 2, 3]       # no process group: identity
    script = tmp_path / "reduce_worker.py"
    script.write_text(REDUCE_WORKER % {"root": ROOT})
    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("MASTER_PORT", None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29661", str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["total"] == [(2 << 40) + 1] + [3 * i for i in range(1, 22)] and line["shots"] == (2 << 40) + 1 and line["errors"] == 3
