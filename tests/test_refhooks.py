"""The hooks for the real denominators (ldpc.BpOsdDecoder as the CPU baseline, Stim's detector sampler as the input
source) exercised with STUB modules: neither wheel exists in the build container or on the GPU box, so these tests inject
`ldpc` / `stim` stand-ins into sys.modules -- an ldpc whose BpOsdDecoder is the oracle's plug-in class, a stim whose sampler is the
oracle's DEM sampler -- and check the plumbing: the probes, the per-shot loop over a process pool, bench.py's `cpu_baseline.kind`
switching on import success, tools/pin_ldpc.py end to end, and the one-line exit when the wheel is absent."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import helpers
import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refhooks  # noqa: E402


class _StubBpOsd(orc.OracleBpOsdDecoder):
    """ldpc.bposd_decoder.BpOsdDecoder's surface as tools/pin_ldpc.py and the loop read it: decode(), .iter, .converge,
    .ms_scaling_factor."""

    def __init__(self, pcm, **kw):
        kw.setdefault("ms_scaling_factor", 1.0)
        self.ms_scaling_factor = kw["ms_scaling_factor"]
        if "error_channel" in kw:
            kw["error_channel"] = np.asarray(kw["error_channel"], dtype=np.float64)
        super().__init__(pcm, **kw)
        self.iter, self.converge = 0, False

    def decode(self, syndrome):
        out = super().decode(syndrome)
        self.converge, self.iter = bool(self.last_flags[0]), int(self.last_flags[1])
        return out


@pytest.fixture
def stub_wheels(monkeypatch):
    ldpc = types.ModuleType("ldpc")
    ldpc.__version__ = "stub-2.x"
    sub = types.ModuleType("ldpc.bposd_decoder")
    sub.BpOsdDecoder = _StubBpOsd
    ldpc.bposd_decoder = sub
    ldpc.BpOsdDecoder = _StubBpOsd
    monkeypatch.setitem(sys.modules, "ldpc", ldpc)
    monkeypatch.setitem(sys.modules, "ldpc.bposd_decoder", sub)

    stim = types.ModuleType("stim")
    stim.__version__ = "stub-1.x"

    class _Sampler:
        def __init__(self, text, seed):
            from quits_amd.decoder.base import detector_error_model_to_matrix
            from quits_amd.dem import Circuit
            self.H, self.L, self.p = detector_error_model_to_matrix(Circuit(text))
            self.seed = seed

        def sample(self, shots, separate_observables=False):
            det, obs, _ = orc.sample_dem(self.H, self.L, self.p, self.seed, 0, shots)
            assert separate_observables
            return det.astype(bool), obs.astype(bool)

    class _Circuit:
        def __init__(self, text):
            self.text = text

        def compile_detector_sampler(self, seed=None):
            return _Sampler(self.text, 0 if seed is None else seed)

    stim.Circuit = _Circuit
    monkeypatch.setitem(sys.modules, "stim", stim)
    return ldpc, stim


def test_probes_report_absence_with_a_reason(monkeypatch):
    monkeypatch.setitem(sys.modules, "ldpc", None)            # import ldpc -> ImportError
    monkeypatch.setitem(sys.modules, "stim", None)
    cls, why = refhooks.probe_ldpc()
    assert cls is None and "Error" in why
    mod, why = refhooks.probe_stim()
    assert mod is None and "Error" in why
    with pytest.raises(RuntimeError):
        refhooks.stim_sample("", 1, 1)


def test_stim_sampler_hook(stub_wheels):
    name = "bb72_custom_r6_p0.003"
    det, obs = refhooks.stim_sample(helpers.circuit_text(name), 64, seed=3)
    H, L, pri = helpers.dem_matrices(name)
    assert det.dtype == np.uint8 and det.shape == (64, H.shape[0]) and obs.shape == (64, L.shape[0])
    d2, o2, _ = orc.sample_dem(H, L, pri, 3, 0, 64)
    assert np.array_equal(det, d2) and np.array_equal(obs, o2)


def test_ldpc_loop_over_process_pool_equals_the_oracle_loop(stub_wheels):
    from quits_amd.dem import Circuit
    name = "bb72_custom_r6_p0.003"
    cd = helpers.code("bb72")
    H, L, pri = helpers.dem_matrices(name)
    det, _, _ = orc.sample_dem(H, L, pri, 11, 0, 48)
    opts = dict(bp_method="minimum_sum", schedule="parallel", max_iter=20, osd_method="osd_0", osd_order=0)
    pred, n1, t1, ta = refhooks.ldpc_window_loop(det, Circuit(helpers.circuit_text(name)), cd["hz"], cd["lz"], 3, 1, opts, ncpu=2)
    wins = helpers.window_set(name, 3, 1)
    for k, w in enumerate(wins):
        w["row0"] = k * cd["hz"].shape[0]
    ref, _ = orc.sliding_window_decode(wins, cd["hz"].shape[0], det, orc.make_params("minimum_sum", "parallel", 20, "osd_0", 0, 1.0, orc.FORM_LDPC_F64))
    assert pred.shape == ref.shape and np.array_equal(pred, ref)
    assert n1 == 24 and t1 > 0 and ta > 0


def _bench_args(**over):
    import argparse
    a = argparse.Namespace(cpu_shots=6, shots=64, bp_method="minimum_sum", schedule="parallel", max_iter=20, osd_method="osd_0",
                           osd_order=0, ref_shots=4)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _bench_baseline(args):
    sys.path.insert(0, ROOT)
    import bench
    from quits_amd.dem import Circuit
    name = "bb72_custom_r6_p0.003"
    cd = helpers.code("bb72")
    H, L, pri = helpers.dem_matrices(name)
    det, obs, _ = orc.sample_dem(H, L, pri, 5, 0, 64)
    circ = Circuit(helpers.circuit_text(name))
    wins = helpers.window_set(name, 3, 1)
    for k, w in enumerate(wins):
        w["row0"] = k * cd["hz"].shape[0]

    def fake_gpu(d):          # stands in for plan.decode (no GPU here): the oracle on the device's LLR grid
        return orc.sliding_window_decode(wins, cd["hz"].shape[0], d, orc.make_params("minimum_sum", "parallel", 20, "osd_0", 0, 1.0, orc.FORM_LDPC_F64),
                                         device_grid=True)[0]
    return bench.cpu_baseline(args, circ, cd["hz"], cd["lz"], 6, 3, 1, (det, obs), fake_gpu, 1.0e6)


def test_bench_cpu_baseline_kind_follows_the_import(stub_wheels, monkeypatch):
    res = _bench_baseline(_bench_args())
    assert res["cpu_baseline"]["kind"] == "reference" and "stub-2.x" in res["cpu_baseline"]["sample"]
    assert res["cpu_baseline_port"]["kind"] == "port" and res["cpu_baseline_1core"]["kind"] == "port"
    assert res["cpu_baseline"]["port_identical_prediction"] == 1.0            # the stub IS the oracle
    assert res["cpu_baseline"]["value"] > 0 and res["cpu_baseline"]["cores"] >= 1
    monkeypatch.setitem(sys.modules, "ldpc", None)
    monkeypatch.setitem(sys.modules, "ldpc.bposd_decoder", None)
    res = _bench_baseline(_bench_args())
    assert res["cpu_baseline"]["kind"] == "port" and "not importable" in res["cpu_baseline"]["reference_probe"]
    assert "cpu_baseline_port" not in res


def test_bench_dump_outputs_dtypes_budget_and_names(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 predictions and a float64 mismatch count; over the byte budget, the same seeded sample of
    rows on every call, in row order; the rank suffix of an N > 1 run."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    pred = np.random.default_rng(1).integers(0, 2, (5000, 12), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), torch.from_numpy(pred), torch.tensor([7]))
    p, m = np.load(tmp_path / "a" / "predictions.npy"), np.load(tmp_path / "a" / "mismatches.npy")
    assert p.dtype == np.float32 and np.array_equal(p, pred)
    assert m.dtype == np.float64 and m.tolist() == [7.0]
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096 + 4 * 12 * 1000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), torch.from_numpy(pred), torch.tensor([7]), "_rank1")
    b, c = np.load(tmp_path / "b" / "predictions_rank1.npy"), np.load(tmp_path / "c" / "predictions_rank1.npy")
    assert b.shape == (1000, 12) and np.array_equal(b, c)
    assert np.array_equal(b, pred[np.sort(np.random.default_rng(2026).choice(5000, 1000, replace=False))])
    assert os.path.exists(tmp_path / "b" / "mismatches_rank1.npy")


def test_pin_ldpc_end_to_end_with_the_stub(stub_wheels, tmp_path, monkeypatch, capsys):
    import pin_ldpc
    monkeypatch.setattr(pin_ldpc, "FIXTURES", [("bb72_custom_r6_p0.003", (3, 1, 0))])
    out = tmp_path / "pin.npz"
    monkeypatch.setattr(sys, "argv", ["pin_ldpc.py", "--shots", "6", "--max-iter", "6", "--osd-order", "2", "--out", str(out)])
    assert pin_ldpc.main() == 0
    z = np.load(out)
    import json
    rep = json.loads(bytes(z["report_json"]).decode())
    assert rep["summary"]["decisions"] == rep["summary"]["total"] == 6 * len(pin_ldpc.TRIPLES)
    assert rep["verify"]["V2_ms_scaling_factor_default"] == 1.0 and rep["verify"]["V3_channel_probs_alias"] is True
    assert rep["verify"]["V1_serial_natural_order"]["holds"]
    assert "bb72_custom_r6_p0.003_W3F1_k0/product_sum_serial_osd_cs/out" in z.files


def test_pin_ldpc_without_the_wheel_is_one_line_and_exit_0():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pin_ldpc.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ldpc not importable") and len(r.stdout.strip().splitlines()) == 1


def test_oracle_matches_ldpc_pin():
    """The day tools/pin_ldpc.py has run on a machine with the wheel, its vectors (ldpc's own outputs) travel as
    tests/golden/ldpc_pin.npz and the oracle must reproduce every case the script reported identical.  Absent here: skipped,
    and the oracle's header keeps saying "parity unpinned" for the BP / OSD arithmetic."""
    import json
    path = os.path.join(helpers.GOLD, "ldpc_pin.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/ldpc_pin.npz not generated: ldpc is not importable in the build container")
    import pin_ldpc
    z = np.load(path)
    rep = json.loads(bytes(z["report_json"]).decode())
    for case in rep["cases"]:
        if case["identical_corrections"] != case["shots"]:
            continue                                   # recorded as a known difference by the pin run; the report names it
        tag, triple = case["case"].split("/")
        bpm, sch, osd = triple.split("_")[0] + "_" + triple.split("_")[1], triple.split("_")[2], "_".join(triple.split("_")[3:])
        name, win = next((n, w) for (n, w) in pin_ldpc.FIXTURES if tag == n + ("" if w is None else "_W%dF%d_k%d" % w))
        H, pri = pin_ldpc.window_of(name, win)
        synd = np.unpackbits(z[tag + "/syndromes"], axis=1)[:, :H.shape[0]]
        want = np.unpackbits(z[case["case"] + "/out"], axis=1)[:, :H.shape[1]]
        order = int(rep.get("osd_order", 4)) if osd != "osd_0" else 0
        got, _ = orc.Graph(H, pri).decode_batch(synd, orc.make_params(bpm, sch, int(rep.get("max_iter", 12)), osd, order, 1.0, orc.FORM_LDPC_F64))
        assert np.array_equal(got, want), case["case"]
