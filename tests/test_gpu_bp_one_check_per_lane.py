"""The scatter kernel with one check per lane (bp_scatter_wide.hip, CPL = 1) on its default path: windows whose accumulators leave no
room in the LDS for twice the workgroups, so that build_scatter gives every check a lane of its own without any switch -- one window
for each of the 256-, 512- and 1024-lane instantiations (tests/test_graph_layout.py lays the same three out on the CPU).  The default
path, the same library with QD_BP_NO_FAST_START=1 (generic start, full last pass), the gather kernel (QD_NO_SCATTER=1) and the recheck
pass (QD_SCATTER_M2_LIMIT=1: every shot with a defect is decoded again by the gather kernel) return the same hard decisions, status
words, OSD-0 outputs and posteriors, and stage 3 equals the double-precision oracle on the same LLR grid."""
import functools

import numpy as np
import pytest

import helpers
import oracle as orc

pytestmark = pytest.mark.gpu

SHOTS = 64
NLLR = 4                        # posteriors of the first NLLR shots BP leaves unconverged
SWITCHES = ("QD_NO_SCATTER", "QD_BP_NO_FAST_START", "QD_SCATTER_M2_LIMIT", "QD_SCATTER_CPL1")
PATHS = (("default", {}), ("generic", {"QD_BP_NO_FAST_START": "1"}), ("gather", {"QD_NO_SCATTER": "1"}), ("recheck", {"QD_SCATTER_M2_LIMIT": "1"}))
# window -> ((checks, faults), lanes of the instantiation)
WINDOWS = {"hgp225_w2": ((216, 2484), 256), "410x5056": ((410, 5056), 512), "800x10933": ((800, 10933), 1024)}


@functools.lru_cache(maxsize=None)
def _window(which):
    """(H, priors, syndromes [SHOTS, m]); shot 0 all zero, shot 1 a single defect, shot 2 every detector set."""
    if which == "hgp225_w2":
        w = helpers.window_set("hgp225_cardinal_r3_p0.01", 2, 1)[0]
        H, pri = w["H"], np.asarray(w["priors"], dtype=np.float64)
    else:
        H, pri = helpers.synthetic_window(*{"410x5056": ([36] * 410, 3, 4, 41001), "800x10933": ([40] * 800, 3, 4, 41002)}[which])
    assert H.shape == WINDOWS[which][0], (which, H.shape)
    s = np.ascontiguousarray(orc.sample_dem(H, H[:1], pri, seed=31, shot0=0, B=SHOTS)[0]).astype(np.uint8)
    s[0] = 0
    s[1] = 0
    s[1, H.shape[0] // 2] = 1
    s[2] = 1
    s.setflags(write=False)
    return H, pri, s


@functools.lru_cache(maxsize=None)
def _reference(which, max_iter):
    """The oracle in double precision on the device's grid: (OSD-0 outputs, flags).  Checked here, on the oracle alone: no shot leaves
    the fine grid, and at max_iter 50 at least two shots converge and at least two do not."""
    H, pri, s = _window(which)
    g, form = orc.device_arithmetic(H, pri, "minimum_sum", "parallel", max_iter, 1.0)
    ref, flags, grid = g.decode_batch(s, orc.make_params("minimum_sum", "parallel", max_iter, "osd_0", 0, 1.0, form), return_grid=True)
    conv = int(flags[:, 0].sum())
    print("%s / max_iter %d: oracle iterations min %d max %d, converged %d of %d" % (which, max_iter, flags[:, 1].min(), flags[:, 1].max(), conv, len(flags)))
    assert g.grid[0] >= 0 and (grid[:, 0] == g.grid[0]).all() and not grid[:, 1].any(), (which, max_iter, grid)
    assert max_iter != 50 or (conv >= 2 and len(flags) - conv >= 2), (which, conv)
    return ref, flags


def _run(monkeypatch, which, env, max_iter):
    import torch
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    H, pri, s = _window(which)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wg = WindowGraph(H, pri)
    dec = BatchDecoder(wg, max_iter=max_iter, osd_method="osd_0")
    det = torch.from_numpy(np.array(s)).cuda()
    out = {}
    bits, status = dec.decode(det, stage=1)
    out[1] = (unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy())
    failed = np.flatnonzero(((out[1][1] >> 16) & 1) == 0)[:NLLR]
    out["llr"] = {int(b): dec.failed_llr(int(b)).cpu().numpy() for b in failed}
    bits, status = dec.decode(det, stage=3)
    out[3] = (unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy())
    return out, dec.info(), wg.info()


def _same(a, b, what):
    for stage in (1, 3):
        bad = np.flatnonzero((a[stage][0] != b[stage][0]).any(axis=1) | (a[stage][1] != b[stage][1]))
        assert bad.size == 0, "%s, stage %d: %d shots differ, first %s" % (what, stage, bad.size, bad[:8])
    assert sorted(a["llr"]) == sorted(b["llr"]), what
    for k in a["llr"]:
        assert np.array_equal(a["llr"][k], b["llr"][k]), "%s: posteriors of shot %d differ" % (what, k)


@pytest.mark.parametrize("max_iter", [1, 3, 50])
@pytest.mark.parametrize("which", list(WINDOWS))
def test_one_check_per_lane_on_its_default_path(gpu, monkeypatch, which, max_iter):
    ref, flags = _reference(which, max_iter)
    outs = {}
    for tag, env in PATHS:
        outs[tag], info, ginfo = _run(monkeypatch, which, env, max_iter)
        if tag == "gather":
            assert not info["scatter_kernel"] and not info["edge_kernel"] and info["llr_grid_bits"] >= 0, (tag, info)
            continue
        assert info["scatter_kernel"] and not info["scatter_wide_kernel"], (tag, info)
        assert (ginfo["scatter_threads"], ginfo["scatter_checks_per_lane"]) == (WINDOWS[which][1], 1), (tag, ginfo)
        assert info["bp_fast_start"] == (tag != "generic"), (tag, info)
    for tag in ("generic", "gather", "recheck"):
        _same(outs["default"], outs[tag], "default path against " + tag)
    for tag, out in outs.items():
        bits, status = out[3]
        assert np.array_equal(bits, ref), tag
        assert np.array_equal((status >> 16) & 1, flags[:, 0]) and np.array_equal(status & 0x3FFF, flags[:, 1]), tag
    st = outs["default"][1][1]
    assert st[0] == (1 << 16) | (1 << 19)                      # the all-zero syndrome: converged, zero vector, no BP
    ran = st[((st >> 19) & 1) == 0]                            # the others: iterations are counted from the same origin
    assert ran.size and (ran & 0x3FFF).min() >= 1 and (ran & 0x3FFF).max() <= max_iter
