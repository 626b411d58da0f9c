"""Relay-BP's device-marginal form without a GPU: the plan's workspace estimate, the binding's names, and the registers of the form's
instantiations (csrc/bp_relay_device.hip) from a device-only compile."""
import os
import re
import subprocess

import pytest

from quits_amd import _lib
from quits_amd.decoder import plan as qplan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Graph:
    def __init__(self, n):
        self.n = n


class _Dec:
    """What workspace_bytes_per_shot reads of a decoder: graph.n and info()."""

    def __init__(self, n, **info):
        self.graph = _Graph(n)
        self._info = info

    def info(self):
        return dict(self._info)


def test_plan_estimate_counts_a_second_row_per_device_form_decoder():
    ns = [18300] + [18900] * 17                                   # QLP [[1020,136]] W = 3 / F = 1: the 18 distinct windows of a lane
    pad = lambda n: (n + 63) // 64 * 64
    old = sum(4 * pad(n) + 64 for n in ns)                        # the estimate before the form existed
    bposd = [_Dec(n, edge_kernel=False) for n in ns]
    lds = [_Dec(n, relay_marginals="lds", relay_lds_bytes=1) for n in ns]
    dev = [_Dec(n, relay_marginals="device", relay_lds_bytes=1) for n in ns]
    assert qplan.workspace_bytes_per_shot(bposd) == old and qplan.workspace_bytes_per_shot(lds) == old
    assert qplan.workspace_bytes_per_shot(dev) == old + sum(4 * pad(n) for n in ns)
    assert qplan.workspace_bytes_per_shot(lds[:3] + dev[:2]) == sum(4 * pad(n) + 64 for n in ns[:3]) + sum(8 * pad(n) + 64 for n in ns[:2])
    assert pad(18900) == 18944 and 4 * pad(18900) == 75776        # "75.6 KB per shot"
    # n that is no multiple of 64, and one that is
    assert qplan.workspace_bytes_per_shot([_Dec(65, relay_marginals="device")]) == 8 * 128 + 64
    assert qplan.workspace_bytes_per_shot([_Dec(128, relay_marginals="device")]) == 8 * 128 + 64
    # the same lanes and chunk as before for a plan without such a decoder; fewer shots in flight with them
    budget = 160.0 * (1 << 30)
    assert qplan.fit_lanes_and_chunk(qplan.workspace_bytes_per_shot(lds), 3, 1 << 16, budget) == qplan.fit_lanes_and_chunk(old, 3, 1 << 16, budget)
    lanes, chunk = qplan.fit_lanes_and_chunk(qplan.workspace_bytes_per_shot(dev), 3, 1 << 16, budget)
    assert lanes * chunk * qplan.workspace_bytes_per_shot(dev) <= budget
    assert lanes * chunk < (lambda lc: lc[0] * lc[1])(qplan.fit_lanes_and_chunk(old, 3, 1 << 16, budget))


def test_binding_names_the_flag_and_the_info_call():
    assert _lib.RELAY_FLAG_MARGINALS_DEVICE == 1 and "qd_decoder_relay_info" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "quits_amd.h")).read()
    assert re.search(r"#define QD_RELAY_FLAG_MARGINALS_DEVICE 1\b", hdr) and "qd_decoder_relay_info" in hdr
    L = _lib.load()
    assert L.qd_version() >= 113 and _lib.require_relay_forms(L) is L


def test_marginals_argument_is_checked_before_any_device_call():
    from quits_amd.decoder.device import RelayBatchDecoder
    with pytest.raises(ValueError):
        RelayBatchDecoder(None, None, marginals="registers")


def test_device_form_stays_within_128_registers_and_out_of_scratch(tmp_path):
    """The 36 instantiations of the device-marginal form, __launch_bounds__(T, 4): at most 128 vector registers, no scratch; the marginal row
    is reached through global_* instructions (a flat access would mean the row's address space was lost on the way to the shared helpers)."""
    cs = os.path.join(ROOT, "quits_amd", "csrc")
    mk = open(os.path.join(cs, "Makefile")).read()
    flags = [f for f in re.search(r"^FLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split() if f != "-shared"]
    out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", "-o",
                          str(tmp_path / "d.s"), os.path.join(cs, "bp_relay_device.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", out.stderr)]
    agprs = [int(x) for x in re.findall(r"AGPRs: (\d+)", out.stderr)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert len(names) == len(vgprs) == len(agprs) == len(scratch)
    kern = [(n, v, a, sc) for n, v, a, sc in zip(names, vgprs, agprs, scratch) if "qd_bp_relay_kernel" in n]
    assert len(kern) == 36 and all(n.endswith("Lb1EEv10BpGraphDev10DecodeArgs9RelayArgs") for n, _, _, _ in kern), [k[0] for k in kern]
    print("device-marginal form: VGPRs %d .. %d" % (min(k[1] for k in kern), max(k[1] for k in kern)))
    assert all(v + a <= 128 and sc == 0 for _, v, a, sc in kern), [k for k in kern if k[1] + k[2] > 128 or k[3]]
    asm = open(tmp_path / "d.s").read()
    assert "global_load_dword" in asm and not re.search(r"^\s+(flat_load|flat_store|scratch_)", asm, re.M)
