#!/usr/bin/env python3
"""BP stage alone on the windows that run the scatter kernel with one check per lane, one library against another (QUITS_AMD_LIB), same box:

  python tools/one_check_per_lane_ab.py PARENT.so [NEW.so] > profiles/one_check_per_lane_ab.txt

Cases: the three windows of tests/test_gpu_bp_one_check_per_lane.py on their default path and the headline window under
QD_SCATTER_CPL1=1.  Per case the two libraries alternate A B A B A B, each run in a fresh process (65 536 shots, max_iter 50, one
warm-up launch, three launches timed with the decoder's profiling events); the checksums of the hard decisions and of status & 0xFFFFF
must agree.  This process does not touch the GPU; it stops at the first child that fails."""
import json, os, subprocess, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("hgp225_w2", "410x5056", "800x10933", "headline_cpl1")


def child(case):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch, helpers
    from quits_amd.decoder.device import BatchDecoder, DemSampler, WindowGraph
    if case == "hgp225_w2":
        w = helpers.window_set("hgp225_cardinal_r3_p0.01", 2, 1)[0]
        H, pri = w["H"], w["priors"]
    elif case == "headline_cpl1":
        H, _, pri = helpers.dem_matrices("bb144_custom_r12_p0.003")
    else:
        H, pri = helpers.synthetic_window(*{"410x5056": ([36] * 410, 3, 4, 41001), "800x10933": ([40] * 800, 3, 4, 41002)}[case])
    det, _ = DemSampler(H, H[:1], pri).sample(65536, seed=5)
    g = WindowGraph(H, pri); d = BatchDecoder(g, max_iter=50, osd_method="osd_0")
    i = d.info()
    assert i["scatter_kernel"] and not i["scatter_wide_kernel"], i          # one check per lane
    bits, st = d.decode(det, stage=1); torch.cuda.synchronize()
    d.set_profiling(True); d.profile()
    ms = []
    for _ in range(3):
        bits, st = d.decode(det, stage=1); torch.cuda.synchronize()
        ms.append(d.profile()["bp_ms"])
    print(json.dumps({"case": case, "shape": "%d x %d" % H.shape, "bp_ms": ms, "crc_bits": "%08x" % zlib.crc32(bits.cpu().numpy().tobytes()),
                      "crc_status": "%08x" % zlib.crc32((st & 0xFFFFF).cpu().numpy().tobytes()), "fast_start": i["bp_fast_start"],
                      "mean_iterations": float((st & 0x3FFF).float().mean())}))


def main():
    libs = {"parent": os.path.abspath(sys.argv[1]), "new": os.path.abspath(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "quits_amd", "lib", "libquits_amd.so"))}
    ok = True
    for case in CASES:
        runs = {"parent": [], "new": []}
        for k in range(6):
            tag = ("parent", "new")[k % 2]
            env = dict(os.environ, QUITS_AMD_LIB=libs[tag])
            env.pop("QD_SCATTER_CPL1", None)
            if case == "headline_cpl1":
                env["QD_SCATTER_CPL1"] = "1"
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case], env=env, capture_output=True, text=True, timeout=240)
            if out.returncode != 0:
                print("%s / %s: child ended with status %d\n%s" % (case, tag, out.returncode, out.stderr[-2000:]), flush=True)
                return 1
            runs[tag].append(json.loads(out.stdout.strip().splitlines()[-1]))
        mean = {t: [sum(r["bp_ms"]) / 3 for r in runs[t]] for t in runs}
        pm, nm = sum(mean["parent"]) / 3, sum(mean["new"]) / 3
        spread = max(mean["parent"]) - min(mean["parent"])
        crc = {(r["crc_bits"], r["crc_status"]) for t in runs for r in runs[t]}
        good = len(crc) == 1 and nm <= pm + spread
        ok = ok and good
        r0 = runs["new"][0]
        print("%-14s %-12s parent %s mean %.3f ms (spread %.3f) | new %s mean %.3f ms | %+.1f %% | crc bits %s status %s %s | new fast start %s, %.2f iterations per shot | %s" % (
            case, r0["shape"], " ".join("%.3f" % x for x in mean["parent"]), pm, spread, " ".join("%.3f" % x for x in mean["new"]), nm, 100.0 * (nm / pm - 1.0),
            r0["crc_bits"], r0["crc_status"], "equal" if len(crc) == 1 else "DIFFER", r0["fast_start"], r0["mean_iterations"],
            "ok" if good else "NOT MET"), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(main())
