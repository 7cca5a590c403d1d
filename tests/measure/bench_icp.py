"""Times the point-to-point ICP mode of the registration handle (riv-slam_amd/icp.py) on scene.py pairs of 8192 x 8192 and
100 000 x 500 000 points, clouds resident on the device, reciprocal correspondences off and on: one estimate (apdgicp_icp_estimate, the
per-iteration probe) at the guess and one align from the guess (PCL's defaults: 10 iterations, transformation epsilon 0; the gate at
2.5 m), with the align's own iteration count, its state, and the launches and host waits it made (apdgicp_icp_debug_counts).  As
context, in the same process on the same handle and clouds with the mode off: apdgicp_linearize at the guess (APD-GICP; it needs the
k-NN covariances, which ICP never computes -- they are computed before the timed calls).  Wall clock around calls that end with the
result on the host (every one of them waits for the handle's stream); warm-up calls first, then the timed ones: median with p10 / p90,
the device otherwise idle.
usage: python tests/measure/bench_icp.py [out.json] [--small-only]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
from bench_scan_filter import timed  # noqa: E402


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    icp = importlib.import_module("riv-slam_amd.icp")
    scene = importlib.import_module("riv-slam_amd.scene")
    args = sys.argv[1:]
    sizes = [(8192, 8192, 20, 200)] + ([] if "--small-only" in args else [(100000, 500000, 3, 20)])
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "cases": []}
    for ns, nt, warm, runs in sizes:
        src, tgt, _, guess = scene.make_pair(ns, nt, scene.pair_seed(5, 0), "odometry")
        h = icp.ICP(icp.pcl_params(max_correspondence_distance=2.5))
        h.setInputSource(torch.from_numpy(src).cuda())
        h.setInputTarget(torch.from_numpy(tgt).cuda())
        case = {"n_source": ns, "n_target": nt}
        for name, recip in (("forward", False), ("reciprocal", True)):
            h.setUseReciprocalCorrespondences(recip)
            e = h.estimate(guess)
            h.align(guess)
            launches, waits = h.debug_counts()
            it = max(1, len(h.trace()["n_corr"]))
            case[name] = {"estimate": timed(lambda: h.estimate(guess), runs=runs, warm=warm), "align": timed(lambda: h.align(guess), runs=runs, warm=warm),
                          "iterations": int(h.result.iterations), "state": icp.STATE_NAMES[h.convergence_state()], "n_corr_at_guess": int(e["n_corr"]),
                          "n_matched_last": int(h.result.n_matched), "launches_per_align": launches, "waits_per_align": waits,
                          "launches_per_iteration": round((launches - 2) / it, 2), "waits_per_iteration": round(waits / it, 2)}
        h.disable()   # context: APD-GICP's linearize on the same handle and clouds
        T0 = guess.astype(np.float64)
        h.linearize(T0)
        case["apdgicp_linearize"] = timed(lambda: h.linearize(T0), runs=runs, warm=warm)
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
        h.close()
    path = next((a for a in args if a.endswith(".json")), os.path.join(ROOT, "profiles", "icp.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
