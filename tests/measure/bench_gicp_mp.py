"""Times the FastGICPMultiPoints mode of the registration handle (riv-slam_amd/gicp_mp.py) on scene.py pairs of 8192 x 8192 and
100 000 x 500 000 points, clouds resident on the device, r = 0.5 and the class's defaults (MP8): one linearize at the guess (wall clock,
median with p10 / p90), its split over transform, count, scan, fill, row sort and the per-point kernel (events at the boundaries, in a
series of their own with profiling on: medians), `total` with the mean and maximum row length, launches and host waits per iteration, and
one align from the guess with its iteration count and end state.  As context, on the same handle, clouds and process with the mode off:
apdgicp_linearize at the guess (APD-GICP), measured before and after, in alternating blocks with this mode's linearize; the spread
between the blocks' medians is reported.  Covariances are computed before anything is timed.

Expectation, written down before the run: at 8k a linearize is launch and wait latency (ten launches, two waits); at 100k x 500k the row
sort and the per-point kernel's divergent rows dominate.
usage: python tests/measure/bench_gicp_mp.py [out.json] [--small-only]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
from bench_scan_filter import timed  # noqa: E402


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    gmp = importlib.import_module("riv-slam_amd.gicp_mp")
    scene = importlib.import_module("riv-slam_amd.scene")
    args = sys.argv[1:]
    sizes = [(8192, 8192, 10, 50, 3)] + ([] if "--small-only" in args else [(100000, 500000, 2, 7, 2)])
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "cases": []}
    for ns, nt, warm, runs, blocks in sizes:
        src, tgt, _, guess = scene.make_pair(ns, nt, scene.pair_seed(5, 0), "odometry")
        h = gmp.FastGICPMultiPoints()
        h.setNeighborSearchRadius(0.5)
        h.setInputSource(torch.from_numpy(src).cuda())
        h.setInputTarget(torch.from_numpy(tgt).cuda())
        T0 = guess.astype(np.float64)
        case = {"n_source": ns, "n_target": nt, "radius": 0.5, "mp_linearize_blocks": [], "apdgicp_linearize_blocks": []}
        for _ in range(blocks):   # alternating blocks: APD before, this mode, (and APD again after the last one)
            h.disable()
            h.linearize(T0)
            case["apdgicp_linearize_blocks"].append(timed(lambda: h.linearize(T0), runs=runs, warm=warm))
            h.enable()
            h.linearize(T0)
            case["mp_linearize_blocks"].append(timed(lambda: h.linearize(T0), runs=runs, warm=warm))
        h.disable()
        h.linearize(T0)
        case["apdgicp_linearize_blocks"].append(timed(lambda: h.linearize(T0), runs=runs, warm=warm))
        h.enable()
        for key in ("mp_linearize_blocks", "apdgicp_linearize_blocks"):
            med = [b["median_ms"] for b in case[key]]
            case[key.replace("_blocks", "")] = {"median_ms": float(np.median(med)), "spread_between_blocks_ms": float(max(med) - min(med))}
        h.setProfiling(True)
        h.linearize(T0)
        phases = []
        for _ in range(runs):
            h.linearize(T0)
            phases.append(h.last_phases())
        h.setProfiling(False)
        case["phases_median_ms"] = {k: float(np.median([p[k] for p in phases])) for k in phases[0]}
        lens = np.diff(h.rows()[0])
        case["total"], case["row_mean"], case["row_max"], case["rows_non_empty"] = int(lens.sum()), float(lens.mean()), int(lens.max()), int((lens > 0).sum())
        h.align(guess)
        launches, waits = h.debug_counts()
        it = len(h.trace()["cost"])
        case["align"] = timed(lambda: h.align(guess), runs=max(2, runs // 10), warm=0)
        case.update({"iterations": int(h.result.iterations), "state": gmp.STATE_NAMES[h.state()], "n_matched_last": int(h.result.n_matched),
                     "launches_per_iteration": round(launches / it, 2), "waits_per_iteration": round(waits / it, 2)})
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
        h.close()
    path = next((a for a in args if a.endswith(".json")), os.path.join(ROOT, "profiles", "gicp_mp.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
