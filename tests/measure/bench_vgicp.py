"""Times the voxelized GICP mode of the registration handle (riv-slam_amd/vgicp.py) next to the APD-GICP path of the SAME handle with the
mode off, on scene.py pairs of 8192 x 8192 and 100 000 x 500 000 points, resolution 1.0, launch parameters (transformation_epsilon 0.1,
max_correspondence_distance 2.0 -- ignored by VGICP --, azimuth variance 1.0), clouds and covariances resident.  Per size: the one-off
voxel map build (a new resolution within 1e-9 of 1.0 per call, so every call rebuilds; ends with the host holding the voxel count); per
DIRECT1 / DIRECT7 / DIRECT27: one linearize at the guess and one align from the guess; and, in the same process on the same clouds,
apdgicp_linearize / apdgicp_align with the mode off, once before and once after the VGICP blocks (their difference is the spread of the
session).  Wall clock around calls that end with the result on the host (every one of them waits for the handle's stream); warm-up calls
first, then the timed ones: median with p10 / p90, the device otherwise idle.
V6 as built: compute_error recomputes M from the stored pose and voxel indices; the stored-M alternative has not been built or measured.
usage: python tests/measure/bench_vgicp.py [out.json] [--small-only]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
from bench_scan_filter import timed  # noqa: E402

LAUNCH = dict(max_correspondence_distance=2.0, transformation_epsilon=0.1, azimuth_variance_deg=1.0)
SEARCH = (("direct1", 0), ("direct7", 1), ("direct27", 2))


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    vg = importlib.import_module("riv-slam_amd.vgicp")
    scene = importlib.import_module("riv-slam_amd.scene")
    args = sys.argv[1:]
    sizes = [(8192, 8192, 20, 200)] + ([] if "--small-only" in args else [(100000, 500000, 3, 20)])
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "resolution": 1.0, "parameters": LAUNCH, "v6_mahalanobis": "recomputed from the stored pose (stored form not measured)", "cases": []}
    for ns, nt, warm, runs in sizes:
        src, tgt, _, guess = scene.make_pair(ns, nt, scene.pair_seed(5, 0), "odometry")
        h = vg.FastVGICP(reg.default_params(**LAUNCH))
        h.setInputSource(torch.from_numpy(src).cuda())
        h.setInputTarget(torch.from_numpy(tgt).cuda())
        T0 = guess.astype(np.float64)
        case = {"n_source": ns, "n_target": nt}

        def apd_block(tag):
            h.disable()
            h.align(guess)
            case[tag] = {"linearize": timed(lambda: h.linearize(T0), runs=runs, warm=warm), "align": timed(lambda: h.align(guess), runs=runs, warm=warm),
                         "iterations": int(h.result.iterations) + 1, "n_matched": int(h.result.n_matched)}
            h.enable()

        apd_block("apdgicp_mode_off_before")
        step = [0]

        def rebuild():
            step[0] += 1
            h.setResolution(1.0 + 1e-9 * step[0])
            return h.voxel_count()
        case["map_build"] = timed(rebuild, runs=runs, warm=warm)
        h.setResolution(1.0)
        case["n_voxels"] = h.voxel_count()
        for name, mode in SEARCH:
            h.setNeighborSearchMethod(mode)
            h.align(guess)
            case[name] = {"linearize": timed(lambda: h.linearize(T0), runs=runs, warm=warm), "align": timed(lambda: h.align(guess), runs=runs, warm=warm),
                          "iterations": int(h.result.iterations) + 1, "n_linearize": int(h.result.n_linearize), "n_compute_error": int(h.result.n_compute_error),
                          "n_correspondences": int(h.result.n_matched), "converged": int(h.result.converged)}
        apd_block("apdgicp_mode_off_after")
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
        del h
    path = next((a for a in args if a.endswith(".json")), os.path.join(ROOT, "profiles", "vgicp.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
