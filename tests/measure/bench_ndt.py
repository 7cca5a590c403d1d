"""Times the NDT mode of the registration handle (riv-slam_amd/ndt.py), P2D / D2D x DIRECT1 / 7 / 27, on scene.py pairs of 8192 x 8192
(resolution 1.0 and 2.0) and 100 000 x 500 000 points (resolution 1.0), default parameters (transformation_epsilon 5e-4, LM), clouds
resident.  Per size and resolution: the one-off voxel map builds of target and source (a new resolution within 1e-9 of the nominal one
per call, so every call rebuilds; ends with the host holding the voxel count); per mode and search: one linearize at the guess and one
align from the guess, with the rows per launch (source voxels in D2D, source points in P2D), the iteration counts and the contributing
terms of the last linearize.  As context, in the same process on the same handle and clouds: voxelized GICP (apdgicp_set_vgicp,
DIRECT1, the same resolution) and APD-GICP (both modes off), linearize and align each -- these need the k-NN covariances, which NDT
never computes; they are computed before the timed calls.  Wall clock around calls that end with the result on the host (every one of
them waits for the handle's stream); warm-up calls first, then the timed ones: median with p10 / p90, the device otherwise idle.
usage: python tests/measure/bench_ndt.py [out.json] [--small-only]"""
import ctypes
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
from bench_scan_filter import timed  # noqa: E402

SEARCH = (("direct1", 0), ("direct7", 1), ("direct27", 2))
MODES = (("p2d", 0), ("d2d", 1))


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    nd = importlib.import_module("riv-slam_amd.ndt")
    vg = importlib.import_module("riv-slam_amd.vgicp")
    scene = importlib.import_module("riv-slam_amd.scene")
    args = sys.argv[1:]
    sizes = [(8192, 8192, (1.0, 2.0), 20, 200)] + ([] if "--small-only" in args else [(100000, 500000, (1.0,), 3, 20)])
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "parameters": "apdgicp_default_params (LM, transformation_epsilon 5e-4, rotation_epsilon 2e-3)", "cases": []}
    for ns, nt, resolutions, warm, runs in sizes:
        src, tgt, _, guess = scene.make_pair(ns, nt, scene.pair_seed(5, 0), "odometry")
        h = nd.NDT(reg.default_params())
        h.setInputSource(torch.from_numpy(src).cuda())
        h.setInputTarget(torch.from_numpy(tgt).cuda())
        T0 = guess.astype(np.float64)
        for res in resolutions:
            case = {"n_source": ns, "n_target": nt, "resolution": res}
            h.enable()
            h.setResolution(res)
            step = [0]

            def rebuild(which):
                step[0] += 1
                h.setResolution(res * (1.0 + 1e-9 * step[0]))
                return h.voxel_count(which)
            case["map_build_target"] = timed(lambda: rebuild(1), runs=runs, warm=warm)
            case["map_build_source"] = timed(lambda: rebuild(0), runs=runs, warm=warm)
            h.setResolution(res)
            case["n_voxels_target"], case["n_voxels_source"] = h.voxel_count(1), h.voxel_count(0)
            for mname, mode in MODES:
                h.setDistanceMode(mode)
                for sname, search in SEARCH:
                    h.setNeighborSearchMethod(search)
                    h.align(guess)
                    r = h.result
                    rows = h.n_rows()
                    case[f"{mname}_{sname}"] = {
                        "rows_per_launch": rows, "blocks_per_launch": (rows + 255) // 256,
                        "linearize": timed(lambda: h.linearize(T0), runs=runs, warm=warm), "align": timed(lambda: h.align(guess), runs=runs, warm=warm),
                        "iterations": int(r.iterations) + 1, "n_linearize": int(r.n_linearize), "n_compute_error": int(r.n_compute_error),
                        "n_contributing_terms": int(r.n_matched), "converged": int(r.converged)}
            # context: voxelized GICP and APD-GICP on the same handle and clouds
            vp = vg.default_vgicp_params()
            vp.resolution = res
            reg._check(h.L.apdgicp_set_vgicp(h.h, ctypes.byref(vp)))
            h.align(guess)
            case["vgicp_direct1"] = {"linearize": timed(lambda: h.linearize(T0), runs=runs, warm=warm), "align": timed(lambda: h.align(guess), runs=runs, warm=warm),
                                     "iterations": int(h.result.iterations) + 1, "n_correspondences": int(h.result.n_matched), "converged": int(h.result.converged)}
            reg._check(h.L.apdgicp_set_vgicp(h.h, None))
            h.align(guess)
            case["apdgicp"] = {"linearize": timed(lambda: h.linearize(T0), runs=runs, warm=warm), "align": timed(lambda: h.align(guess), runs=runs, warm=warm),
                               "iterations": int(h.result.iterations) + 1, "n_matched": int(h.result.n_matched), "converged": int(h.result.converged)}
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
        del h
    path = next((a for a in args if a.endswith(".json")), os.path.join(ROOT, "profiles", "ndt.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
