"""Times the FAST_VGICP_CUDA mode of the registration handle (riv-slam_amd/vgicp_cuda.py) on scene.py pairs of 8192 x 8192 and
100 000 x 500 000 points, device input, resolution 1.0, launch parameters (transformation_epsilon 0.1; max_correspondence_distance 2.0 and
the azimuth variance are not read by this mode), PLANE.  Per size:
  prepare_source / prepare_target   one preparation (k-NN, VC2, VC3, compaction, one host wait): the regularisation alternates between PLANE
                                    and MIN_EIG from call to call, so every call prepares anew (the same kernels; MIN_EIG keeps every point);
  map_build                         a new resolution within 1e-9 of 1.0 per call, so every call rebuilds (ends with the voxel count on the host);
  direct1 / direct7 / direct27 / radius1.5   one linearize at the guess and one align from the guess, with the kept shares, the offsets,
                                    the iteration counts and the correspondences;
  fast_vgicp_before / _after        the SAME handle in the FAST_VGICP mode (DIRECT7) over the same clouds, once before and once after the blocks
                                    above: context, and their difference is the spread of the session.
Wall clock around calls that end with the result on the host; warm-up calls first, then the timed ones: median with p10 / p90, the device
otherwise idle.
usage: python tests/measure/bench_vgicp_cuda.py [out.json] [--small-only]"""
import ctypes as C
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


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    vc = importlib.import_module("riv-slam_amd.vgicp_cuda")
    vg = importlib.import_module("riv-slam_amd.vgicp")
    scene = importlib.import_module("riv-slam_amd.scene")
    args = sys.argv[1:]
    sizes = [(8192, 8192, 20, 200)] + ([] if "--small-only" in args else [(100000, 500000, 3, 20)])
    search = (("direct1", vc.DIRECT1, -1.0), ("direct7", vc.DIRECT7, -1.0), ("direct27", vc.DIRECT27, -1.0), ("radius1.5", vc.DIRECT_RADIUS, 1.5))
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "resolution": 1.0, "parameters": LAUNCH, "cases": []}
    for ns, nt, warm, runs in sizes:
        src, tgt, _, guess = scene.make_pair(ns, nt, scene.pair_seed(5, 0), "odometry")
        h = vc.FastVGICPCuda(reg.default_params(**LAUNCH))
        h.setInputSource(torch.from_numpy(src).cuda())
        h.setInputTarget(torch.from_numpy(tgt).cuda())
        T0 = guess.astype(np.float64)
        case = {"n_source": ns, "n_target": nt}
        vgp = vg.default_vgicp_params()
        vgp.neighbor_search = vg.DIRECT7

        def vgicp_block(tag):
            reg._check(h.L.apdgicp_set_vgicp(h.h, C.byref(vgp)))
            h.align(guess)
            case[tag] = {"search": "direct7", "linearize": timed(lambda: h.linearize(T0), runs=runs, warm=warm), "align": timed(lambda: h.align(guess), runs=runs, warm=warm),
                         "iterations": int(h.result.iterations) + 1, "n_correspondences": int(h.result.n_matched)}
            h.enable()

        vgicp_block("fast_vgicp_before")
        flip = [0]

        def prepare(which):
            flip[0] += 1
            h.setRegularizationMethod(vc.MIN_EIG if flip[0] % 2 else vc.PLANE)
            return len(h.kept(which))
        case["prepare_source"] = timed(lambda: prepare(0), runs=runs, warm=warm)
        case["prepare_target"] = timed(lambda: prepare(1), runs=runs, warm=warm)
        h.setRegularizationMethod(vc.PLANE)
        case["kept_source"], case["kept_target"] = len(h.kept(0)), len(h.kept(1))
        step = [0]

        def rebuild():
            step[0] += 1
            h.setResolution(1.0 + 1e-9 * step[0])
            return h.voxel_count()
        case["map_build"] = timed(rebuild, runs=runs, warm=warm)
        h.setResolution(1.0)
        case["n_voxels"] = h.voxel_count()
        for name, mode, radius in search:
            h.setNeighborSearchMethod(mode, radius)
            h.align(guess)
            case[name] = {"n_offsets": len(h.offsets()), "linearize": timed(lambda: h.linearize(T0), runs=runs, warm=warm),
                          "align": timed(lambda: h.align(guess), runs=runs, warm=warm), "iterations": int(h.result.iterations) + 1,
                          "n_linearize": int(h.result.n_linearize), "n_compute_error": int(h.result.n_compute_error), "n_correspondences": int(h.result.n_matched),
                          "converged": int(h.result.converged)}
        vgicp_block("fast_vgicp_after")
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
        del h
    path = next((a for a in args if a.endswith(".json")), os.path.join(ROOT, "profiles", "vgicp_cuda.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
