"""Times downsample_method APPROX_VOXELGRID (riv-slam_amd/csrc/apd_approx_voxel.hpp) against VOXELGRID, the existing path and the baseline,
on the same clouds in the same process: the first n = 512 and n = 8 192 points of a scene.raw_scan behind the range gate (one cloud, no pose) and a submap-like cloud of 100 000
points (ten keyframes of 10 000 points with their relative poses), leaf 0.1, DEVICE input, one wait per call.  Protocol: 30 warm-up calls
per method, then six alternating blocks (VOXELGRID, APPROX, VOXELGRID, ...) of 50 timed SubmapAssembler.assemble calls each -- wall clock
around a call that ends with the host holding n_out -- median with p10 / p90 over a method's 300 calls.  ScanFilter.run (gate, grid,
STATISTICAL 20 / 1.0) at n = 8 192 the same way with both methods.  Launches per call are counted from the host code's loops, a function
of n (kernel launches; each call adds one device-to-host copy of the count and one wait; VOXELGRID one host-to-device copy of its box).
No bar is set for this stage; the numbers are observations.
usage: python tests/measure/bench_approx_voxel.py [out.json]"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
WARM, BLOCKS, RUNS = 30, 6, 50


def launches(n, method):
    """kernel launches of one apdgicp_submap_assemble with a leaf (riv-slam_amd/csrc/apdgicp_hip.hip)"""
    if method == "APPROX_VOXELGRID":
        return 1 + 1 + 2 * 4 + 1 + 2 + 1 + 1   # transform, keys, two radix passes of four, heads, the eviction scan, entries, centroids
    np2, sort = 4096, 1
    while np2 < n:
        np2 <<= 1
    k = 2 * 4096
    while k <= np2:                            # enqueue_bitonic_sort (apd_sort.hpp)
        j = k >> 1
        while j >= 4096:
            sort, j = sort + 1, j >> 1
        sort, k = sort + 1, k << 1
    return 1 + 1 + 1 + sort + 1 + 1 + 1        # transform, box, keys, the bitonic sort, heads, block sums, centroids


def alternate(fns):
    """fns: {name: callable}; alternating blocks, all of a name's samples together"""
    for f in fns.values():
        for _ in range(WARM):
            f()
    t = {k: [] for k in fns}
    for _ in range(BLOCKS):
        for k, f in fns.items():
            for _ in range(RUNS):
                t0 = time.perf_counter()
                f()
                t[k].append(time.perf_counter() - t0)
    return {k: {"median_ms": float(np.median(v) * 1e3), "p10_ms": float(np.percentile(v, 10) * 1e3), "p90_ms": float(np.percentile(v, 90) * 1e3),
                "runs": len(v)} for k, v in t.items()}


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    sf = importlib.import_module("riv-slam_amd.scan_filter")
    sub = importlib.import_module("riv-slam_amd.submap")
    scene = importlib.import_module("riv-slam_amd.scene")
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "cases": []}
    methods = ("VOXELGRID", "APPROX_VOXELGRID")
    shapes = []
    for n in (512, 8192):
        raw = scene.raw_scan(n + n // 8, 3)   # the scan as downsample() sees it: behind the range gate (1 .. 100 m, -5 .. 20 m), the first n points
        d = np.linalg.norm(raw[:, :3].astype(np.float64), axis=1)
        raw = np.ascontiguousarray(raw[(d > 1.0) & (d < 100.0) & (raw[:, 2] > -5.0) & (raw[:, 2] < 20.0)][:n])
        assert len(raw) == n
        shapes.append((f"scan{n}", [raw], None))
    rng = np.random.default_rng(0)
    clouds, odoms, T = [], [], np.eye(4)
    for f in range(11):
        s, _, Tt, _ = scene.make_pair(10000, 16, scene.pair_seed(77, f), "odometry")
        clouds.append(np.ascontiguousarray(np.concatenate([s[:, :3], rng.uniform(0, 40, (len(s), 1)).astype(np.float32)], 1)))
        T = T @ Tt
        odoms.append(T.copy())
    shapes.append(("submap100000", clouds[:-1], sub.relative_poses(odoms[:-1], odoms[-1])))
    for name, cl, poses in shapes:
        dev = [torch.from_numpy(c).cuda() for c in cl]
        torch.cuda.synchronize()
        a = sub.SubmapAssembler()
        n = sum(len(c) for c in cl)
        case = {"shape": name, "n": n, "leaf": 0.1, "input": "device", "call": "SubmapAssembler.assemble"}
        case["ms"] = alternate({m: (lambda m=m: a.assemble(dev, poses, 0.1, method=m)) for m in methods})
        case["n_out"] = {m: a.assemble(dev, poses, 0.1, method=m) for m in methods}
        case["kernel_launches"] = {m: launches(n, m) for m in methods}
        case["approx_over_voxelgrid"] = case["ms"]["APPROX_VOXELGRID"]["median_ms"] / case["ms"]["VOXELGRID"]["median_ms"]
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    raw = scene.raw_scan(8192, 3)
    dev = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    filters = {m: sf.ScanFilter(downsample_method=m) for m in methods}
    case = {"shape": "scan8192", "n": len(raw), "leaf": 0.1, "input": "device", "call": "ScanFilter.run (gate, grid, STATISTICAL 20 / 1.0)"}
    case["ms"] = alternate({m: (lambda m=m: filters[m].run(dev)) for m in methods})
    case["stage_counts"] = {m: list(filters[m].stage_counts()) for m in methods}
    case["approx_over_voxelgrid"] = case["ms"]["APPROX_VOXELGRID"]["median_ms"] / case["ms"]["VOXELGRID"]["median_ms"]
    print(json.dumps(case), flush=True)
    out["cases"].append(case)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "approx_voxel.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
