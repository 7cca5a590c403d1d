"""Times the device scan preprocessing (riv-slam_amd/scan_filter.py): the full chain range gate -> voxel grid 0.1 -> STATISTICAL 20 / 1.0
and its stages, on a raw_scan of 8192 and of 16384 points, from host and from device memory.  Protocol: 30 warm-up runs, then 300 timed
runs per configuration (wall clock around a call that ends with the host holding n_out), median with p10 / p90.  Stage times are
differences of medians of nested configurations (gate only; gate + voxel grid; the full chain).  Beside them, in the same process:
apdgicp_compute_covariances of the SAME downsampled cloud (set as a device-resident source, k = 21: pack, sort, boxes, the covariance
k-NN, one wait) -- the parent's kernel with the larger epilogue -- and the checker's kd-tree on the CPU for the same statistic.
usage: python tests/measure/bench_scan_filter.py [out.json]"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
WARM, RUNS = 30, 300


def timed(fn, runs=RUNS, warm=WARM):
    for _ in range(warm):
        fn()
    t = np.empty(runs)
    for i in range(runs):
        t0 = time.perf_counter()
        fn()
        t[i] = time.perf_counter() - t0
    return {"median_ms": float(np.median(t) * 1e3), "p10_ms": float(np.percentile(t, 10) * 1e3), "p90_ms": float(np.percentile(t, 90) * 1e3), "runs": runs}


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    sf = importlib.import_module("riv-slam_amd.scan_filter")
    scene = importlib.import_module("riv-slam_amd.scene")
    import ref as R
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "cases": []}
    for n in (8192, 16384):
        raw = scene.raw_scan(n, 3)
        for where in ("host", "device"):
            cloud = torch.from_numpy(raw).cuda() if where == "device" else raw
            case = {"n": n, "input": where}
            gate = sf.ScanFilter(leaf=None, outlier_method="NONE")
            vox = sf.ScanFilter(outlier_method="NONE")
            full = sf.ScanFilter()
            case["gate_only"] = timed(lambda: gate.run(cloud))
            case["gate_voxel"] = timed(lambda: vox.run(cloud))
            case["full_chain"] = timed(lambda: full.run(cloud))
            case["stage_counts"] = list(full.stage_counts())
            case["voxel_stage_ms"] = case["gate_voxel"]["median_ms"] - case["gate_only"]["median_ms"]
            case["statistic_stage_ms"] = case["full_chain"]["median_ms"] - case["gate_voxel"]["median_ms"]
            # the parent's kernel on the same cloud, same process
            vox.run(cloud)
            pts = vox.points()
            h = reg.FastAPDGICP(reg.default_params(k_correspondences=21))

            def cov():
                h.setInputSource(pts)
                h.computeCovariances(reg.SOURCE)
            case["compute_covariances_same_cloud"] = timed(cov)
            case["statistic_over_covariances"] = case["statistic_stage_ms"] / case["compute_covariances_same_cloud"]["median_ms"]
            if where == "host":
                s2 = vox.to_numpy()

                def cpu():
                    o = R.RefAPDGICP(R.default_params())
                    o.setInputTarget(np.ascontiguousarray(s2[:, :3]))
                    o.knn_kdtree_batch("target", s2[:, :3], 21)
                case["cpu_kdtree_same_statistic"] = timed(cpu, runs=10, warm=2)
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scan_filter.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
