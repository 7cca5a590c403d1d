"""Times the device floor detector (riv-slam_amd/floor_detection.py) on a floor_scan of 8192 and of 131072 points with K = 64 and K = 1024
hypotheses, normal filtering on (the launch default) and off, from device memory.  Protocol: 30 warm-up runs, then 200 timed runs per
configuration (wall clock around a call that ends with the host holding the result record), median with p10 / p90, the device otherwise
idle.  The callback's memory is reset before every run, so that every run does the same work.  The scoring launch reads each 16-byte
point once per group of 64 hypotheses: its byte floor is 16 * m * ceil(K / 64) bytes at 8 TB/s.  This script does not time a launch alone
(that is the kernel trace, profiles/floor_detection_kernel_stats.md); `normal_filter_ms` = median(on) - median(off) bounds the k-NN stage
(pack, sort, boxes, search, and the second wait) from above, `more_hypotheses_ms` = median(K = 1024) - median(K = 64) the 15 more scoring
groups.  For scale only: the numpy restatement (tests/floor_detection_np.py) on the 8192-point scan.
usage: python tests/measure/bench_floor_detection.py [out.json] [--n N ...] [--runs R]"""
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
    import floor_detection_np as F
    reg = importlib.import_module("riv-slam_amd.registration")
    fd = importlib.import_module("riv-slam_amd.floor_detection")
    scene = importlib.import_module("riv-slam_amd.scene")
    args = [a for a in sys.argv[1:]]
    runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 200
    sizes = [int(a) for a in args[args.index("--n") + 1:] if a.isdigit()] if "--n" in args else [8192, 131072]
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "cases": []}
    for n in sizes:
        raw = scene.floor_scan(n, 3)
        cloud = torch.from_numpy(raw).cuda()
        case = {"n": n, "input": "device"}
        for nf in (1, 0):
            for K in (64, 1024):
                det = fd.FloorDetector(n_hypotheses=K, use_normal_filtering=nf)
                words = np.random.default_rng(0).integers(0, 2**32, (K, 3), dtype=np.uint32)

                def once():
                    det.reset()
                    return det.run(cloud, words=words)
                case[f"nf{nf}_K{K}"] = timed(once, runs=runs, warm=30)
                r = det.result
                case[f"nf{nf}_m"], case["n_clipped"], case[f"nf{nf}_K{K}_iterations"] = r.n_filtered, r.n_clipped, r.iterations
        for nf in (1, 0):
            more = (case[f"nf{nf}_K1024"]["median_ms"] - case[f"nf{nf}_K64"]["median_ms"]) * 1e-3
            floor = 16.0 * case[f"nf{nf}_m"] * ((1024 + 63) // 64) / 8e12
            case[f"nf{nf}_score_byte_floor_ms_K1024"], case[f"nf{nf}_more_hypotheses_ms"] = floor * 1e3, more * 1e3
        case["normal_filter_ms_K64"] = case["nf1_K64"]["median_ms"] - case["nf0_K64"]["median_ms"]
        if n <= 8192:
            w = np.random.default_rng(0).integers(0, 2**32, (64, 3), dtype=np.uint32)
            case["numpy_restatement_nf1_K64"] = timed(lambda: F.detect(raw, F.Config(), w, F.State.initial(F.Config())), runs=5, warm=1)
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    path = next((a for a in args if a.endswith(".json")), os.path.join(ROOT, "profiles", "floor_detection.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
