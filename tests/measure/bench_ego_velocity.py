"""Times the device ego-velocity estimator (riv-slam_amd/ego_velocity.py) on a raw_doppler_scan of 8192 and of 16384 points, with K = 3 (the
reference's setRansacIter at its defaults) and K = 1024 hypotheses, from host and from device memory.  Protocol: 30 warm-up runs, then 300
timed runs per configuration (wall clock around a call that ends with the host holding the result record), median with p10 / p90.  The
scoring launch reads each 32-byte row once per group of 64 hypotheses, so its byte floor is 32 * m * ceil(K / 64) bytes at 8 TB/s.  This
script does not time that launch alone: it records the floor beside `more_hypotheses_ms` = median(K = 1024) - median(K = 3), the
END-TO-END cost of 1021 more hypotheses -- 15 more scoring groups, but also their solves, the larger arg-max and the 20 KB of words --
which bounds the scoring launch from above; `more_hypotheses_over_score_floor` is that bound over the floor, not the launch's own ratio
(blocks of the grid, which is sized by n, beyond m leave at once).  The launch's own time is in a kernel trace (docs/experiments.md).  Context, same process: the
scan-filter chain of the same scan's {x, y, z, intensity} and the numpy restatement (tests/ego_velocity_np.py, K = 3).
usage: python tests/measure/bench_ego_velocity.py [out.json]"""
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
    import ego_velocity_np as E
    reg = importlib.import_module("riv-slam_amd.registration")
    ev = importlib.import_module("riv-slam_amd.ego_velocity")
    sf = importlib.import_module("riv-slam_amd.scan_filter")
    scene = importlib.import_module("riv-slam_amd.scene")
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "cases": []}
    for n in (8192, 16384):
        raw = scene.raw_doppler_scan(n, 3)
        for where in ("host", "device"):
            cloud = torch.from_numpy(raw).cuda() if where == "device" else raw
            case = {"n": n, "input": where}
            for K in (3, 1024):
                est = ev.EgoVelocityEstimator(n_hypotheses=K)
                words = np.random.default_rng(0).integers(0, 2**32, (K, 5), dtype=np.uint32)
                case[f"K{K}"] = timed(lambda: est.run(cloud, words=words))
                case["m"] = est.result.m
            more = (case["K1024"]["median_ms"] - case["K3"]["median_ms"]) * 1e-3
            floor = 32.0 * case["m"] * ((1024 + 63) // 64) / 8e12
            case["score_byte_floor_ms_K1024"] = floor * 1e3
            case["more_hypotheses_ms"] = more * 1e3
            case["more_hypotheses_over_score_floor"] = more / floor if more > 0 else None
            flt = sf.ScanFilter()
            xyzi = torch.from_numpy(np.ascontiguousarray(raw[:, :4])).cuda() if where == "device" else np.ascontiguousarray(raw[:, :4])
            case["scan_filter_chain_same_scan"] = timed(lambda: flt.run(xyzi))
            if where == "host":
                w3 = np.random.default_rng(0).integers(0, 2**32, (3, 5), dtype=np.uint32)
                case["numpy_restatement_K3"] = timed(lambda: E.estimate(raw, E.Config(), w3), runs=10, warm=2)
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ego_velocity.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
