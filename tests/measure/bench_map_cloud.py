"""Times the device map cloud generator (riv-slam_amd/map_cloud.py) on synthetic keyframes along a trajectory of scene.py
(tests/map_cloud_np.py: trajectory_keyframes), 64 x 8192 and 1024 x 8192 points, at map_cloud_resolution = 0.05, with the clouds resident:
only generate() is timed.  Protocol: 5 warm-up calls, then 30 timed calls per configuration (wall clock around a call that ends with the
host holding n_out), median with p10 / p90, the device otherwise idle; per stage the median of the device times the library takes with
events around its own launches (transform + gate, box replay with its host round trips, keys + sort, heads + centres).  For scale only:
the numpy restatement (tests/map_cloud_np.py) on the small case.
usage: python tests/measure/bench_map_cloud.py [out.json] [--keyframes K ...] [--runs R]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
from bench_scan_filter import timed  # noqa: E402

STAGES = ("transform_gate", "box_replay", "keys_sort", "heads_centres")


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    import map_cloud_np as M
    reg = importlib.import_module("riv-slam_amd.registration")
    mc = importlib.import_module("riv-slam_amd.map_cloud")
    scene = importlib.import_module("riv-slam_amd.scene")
    args = [a for a in sys.argv[1:]]
    runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 30
    counts = [int(a) for a in args[args.index("--keyframes") + 1:] if a.isdigit()] if "--keyframes" in args else [64, 1024]
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "resolution": 0.05, "points_per_keyframe": 8192, "cases": []}
    for K in counts:
        clouds, poses = M.trajectory_keyframes(scene, K, 8192, 7, origin=(250.0, -120.0, 3.0))
        case = {"keyframes": K}
        gen = mc.MapCloudGenerator()
        for c in clouds:
            gen.add_keyframe(c)
        stage = []

        def once():
            n = gen.generate(poses, None, 0.05)
            stage.append(gen.info()["stage_ms"])
            return n
        case["radix"] = timed(once, runs=runs, warm=5)
        med = np.median(np.array(stage[-runs:]), axis=0)
        case["radix"]["stage_ms"] = {k: float(v) for k, v in zip(STAGES, med)}
        info = gen.info()
        case.update(n_input=info["n_input"], n_pushed=info["n_pushed"], n_out=info["n_out"], depth=info["depth"], rounds=info["rounds"],
                    radix_passes=info["sort_passes"])
        del gen
        if K <= 64:
            case["numpy_restatement"] = timed(lambda: M.generate(clouds, poses, 0.05), runs=3, warm=1)
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    path = next((a for a in args if a.endswith(".json")), os.path.join(ROOT, "profiles", "map_cloud.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
