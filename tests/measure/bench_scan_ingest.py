"""Times scan ingest and deskew (riv-slam_amd/scan_ingest.py) from DEVICE input at n = 512, 8 192 and 100 000, and the whole callback at
8 192 points.  Per size: `run` on a 48-byte array of structures (a PointCloud2 with doppler, xyz and intensity fields; ~5 % of the powers
below the threshold) and `deskew` + frame transform on the rows it produced (wall clock around the call followed by synchronize(): the
call itself does not wait), launches and waits as the library counts them.  Chain at 8 192 points (scene.raw_doppler_scan, host message
in, filtered scan resident): preprocess_scan as built, against the same chain with the deskew done the way the tree forced it before
this stage -- the source cloud copied to the host, the restatement's arithmetic vectorised in numpy (tests/scan_ingest_np.py), copied
back.  Protocol: 30 warm-up runs, 300 timed (100 at n = 100 000 and for the chains), median with p10 / p90.  No bar is set for this stage;
the numbers are observations.
usage: python tests/measure/bench_scan_ingest.py [out.json]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
from bench_scan_filter import timed  # noqa: E402
import scan_ingest_np as S  # noqa: E402

OMEGA = (0.31, -0.22, 0.47)


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    ing = importlib.import_module("riv-slam_amd.scan_ingest")
    ev = importlib.import_module("riv-slam_amd.ego_velocity")
    sf = importlib.import_module("riv-slam_amd.scan_filter")
    scene = importlib.import_module("riv-slam_amd.scene")
    T = scene.make_transform([0.3, -0.1, 1.2], 0.4, -0.25, 0.15).astype(np.float32)
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "cases": []}
    for n in (512, 8192, 100000):
        rng = np.random.default_rng(n)
        msg = rng.uniform(-60, 60, (n, 12)).astype(np.float32)
        msg[:, 10] = rng.uniform(0, 40, n)
        t = torch.from_numpy(msg).cuda()
        h = ing.ScanIngest(power_threshold=2.0)
        runs = 100 if n > 50000 else 300
        case = {"n": n, "input": "device, 48-byte records"}
        case["run"] = timed(lambda: h.run(t[:, 5:8], t[:, 10], t[:, 1]), runs=runs)
        case["run"].update(h.stats(), n_out=h.n)
        rows = h.points()

        def deskew():
            h.deskew(rows, OMEGA, 0.1, T)
            h.synchronize()
        case["deskew"] = timed(deskew, runs=runs)
        h.deskew(rows, OMEGA, 0.1, T)
        case["deskew"].update(h.stats(), n=rows.n)
        h.synchronize()
        print(json.dumps(case), flush=True)
        out["cases"].append(case)

    # the whole callback at 8 192 points
    raw = scene.raw_doppler_scan(8192, 3)
    raw[~np.isfinite(raw[:, :3]).all(axis=1), :3] = 1.25
    obj, est, flt = ing.ScanIngest(power_threshold=2.0), ev.EgoVelocityEstimator(), sf.ScanFilter()
    words = np.random.default_rng(0).integers(0, 2**32, (ev.hypothesis_count(est.params), est.params.N_ransac_points), dtype=np.uint32)
    xyz, power, dop = np.ascontiguousarray(raw[:, :3]), np.ascontiguousarray(raw[:, 3]), np.ascontiguousarray(raw[:, 4])

    def chain_device():
        return ing.preprocess_scan(obj, est, flt, xyz, power, dop, enable_dynamic_object_removal=True, ang_vel=OMEGA, T=T, words=words)["n_filtered"]

    def chain_host_deskew():
        obj.run(xyz, power, dop)
        est.run(obj.points(), words=words)
        src = est.to_numpy("inliers")["xyzi"]                      # the inliers copied to the host ...
        return flt.run(S.deskew(src, OMEGA, 0.1, T))               # ... deskewed there and copied back by the scan filter's staging

    n_dev, n_host = chain_device(), chain_host_deskew()
    chain = {"n": len(raw), "n_filtered": n_dev, "same_size_both_ways": bool(n_dev == n_host),
             "preprocess_scan": timed(chain_device, runs=100), "deskew_on_the_host": timed(chain_host_deskew, runs=100)}
    chain["speedup"] = chain["deskew_on_the_host"]["median_ms"] / chain["preprocess_scan"]["median_ms"]
    print(json.dumps(chain), flush=True)
    out["chain_8192"] = chain
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scan_ingest.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
