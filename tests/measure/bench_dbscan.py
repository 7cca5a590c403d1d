"""Times the device DBSCAN (riv-slam_amd/dbscan.py) from DEVICE input at n = 512 (a radar outlier cloud), 8 192 and 100 000: gaussian blobs of
sigma 0.3 (about 100 points each) with 5 % uniform noise over their bounding box, xyz + a Doppler lane, eps 0.35, minPts 5, clusters of >= 10.
Protocol: 30 warm-up runs, then 300 timed runs per size (100 at n = 100 000; wall clock around a run, which ends with the host holding K),
median with p10 / p90.  Launches and waits per run are the library's own count.  The split into phases is a SEPARATE series of 100 runs with
the handle's profiling on (device events at the phase boundaries, medians): sort = cells + radix sort + sorted copy, count, union + flatten,
border, output = rank sort + the wait + member lists + labels + table.  No bar is set for this stage; the numbers are observations.
usage: python tests/measure/bench_dbscan.py [out.json]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
from bench_scan_filter import timed  # noqa: E402


def blobs(n, seed=0):
    rng = np.random.default_rng(seed)
    n_noise = n // 20
    k = max(1, (n - n_noise) // 100)
    side = 4.0 * k ** (1.0 / 3.0)          # the blobs' centres keep their density as n grows
    centres = rng.uniform(-side, side, (k, 3))
    pts = centres[rng.integers(0, k, n - n_noise)] + 0.3 * rng.normal(size=(n - n_noise, 3))
    pts = np.concatenate([pts, rng.uniform(-side - 1, side + 1, (n_noise, 3))])
    rows = np.concatenate([pts, rng.normal(size=(n, 1)) * 5], axis=1).astype(np.float32)
    return np.ascontiguousarray(rows[rng.permutation(n)])


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    db = importlib.import_module("riv-slam_amd.dbscan")
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "cases": []}
    for n in (512, 8192, 100000):
        t = torch.from_numpy(blobs(n)).cuda()
        h = db.DBSCAN(eps=0.35, min_pts=5, min_cluster_size=10)
        case = {"n": n, "input": "device"}
        case["run"] = timed(lambda: h.run(t, t[:, 3]), runs=100 if n > 50000 else 300)
        st = h.stats()
        lab = h.labels()
        case.update(clusters=h.n_clusters, members=int(h.members()[0][-1]), noise_points=int(np.count_nonzero(lab < 0)), launches=st["launches"], waits=st["waits"])
        h.set_profiling(True)
        series = []
        for i in range(120):
            h.run(t, t[:, 3])
            if i >= 20:
                series.append(list(h.stats()["phase_ms"].values()))
        med = np.median(np.array(series), axis=0)
        case["phase_ms_median"] = dict(zip(("sort", "count", "union_flatten", "border", "output"), (float(v) for v in med)))
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dbscan.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
