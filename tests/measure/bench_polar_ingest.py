"""Times the polar ingest and the distance histogram (riv-slam_amd/scan_ingest.py) at n = 512, 8 192 and 100 000 targets, from 76-byte
records on the device and on the host.  Per size and input, wall clock around the call followed by synchronize():
  run_polar      one launch, no wait of its own;
  run            the Cartesian ingest of the converted cloud (the rows run_polar produced, as a 32-byte array of structures, gate on, no
                 power below the threshold): three launches and the one wait for n_out -- context, not a competitor;
  histogram_add  of the rows: two launches, no wait of its own.
Chain at 8 192 targets (scene.raw_doppler_scan converted to polar in fp64, host message in, filtered scan resident): preprocess_polar_scan
as built, against the same chain with the conversion done in numpy on the host (tests/polar_ingest_np.py) and the Cartesian cloud
uploaded through run(gate = 0) -- what a user with a polar radar had to do before -- and preprocess_polar_scan without the histogram.
Protocol: the series of one size alternate in blocks of 50 timed calls (10 warm-up calls in front of each block), 4 blocks per series in
one process; the median of all timed calls per series, and the medians of the single blocks: `spread` is (largest - smallest block
median) / overall median, the noise against which a ratio between two series is to be read.  No bar is set; the numbers are observations.
usage: python tests/measure/bench_polar_ingest.py [out.json]"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
import polar_ingest_np as P  # noqa: E402

OMEGA = (0.31, -0.22, 0.47)
BLOCKS, PER_BLOCK, WARM = 4, 50, 10


def alternate(series: dict) -> dict:
    """series: name -> callable.  Blocks of the series in turn; -> name -> dict(median_ms, block_medians_ms, spread, runs)"""
    t = {k: [] for k in series}
    for _ in range(BLOCKS):
        for k, fn in series.items():
            for _ in range(WARM):
                fn()
            b = np.empty(PER_BLOCK)
            for i in range(PER_BLOCK):
                t0 = time.perf_counter()
                fn()
                b[i] = time.perf_counter() - t0
            t[k].append(b)
    out = {}
    for k, blocks in t.items():
        med = float(np.median(np.concatenate(blocks)) * 1e3)
        bm = [float(np.median(b) * 1e3) for b in blocks]
        out[k] = {"median_ms": med, "block_medians_ms": bm, "spread": (max(bm) - min(bm)) / med, "runs": BLOCKS * PER_BLOCK}
    return out


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
        rec = P.targets(*P.fixture(n, n))
        h = ing.ScanIngest(power_threshold=-1.0)
        h.run_polar(rec)
        cart = h.to_numpy()["rows"]                                   # the converted cloud as 32-byte records
        for where in ("device", "host"):
            r = rec if where == "host" else torch.from_numpy(rec).cuda()
            c = cart if where == "host" else torch.from_numpy(cart).cuda()

            def run_polar():
                h.run_polar(r)
                h.synchronize()

            def run():
                h.run(c[:, :3], c[:, 3], c[:, 4])
                h.synchronize()

            def histogram_add():
                h.histogram_add(c)
                h.synchronize()
            case = {"n": n, "input": f"{where}, 76-byte records"}
            case.update(alternate({"run_polar": run_polar, "run": run, "histogram_add": histogram_add}))
            h.run_polar(r)
            case["run_polar"].update(h.stats())
            h.run(c[:, :3], c[:, 3], c[:, 4])
            case["run"].update(h.stats())
            h.histogram_add(c)
            case["histogram_add"].update(h.stats())
            h.synchronize()
            print(json.dumps(case), flush=True)
            out["cases"].append(case)

    # the whole callback at 8 192 targets
    raw = scene.raw_doppler_scan(8192, 3)
    raw[~np.isfinite(raw[:, :3]).all(axis=1), :3] = 1.25
    x, y, z = (raw[:, q].astype(np.float64) for q in range(3))
    rec = P.targets(np.sqrt(x * x + y * y + z * z), np.arctan2(y, x), np.arctan2(-z, np.hypot(x, y)), raw[:, 3], raw[:, 4])
    obj, est, flt = ing.ScanIngest(gate=0), ev.EgoVelocityEstimator(), sf.ScanFilter()
    words = np.random.default_rng(0).integers(0, 2**32, (ev.hypothesis_count(est.params), est.params.N_ransac_points), dtype=np.uint32)

    def chain_device():
        return ing.preprocess_polar_scan(obj, est, flt, rec, ang_vel=OMEGA, T=T, words=words)["n_filtered"]

    def chain_device_no_histogram():
        return ing.preprocess_polar_scan(obj, est, flt, rec, ang_vel=OMEGA, T=T, words=words, histogram=False)["n_filtered"]

    def chain_host_conversion():
        rows = P.polar_rows(rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 4], rec[:, 3])[0]      # the conversion on the host ...
        return ing.preprocess_scan(obj, est, flt, rows[:, :3], rows[:, 3], rows[:, 4], enable_dynamic_object_removal=True, ang_vel=OMEGA, T=T, words=words,
                                   histogram=True)["n_filtered"]                          # ... uploaded; the rest as built
    n_dev, n_host = chain_device(), chain_host_conversion()
    chain = {"n": len(rec), "n_filtered": n_dev, "n_filtered_host_conversion": n_host}
    chain.update(alternate({"preprocess_polar_scan": chain_device, "without_histogram": chain_device_no_histogram, "conversion_on_the_host": chain_host_conversion}))
    chain["speedup_over_host_conversion"] = chain["conversion_on_the_host"]["median_ms"] / chain["preprocess_polar_scan"]["median_ms"]
    chain["histogram_cost_ms"] = chain["preprocess_polar_scan"]["median_ms"] - chain["without_histogram"]["median_ms"]
    print(json.dumps(chain), flush=True)
    out["chain_8192"] = chain
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "polar_ingest.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
