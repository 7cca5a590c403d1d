"""Times voxelized GICP on a batch handle (riv-slam_amd/vgicp.py BatchVGICP: per-slot voxel maps, the GN / LM loop on the device) against the
only way the single handle offers to register many pairs: one handle looping setInputSource / setInputTarget / align.  Workload: 32 scene.py
pairs of 8192 x 8192 points, device-resident tensors, FRESH clouds in every repetition (so every repetition sorts, computes covariances and
builds the voxel maps again), launch parameters (transformation_epsilon 0.1, max_correspondence_distance 2.0 -- ignored by VGICP --, azimuth
variance 1.0), resolution 1.0, DIRECT1 / DIRECT7 / DIRECT27.  Both ways run in the same process on the same box, alternating blocks.
  (a) single_loop      one FastVGICP handle: for each of the 32 pairs setInputSource, setInputTarget, align(guess)
  (b) batch            one BatchVGICP handle: set_clouds(64 clouds), align(32 pairs)
      batch_ticks      align again over the unchanged clouds: no sort, no covariances, no map build -- the optimiser ticks and the records alone
      batch_rebuild    align after a resolution change of 1e-9 on unchanged clouds: ticks + the 32 map builds; map_build_ms = this - batch_ticks
      batch_prepare    set_clouds + compute_covariances alone (sort, covariances, one wait)
  (c) apd_batch        BatchAPDGICP over the same clouds (set_clouds + align), for context: another cost function, another iteration count
ticks: the largest n_linearize + n_compute_error of a pair (what the device had to run) and the ticks the host enqueued (whole chunks, one
chunk ahead).  chunk_sweep: batch_ticks for APDGICP_VGB_CHUNK = 1 / 2 / 4 / 8 / 16, DIRECT7, each on a handle of its own, with the launch parameters and with the
default epsilons (transformation_epsilon 0.01: longer runs).
Wall clock around calls that end with the records on the host; warm-up calls first, then the timed ones: median with p10 / p90, the device
otherwise idle.
usage: python tests/measure/bench_vgicp_batch.py [out.json] [--runs N]"""
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
SEARCH = (("direct1", 0), ("direct7", 1), ("direct27", 2))
N_PAIRS, N_PTS = 32, 8192


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    vg = importlib.import_module("riv-slam_amd.vgicp")
    scene = importlib.import_module("riv-slam_amd.scene")
    args = sys.argv[1:]
    runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 20
    warm = 3
    made = [scene.make_pair(N_PTS, N_PTS, scene.pair_seed(5, i), "odometry") for i in range(N_PAIRS)]
    srcs = [torch.from_numpy(m[0]).cuda() for m in made]
    tgts = [torch.from_numpy(m[1]).cuda() for m in made]
    guesses = [m[3] for m in made]
    clouds = tgts + srcs                                        # slots 0 .. 31 targets, 32 .. 63 sources
    pair_ids = [(N_PAIRS + i, i) for i in range(N_PAIRS)]
    params = reg.default_params(**LAUNCH)
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "pairs": N_PAIRS, "points": N_PTS, "resolution": 1.0, "parameters": LAUNCH, "runs": runs, "cases": {}}

    single = vg.FastVGICP(params)
    batch = vg.BatchVGICP(params)
    packed = batch.pack_clouds(clouds)
    pairs = batch.make_pairs(pair_ids, guesses)
    apd = reg.BatchAPDGICP(params)

    def single_loop():
        for i in range(N_PAIRS):
            single.setInputSource(srcs[i])
            single.setInputTarget(tgts[i])
            single.align(guesses[i])

    def batch_fresh():
        batch.set_clouds(0, packed)
        return batch.align(pairs)

    def batch_prepare():
        batch.set_clouds(0, packed)
        batch.compute_covariances()

    step = [0]

    def batch_rebuild():
        step[0] += 1
        batch.setResolution(1.0 + 1e-9 * step[0])
        return batch.align(pairs)

    def apd_fresh():
        apd.set_clouds(0, packed)
        return apd.align(pairs)

    for name, mode in SEARCH:
        single.setNeighborSearchMethod(mode)
        batch.setNeighborSearchMethod(mode)
        batch.setResolution(1.0)
        case = {}
        case["single_loop"] = timed(single_loop, runs=runs, warm=warm)
        case["batch"] = timed(batch_fresh, runs=runs, warm=warm)
        case["single_loop_again"] = timed(single_loop, runs=runs, warm=warm)
        recs = batch_fresh()
        case["batch_ticks"] = timed(lambda: batch.align(pairs), runs=runs, warm=warm)
        case["ticks_enqueued"] = batch.last_ticks()[0]
        case["ticks_needed"] = int((recs["n_linearize"] + recs["n_compute_error"]).max())
        case["ticks_per_pair_mean"] = float((recs["n_linearize"] + recs["n_compute_error"]).mean())
        case["converged"] = int(recs["converged"].sum())
        case["correspondences_mean"] = float(recs["n_matched"].mean())
        case["maps_built_per_batch"] = N_PAIRS
        case["batch_rebuild"] = timed(batch_rebuild, runs=runs, warm=warm)
        batch.setResolution(1.0)
        case["batch_prepare"] = timed(batch_prepare, runs=runs, warm=warm)
        a = min(case["single_loop"]["median_ms"], case["single_loop_again"]["median_ms"])
        b = case["batch"]["median_ms"]
        case["map_build_ms"] = case["batch_rebuild"]["median_ms"] - case["batch_ticks"]["median_ms"]
        case["single_loop_registrations_per_s"] = N_PAIRS / a * 1e3
        case["batch_registrations_per_s"] = N_PAIRS / b * 1e3
        case["batch_over_single_loop"] = b / a     # below 1: the batch is faster (the faster of the two single-loop blocks is the baseline)
        print(name, json.dumps(case), flush=True)
        out["cases"][name] = case
    out["apd_batch"] = timed(apd_fresh, runs=runs, warm=warm)
    out["apd_batch"]["registrations_per_s"] = N_PAIRS / out["apd_batch"]["median_ms"] * 1e3
    print("apd_batch", json.dumps(out["apd_batch"]), flush=True)

    for key, prm in (("chunk_sweep_direct7_batch_ticks", params), ("chunk_sweep_direct7_batch_ticks_default_epsilons", reg.default_params())):
        sweep = {}
        for chunk in (1, 2, 4, 8, 16):
            os.environ["APDGICP_VGB_CHUNK"] = str(chunk)      # read when the mode is first switched on
            h = vg.BatchVGICP(prm)
            h.setNeighborSearchMethod(vg.DIRECT7)
            h.set_clouds(0, packed)
            recs = h.align(pairs)
            sweep[str(chunk)] = dict(timed(lambda: h.align(pairs), runs=runs, warm=warm), ticks_enqueued=h.last_ticks()[0],
                                     ticks_needed=int((recs["n_linearize"] + recs["n_compute_error"]).max()))
            del h
        os.environ.pop("APDGICP_VGB_CHUNK", None)
        out[key] = sweep
        print(key, json.dumps(sweep), flush=True)

    path = next((a for a in args if a.endswith(".json")), os.path.join(ROOT, "profiles", "vgicp_batch.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
