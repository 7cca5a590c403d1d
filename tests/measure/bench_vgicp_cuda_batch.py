"""Times FAST_VGICP_CUDA on a batch handle (riv-slam_amd/vgicp_cuda.py BatchVGICPCuda: per-slot prepared clouds and voxel maps, the GN / LM loop
on the device) against the only way the single handle offers to register many pairs: one FastVGICPCuda handle looping setInputSource /
setInputTarget / align.  Workload: 32 scene.py pairs of 8192 x 8192 points, device-resident tensors, FRESH clouds in every repetition (so every
repetition sorts, prepares and builds the voxel maps again), launch parameters (transformation_epsilon 0.1, max_correspondence_distance 2.0 --
not read by this mode --, azimuth variance 1.0), resolution 1.0, PLANE, DIRECT1 / DIRECT7 / DIRECT27 / DIRECT_RADIUS 1.5.  Both ways run in
the same process on the same box, in alternating blocks; the difference of the two single-loop blocks is the spread.
  (a) single_loop / single_loop_again   one handle: for each of the 32 pairs setInputSource, setInputTarget, align(guess)
  (b) batch                             one handle: set_clouds(64 clouds), align(32 pairs)
      batch_ticks                       align again over the unchanged clouds: no sort, no preparation, no map build
      phases                            a separate series with apdgicp_batch_set_profiling on: preparation / map builds / ticks of a fresh batch by
                                        the host clock at the phase boundaries, each behind a stream wait (medians over the series)
  (c) loop_verification                 one resident target x 32 candidates through loop_verifier's pair list: warm (nothing set again: ticks
                                        only) and with the 32 candidates set again (their preparation, no map build); against one handle that keeps
                                        its target and loops setInputSource / align over the candidates
Wall clock around calls that end with the records on the host; warm-up calls first, then the timed ones: median with p10 / p90, the device
otherwise idle.
usage: python tests/measure/bench_vgicp_cuda_batch.py [out.json] [--runs N]"""
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
SEARCH = (("direct1", 0, 1.5), ("direct7", 1, 1.5), ("direct27", 2, 1.5), ("radius1.5", 3, 1.5))
N_PAIRS, N_PTS = 32, 8192


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    vc = importlib.import_module("riv-slam_amd.vgicp_cuda")
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

    single = vc.FastVGICPCuda(params)
    batch = vc.BatchVGICPCuda(params)
    packed = batch.pack_clouds(clouds)
    pairs = batch.make_pairs(pair_ids, guesses)
    # loop verification: target 0 resident in slot 0, the 32 sources as candidates in slots 1 .. 32, every candidate from pair 0's guess
    lv = vc.BatchVGICPCuda(params)
    lv_cands = lv.pack_clouds(srcs)
    lv_pairs = lv.make_pairs([(1 + i, 0) for i in range(N_PAIRS)], [guesses[0]] * N_PAIRS)
    lv_single = vc.FastVGICPCuda(params)

    def single_loop():
        for i in range(N_PAIRS):
            single.setInputSource(srcs[i])
            single.setInputTarget(tgts[i])
            single.align(guesses[i])

    def batch_fresh():
        batch.set_clouds(0, packed)
        return batch.align(pairs)

    def lv_again():
        lv.set_clouds(1, lv_cands)
        return lv.align(lv_pairs)

    def lv_single_loop():
        for i in range(N_PAIRS):
            lv_single.setInputSource(srcs[i])
            lv_single.align(guesses[0])

    for name, mode, radius in SEARCH:
        for h in (single, batch, lv, lv_single):
            h.setNeighborSearchMethod(mode, radius)
        case = {"offsets": len(batch.offsets())}
        case["single_loop"] = timed(single_loop, runs=runs, warm=warm)
        case["batch"] = timed(batch_fresh, runs=runs, warm=warm)
        case["single_loop_again"] = timed(single_loop, runs=runs, warm=warm)
        recs = batch_fresh()
        case["batch_ticks"] = timed(lambda: batch.align(pairs), runs=runs, warm=warm)
        case["ticks_enqueued"] = batch.debug_counts()[2]
        case["ticks_needed"] = int((recs["n_linearize"] + recs["n_compute_error"]).max())
        case["ticks_per_pair_mean"] = float((recs["n_linearize"] + recs["n_compute_error"]).mean())
        case["converged"] = int(recs["converged"].sum())
        case["correspondences_mean"] = float(recs["n_matched"].mean())
        case["kept_points_mean"] = float(np.mean([len(batch.kept(s)) for s in range(0, 2 * N_PAIRS, 8)]))
        batch.set_profiling(True)
        ph = []
        for _ in range(warm + runs):
            batch_fresh()
            ph.append(batch.last_phases())
        batch.set_profiling(False)
        ph = np.array(ph[warm:])
        case["phases_ms"] = {"prepare": float(np.median(ph[:, 0])), "map_builds": float(np.median(ph[:, 1])), "ticks": float(np.median(ph[:, 2]))}
        a, a2 = case["single_loop"]["median_ms"], case["single_loop_again"]["median_ms"]
        b = case["batch"]["median_ms"]
        case["single_loop_spread"] = abs(a - a2) / min(a, a2)
        case["single_loop_registrations_per_s"] = N_PAIRS / min(a, a2) * 1e3
        case["batch_registrations_per_s"] = N_PAIRS / b * 1e3
        case["batch_over_single_loop"] = b / min(a, a2)     # below 1: the batch is faster (the faster of the two single-loop blocks is the baseline)
        # loop verification
        lv.clear()
        lv.set_clouds(0, lv.pack_clouds([tgts[0]] + srcs))
        lv_single.setInputTarget(tgts[0])
        lrecs = lv.align(lv_pairs)
        v = {"warm": timed(lambda: lv.align(lv_pairs), runs=runs, warm=warm), "candidates_set_again": timed(lv_again, runs=runs, warm=warm),
             "single_loop": timed(lv_single_loop, runs=runs, warm=warm), "converged": int(lrecs["converged"].sum()), "maps_built": lv.build_count()[1]}
        v["candidates_set_again_over_single_loop"] = v["candidates_set_again"]["median_ms"] / v["single_loop"]["median_ms"]
        case["loop_verification"] = v
        print(name, json.dumps(case), flush=True)
        out["cases"][name] = case

    path = next((a for a in args if a.endswith(".json")), os.path.join(ROOT, "profiles", "vgicp_cuda_batch.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
