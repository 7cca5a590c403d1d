"""Times NDT on a batch handle (riv-slam_amd/ndt.py BatchNDT: per-slot voxel maps, the GN / LM loop on the device) against the only way the
single handle offers to register many pairs: one NDT handle looping setInputSource / setInputTarget / align.  Device-resident tensors,
default parameters (Levenberg-Marquardt, transformation_epsilon 5e-4), resolution 1.0 and 2.0, P2D and D2D, DIRECT1 / DIRECT7 / DIRECT27.
Both ways run in the same process on the same box, in alternating blocks.
Shape (a), throughput: 32 scene.py pairs of 8192 x 8192 points, FRESH clouds in every repetition (so every repetition sorts and builds the
voxel maps again).
  single_loop      one NDT handle: for each of the 32 pairs setInputSource, setInputTarget, align(guess); timed twice, before and after the
                   batch block: the difference of the two medians is the run-to-run spread the ratios are read against
  batch            one BatchNDT handle: set_clouds(64 clouds), align(32 pairs)
  batch_ticks      align again over the unchanged clouds: no sort, no map build -- the optimiser ticks and the records alone
  batch_rebuild    align after a resolution change of 1e-9 on unchanged clouds: ticks + the map builds (32 in P2D, 64 in D2D);
                   map_build_ms = this - batch_ticks, sort_and_upload_ms = batch - this
  ticks            the largest n_linearize + n_compute_error of a pair (what the device had to run) and the ticks the host enqueued (whole
                   chunks, one chunk ahead)
Shape (b), loop verification, DIRECT7: one resident target x 32 candidate sources of 8192 points (scene.make_keyframe_set).
  verify_single    one NDT handle: setInputTarget once, then per candidate setInputSource, align(guess)
  verify_warm      the batch over unchanged slots: every map cached from the batch before
  verify_cold      the 32 candidate slots set again in every repetition (sorted again; D2D: their maps built again), the target resident
Wall clock around calls that end with the records on the host; warm-up calls first, then the timed ones: median with p10 / p90, the device
otherwise idle.
usage: python tests/measure/bench_ndt_batch.py [out.json] [--runs N]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
from bench_scan_filter import timed  # noqa: E402

SEARCH = (("direct1", 0), ("direct7", 1), ("direct27", 2))
MODES = (("p2d", 0), ("d2d", 1))
RESOLUTIONS = (1.0, 2.0)
N_PAIRS, N_PTS = 32, 8192


def _ticks(recs):
    t = recs["n_linearize"] + recs["n_compute_error"]
    return {"ticks_needed": int(t.max()), "ticks_per_pair_mean": float(t.mean()), "iterations_min": int(recs["iterations"].min()),
            "iterations_max": int(recs["iterations"].max()), "converged": int(recs["converged"].sum()), "terms_mean": float(recs["n_matched"].mean())}


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    nd = importlib.import_module("riv-slam_amd.ndt")
    scene = importlib.import_module("riv-slam_amd.scene")
    args = sys.argv[1:]
    runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 10
    warm = 2
    params = reg.default_params()
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "pairs": N_PAIRS, "points": N_PTS, "runs": runs, "throughput": {}, "loop_verification": {}}

    made = [scene.make_pair(N_PTS, N_PTS, scene.pair_seed(5, i), "odometry") for i in range(N_PAIRS)]
    srcs = [torch.from_numpy(m[0]).cuda() for m in made]
    tgts = [torch.from_numpy(m[1]).cuda() for m in made]
    guesses = [m[3] for m in made]
    pair_ids = [(N_PAIRS + i, i) for i in range(N_PAIRS)]      # slots 0 .. 31 targets, 32 .. 63 sources
    kf_tgt, kf_cands, _, to_keyframe = scene.make_keyframe_set(N_PTS, N_PTS, N_PAIRS, scene.pair_seed(5, 100))
    kf_guesses = [np.linalg.inv(t.astype(np.float64)).astype(np.float32) for t in to_keyframe]
    kf_tgt = torch.from_numpy(kf_tgt).cuda()
    kf_cands = [torch.from_numpy(c).cuda() for c in kf_cands]

    single = nd.NDT(params)
    batch = nd.BatchNDT(params)
    packed = batch.pack_clouds(tgts + srcs)
    pairs = batch.make_pairs(pair_ids, guesses)
    verifier = nd.BatchNDT(params)
    kf_packed = verifier.pack_clouds(kf_cands)
    kf_pairs = verifier.make_pairs([(1 + i, 0) for i in range(N_PAIRS)], kf_guesses)
    step = [0]

    def single_loop():
        for i in range(N_PAIRS):
            single.setInputSource(srcs[i])
            single.setInputTarget(tgts[i])
            single.align(guesses[i])

    def batch_fresh():
        batch.set_clouds(0, packed)
        return batch.align(pairs)

    def verify_single():
        single.setInputTarget(kf_tgt)
        for i in range(N_PAIRS):
            single.setInputSource(kf_cands[i])
            single.align(kf_guesses[i])

    def verify_cold():
        verifier.set_clouds(1, kf_packed)
        return verifier.align(kf_pairs)

    for res in RESOLUTIONS:
        for mname, mode in MODES:
            for sname, search in SEARCH:
                for h in (single, batch):
                    h.setResolution(res)
                    h.setDistanceMode(mode)
                    h.setNeighborSearchMethod(search)

                def batch_rebuild():
                    step[0] += 1
                    batch.setResolution(res + 1e-9 * (1 + step[0] % 7))
                    return batch.align(pairs)

                case = {"maps_built_per_batch": N_PAIRS * (2 if mode == nd.D2D else 1)}
                case["single_loop"] = timed(single_loop, runs=runs, warm=warm)
                case["batch"] = timed(batch_fresh, runs=runs, warm=warm)
                case["single_loop_again"] = timed(single_loop, runs=runs, warm=warm)
                recs = batch_fresh()
                case["batch_ticks"] = timed(lambda: batch.align(pairs), runs=runs, warm=warm)
                case["ticks_enqueued"] = batch.last_ticks()[0]
                case.update(_ticks(recs))
                case["batch_rebuild"] = timed(batch_rebuild, runs=runs, warm=warm)
                batch.setResolution(res)
                a1, a2 = case["single_loop"]["median_ms"], case["single_loop_again"]["median_ms"]
                a, b = min(a1, a2), case["batch"]["median_ms"]
                case["map_build_ms"] = case["batch_rebuild"]["median_ms"] - case["batch_ticks"]["median_ms"]
                case["sort_and_upload_ms"] = b - case["batch_rebuild"]["median_ms"]
                case["single_loop_spread"] = abs(a1 - a2) / a          # of the two blocks of the same code in this process
                case["batch_over_single_loop"] = b / a                 # below 1: the batch is faster (the faster single-loop block is the baseline)
                case["faster_by_more_than_the_spread"] = bool(b < a * (1.0 - case["single_loop_spread"]))
                key = f"res{res:g}_{mname}_{sname}"
                print(key, json.dumps(case), flush=True)
                out["throughput"][key] = case

            # shape (b), DIRECT7
            for h in (single, verifier):
                h.setResolution(res)
                h.setDistanceMode(mode)
                h.setNeighborSearchMethod(1)
            verifier.clear()
            verifier.set_clouds(0, verifier.pack_clouds([kf_tgt] + kf_cands))
            recs = verifier.align(kf_pairs)
            case = dict(_ticks(recs))
            case["verify_single"] = timed(verify_single, runs=runs, warm=warm)
            case["verify_warm"] = timed(lambda: verifier.align(kf_pairs), runs=runs, warm=warm)
            case["ticks_enqueued"] = verifier.last_ticks()[0]
            case["verify_cold"] = timed(verify_cold, runs=runs, warm=warm)
            case["verify_single_again"] = timed(verify_single, runs=runs, warm=warm)
            a1, a2 = case["verify_single"]["median_ms"], case["verify_single_again"]["median_ms"]
            a = min(a1, a2)
            case["single_spread"] = abs(a1 - a2) / a
            case["warm_over_single"] = case["verify_warm"]["median_ms"] / a
            case["cold_over_single"] = case["verify_cold"]["median_ms"] / a
            key = f"res{res:g}_{mname}_direct7"
            print("verify", key, json.dumps(case), flush=True)
            out["loop_verification"][key] = case

    path = next((a for a in args if a.endswith(".json")), os.path.join(ROOT, "profiles", "ndt_batch.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
