#!/usr/bin/env python3
"""bench.py -- APD-GICP registrations/s on MI355X (BASELINE.json metric).

A "step" registers, on every GPU, one batch of P independent 8k x 8k synthetic radar scan pairs
(BASELINE configs[1] = "single scan-to-scan APD-GICP, 8k-pt source/target, 20 GN iters"; P = 32 pairs
per GPU is the per-GPU shard of configs[3], 256 pairs over 8 GPUs -> weak scaling).  The raw clouds
are resident in HBM before the timed region; a step packs them, computes BOTH clouds' k-NN covariances
(nothing cached), runs 20 Gauss-Newton iterations per pair on the device and, for N > 1, all-gathers
the 96-byte result records with RCCL.  Synthetic data, seeded (riv-slam_amd/scene.py).

  python bench.py --gpus N --steps K --warmup W        N > 1 without a launcher: bench.py starts its own N ranks
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Timing protocol: W warm-up steps, then the region "exactly K steps, barrier + device synchronise on both
sides, MAX over ranks" is repeated R times (--repeats; default 1, so a plain run times exactly K steps, and 20 with
--full); `value` / `ms_per_step` are the MEDIAN repetition, p10 / p90 / mean / the first repetition are printed beside
it, and each repetition is also timed with HIP events recorded on the handles' own streams (`timing.event_ms_per_step`).
Rank 0 prints ONE JSON line.

A plain run measures the headline only.  --full adds the legs that take runs of their own (one GPU): single-pair
latency, the executed-flops and brute-force diagnostics, the pooled LM loop batch, the dense C5 pair and the CPU
baseline with its parity check.  --dump-outputs DIR writes the records of the last timed step, one .npy per field.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_PTS = 8192
GN_ITERS = 20
FP32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: fp32 vector peak (FMA-based)
HBM_PEAK_GBS = 8000.0
# measured plain (non-packed, non-fused) fp32 VALU issue ceiling of this chip: 62e12 lane-ops/s / 64 lanes
# (tools/ubench_valu.hip, profiles/r01_ubench_valu.txt) -- the roof of the exact, FMA-free nearest-neighbour arithmetic
VALU_WAVE_INSTR_PEAK = 62.0e12 / 64
# the chip's theoretical VALU issue ceiling: 1024 SIMD-32 x 2.4 GHz / 2 cycles per wave64 instruction (MI355X_MICROARCH.md)
VALU_WAVE_INSTR_THEORETICAL = 1024 * 2.4e9 / 2
SIMDS, GFX_CLOCK_HZ = 1024, 2.4e9   # (GRBM_GUI_ACTIVE / 8 XCDs / launch time under these kernels: 2.33 - 2.34 GHz, profiles/r05_pmc_occ.md)
LM_LAUNCH = dict(max_correspondence_distance=2.0, transformation_epsilon=0.1, azimuth_variance_deg=1.0)   # the launch file's registration parameters (LM, L:17)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=None,
                    help="repetitions of the timed K-step region (median / p10 / p90 are reported); default 1, 20 with --full")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beside the headline (one GPU): single-pair latency, diagnostics, LM loop batch, C5, CPU baseline")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0 writes the records of the last timed step to DIR/<field>.npy (float32 / float64, one file per record field)")
    ap.add_argument("--pairs-per-gpu", type=int, default=32)
    ap.add_argument("--points", type=int, default=N_PTS)
    ap.add_argument("--kind", default="odometry", choices=("odometry", "loop"), help="scene.make_pair kind of the synthetic pairs")
    ap.add_argument("--optimizer", default="gn", choices=("gn", "lm"),
                    help="gn: BASELINE configs[1] (20 Gauss-Newton iterations, no early exit); lm: the reference's optimiser with the launch parameters "
                         "(with --kind loop: SURVEY 8d's C4 shard) on ONE pooled handle with --handles batches in flight")
    ap.add_argument("--handles", type=int, default=0, help="batch handles = steps kept in flight (0: 4; 1: one handle with three pair groups)")
    ap.add_argument("--depth", type=int, default=1, help="steps in flight PER handle (Gauss-Newton only; a handle alternates between two record buffers, so 1 or 2)")
    ap.add_argument("--groups", type=int, default=1, help="pair groups (HIP streams) per handle when several handles are in flight")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="budget of the cpu_baseline leg (--full; rank 0, N=1 only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-diagnostics", action="store_true", help="with --full: skip the untimed executed-flops / brute-force legs")
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed (RCCL) even for one rank (self-test of the N>1 path)")
    ap.add_argument("--ranks-share-gpu", action="store_true",
                    help="every rank uses GPU 0: exercises the N > 1 loop (late gather, barrier, MAX over ranks) on a one-GPU box; needs "
                         "--dist-backend gloo (RCCL refuses two ranks on one device).  A self-test, not a scaling measurement")
    ap.add_argument("--dist-backend", default="nccl", choices=("nccl", "gloo"),
                    help="nccl = RCCL over xGMI, records gathered from device memory (the measured configuration); gloo: the 96-byte records "
                         "travel as CPU tensors through the same gather / barrier / all_reduce(MAX) code")
    ap.add_argument("--host-clouds", action="store_true",
                    help="every step hands the library HOST clouds (numpy, pageable) instead of resident device buffers: the PCIe-inclusive rate "
                         "DESIGN.md quotes beside the headline -- never the headline itself")
    ap.add_argument("--fp32-point-math", action="store_true",
                    help="APDGICP_FLAG_FP32_POINT_MATH: the opt-in fp32 per-point algebra (NOT the reference's precision: an A/B line, never the headline)")
    ap.add_argument("--extra-flags", type=int, default=0, help="experiments only: OR these bits into apdgicp_params.flags (e.g. 1 = plain GICP: what the sensor model costs)")
    ap.add_argument("--dump-records", default=None, help="rank 0 writes the gathered records of the last step (uint8 [pairs, 96]) to this .npy file")
    return ap.parse_args()


def spawn_ranks(args) -> int:
    """`python bench.py --gpus N` without a launcher: N fresh child processes, one per GPU, started BEFORE this process has
    imported torch or touched HIP (a process that has initialised the GPU must never exec or fork workers).  Rank 0 inherits
    stdout and prints the JSON line; the parent only waits."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    deadline = time.time() + 3600
    alive = list(procs)
    while alive:
        for p in list(alive):
            code = p.poll()
            if code is None:
                continue
            alive.remove(p)
            if code != 0:
                rc = rc or code
                for q in alive:      # one rank failed: the others would wait in a collective forever
                    q.terminate()
        if time.time() > deadline:
            for q in alive:
                q.kill()
            return rc or 124
        time.sleep(0.05)
    return rc


def load_pmc(path=None, stamp=None):
    """The committed PMC profile (profiles/pmc_nn_latest.json), or (None, reason): counters belong to the kernels they were
    collected from, so a file whose source stamp (tools/pmc_nn_json.py: hash of riv-slam_amd/csrc/*) differs from the sources
    this run was built from is refused -- the line then prints null for every PMC-derived field and says why."""
    path = path or os.path.join(ROOT, "profiles", "pmc_nn_latest.json")
    try:
        with open(path) as fh:
            pmc = json.load(fh)
    except Exception as e:  # noqa: BLE001
        return None, f"{os.path.relpath(path, ROOT)}: {type(e).__name__}"
    if stamp is None:
        # the stamp compiled into the library this process loaded (apdgicp_source_stamp) -- which the loader has already compared
        # with the sources on disk (registration.load_library refuses a library built from other sources)
        stamp = importlib.import_module("riv-slam_amd.registration").source_stamp()
    have = pmc.get("source_stamp")
    if have != stamp:
        return None, (f"{os.path.relpath(path, ROOT)} was collected from kernel sources {have or '(unstamped)'}, this run is built from {stamp}: "
                      "re-run tools/refresh_evidence.sh and commit the file")
    return pmc, None


def scaling_efficiency(value, world, args, lm):
    """value / (world x the committed one-GPU value of the same workload): profiles/r06_bench.json for the default line, profiles/r06_bench_lm_loop.json for
    --kind loop --optimizer lm.  None when the workload differs from the committed one (pairs per GPU, points, host clouds, shared GPU)."""
    if args.ranks_share_gpu or args.host_clouds or args.points != N_PTS or args.pairs_per_gpu != 32:
        return {"value": None, "reason": "not a scaling point: ranks share one GPU, host clouds, or another workload than the committed one-GPU line"}
    name = "r06_bench_lm_loop.json" if lm and args.kind == "loop" else ("r06_bench.json" if not lm and args.kind == "odometry" else None)
    try:
        with open(os.path.join(ROOT, "profiles", name)) as fh:
            one = json.loads(fh.read().strip().splitlines()[-1])
        if one.get("n_gpus") != 1:
            return None
        return {"value": round(value / (world * one["value"]), 4), "one_gpu_value": one["value"], "one_gpu_source": "profiles/" + name}
    except Exception:  # noqa: BLE001
        return None


def c5_pmc_fields(load):
    """c5_dense: the dense search launch's own vector-issue occupancy from the committed counter profile of tools/c5_profile.sh (profiles/pmc_c5.json; refused
    -- null and the reason -- when it was collected from other kernel sources than the loaded library's)."""
    pmc, why = load(os.path.join(ROOT, "profiles", "pmc_c5.json"))
    if not pmc:
        return {"valu_busy_of_the_search_launch": None, "pmc_profile": {"rejected": why}}
    return {"valu_busy_of_the_search_launch": round(pmc.get("valu_busy_of_the_launch_alone", 0.0), 3),
            "search_launch_pmc": {"avg_us_alone": round(pmc.get("avg_us_serialised_by_pmc", 0.0), 1), "SQ_INSTS_VALU": pmc.get("SQ_INSTS_VALU"),
                                  "SQ_INSTS_SALU": pmc.get("SQ_INSTS_SALU"), "SQ_WAVES": pmc.get("SQ_WAVES"),
                                  "hbm_bytes": ((2.0 * pmc["FETCH_SIZE"] + pmc["WRITE_SIZE"]) * 1024 if "FETCH_SIZE" in pmc and "WRITE_SIZE" in pmc else None),
                                  "source": pmc.get("source")}}


def percentiles(xs):
    import numpy as np
    a = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(a)), 4), "p10": round(float(np.percentile(a, 10)), 4), "p90": round(float(np.percentile(a, 90)), 4),
            "mean": round(float(a.mean()), 4), "min": round(float(a.min()), 4), "max": round(float(a.max()), 4)}


def bench_params(reg, optimizer="gn"):
    # configs[1]: GN, 20 iterations, never early-exit; gate / APD variances as shipped in the launch file
    if optimizer == "lm":
        return reg.default_params(**LM_LAUNCH)
    return reg.default_params(optimizer=reg.OPT_GN, max_iterations=GN_ITERS, transformation_epsilon=1e-300, rotation_epsilon=1e-300,
                              max_correspondence_distance=2.0, azimuth_variance_deg=1.0)


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    if os.environ.get("APDGICP_BENCH_SPAWN_PROBE"):   # tests/test_sharded_cpu.py: what a spawned rank sees, before any GPU / torch work
        print(json.dumps({"rank": int(os.environ.get("RANK", "0")), "world": int(os.environ.get("WORLD_SIZE", "1")),
                          "local_rank": int(os.environ.get("LOCAL_RANK", "0")), "master": os.environ.get("MASTER_ADDR"),
                          "torch_imported": "torch" in sys.modules}), flush=True)
        return

    # Three or four batch handles (one stream each) plus RCCL's stream are busy at once; the HIP runtime multiplexes the streams
    # of a process onto 4 hardware queues by default, and a fifth busy stream costs ~5 %.  Must be in the environment before
    # the runtime initialises.  The OpenMP settings are those of the cpu_baseline leg (stated in its JSON object).
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    os.environ.setdefault("OMP_PROC_BIND", "false")
    os.environ.setdefault("OMP_WAIT_POLICY", "passive")
    import importlib

    import numpy as np
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU fallback)"
    gloo = args.dist_backend == "gloo"
    if args.ranks_share_gpu:
        if world > 1 and not gloo:
            raise SystemExit("--ranks-share-gpu needs --dist-backend gloo: RCCL refuses two ranks on one device")
        local_rank = 0
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or args.force_dist
    rccl_version = None

    import __graft_entry__ as ge
    ge.build()
    reg = importlib.import_module("riv-slam_amd.registration")
    scene = importlib.import_module("riv-slam_amd.scene")
    sharded = importlib.import_module("riv-slam_amd.sharded")

    P, n, K = args.pairs_per_gpu, args.points, args.steps
    total_pairs = P * world
    my_b, my_e = sharded.block_partition(total_pairs, world)[rank]
    assert my_e - my_b == P

    # ---- synthetic inputs, generated on the host, resident in HBM before timing
    d_clouds, h_pairs, guesses = [], [], []
    for p in range(my_b, my_e):
        s, t, _, g = scene.make_pair(n, n, scene.pair_seed(2, p), args.kind)
        if args.kind == "loop":
            g = np.eye(4, dtype=np.float32)     # loop_detector.cpp:225 aligns loop candidates from the identity
        h_pairs.append((s, t, g))
        d_clouds += [torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()]
        guesses.append(g)
    pair_idx = [(2 * i, 2 * i + 1) for i in range(P)]
    torch.cuda.synchronize()

    lm = args.optimizer == "lm"
    params = bench_params(reg, args.optimizer)
    if args.fp32_point_math:
        params.flags |= reg.FLAG_FP32_POINT_MATH
    params.flags |= args.extra_flags
    # Consecutive steps are independent batches, so several of them are kept in flight: step s runs on batch handle s % H
    # (H = --handles, 4 by default), each handle with ONE pair group = one HIP stream.  A step alone leaves the GPU
    # underfed (32 pairs: three groups of latency-bound tick kernels); with several steps at different phases one handle's
    # covariance kernels fill the gaps of the others' ticks.  Every handle registers its own copy of the step's clouds.
    # Levenberg-Marquardt (--optimizer lm): ONE handle; its pair pool merges the H batches in flight, each in its own range of
    # cloud slots (include/apdgicp_hip.h), H = 24 by default.
    H = args.handles if args.handles > 0 else (24 if lm else 4)   # r02 (lazy group streams: every handle's stream on a hardware queue of its own): 3 / 4 / 5 / 6 handles 1.00 / 0.92 / 0.99 / 0.99 ms per step; with a process group 1.00 / 0.96 / 1.14
    batches = []
    for _ in range(1 if lm else H):
        bh = reg.BatchAPDGICP(params, device=local_rank)
        bh.set_profiling(os.environ.get("APDGICP_BENCH_NOPROF", "0") != "1")
        if H > 1 and not lm:
            bh.set_pair_groups(max(1, args.groups))
        batches.append(bh)
    batch = batches[0]
    if lm:   # batches one handle keeps in flight: the pool's lanes; without the pool (APDGICP_LM_POOL=0, brute-force search) two record buffers
        lanes = int(batch.L.apdgicp_batch_is_pooled(batch.b))
        H = max(1, min(H, lanes if lanes > 0 else 2))
    # The process group comes AFTER the handles: the runtime deals streams onto its hardware queues in creation order, and RCCL
    # creates streams of its own -- behind the handles' they leave every handle's tick stream a queue to itself (the C++ aligner:
    # 1.01 -> 0.83 ms per step with the communicator created after the handles; here, with torch's lazily created streams, the
    # order measured the same either way: 0.770 ms per step with --force-dist).
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        # (stdout carries ONE JSON line: with NCCL_DEBUG=VERSION in the environment RCCL writes its version banner to the C-level
        # stdout when the communicator is created -- that goes to stderr here)
        import ctypes
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            if gloo:
                os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")   # one node: never resolve the (possibly unresolvable) hostname
                import datetime
                dist.init_process_group(backend="gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
            else:
                dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
            dist.barrier()
            torch.cuda.synchronize()
        finally:
            try:
                ctypes.CDLL(None).fflush(None)
            finally:
                os.dup2(saved_fd, 1)
                os.close(saved_fd)
        try:
            rccl_version = None if gloo else ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            rccl_version = "unknown"
    # slot s % H of the schedule: (handle, first cloud slot, pair table)
    D = 1 if lm else max(1, min(2, args.depth))
    S = H * D   # steps in flight
    slots = [(batches[0], 2 * P * h, batch.make_pairs([(2 * P * h + a, 2 * P * h + b_) for a, b_ in pair_idx], guesses)) if lm else
             (batches[h % H], 0, batch.make_pairs(pair_idx, guesses)) for h in range(S)]
    pairs_arr = slots[0][2]
    # the pointer array a C caller would hold; the clouds themselves are re-registered every step
    clouds_arg = batch.pack_clouds([c for s_, t_, _g in h_pairs for c in (s_, t_)] if args.host_clouds else d_clouds)
    hstreams = [torch.cuda.ExternalStream(bh.stream_ptr(), device=local_rank) for bh in batches]

    class Engine:  # this rank's block through the C ABI, synchronous form (ShardedBatchAligner.align); the timed loop uses gather() only
        def align_block(self, _indices):
            batch.set_clouds(0, clouds_arg)
            return batch.align_device(pairs_arr)

    aligner = sharded.ShardedBatchAligner(Engine())
    nn_acc = [0.0, 0, 0]

    # A step = set this rank's 64 fresh clouds (packed, sorted, covariances recomputed) + register its 32 pairs + (N > 1)
    # all-gather the records.  enqueue returns without waiting (Gauss-Newton: the run length is known); a step is collected
    # -- waited for, gathered -- just before its handle is needed again, H steps later.
    def enqueue_step(h):
        bh, base, arr = slots[h]
        # (resident inputs, complete long ago: no wait on torch's stream, which carries the all-gathers -- except with two steps in flight per handle:
        # this enqueue reuses the record buffer whose all-gather was issued a moment ago, so the handle's stream waits for it, on the device)
        bh.set_clouds(base, clouds_arg, producer_wait=(D > 1 and use_dist and not gloo))
        return bh.align_enqueue(arr)

    # N > 1: the all-gather of a step reads that step's record buffer, which its handle overwrites two enqueues later (the
    # handle alternates between two buffers).  So the host does not wait for the collective where it issues it, but one round
    # later, when the same handle is collected again -- just in front of the enqueue that could reuse the buffer.  Waiting at
    # once made every rank wait for the slowest rank's same step, every step; this way ranks may drift by a few steps.
    gather_done = {}   # slot -> event behind its last all-gather
    lat = []           # submit -> collect of every step of the timed region, seconds
    gather_ev = []     # (event in front, event behind) of the all-gathers of the timed region (RCCL: on torch's current stream)
    gather_host = []   # gloo: host seconds inside the gather call (the collective is complete when it returns)

    def collect_step(h, ticket, t_submit):
        bh = slots[h][0]
        ev = gather_done.get(h)
        if ev is not None:
            ev.synchronize()
        if gloo:   # (self-test backend: the records leave as a CPU tensor; the collective is complete when gather returns)
            local = torch.from_numpy(bh.align_collect(ticket, device=False).view(np.uint8).reshape(-1, sharded.RESULT_BYTES))
        else:
            local = bh.align_collect(ticket, device=True)    # zero-copy view of that step's records on the device
        lat.append(time.perf_counter() - t_submit)
        timed_gather = use_dist and not gloo and len(gather_ev) < 256
        if timed_gather:
            g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g0.record(torch.cuda.current_stream())
        t_g = time.perf_counter()
        out = aligner.gather(local, total_pairs, wait=False)
        if use_dist and gloo:
            gather_host.append(time.perf_counter() - t_g)
        if timed_gather:
            g1.record(torch.cuda.current_stream())
            gather_ev.append((g0, g1))
        if use_dist and not gloo:
            if ev is None:
                ev = gather_done[h] = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
        ms, k, pr = bh.last_nn_profile()
        nn_acc[0] += ms
        nn_acc[1] += k
        nn_acc[2] += pr
        return out

    def run_steps(count):
        tickets, out = [None] * S, None
        for s in range(count):
            h = s % S
            if tickets[h] is not None:
                out = collect_step(h, *tickets[h])
            t_sub = time.perf_counter()
            tickets[h] = (enqueue_step(h), t_sub)
        for s in range(count, count + S):   # the steps still in flight, oldest first
            h = s % S
            if tickets[h] is not None:
                out = collect_step(h, *tickets[h])
                tickets[h] = None
        for ev in gather_done.values():      # every collective of this run has read its records (and `out` is complete)
            ev.synchronize()
        return out

    def sync_all():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    run_steps(args.warmup)
    R = max(1, args.repeats if args.repeats is not None else (20 if args.full else 1))
    host_s, event_ms = [], []
    ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(R)]
    ev1 = [[torch.cuda.Event(enable_timing=True) for _ in range(H + 1)] for _ in range(R)]
    nn_acc[:] = [0.0, 0, 0]
    lat.clear()
    gather_ev.clear()
    gather_host.clear()
    gathered = None
    pool0 = batch.pool_counters() if lm else (0, 0, 0)
    for r in range(R):
        sync_all()
        ev0[r].record(hstreams[0])           # the GPU is idle: this timestamp is the start of the region on the device clock
        t0 = time.perf_counter()
        gathered = run_steps(K)              # every step enqueued AND collected (and gathered) inside the timed region
        for h in range(len(hstreams)):
            ev1[r][h].record(hstreams[h])    # behind the last batch of every handle ...
        ev1[r][len(hstreams)].record(torch.cuda.current_stream())   # ... and behind the last gather
        sync_all()
        host_s.append(time.perf_counter() - t0)
        event_ms.append(max(ev0[r].elapsed_time(e) for e in ev1[r][:len(hstreams) + 1]))
    pool1 = batch.pool_counters() if lm else (0, 0, 0)
    slot_ticks_per_step = (pool1[2] - pool0[2]) / float(R * K) if lm else None
    nn_ms, nn_launches, nn_pairs = nn_acc
    host_t = torch.tensor(host_s, dtype=torch.float64, device="cpu" if gloo else "cuda")
    per_rank = None
    if use_dist:
        # every rank's own median time per step (before the MAX): the imbalance between ranks, for the first real SCALE run
        mine = torch.tensor([float(np.median(host_s)) / K * 1e3], dtype=torch.float64, device=host_t.device)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [round(float(v.item()), 4) for v in allr]
        dist.all_reduce(host_t, op=dist.ReduceOp.MAX)     # per repetition: the slowest rank
    host_s = [float(v) for v in host_t.cpu()]
    if gather_ev:
        torch.cuda.synchronize()
        gather_ms = [a.elapsed_time(b) for a, b in gather_ev]
    else:
        gather_ms = [t * 1e3 for t in gather_host]
    elapsed = float(np.median(host_s))
    ms_per_step = elapsed / K * 1e3
    value = total_pairs * K / elapsed
    ticks, nn_S, nn_T = batch.last_ticks()

    out = None
    if rank == 0:
        recs = sharded.records_from_bytes(gathered)
        assert len(recs) == total_pairs and (lm or int(recs["n_linearize"].min()) == GN_ITERS)
        if args.dump_outputs:
            # what a caller of the step receives: the records of all pairs, field by field (T: fp32 column-major 4x4 per pair,
            # final_cost fp64, the integer counters and flags as fp64)
            os.makedirs(args.dump_outputs, exist_ok=True)
            for name in recs.dtype.names:
                a = recs[name]
                np.save(os.path.join(args.dump_outputs, f"{name}.npy"), a.astype(np.float32 if a.dtype == np.float32 else np.float64))
        nn_mode = os.environ.get("APDGICP_NN_MODE", "pruned")
        # ---- roofline of the dominant kernel, the nearest-neighbour search: ALGORITHMIC HBM bytes per launch = per pair
        # 16(N+M) (both sorted clouds) + 16N (warm-start hints) + 8N (result), SURVEY 8d / DESIGN 3, over the kernel's own
        # begin/end timestamps (hipExtLaunchKernelGGL events on the launching stream, sampled launches of the timed region)
        avg_nn_ms = nn_ms / max(1, nn_launches)
        pairs_per_launch = nn_pairs / max(1, nn_launches)
        nn_kernel = batch.last_nn_kernel()
        keeps = nn_kernel.startswith("k_nn_compact") or os.environ.get("APDGICP_NN_SKIN", "1") != "0"
        # ALGORITHMIC bytes per pair and launch, SURVEY 8d: the search's share of B_lin = both sorted clouds 16(N+M) + the result 8N
        # = 40N for N = M; a whole tick (search + linearize) B_lin = 124N.  What the implementation moves on top of that -- the
        # warm-start hints (16N) and the neighbour-keeping records (16N) -- is traffic, not algorithm: it shows in `traffic`.
        bytes_per_pair = 16.0 * (n + n) + 8.0 * n
        bytes_per_launch = bytes_per_pair * pairs_per_launch
        nn_gbs = bytes_per_launch / (avg_nn_ms * 1e-3) / 1e9 if avg_nn_ms > 0 else 0.0
        # whole-registration algorithmic bytes, SURVEY 8d: B_reg = 40(N+M) + L(108N + 16M) (+ 56N per compute_error, LM)
        n_lin = float(recs["n_linearize"].mean())
        n_err = float(recs["n_compute_error"].mean())
        b_reg = 40.0 * (2 * n) + n_lin * (108.0 * n + 16.0 * n) + n_err * 56.0 * n
        hbm_gbs = b_reg * P / (ms_per_step * 1e-3) / 1e9
        traffic, issue = None, None
        pmc, pmc_rejected = load_pmc(os.path.join(ROOT, "profiles", "pmc_lm_loop.json") if lm else None)
        if lm and pmc and pmc.get("points") == n and pmc.get("kind") == args.kind and pmc.get("kernel", "").replace(" ", "") == batch.last_nn_kernel().replace(" ", ""):
            # pooled LM ticks: launches differ in size, the committed counters are per listed pair slot (tools/pmc_lm_json.py)
            ps = pmc["per_slot"][pmc["kernel"]]
            if pmc.get("hbm_bytes_per_slot"):
                traffic = int(round(pmc["hbm_bytes_per_slot"] * pairs_per_launch))
            if ps.get("SQ_INSTS_VALU") and avg_nn_ms > 0:
                valu_rate = ps["SQ_INSTS_VALU"] * pairs_per_launch / (avg_nn_ms * 1e-3)
                issue = {"bound": "valu-issue", "achieved": round(valu_rate / 1e9, 2), "peak": round(VALU_WAVE_INSTR_PEAK / 1e9, 2),
                         "unit": "G wave-instructions/s", "frac": round(valu_rate / VALU_WAVE_INSTR_PEAK, 4),
                         "peak_theoretical": round(VALU_WAVE_INSTR_THEORETICAL / 1e9, 1), "frac_of_theoretical": round(valu_rate / VALU_WAVE_INSTR_THEORETICAL, 4),
                         "valu_instructions_per_pair": ps["SQ_INSTS_VALU"], "source": pmc.get("source"),
                         "note": "VALU wave-instructions per listed pair (PMC, committed profile of the same workload) x pairs per timed launch / the launch time"}
        # PMC numbers come from a separate committed profiling run (rocprofv3 --pmc passes cannot run inside this process):
        # reported only when that run had this launch shape, and tagged with where they come from
        step_issue = None
        if lm and pmc and issue and slot_ticks_per_step and P == 32 and n == N_PTS:
            # the pooled LM batch against the vector issue slots: per listed pair slot the tick kernels' SQ_ACTIVE_INST_VALU (pmc_lm_loop.json) x the
            # slots the pool's tick launches covered per batch (apdgicp_batch_pool_counters, THIS run) + the batch's cloud kernels -- pack, sort,
            # merge, boxes, covariance k-NN, regularisation over 64 clouds of 8192 points: the launch shapes of pmc_nn_latest.json's step_kernels
            cloud_pmc, _why = load_pmc(None)
            tick_busy = sum(cs.get("SQ_ACTIVE_INST_VALU", 0.0) for cs in pmc["per_slot"].values()) * slot_ticks_per_step
            tick_insts = sum(cs.get("SQ_INSTS_VALU", 0.0) for cs in pmc["per_slot"].values()) * slot_ticks_per_step
            cloud_busy = cloud_insts = 0.0
            for name, cs in ((cloud_pmc or {}).get("step_kernels") or {}).items():
                if "k_nn_" in name or "k_linearize" in name:
                    continue
                cloud_busy += cs.get("SQ_ACTIVE_INST_VALU", 0.0)
                cloud_insts += cs.get("SQ_INSTS_VALU", 0.0)
            if cloud_busy > 0:
                busy = (tick_busy + cloud_busy) * 4.0 / (SIMDS * GFX_CLOCK_HZ * ms_per_step * 1e-3)
                step_issue = {"bound": "valu-issue", "valu_busy": round(busy, 3), "slot_ticks_per_batch": round(slot_ticks_per_step, 1),
                              "valu_instructions_per_batch": {"ticks": tick_insts, "clouds": cloud_insts},
                              "busy_quad_cycles_per_batch": {"ticks": tick_busy, "clouds": cloud_busy},
                              "sources": [pmc.get("source"), (cloud_pmc or {}).get("source", "profiles/pmc_nn_latest.json")],
                              "valu_busy_note": "sum of SQ_ACTIVE_INST_VALU (quad-cycles) over a batch's launches x 4 / (1024 SIMDs x 2.4 GHz x ms per batch): tick kernels per "
                                                "listed pair slot (committed profile of this workload) x the slots this run's tick launches covered, plus the cloud kernels "
                                                "of 64 clouds (committed profile of the same launch shapes, odometry clouds: the covariance work does not depend on the pose)"}
        if not lm and pmc and pmc.get("points") == n and pmc.get("pairs_per_launch") == round(pairs_per_launch) and pmc.get("nn_mode", "pruned") == nn_mode \
                and pmc.get("kind", "odometry") == args.kind and pmc.get("kernel", "").replace(" ", "") == nn_kernel.replace(" ", ""):
            traffic = pmc.get("hbm_bytes_per_launch")
            if pmc.get("SQ_INSTS_VALU"):
                valu_rate = pmc["SQ_INSTS_VALU"] / (avg_nn_ms * 1e-3)
                issue = {"bound": "valu-issue", "achieved": round(valu_rate / 1e9, 2), "peak": round(VALU_WAVE_INSTR_PEAK / 1e9, 2),
                         "unit": "G wave-instructions/s", "frac": round(valu_rate / VALU_WAVE_INSTR_PEAK, 4),
                         "peak_theoretical": round(VALU_WAVE_INSTR_THEORETICAL / 1e9, 1), "frac_of_theoretical": round(valu_rate / VALU_WAVE_INSTR_THEORETICAL, 4),
                         "valu_instructions_per_launch": pmc["SQ_INSTS_VALU"], "source": pmc.get("source", "profiles/pmc_nn_latest.json"),
                         "note": "VALU wave-instructions per launch (PMC, committed profile of the same launch shape) / this run's launch "
                                 "time, against the measured plain-fp32 issue ceiling (62 Tlane-op/s / 64)"}
            # the whole step against the same roof: VALU instructions of every batch kernel x its launches per step / ms_per_step
            sk = pmc.get("step_kernels") or {}
            per_step, busy_units = 0.0, 0.0
            for name, cs in sk.items():
                launches = GN_ITERS if ("k_nn_" in name or "k_linearize" in name) else 1
                per_step += cs.get("SQ_INSTS_VALU", 0.0) * launches
                busy_units += cs.get("SQ_ACTIVE_INST_VALU", 0.0) * launches
            if per_step > 0 and P == 32:
                rate = per_step / (ms_per_step * 1e-3)
                step_issue = {"bound": "valu-issue", "achieved": round(rate / 1e9, 1), "peak": round(VALU_WAVE_INSTR_PEAK / 1e9, 2),
                              "unit": "G wave-instructions/s", "frac": round(rate / VALU_WAVE_INSTR_PEAK, 4),
                              "peak_theoretical": round(VALU_WAVE_INSTR_THEORETICAL / 1e9, 1), "frac_of_theoretical": round(rate / VALU_WAVE_INSTR_THEORETICAL, 4),
                              "valu_instructions_per_step": per_step, "source": pmc.get("source"),
                              "note": "sum over the step's batch kernels (search and linearize x 20 ticks, covariances, sort, pack) of their PMC "
                                      "VALU instruction counts / ms_per_step; `peak` is the ceiling of the FAST instruction class only (plain fp32 "
                                      "add / mul / fma, integer add / logic / mov: 2.5 cycles per wave-instruction on a SIMD); everything else -- "
                                      "min / max, compares, selects, shifts, DPP, readlane, packed fp32, all fp64 -- holds the SIMD for 4.3 "
                                      "(tools/ubench_issue.hip, profiles/r05_ubench_issue.txt): see valu_busy"}
                if busy_units > 0:
                    # the profiler's own VALUBusy formula (SQ_ACTIVE_INST_VALU x 4 / SIMDs / gfx cycles) over the step: the counter advances by one
                    # quad-cycle per vector instruction of either class, so this is an UPPER estimate by the share of fast-class instructions
                    busy = busy_units * 4.0 / (SIMDS * GFX_CLOCK_HZ * ms_per_step * 1e-3)
                    step_issue["valu_busy"] = round(busy, 3)
                    step_issue["valu_busy_note"] = ("sum of SQ_ACTIVE_INST_VALU (quad-cycles) over the step's launches x 4 / (1024 SIMDs x 2.4 GHz x ms_per_step): "
                                                    "the share of the step during which a SIMD's vector issue slot is held -- what binds the step; an upper "
                                                    "estimate (fast-class instructions are counted at 4 cycles, they take 2.5)")
        out = {
            "metric": ("APD-GICP registrations/s (8k-pt scan pairs, GN-20, covariances recomputed)" if not lm else
                       "APD-GICP registrations/s (8k-pt pairs, Levenberg-Marquardt with the launch parameters, covariances recomputed)"),
            "value": round(value, 2), "unit": "registrations/s", "n_gpus": world, "steps": K, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ("f32 nearest-neighbour search + f64 covariance/Mahalanobis/Hessian" if not args.fp32_point_math else
                      "f32 nearest-neighbour search + f32 per-point Mahalanobis/Jacobian terms (APDGICP_FLAG_FP32_POINT_MATH, opt-in: NOT the reference's precision) + f64 covariances/sums/solve"),
            "data": "synthetic",
            "inputs": ("HOST clouds every step (numpy, pageable; packed into pinned memory by the library, read over PCIe): the PCIe-inclusive rate, NOT the headline"
                       if args.host_clouds else "resident in HBM before the timed region"),
            "config": {"workload": (f"BASELINE configs[1] (8k x 8k scan pair, 20 GN iterations) x {P} independent pairs per GPU per step "
                                    f"(= per-GPU shard of configs[3]); pair kind '{args.kind}'" if not lm else
                                    f"BASELINE configs[3], per-GPU shard as SURVEY 8d specifies it: {P} pairs per GPU per step, kind '{args.kind}'"
                                    f"{' from the identity (loop_detector.cpp:225)' if args.kind == 'loop' else ''}, LM with the launch parameters"),
                       "points": n, "pairs_per_gpu": P, "optimizer": args.optimizer,
                       "gn_iterations": GN_ITERS if not lm else None,
                       "linearizations_per_pair": {"mean": round(n_lin, 2), "min": int(recs["n_linearize"].min()), "max": int(recs["n_linearize"].max())},
                       "kind": args.kind, "nn_mode": nn_mode, "nn_sources_per_lane": nn_S, "nn_target_splits": nn_T,
                       "ticks": ticks, "steps_in_flight": S, "batch_handles": len(batches)},
            "world_size": dist.get_world_size() if use_dist else 1, "rccl_version": rccl_version,
            "dist_backend": (args.dist_backend if use_dist else None), "ranks_share_gpu": bool(args.ranks_share_gpu),
            "timing": {"repeats": R, "steps_per_repeat": K, "statistic": "median over repeats (each: K steps, barrier + sync both sides, max over ranks)",
                       "host_ms_per_step": percentiles([t / K * 1e3 for t in host_s]),
                       "event_ms_per_step": percentiles([t / K for t in event_ms]),
                       "first_repeat_ms_per_step": round(host_s[0] / K * 1e3, 4),
                       "step_latency_ms": percentiles([t * 1e3 for t in lat]),
                       "step_latency_note": f"submit -> collect of one step (host clock): {H} steps are in flight, so a step's kernels may take up to "
                                            "this long although a step LEAVES every ms_per_step",
                       "registrations_per_s": {"p10": round(total_pairs * K / float(np.percentile(host_s, 90)), 1),
                                               "p90": round(total_pairs * K / float(np.percentile(host_s, 10)), 1)}},
            "ms_per_gn_iter_batched": round(ms_per_step / GN_ITERS, 4) if not lm else None,
            "multi_rank": ({"ranks": world, "ms_per_step_per_rank": per_rank, "ms_per_step_min": min(per_rank), "ms_per_step_max": max(per_rank),
                            "imbalance": round(max(per_rank) / min(per_rank) - 1.0, 4),
                            "gather_ms": (percentiles(gather_ms) if gather_ms else None),
                            "gather_note": ("one all_gather_into_tensor of the 96-byte records per step (RCCL): HIP events around the collective on the stream that carries it"
                                            if not gloo else "gloo self-test: host time inside the gather call (CPU tensors)"),
                            "weak_scaling_efficiency": scaling_efficiency(value, world, args, lm),
                            "note": "value = all ranks' pairs / the slowest rank's time (MAX over ranks per repetition); per-rank figures are each rank's own median"}
                           if use_dist else None),
            "roofline": {"kernel": nn_kernel + (" (exact fp32 nearest neighbour: Hilbert-sorted clouds, bounding-box pruning, LDS-staged target "
                                                "groups, neighbours kept while provably unchanged)" if nn_mode != "brute" else
                                                " (brute-force fp32 nearest neighbour, LDS-tiled)"),
                         "bound": "hbm", "bound_note": "the roof the contract asks the line to be priced against; the roof that BINDS this kernel and the step is vector "
                                                       "instruction issue -- binding_roof, roofline_issue, roofline_issue_step.valu_busy",
                         "achieved": round(nn_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(nn_gbs / HBM_PEAK_GBS, 4), "traffic": traffic,
                         "traffic_over_algorithmic": (round(traffic / bytes_per_launch, 3) if traffic and bytes_per_launch else None),
                         "binding_roof": "instruction issue (vector + scalar), not HBM: see roofline_issue; the HBM fraction is the north star's extra",
                         "kernel_ms_per_step": round(avg_nn_ms * (ticks if not lm else n_lin), 4),
                         "concurrency_note": "kernel_ms_per_step (average launch x launches per step) is NOT additive against ms_per_step: the launches of one step overlap "
                                             "with those of the other steps in flight (it is bounded by timing.step_latency_ms, not by ms_per_step); a statement, not a check",
                         # non-overlapped accounting: H steps are in flight, each on a stream of its own, and a step stays H x ms_per_step on
                         # its stream; the search kernel's share of ALL stream time = sum of its launch times / (wall x busy streams) <= 1
                         "concurrency": {"steps_in_flight": H if not lm else None, "busy_streams": (H if not lm else 2),
                                         "kernel_time_over_wall_x_streams": round(avg_nn_ms * (ticks if not lm else n_lin) / (ms_per_step * (H if not lm else 2)), 4)
                                         if not lm else None,
                                         "note": "sum of this kernel's launch durations per step / (ms_per_step x streams in flight): the share of the busy streams' time "
                                                 "the dominant kernel holds (<= 1); durations are those of launches that share the GPU with the other steps' kernels, "
                                                 "so they are not additive against ms_per_step"},
                         "traffic_source": (pmc.get("source", "profiles/pmc_nn_latest.json") if traffic else None),
                         "avg_launch_ms": round(avg_nn_ms, 5), "launches_timed": nn_launches, "pairs_per_launch": round(pairs_per_launch, 2),
                         "algorithmic_bytes_per_launch": bytes_per_launch,
                         "note": "achieved = SURVEY 8d's algorithmic bytes per launch (16(N+M) + 8N = 40N per pair) / the kernel's average duration in "
                                 "the timed region (HIP events on the launching stream).  The working set is MALL/L2 resident and the kernel "
                                 "is issue/latency bound, so the HBM fraction is small by construction; roofline_issue is the roof that binds.  "
                                 "`traffic` (PMC, committed profile of the same sources) also carries the warm-start hints and neighbour-keeping records: see traffic_over_algorithmic"},
            "roofline_issue": issue,
            "roofline_issue_step": step_issue,
            "library_source_stamp": importlib.import_module("riv-slam_amd.registration").source_stamp(),
            "library_build_flags": importlib.import_module("riv-slam_amd.registration").build_flags(),
            "pmc_profile": ({"source_stamp": pmc.get("source_stamp"), "file": "profiles/pmc_lm_loop.json" if lm else "profiles/pmc_nn_latest.json"} if pmc else {"rejected": pmc_rejected}),
            "roofline_step_hbm": {"bound": "hbm", "achieved": round(hbm_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": round(hbm_gbs / HBM_PEAK_GBS, 5), "algorithmic_bytes_per_registration": b_reg,
                                  "note": "whole step: B_reg x pairs / ms_per_step; B_reg = 40(N+M) + L(108N+16M) + E 56N with the run's mean L, E"},
        }

        if world == 1 and args.full and not args.no_diagnostics and not lm:
            # ---- outside the timed region: what the pruned kernel really executes, and the brute-force kernel on the same data
            def one_step(env):
                old = {k_: os.environ.get(k_) for k_ in env}
                os.environ.update(env)
                try:
                    bb = reg.BatchAPDGICP(params, device=local_rank)
                finally:
                    for k_, v_ in old.items():
                        if v_ is None:
                            os.environ.pop(k_, None)
                        else:
                            os.environ[k_] = v_
                bb.set_profiling(True)
                if H > 1:
                    bb.set_pair_groups(1)      # the timed handles' regime: ONE launch over all the pairs of the step (k_nn_compact; the brute-force leg:
                                               # k_nn_partial over 32 pairs -- with three pair groups it launched 10 - 11 pairs = 176 blocks on 256 CUs)
                for _ in range(2):
                    bb.set_clouds(0, d_clouds)
                    bb.align_async(pairs_arr)
                    bb.synchronize()
                return bb
            flops_alg = 8.0 * n * n * pairs_per_launch      # what a brute-force search of the same launch evaluates
            if nn_mode != "brute":
                bs = one_step({"APDGICP_STATS": "1"})
                st = bs.debug_stats()
                waves_per_launch = (n / 64.0) * pairs_per_launch
                chunks_scanned = float(st[2]) / max(1.0, float(st[3])) * waves_per_launch   # 16-target chunk scans per launch
                executed = chunks_scanned * 16 * 64 * 8.0          # x 64 lanes (queries) x 8 flop
                out["nn_work"] = {"executed_distance_flops_per_launch": executed, "bruteforce_flops_per_launch": flops_alg,
                                  "executed_share_of_bruteforce": round(executed / flops_alg, 5),
                                  "points_that_kept_their_neighbour_share": round(float(st[6]) / max(1.0, float(st[3]) * 64.0), 4),
                                  "executed_TFLOPs": round(executed / (avg_nn_ms * 1e-3) / 1e12, 2),
                                  "bruteforce_equivalent_TFLOPs": round(flops_alg / (avg_nn_ms * 1e-3) / 1e12, 1),
                                  "note": "the pruned search returns the brute-force result bit for bit; bruteforce_equivalent is NOT a hardware "
                                          "rate (it counts pairs that were proven irrelevant, not evaluated)"}
                del bs
            bf = one_step({"APDGICP_NN_MODE": "brute", "APDGICP_KNN_MODE": "brute", "APDGICP_PROFILE_STRIDE": "1"})
            ms_b, k_b, pr_b = bf.last_nn_profile()
            tf_b = 8.0 * n * n * pr_b / max(1e-9, ms_b * 1e-3) / 1e12
            _, sb, tb = bf.last_ticks()
            out["roofline_bruteforce"] = {"kernel": f"k_nn_partial<{sb}> (every pair evaluated, LDS-tiled, T={tb} target splits)", "bound": "valu-fp32",
                                          "achieved": round(tf_b, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                                          "frac": round(tf_b / FP32_PEAK_TFLOPS, 4), "avg_launch_ms": round(ms_b / max(1, k_b), 4),
                                          "pairs_per_launch": round(pr_b / max(1, k_b), 2), "launches_timed": int(k_b),
                                          "note": "same results bit for bit; exact non-fused arithmetic (no FMA) caps this formulation at "
                                                  "~0.4 of the FMA-based spec peak (profiles/r01_ubench_valu.txt)"}
            del bf

        if world == 1 and args.full:
            # ---- single-pair latency (configs[1] exactly): one handle, one registration at a time
            s, t, g = h_pairs[0]
            one = reg.FastAPDGICP(params, device=local_rank)
            ds, dt = d_clouds[0], d_clouds[1]

            def timed(fn, reps=20):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                ts = []
                for _ in range(reps):
                    t1 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t1) * 1e3)
                return ts
            single = timed(lambda: (one.setInputSource(ds), one.setInputTarget(dt), one.align(g)))
            # ms per GN iteration (BASELINE metric, second component): the same registration with both clouds' covariances
            # cached (pointer-equality tokens), i.e. 20 x (search + Mahalanobis + H/b + step) on device-resident data
            cached = timed(lambda: (one.setInputSource(ds, token=11), one.setInputTarget(dt, token=12), one.align(g)))
            out["single_pair"] = {"ms_per_registration": percentiles(single), "registrations_per_s": round(1e3 / float(np.median(single)), 1),
                                  "ms_per_gn_iteration": round(float(np.median(cached)) / GN_ITERS, 4) if not lm else None}

            if not lm and not args.no_diagnostics:
                # ---- second object: SURVEY 8d's C4 shard -- 32 loop-closure candidates at 8192 points, aligned
                # from the identity (loop_detector.cpp:225) by Levenberg-Marquardt with the launch parameters, both clouds fresh every
                # batch -- on ONE handle and ONE host thread, 24 batches in flight in the handle's pair pool (two pair lists on two streams)
                # The handles of the legs above are closed first: the HIP runtime deals a process's streams onto its hardware queues
                # (GPU_MAX_HW_QUEUES = 8) in creation order, and with the four batch handles and the single-registration handle still
                # alive two of the four streams this pooled handle ticks on shared a queue (round 5: 1.02 instead of 0.90 ms per batch
                # when an earlier leg happened to create two streams fewer).  A closed handle's stream is gone; nothing below uses them.
                for bh_ in batches:
                    bh_.close()
                one.close()
                torch.cuda.synchronize()
                # (a timed repetition fills the empty pool, runs, and drains it: at 40 batches -- rounds 4 and 5 -- 24 of them were fill or
                # drain, 0.88 ms per batch; 240 leave 10 % of them there)
                F4, P4, LM_STEPS = 24, 32, 240
                lm_clouds, lm_host = [], []
                for p_ in range(P4):
                    s_, t_, _, _ = scene.make_pair(n, n, scene.pair_seed(4, p_), "loop")
                    lm_host.append((s_, t_))
                    lm_clouds += [torch.from_numpy(s_).cuda(), torch.from_numpy(t_).cuda()]
                torch.cuda.synchronize()
                bl = reg.BatchAPDGICP(reg.default_params(**LM_LAUNCH), device=local_rank)
                lm_packed = bl.pack_clouds(lm_clouds)
                eye = [np.eye(4, dtype=np.float32)] * P4
                lm_pairs = [bl.make_pairs([(2 * P4 * f + 2 * i, 2 * P4 * f + 2 * i + 1) for i in range(P4)], eye) for f in range(F4)]

                def lm_steps(count):
                    tk, res_ = [None] * F4, None
                    for s_i in range(count):
                        f = s_i % F4
                        if tk[f] is not None:
                            res_ = bl.align_collect(tk[f])
                        bl.set_clouds(2 * P4 * f, lm_packed, producer_wait=False)
                        tk[f] = bl.align_enqueue(lm_pairs[f])
                    for s_i in range(count, count + F4):
                        if tk[s_i % F4] is not None:
                            res_ = bl.align_collect(tk[s_i % F4])
                            tk[s_i % F4] = None
                    return res_
                lm_steps(2 * F4)
                lm_ms = []
                for _ in range(5):
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    lm_recs = lm_steps(LM_STEPS)
                    bl.synchronize()
                    lm_ms.append((time.perf_counter() - t1) / LM_STEPS * 1e3)
                lm_med = float(np.median(lm_ms))
                its = [int(x) for x in lm_recs["n_linearize"]]
                out["lm_loop_batch"] = {"metric": "ms per batch of 32 loop-closure registrations (8k x 8k, identity guess, LM with the launch parameters, covariances recomputed)",
                                        "value": round(lm_med, 4), "unit": "ms per batch", "higher_is_better": False,
                                        "registrations_per_s": round(P4 * 1e3 / lm_med, 1), "ms_per_batch": percentiles(lm_ms),
                                        "handles": 1, "host_threads": 1, "batches_in_flight": F4, "batches_per_timed_repetition": LM_STEPS,
                                        "linearizations_per_pair": {"min": min(its), "median": float(np.median(its)), "max": max(its), "sum": sum(its)},
                                        "compute_error_evaluations": int(lm_recs["n_compute_error"].sum()), "converged": int(lm_recs["converged"].sum()),
                                        "note": "pooled Levenberg-Marquardt batches (include/apdgicp_hip.h): every tick is one launch over the pairs of all batches "
                                                "in flight that still run; round 2's host-polled loop: 5.2 ms per batch on one handle"}
                del bl

                # ---- third object: BASELINE configs[4] as SURVEY 8d states it -- ONE dense pair, 100k-point source against a 500k-point
                # accumulated map (the scan-to-submap target of scan_matching_odometry_nodelet.cpp:606-618), GN-20, one GPU
                N5, M5 = 100_000, 500_000
                s5, t5, _, g5 = scene.make_pair(N5, M5, scene.pair_seed(5, 0), "odometry")
                d5 = [torch.from_numpy(s5).cuda(), torch.from_numpy(t5).cuda()]
                def c5_handle(stats):
                    old_stats = os.environ.get("APDGICP_STATS")
                    if stats:
                        os.environ["APDGICP_STATS"] = "1"
                    try:
                        return reg.BatchAPDGICP(params, device=local_rank)
                    finally:
                        if stats and old_stats is None:
                            os.environ.pop("APDGICP_STATS", None)
                        elif stats:
                            os.environ["APDGICP_STATS"] = old_stats
                b5 = c5_handle(False)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                b5.set_clouds(0, d5)
                r5 = b5.align([(0, 1)], [g5])
                first5 = (time.perf_counter() - t1) * 1e3        # pack + sort + both clouds' covariances + 20 iterations
                c5_ms = timed(lambda: b5.align([(0, 1)], [g5]), 10)   # covariances cached: 20 x (search + Mahalanobis + H/b + step)
                c5_med = float(np.median(c5_ms))
                nn5 = b5.last_nn_kernel()
                del b5
                b5 = c5_handle(True)                             # a second handle with the diagnostics counters on (they slow the kernels down)
                b5.set_clouds(0, d5)
                b5.align([(0, 1)], [g5])
                b5.debug_stats()                                 # (reading resets the counters)
                b5.align([(0, 1)], [g5])
                st5 = b5.debug_stats()
                del b5
                b_lin5, f_lin5 = 108.0 * N5 + 16.0 * M5, 8.0 * N5 * M5          # per linearize
                b_reg5 = 40.0 * (N5 + M5) + GN_ITERS * b_lin5                    # = 400 MB
                f_reg5 = 8.0 * (float(N5) ** 2 + float(M5) ** 2) + GN_ITERS * f_lin5
                executed5 = float(st5[2]) * 16 * 64 * 8.0 / GN_ITERS             # distance flops per iteration: scanned 16-target chunks x 64 lanes x 8
                out["c5_dense"] = {
                    "workload": "BASELINE configs[4]: 100k-pt source x 500k-pt accumulated map, GN-20, 1 GPU (one pair: no batch to hide latency behind)",
                    "ms_per_gn_iteration": round(c5_med / GN_ITERS, 4), "ms_per_registration_covariances_cached": percentiles(c5_ms),
                    "ms_first_registration_incl_sort_and_covariances": round(first5, 2), "n_linearize": int(r5["n_linearize"][0]),
                    "kernel": nn5,
                    **c5_pmc_fields(load_pmc),
                    "hbm_fraction": round(GN_ITERS * b_lin5 / (c5_med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                    "hbm_fraction_first_registration": round(b_reg5 / (first5 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                    "valu_fraction_bruteforce_equivalent": round(GN_ITERS * f_lin5 / (c5_med * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 2),
                    "valu_fraction_executed": round(GN_ITERS * executed5 / (c5_med * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 4),
                    "executed_share_of_bruteforce": round(executed5 / f_lin5, 6),
                    "algorithmic": {"B_lin_bytes": b_lin5, "B_reg_bytes": b_reg5, "F_lin_flops": f_lin5, "F_reg_flops": f_reg5},
                    "note": "SURVEY 8d: B_reg = 40(N+M) + L(108N+16M) = 400 MB, F_reg = 8(N^2+M^2) + L 8NM = 1.0e13 for L = 20.  hbm_fraction = "
                            "L B_lin / t / 8 TB/s over the cached-covariance registration; valu_fraction_bruteforce_equivalent = L F_lin / t / 157.3 TF "
                            "is NOT a hardware rate (> 1: the pruned search proves most pairs irrelevant instead of evaluating them, and returns "
                            "the brute-force result bit for bit); valu_fraction_executed counts the distance evaluations really issued"}
                del d5

            if not args.no_cpu_baseline:
                # ---- CPU baseline: the oracle's OpenMP restatement ("port") on the same pairs, bounded sample, thread sweep.
                # Same work per registration as the GPU step: both clouds set fresh (kd-trees and covariances rebuilt), GN-20.
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import ref as R_
                kw = (dict(optimizer=1, max_iterations=GN_ITERS, transformation_epsilon=1e-300, rotation_epsilon=1e-300,
                           max_correspondence_distance=2.0, azimuth_variance_deg=1.0) if not lm else dict(LM_LAUNCH))
                ncores = os.cpu_count() or 1
                sweep_threads = sorted({c for c in (8, 16, 32, 64, ncores) if c <= ncores})
                share = args.cpu_seconds / (len(sweep_threads) + 3)
                worst_t, worst_r, checked, cursor = 0.0, 0.0, 0, 0
                sweep = {}

                def run_cfg(threads, budget, cap=True):   # cap: at most one pass over the P pairs (the sweep); the repeats run for their whole share
                    nonlocal worst_t, worst_r, checked, cursor
                    o = R_.RefAPDGICP(R_.default_params(**kw), num_threads=threads)
                    s0, t0_, g0 = h_pairs[0]
                    o.setInputSource(s0), o.setInputTarget(t0_), o.align(g0)      # untimed: thread pool start-up, page faults
                    done, tc = 0, time.perf_counter()
                    while done < 2 or (time.perf_counter() - tc) < budget:
                        i = cursor % P
                        s_, t_, g_ = h_pairs[i]
                        o.setInputSource(s_), o.setInputTarget(t_)
                        To = o.align(g_)
                        te, re_ = scene.pose_error(To, reg.result_matrix(recs[i]))
                        worst_t, worst_r, checked = max(worst_t, te), max(worst_r, re_), checked + 1
                        cursor += 1
                        done += 1
                        if cap and done >= P:
                            break
                    return done / (time.perf_counter() - tc), done, o.num_threads
                for th in sweep_threads:
                    rate, done, used = run_cfg(th, share)
                    sweep[str(used)] = {"registrations_per_s": round(rate, 3), "pairs": done}
                best_threads = max(sweep, key=lambda k_: sweep[k_]["registrations_per_s"])
                reps_cpu = [run_cfg(int(best_threads), share, cap=False) for _ in range(3)]     # three repeats at the best thread count: median + spread
                rates = sorted(r_[0] for r_ in reps_cpu)
                rate, done, used = rates[1], sum(r_[1] for r_ in reps_cpu), reps_cpu[0][2]
                try:   # the flags the checker was built with (oracle/Makefile: -O3 like the reference's Release build, no contraction)
                    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
                    cxxflags = next(l.split("?=", 1)[1].strip() for l in mk.splitlines() if l.startswith("CXXFLAGS"))
                except Exception:  # noqa: BLE001
                    cxxflags = None
                out["cpu_baseline"] = {"value": round(rate, 3), "unit": "registrations/s", "cores": used, "kind": "port", "build_flags": cxxflags,
                                       "repeats": {"n": 3, "statistic": "median", "min": round(rates[0], 3), "max": round(rates[2], 3),
                                                   "spread_rel": round((rates[2] - rates[0]) / rates[1], 3)},
                                       "sample": f"{done} registrations over the {P} timed pairs in three repeats of {share:.1f} s at the best thread count of the sweep (same clouds, "
                                                 f"both clouds set fresh, {'GN-20' if not lm else 'LM with the launch parameters'}; kd-tree + OpenMP restatement "
                                                 f"of the reference, not the reference binary)",
                                       "thread_sweep": sweep, "all_cores": {"cores": ncores, **sweep.get(str(ncores), {})},
                                       "openmp": {"OMP_PROC_BIND": os.environ.get("OMP_PROC_BIND"), "OMP_WAIT_POLICY": os.environ.get("OMP_WAIT_POLICY"),
                                                  "schedule": "guided,8"}}
                out["vs_cpu_baseline"] = round(value / rate, 1)
                out["parity"] = {"pairs_checked": checked, "max_t_err_m": worst_t, "max_r_err_rad": worst_r, "tolerance": "1e-3 m / 1e-4 rad",
                                 "oracle": "parity unpinned (restatement; the reference cannot be built in this image)"}
                assert worst_t <= 1e-3 and worst_r <= 1e-4, (worst_t, worst_r)
        if args.dump_records:
            np.save(args.dump_records, gathered.detach().cpu().numpy())
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
