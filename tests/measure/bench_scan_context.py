"""Times the device Scan Context database (riv-slam_amd/scan_context.py) beside a plain single-thread C++ restatement of the same rules
(tests/measure/scan_context_ref.cpp, g++ -O3 -ffp-contract=off, built by this script).  Cases: the descriptor of one device-resident cloud of
8192 points; detect over 256, 4096 and 32 768 candidates with the reference's knobs (num_candidates 3, search_ratio 0.1) and with the
exhaustive ones (0, 1.0); detect_batch of 8 queries over 4096 candidates each.  The database holds 32 800 descriptors of 40 "places" seen
with noise (tests/scan_context_np.py: database_descriptors); the query is the newest one.  Protocol: 10 warm-up calls, then 30 timed calls
per case (wall clock around a call that ends with the host holding the records), median with p10 / p90, the device otherwise idle; the
CPU baseline the same way on the same inputs (3 calls where one takes more than 0.2 s), and its records are compared with the device's
byte for byte.
usage: python tests/measure/bench_scan_context.py [out.json] [--runs R]"""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)
from bench_scan_filter import timed  # noqa: E402

KNOBS = {"reference": dict(num_candidates=3, search_ratio=0.1), "exhaustive": dict(num_candidates=0, search_ratio=1.0)}


def build_ref():
    src, out = os.path.join(HERE, "scan_context_ref.cpp"), os.path.join(HERE, "_build", "libscan_context_ref.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), src, "-o", out])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.sc_ref_build.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int64, vp, vp, vp, vp]
    L.sc_ref_build.restype = None
    L.sc_ref_detect.argtypes = [vp, vp, vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.sc_ref_detect.restype = C.c_int
    return L


def main():
    import __graft_entry__ as g
    g.build()
    import torch
    from scan_context_np import database_descriptors, fov_cloud
    reg = importlib.import_module("riv-slam_amd.registration")
    scm = importlib.import_module("riv-slam_amd.scan_context")
    args = sys.argv[1:]
    runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 30
    ref = build_ref()
    ptr = reg._ptr
    out = {"library_stamp": reg.source_stamp(), "build_flags": reg.build_flags(), "device": torch.cuda.get_device_name(0), "protocol": __doc__.split("usage")[0].strip(),
           "cases": []}
    rng = np.random.default_rng(1)
    sc = scm.ScanContext()
    # ---- descriptor build, 8192 points, device-resident
    cloud = fov_cloud(rng, 8192)
    dev = torch.from_numpy(cloud).cuda()
    torch.cuda.synchronize()

    def build_once():
        sc.clear()
        return sc.add(dev)
    case = {"case": "build_8192_device_resident", "device": timed(build_once, runs=runs, warm=10)}
    R, S = 40, 20
    d, rk, sk, cn = np.zeros((R, S), np.float32), np.zeros(R, np.float32), np.zeros(S), np.zeros(S)
    case["cpu_single_thread"] = timed(lambda: ref.sc_ref_build(C.byref(sc.params), ptr(cloud), len(cloud), 4, 3, ptr(d), ptr(rk), ptr(sk), ptr(cn)), runs=runs, warm=3)
    got = sc.descriptors(0, 1)
    case["equal"] = bool(got["desc"][0].tobytes() == d.tobytes() and got["ring_key"][0].tobytes() == rk.tobytes() and got["col_norm"][0].tobytes() == cn.tobytes())
    print(json.dumps(case), flush=True)
    out["cases"].append(case)
    # ---- the database
    sc.clear()
    N = 32800
    descs = database_descriptors(rng, N)
    for x in descs:
        sc.add_descriptor(x)
    db = sc.descriptors()
    q = N - 1
    order = rng.permutation(N - 20).astype(np.int32)
    for name, knobs in KNOBS.items():
        sc.set_params(**knobs)
        for n in (256, 4096, 32768):
            cand = np.ascontiguousarray(order[:n])
            case = {"case": f"detect_{name}_{n}", "device": timed(lambda: sc.detect(q, cand, 4), runs=runs, warm=10)}
            rec, loop, yaw = np.zeros(4, dtype=scm.MATCH_DTYPE), C.c_int32(), C.c_float()

            def cpu():
                return ref.sc_ref_detect(C.byref(sc.params), ptr(db["desc"]), ptr(db["ring_key"]), ptr(db["sector_key"]), ptr(db["col_norm"]), q, ptr(cand), n, 4,
                                         ptr(rec), C.byref(loop), C.byref(yaw))
            slow = name == "exhaustive" and n > 4096
            case["cpu_single_thread"] = timed(cpu, runs=3 if slow else runs, warm=1 if slow else 3)
            det = sc.detect(q, cand, 4)
            case["equal"] = bool(det.matches.tobytes() == rec[:len(det.matches)].tobytes() and det.loop_id == loop.value)
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
        queries = [N - 1 - 3 * i for i in range(8)]
        lists = [np.ascontiguousarray(rng.permutation(N - 100)[:4096].astype(np.int32)) for _ in queries]
        case = {"case": f"detect_batch_{name}_8x4096", "device": timed(lambda: sc.detect_batch(queries, lists, 4), runs=runs, warm=10),
                "device_single_calls": timed(lambda: [sc.detect(a, b, 4) for a, b in zip(queries, lists)], runs=runs, warm=3)}
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    path = next((a for a in args if a.endswith(".json")), os.path.join(ROOT, "profiles", "scan_context.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
