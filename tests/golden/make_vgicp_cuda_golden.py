#!/usr/bin/env python3
"""Generates tests/golden/vgicp_cuda_pair.npz -- the clouds of tests/test_vgicp_cuda.py and tests/test_vgicp_cuda_cpu.py.

Content: a scene.py odometry pair (1 600 + 1 600 points) plus line clutter -- points along thin segments that stand in the scene (poles,
edges), the same segments seen from both poses, noise sigma 2 mm -- shuffled, 2 048 points per cloud; `line`: 48 points along ONE
segment (every neighbourhood is line-like: PLANE drops the whole cloud); the guess; and, recorded from the restatement
(tests/vgicp_cuda_np.py), the kept lists of the two clouds.

Conditions, asserted here on the restatement alone, for the two clouds AND for every prefix of them the tests use (SIZES):
  - no point has |lambda1 - 0.1 lambda2| <= 1e-9 lambda2          (no point sits on the PLANE threshold)
  - every kept point has (lambda1 - lambda0) >= 1e-6 lambda2      (the smallest eigenvalue's vector is well defined)
  - between 5 % and 50 % of each full cloud is dropped
  - the LM and GN runs of the align tests keep every transformed point >= 1e-9 voxel edges away from a voxel face.
The first seed (counted up from SEED0) that meets them is taken.  Run:  python tests/golden/make_vgicp_cuda_golden.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import apdgicp_np as anp  # noqa: E402
import vgicp_cuda_np as VC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vgicp_cuda_pair.npz")
SIZES = (20, 21, 63, 64, 65, 255, 256, 257, 2048)
N_SCENE, N_SEG, PER_SEG, SIGMA = 1600, 14, 32, 2e-3
SEED0 = 20261021
ALIGN_CASES = (("d1", VC.DIRECT1, 1.5), ("d7", VC.DIRECT7, 1.5), ("d27", VC.DIRECT27, 1.5), ("r1.5", VC.DIRECT_RADIUS, 1.5))
FACE_MARGIN = 1e-9


def make(seed: int):
    scene = importlib.import_module("riv-slam_amd.scene")
    src, tgt, T_true, guess = scene.make_pair(N_SCENE, N_SCENE, scene.pair_seed(9, seed % 1000), "odometry")
    rng = np.random.default_rng(seed)
    lo, hi = np.percentile(tgt, 10, axis=0), np.percentile(tgt, 90, axis=0)
    a = rng.uniform(lo, hi, size=(N_SEG, 3))                      # segment starts, inside the scene (target frame)
    d = rng.normal(size=(N_SEG, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    length = rng.uniform(0.8, 2.0, size=N_SEG)
    Ti = np.linalg.inv(T_true.astype(np.float64))

    def seen(frame_from_target):
        s = rng.uniform(0.0, 1.0, size=(N_SEG, PER_SEG, 1))
        p = (a[:, None, :] + s * (length[:, None, None] * d[:, None, :])).reshape(-1, 3)
        p = p @ frame_from_target[:3, :3].T + frame_from_target[:3, 3]
        return (p + rng.normal(scale=SIGMA, size=p.shape)).astype(np.float32)

    tgt = np.concatenate([tgt[:, :3], seen(np.eye(4))])[rng.permutation(N_SCENE + N_SEG * PER_SEG)]
    src = np.concatenate([src[:, :3], seen(Ti)])[rng.permutation(N_SCENE + N_SEG * PER_SEG)]
    s = rng.uniform(0.0, 1.5, size=(48, 1))
    line = (np.array([3.0, -1.0, 0.5]) + s * np.array([0.6, 0.64, 0.48]) + rng.normal(scale=SIGMA, size=(48, 3))).astype(np.float32)
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt), line, guess


def conditions(src, tgt, line, guess):
    """None when every condition holds, else what failed."""
    for name, cloud in (("source", src), ("target", tgt)):
        for n in SIZES:
            c = VC.filter_conditions(VC.raw_covariances(cloud[:n], VC.neighbours(cloud[:n])))
            if not c["threshold_margin"] > 1e-9:
                return f"{name}[:{n}] threshold margin {c['threshold_margin']}"
            if not c["gap_margin"] >= 1e-6:
                return f"{name}[:{n}] gap margin {c['gap_margin']}"
            if n == 2048 and not 0.05 <= c["dropped"] <= 0.50:
                return f"{name} dropped share {c['dropped']}"
    c = VC.filter_conditions(VC.raw_covariances(line, VC.neighbours(line)))
    if c["dropped"] != 1.0 or not c["threshold_margin"] > 1e-9:
        return f"line: dropped {c['dropped']}"
    for tag, search, radius in ALIGN_CASES:
        for opt in (0, 1):
            o = VC.FastVGICPCuda(anp.Params(optimizer=opt), 1.0, search, radius)
            o.setInputSource(src)
            o.setInputTarget(tgt)
            o.align(guess)
            if not (o.face_margin_min >= FACE_MARGIN and o.n_matched > 300):
                return f"align {tag} optimizer {opt}: face margin {o.face_margin_min}, matched {o.n_matched}"
    return None


def main():
    for seed in range(SEED0, SEED0 + 50):
        src, tgt, line, guess = make(seed)
        why = conditions(src, tgt, line, guess)
        print(seed, why or "ok")
        if why is None:
            break
    else:
        raise SystemExit("no seed met the conditions")
    ps, pt = VC.prepare(src), VC.prepare(tgt)
    np.savez_compressed(OUT, source=src, target=tgt, line=line, guess=guess.astype(np.float32), seed=np.int64(seed), source_kept=ps["kept_index"],
                        target_kept=pt["kept_index"])
    print(OUT, os.path.getsize(OUT), "bytes; kept", len(ps["kept_index"]), len(pt["kept_index"]), "of", len(src), len(tgt))


if __name__ == "__main__":
    main()
