"""numpy restatement of the device map cloud generator (riv-slam_amd/csrc/apd_map.hpp), rule by rule as include/apdgicp_hip.h states them
(section "map cloud generation", M1 .. M6): the expected values of tests/test_map_cloud.py.  Every fp32 operation is a numpy float32
operation (rounded on its own, never contracted), every fp64 operation a Python float / numpy float64 one.  M3 is the sequential loop
over the points (box_seq); box_rounds is the "first violator per round" form the device runs.  Everything else is vectorised."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
EPS = float(np.finfo(np.float32).eps)
MAX_DEPTH = 21


class DepthLimit(Exception):
    """the octree would be deeper than MAX_DEPTH levels (the device returns APDGICP_ERR_UNSUPPORTED)"""


def xyzi(cloud) -> np.ndarray:
    """[n, 4] float32 {x, y, z, intensity}; a cloud without a fourth column gets intensity 0"""
    c = np.asarray(cloud, dtype=F32)
    c = c.reshape(len(c), c.shape[1] if c.ndim == 2 else 4)
    out = np.zeros((len(c), 4), dtype=F32)
    out[:, :min(4, c.shape[1])] = c[:, :4]
    return out


def push(clouds, poses, linear_chain: bool = False) -> np.ndarray:
    """M1: the pushed cloud [n, 4] float32"""
    parts = []
    with np.errstate(all="ignore"):
        for cloud, pose in zip(clouds, poses):
            c = xyzi(cloud)
            x, y, z = (np.ascontiguousarray(c[:, q]) for q in range(3))
            d = np.sqrt((x * x + y * y) + z * z).astype(np.float64)
            keep = ~(d > 50.0)
            P = np.asarray(pose, dtype=np.float64).astype(F32)
            out = np.empty_like(c)
            for r in range(3):
                a, b = P[r, 0] * x + P[r, 1] * y, P[r, 2] * z
                out[:, r] = (a + b) + P[r, 3] if linear_chain else a + (b + P[r, 3])
            out[:, 3] = c[:, 3]
            parts.append(out[keep])
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, 4), dtype=F32)


def finite_rows(p: np.ndarray) -> np.ndarray:
    return np.isfinite(p[:, :3]).all(axis=1)


def _first_box(p, res):
    """the first finite point: a voxel around it, then getKeyBitSize"""
    mn = [p[a] - res / 2 for a in range(3)]
    mx = [p[a] + res / 2 for a in range(3)]
    mk = [math.ceil((mx[a] - mn[a] - EPS) / res) for a in range(3)]
    m = max(mk[0], mk[1], mk[2], 2)
    if m > 2 ** MAX_DEPTH:
        raise DepthLimit()
    depth = int(math.ceil(math.log2(m) - EPS))
    side = 2.0 ** depth * res
    for a in range(3):
        o = (side - (mx[a] - mn[a])) / 2
        if o > EPS:
            mn[a] -= o
            mx[a] += o
    return mn, mx, depth


def _grow(p, mn, mx, depth, res):
    """adoptBoundingBoxToPoint for a later point; returns the new depth (mn, mx are updated in place)"""
    while True:
        up = [p[a] >= mx[a] for a in range(3)]
        if not (any(up) or any(p[a] < mn[a] for a in range(3))):
            return depth
        if depth + 1 > MAX_DEPTH:
            raise DepthLimit()
        side = float(1 << depth) * res
        for a in range(3):
            if not up[a]:
                mn[a] -= side
        depth += 1
        length = float(1 << depth) * res - EPS
        for a in range(3):
            mx[a] = mn[a] + length


def box_seq(pushed: np.ndarray, res: float):
    """M3, sequential: (min[3], max[3], depth, rounds) as float64 arrays / ints; None without a finite point"""
    pts = pushed[finite_rows(pushed), :3].astype(np.float64).tolist()
    if not pts:
        return None
    mn, mx, depth = _first_box(pts[0], res)
    rounds = 0
    for p in pts[1:]:
        if p[0] < mn[0] or p[1] < mn[1] or p[2] < mn[2] or p[0] >= mx[0] or p[1] >= mx[1] or p[2] >= mx[2]:
            depth = _grow(p, mn, mx, depth, res)
            rounds += 1
    return np.array(mn), np.array(mx), depth, rounds


def box_rounds(pushed: np.ndarray, res: float):
    """M3 as the device runs it: per round the first point at or after a cursor that violates the current box"""
    pts = pushed[finite_rows(pushed), :3].astype(np.float64)
    if not len(pts):
        return None
    mn, mx, depth = _first_box(pts[0].tolist(), res)
    cursor, rounds = 1, 0
    while True:
        rest = pts[cursor:]
        bad = ((rest < np.array(mn)) | (rest >= np.array(mx))).any(axis=1)
        hit = np.flatnonzero(bad)
        if not len(hit):
            return np.array(mn), np.array(mx), depth, rounds
        i = cursor + int(hit[0])
        depth = _grow(pts[i].tolist(), mn, mx, depth, res)
        cursor, rounds = i + 1, rounds + 1


def keys_of(pushed: np.ndarray, mn: np.ndarray, res: float) -> np.ndarray:
    """M4: [n_finite, 3] integer keys of the finite pushed points"""
    p = pushed[finite_rows(pushed), :3].astype(np.float64)
    return ((p - mn) / res).astype(np.int64)


def interleave(k: np.ndarray, depth: int) -> np.ndarray:
    """M5's order: bit triple of level L = (kx_L << 2) | (ky_L << 1) | kz_L"""
    k = k.astype(np.uint64)
    out = np.zeros(len(k), dtype=np.uint64)
    for b in range(depth):
        for a in range(3):
            out |= ((k[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return out


def generate(clouds, poses, resolution: float = 0.05, linear_chain: bool = False, box=box_seq) -> dict:
    """M1 .. M6: dict(points [n_out, 4] float32, pushed, n_input, n_pushed, n_finite, n_out, depth, rounds, min, max, keys [n_out] uint64)"""
    if not len(clouds):
        raise ValueError("no keyframes")
    pushed = push(clouds, poses, linear_chain)
    n_fin = int(finite_rows(pushed).sum())
    out = dict(pushed=pushed, n_input=int(sum(len(c) for c in clouds)), n_pushed=len(pushed), n_finite=n_fin, depth=0, rounds=0,
               min=np.zeros(3), max=np.zeros(3), keys=np.zeros(0, dtype=np.uint64))
    if resolution <= 0.0:
        out.update(points=pushed, n_out=len(pushed))
        return out
    if n_fin == 0:
        out.update(points=np.zeros((0, 4), dtype=F32), n_out=0)
        return out
    mn, mx, depth, rounds = box(pushed, resolution)
    k = keys_of(pushed, mn, resolution)
    assert k.min() >= 0 and k.max() < (1 << depth), "a key outside [0, 2^depth)"
    code = interleave(k, depth)
    ucode, first = np.unique(code, return_index=True)
    centres = np.zeros((len(ucode), 4), dtype=F32)
    centres[:, :3] = ((k[first].astype(np.float64) + 0.5) * resolution + mn).astype(F32)
    out.update(points=centres, n_out=len(centres), depth=depth, rounds=rounds, min=mn, max=mx, keys=ucode)
    return out


def trajectory_keyframes(scene, n_keyframes: int, n_points: int, seed: int, n_distinct: int = 32, origin=(0.0, 0.0, 0.0)):
    """Synthetic keyframes on a trajectory of riv-slam_amd/scene.py: the sensor advances by make_keyframe_set's odometry step per keyframe
    (0.2 - 1.0 m, a few degrees); the clouds are scans of scene.Scene in the sensor frame with an intensity column, `n_distinct` different
    ones used in turn (the scene is 110 m long, a trajectory of a thousand keyframes is not).  Returns ([cloud [n_points, 4] f32], [pose 4x4 f64])."""
    rng = np.random.default_rng(seed)
    world = scene.Scene(rng)
    base = []
    for q in range(min(n_distinct, n_keyframes)):
        T = scene.make_transform(np.array([0.5 * q, 0.0, 0.0]), np.deg2rad(rng.uniform(-2, 2)))
        c = np.zeros((n_points, 4), dtype=F32)
        c[:, :3] = scene._observe(rng, world, T, n_points)
        c[:, 3] = rng.uniform(0.0, 60.0, n_points).astype(F32)
        base.append(c)
    poses, T = [], scene.make_transform(np.asarray(origin, dtype=np.float64))
    for _ in range(n_keyframes):
        poses.append(T.copy())
        step = scene.make_transform(np.array([rng.uniform(0.2, 1.0), rng.uniform(-0.1, 0.1), rng.uniform(-0.03, 0.03)]),
                                    np.deg2rad(rng.uniform(-2, 2)), *np.deg2rad(rng.uniform(-0.3, 0.3, size=2)))
        T = T @ step
    return [base[q % len(base)] for q in range(n_keyframes)], poses
