"""Restatement of the exact k-nearest and radius queries of the target (Q1 .. Q9 of include/apdgicp_hip.h), in numpy.

A dense key matrix, one row per query, built with the fp32 arithmetic of Q1 -- every difference, product and sum rounded to float32
on its own -- and cut per Q2 / Q4 / Q5.  Nothing here knows how the device walks the target: a row is computed from the whole
target at once, so it is independent of any visiting order.  `*_literal` are a second form (a plain Python sort of every
(distance, index) pair of a query) that tests/test_search_cpu.py holds the matrix form against.
"""
import numpy as np

F32 = np.float32
K_MAX = 64


def sqdist_f32(q, t):
    """[nq, nt] float32: ((tx - qx)^2 + (ty - qy)^2) + (tz - qz)^2, each operation rounded (Q1)"""
    q = np.ascontiguousarray(q, dtype=F32)
    t = np.ascontiguousarray(t, dtype=F32)
    d = t[None, :, 0] - q[:, None, 0]
    r = d * d
    d = t[None, :, 1] - q[:, None, 1]
    r = r + d * d
    d = t[None, :, 2] - q[:, None, 2]
    r = r + d * d
    assert r.dtype == F32
    return r


def keys(q, t):
    """[nq, nt] uint64: bits of the distance << 32 | target index (Q1); unique along a row"""
    d = sqdist_f32(q, t)
    return (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(t.shape[0], dtype=np.uint64)[None, :]


def r2_of(radius):
    """Q4: the float PCL hands to FLANN"""
    return F32(np.float64(radius) * np.float64(radius))


def _split(key):
    idx = (key & np.uint64(0xFFFFFFFF)).astype(np.int64).astype(np.int32)
    dist = (key >> np.uint64(32)).astype(np.uint32).view(F32)
    return idx, dist


def knn(q, t, k, chunk=256):
    """Q2: (index [nq, k] int32, sq_dist [nq, k] float32, n_found); the tail of a row is -1 / +Inf"""
    assert 1 <= k <= K_MAX
    q = np.asarray(q, dtype=F32)[:, :3]
    nq, m = q.shape[0], t.shape[0]
    nf = min(k, m)
    idx = np.full((nq, k), -1, dtype=np.int32)
    dist = np.full((nq, k), np.inf, dtype=F32)
    for s in range(0, nq, chunk):
        ky = keys(q[s:s + chunk], t)
        if nf < m:
            ky = np.partition(ky, nf - 1, axis=1)[:, :nf]   # the nf smallest keys of a row, as a set (keys are unique) ...
        ky = np.sort(ky, axis=1)                            # ... then ascending
        idx[s:s + chunk, :nf], dist[s:s + chunk, :nf] = _split(ky)
    return idx, dist, nf


def radius_search(q, t, radius, max_nn=0, chunk=256):
    """Q4 / Q5 / Q6: (row_start [nq + 1] int64, index [total] int32, sq_dist [total] float32)"""
    q = np.asarray(q, dtype=F32)[:, :3]
    nq, m = q.shape[0], t.shape[0]
    r2 = r2_of(radius)
    rows = []
    for s in range(0, nq, chunk):
        ky = keys(q[s:s + chunk], t)
        hit = (ky >> np.uint64(32)).astype(np.uint32).view(F32) < r2   # strictly
        for i in range(ky.shape[0]):
            row = np.sort(ky[i][hit[i]])
            if 0 < max_nn < m:
                row = row[:max_nn]
            rows.append(row)
    row_start = np.zeros(nq + 1, dtype=np.int64)
    row_start[1:] = np.cumsum([len(r) for r in rows])
    allk = np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint64)
    idx, dist = _split(allk.astype(np.uint64))
    return row_start, idx, dist


# ---- the literal form: per query, every (distance, index) pair sorted as Python tuples
def _pairs(qi, t):
    out = []
    for j in range(t.shape[0]):
        dx, dy, dz = F32(t[j, 0] - qi[0]), F32(t[j, 1] - qi[1]), F32(t[j, 2] - qi[2])
        r = F32(dx * dx)
        r = F32(r + F32(dy * dy))
        r = F32(r + F32(dz * dz))
        out.append((float(r), j))
    out.sort()
    return out


def knn_literal(q, t, k):
    q = np.asarray(q, dtype=F32)
    t = np.asarray(t, dtype=F32)
    idx = np.full((len(q), k), -1, dtype=np.int32)
    dist = np.full((len(q), k), np.inf, dtype=F32)
    for i in range(len(q)):
        for r, (d, j) in enumerate(_pairs(q[i], t)[:k]):
            idx[i, r], dist[i, r] = j, d
    return idx, dist, min(k, len(t))


def radius_search_literal(q, t, radius, max_nn=0):
    q = np.asarray(q, dtype=F32)
    t = np.asarray(t, dtype=F32)
    r2 = float(r2_of(radius))
    starts, idx, dist = [0], [], []
    for i in range(len(q)):
        row = [(d, j) for d, j in _pairs(q[i], t) if d < r2]
        if 0 < max_nn < len(t):
            row = row[:max_nn]
        idx += [j for _, j in row]
        dist += [d for d, _ in row]
        starts.append(len(idx))
    return np.array(starts, dtype=np.int64), np.array(idx, dtype=np.int32), np.array(dist, dtype=F32)
