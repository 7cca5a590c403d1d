"""The restatement the DBSCAN tests compare with: the literal sequential loop of DBSCANSimpleCluster::extract
(radar_graph_slam/include/dbscan/DBSCAN_simple.h:27-90) over a dense matrix of radiusSearch's comparison (:118-142), plus the tie rule
for equal sizes (ascending seed) that include/apdgicp_hip.h adds as D7.  It is NOT the D3 - D6 form the device computes: queue, states
and noise marks are kept exactly as the reference keeps them, so the checker and the parallel form stay independent.
"""
from __future__ import annotations

import numpy as np

UN_PROCESSED, PROCESSING, PROCESSED = 0, 1, 2


def adjacency(xyz: np.ndarray, eps: float) -> np.ndarray:
    """[n, n] bool, D1: (double)(x_i' - x_i) per axis -- the fp32 difference widened --, products and sum in fp64 left to right, <= eps * eps
    in fp64; the diagonal is False (radiusSearch skips i == index)."""
    p = np.ascontiguousarray(xyz, dtype=np.float32)[:, :3]
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = None
        for axis in range(3):  # [index, i] = points[i] - points[index], in fp32, then widened
            d = (p[None, :, axis] - p[:, None, axis]).astype(np.float64)
            d2 = d * d if d2 is None else d2 + d * d
        a = d2 <= np.float64(eps) * np.float64(eps)
    np.fill_diagonal(a, False)
    return a


def radius_search(adj: np.ndarray, index: int) -> list:
    """radiusSearch: the point itself first, then every other accepted point in index order"""
    return [index] + np.flatnonzero(adj[index]).tolist()


def extract(xyz: np.ndarray, eps: float, min_pts: int = 1, min_cluster_size: int = 1, max_cluster_size: int = 2**31 - 1) -> dict:
    """-> dict(clusters = member lists (ascending index, largest first, equal sizes by ascending seed), seeds = their seeds,
    all_clusters = {seed: member list} before the size filter, cnt, core, primary = the seed of the first cluster a point was queued by (-1: none),
    labels = the rank of the kept primary cluster or -1)"""
    n = int(np.asarray(xyz).shape[0])
    adj = adjacency(np.asarray(xyz, dtype=np.float32).reshape(n, -1), eps)
    is_noise = [False] * n
    types = [UN_PROCESSED] * n
    primary = np.full(n, -1, dtype=np.int32)
    found = []  # (seed, sorted members) of the clusters that pass the size filter, in creation order
    all_clusters = {}
    for i in range(n):
        if types[i] == PROCESSED:
            continue
        nn = radius_search(adj, i)
        if len(nn) < min_pts:
            is_noise[i] = True
            continue
        queue = [i]
        types[i] = PROCESSED
        for j in nn:
            if j != i:
                queue.append(j)
                types[j] = PROCESSING
        k = 1
        while k < len(queue):
            c = queue[k]
            if is_noise[c] or types[c] == PROCESSED:
                types[c] = PROCESSED
                k += 1
                continue
            nn = radius_search(adj, c)
            if len(nn) >= min_pts:
                for j in nn:
                    if types[j] == UN_PROCESSED:
                        queue.append(j)
                        types[j] = PROCESSING
            types[c] = PROCESSED
            k += 1
        for c in queue:
            if primary[c] < 0:
                primary[c] = i
        members = sorted(set(queue))
        assert len(members) == len(queue)  # DB:82-83 change nothing
        all_clusters[i] = members
        if min_cluster_size <= len(queue) <= max_cluster_size:
            found.append((i, members))
    found.sort(key=lambda t: (-len(t[1]), t[0]))  # DB:89 + the D7 tie rule
    rank = {seed: r for r, (seed, _) in enumerate(found)}
    labels = np.array([rank.get(int(s), -1) for s in primary], dtype=np.int32)
    cnt = (1 + adj.sum(axis=1)).astype(np.int32)
    return dict(clusters=[np.array(m, dtype=np.int32) for _, m in found], seeds=np.array([s for s, _ in found], dtype=np.int32), all_clusters=all_clusters, cnt=cnt,
                core=cnt >= min_pts, primary=primary, labels=labels)


def table(xyz: np.ndarray, res: dict, core: np.ndarray, doppler: np.ndarray | None = None) -> dict:
    """the per-cluster table over the member lists: centroid (fp64 mean of the widened coordinates), fp32 min / max, core members, Doppler"""
    p = np.asarray(xyz, dtype=np.float32)[:, :3]
    K = len(res["clusters"])
    t = dict(centroid=np.zeros((K, 3)), min=np.zeros((K, 3), dtype=np.float32), max=np.zeros((K, 3), dtype=np.float32), size=np.zeros(K, dtype=np.int32),
             n_core=np.zeros(K, dtype=np.int32), seed=res["seeds"].copy(), doppler_mean=np.zeros(K), doppler_min=np.zeros(K, dtype=np.float32),
             doppler_max=np.zeros(K, dtype=np.float32))
    with np.errstate(invalid="ignore"):
        for r, m in enumerate(res["clusters"]):
            q = p[m]
            t["centroid"][r] = q.astype(np.float64).sum(axis=0) / len(m)
            t["min"][r], t["max"][r] = q.min(axis=0), q.max(axis=0)
            t["size"][r], t["n_core"][r] = len(m), int(np.count_nonzero(core[m]))
            if doppler is not None:
                d = np.asarray(doppler, dtype=np.float32)[m]
                t["doppler_mean"][r] = d.astype(np.float64).sum() / len(m)
                t["doppler_min"][r], t["doppler_max"][r] = d.min(), d.max()
    return t
