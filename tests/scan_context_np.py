"""numpy restatement of include/apdgicp_hip.h's "Scan Context place recognition" section (rules S1 .. S8), read against
radar_graph_slam/src/radar_graph_slam/Scancontext.cpp ("SC:").  Test infrastructure: the device results are compared with this bit for bit.

Every sum is an explicit ascending loop with one accumulator (np.sum is pairwise and would not reproduce the orders); numpy is used only
ELEMENTWISE across things that do not interact (the points of a cloud, the candidates of a query), where each element sees exactly the IEEE
operations of the scalar code.  atan2f is apdgicp_np.atan2f_fdlibm.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np

import apdgicp_np as anp

F32, F64 = np.float32, np.float64


@dataclass
class Params:
    num_ring: int = 40
    num_sector: int = 20
    max_radius: float = 80.0
    azimuth_max: float = 56.5
    azimuth_min: float = -56.5
    num_exclude_recent: int = 10
    num_candidates: int = 3
    search_ratio: float = 0.1
    dist_thresh: float = 0.5


def bins_of(xy: np.ndarray, p: Params):
    """S1's gate and bin indices (SC:183-195) of [n, 2] fp32 points -> (kept mask, ring 1..R, sector 1..S)"""
    x, y = np.ascontiguousarray(xy[:, 0], dtype=F32), np.ascontiguousarray(xy[:, 1], dtype=F32)
    with np.errstate(all="ignore"):
        rng = np.sqrt((x * x + y * y).astype(F32)).astype(F32)
        ang = (((anp.atan2f_fdlibm(x, y).astype(F64) - F64(math.pi / 2)) * F64(180.0)) / F64(math.pi)).astype(F32)
        keep = ~((np.abs(ang).astype(F64) > p.azimuth_max) | (rng.astype(F64) > p.max_radius))
        fr = np.ceil((rng.astype(F64) / F64(p.max_radius)) * F64(p.num_ring))
        fs = np.ceil(((ang.astype(F64) - F64(p.azimuth_min)) / (F64(p.azimuth_max) - F64(p.azimuth_min))) * F64(p.num_sector))
    fr = np.where(np.isfinite(fr), fr, 1.0)
    fs = np.where(np.isfinite(fs), fs, 1.0)
    ring = np.clip(fr, 1, p.num_ring).astype(np.int64)
    sector = np.clip(fs, 1, p.num_sector).astype(np.int64)
    return keep, ring, sector


def make_descriptor(cloud: np.ndarray, p: Params, intensity_column: int | None = 3) -> np.ndarray:
    """S1 (SC:162-214): [R, S] fp32"""
    cloud = np.asarray(cloud, dtype=F32)
    d = np.full((p.num_ring, p.num_sector), -1000.0, dtype=F32)
    if len(cloud):
        inten = cloud[:, intensity_column] if intensity_column is not None and intensity_column < cloud.shape[1] else np.zeros(len(cloud), dtype=F32)
        fin = np.isfinite(cloud[:, 0]) & np.isfinite(cloud[:, 1]) & np.isfinite(inten)   # S8
        keep, ring, sector = bins_of(np.where(fin[:, None], cloud[:, :2], F32(0.0)), p)
        for i in np.nonzero(fin & keep)[0]:     # the reference's sequential loop
            r, c = ring[i] - 1, sector[i] - 1
            if d[r, c] < inten[i]:
                d[r, c] = inten[i]
    d[d == F32(-1000.0)] = F32(0.0)
    d[d == 0] = F32(0.0)    # -0.0 -> +0.0 (S8)
    return d


def keys_of(d: np.ndarray):
    """S2 (SC:217-246): ring_key [R] fp32, sector_key [S] fp64, col_norm [S] fp64"""
    R, S = d.shape
    dd = d.astype(F64)
    a = np.zeros(R, dtype=F64)
    for c in range(S):
        a = a + dd[:, c]
    ring_key = (a / F64(S)).astype(F32)
    m, q = np.zeros(S, dtype=F64), np.zeros(S, dtype=F64)
    for r in range(R):
        m = m + dd[r, :]
        q = q + dd[r, :] * dd[r, :]
    return ring_key, m / F64(R), np.sqrt(q)


def shifted(B: np.ndarray, s: int) -> np.ndarray:
    """circshift (SC:42-62): shifted(B, s)[:, j] = B[:, (j - s) mod S]"""
    S = B.shape[-1]
    return B[..., (np.arange(S) - s) % S]


def search_radius(search_ratio: float, S: int) -> int:
    """SC:134 -- C's round (half away from zero), not Python's"""
    return int(math.floor(0.5 * search_ratio * S + 0.5))


def shift_set(a: int, radius: int, S: int) -> list:
    """SC:135-141: a and (a +- i) mod S, ascending"""
    s = {a}
    for i in range(1, radius + 1):
        s.add((a + i) % S)
        s.add((a - i) % S)
    return sorted(s)


class ScanContextNP:
    def __init__(self, params: Params | None = None, **kw):
        self.p = replace(params or Params(), **kw)
        self.desc, self.ring_key, self.sector_key, self.col_norm = [], [], [], []
        self._table = {}   # (query, candidate) -> (alignment, dist per shift)

    def __len__(self):
        return len(self.desc)

    def add_descriptor(self, d) -> int:
        d = np.array(d, dtype=F32)
        assert d.shape == (self.p.num_ring, self.p.num_sector)
        d[d == 0] = F32(0.0)
        rk, sk, cn = keys_of(d)
        self.desc.append(d), self.ring_key.append(rk), self.sector_key.append(sk), self.col_norm.append(cn)
        return len(self.desc) - 1

    def add(self, cloud, intensity_column: int | None = 3) -> int:
        return self.add_descriptor(make_descriptor(cloud, self.p, intensity_column))

    def clear(self):
        self.desc, self.ring_key, self.sector_key, self.col_norm, self._table = [], [], [], [], {}

    def ring_d2(self, q: int, ids) -> np.ndarray:
        """S4 (nanoflann's L2_Simple_Adaptor): fp32, ascending r"""
        K = np.stack([self.ring_key[i] for i in ids]).astype(F32)
        qk = self.ring_key[q]
        d2 = np.zeros(len(ids), dtype=F32)
        for r in range(self.p.num_ring):
            diff = (qk[r] - K[:, r]).astype(F32)
            d2 = (d2 + (diff * diff).astype(F32)).astype(F32)
        return d2

    def _score(self, q: int, ids):
        """S5 + S6's dist(s) for EVERY shift, of the candidates not in the table yet (elementwise over the candidates)"""
        todo = [i for i in dict.fromkeys(ids) if (q, i) not in self._table]
        if not todo:
            return
        R, S = self.p.num_ring, self.p.num_sector
        qd, qv, qn = self.desc[q].astype(F64), self.sector_key[q], self.col_norm[q]
        KD = np.stack([self.desc[i] for i in todo]).astype(F64)       # [n, R, S]
        KV, KN = np.stack([self.sector_key[i] for i in todo]), np.stack([self.col_norm[i] for i in todo])
        n = len(todo)
        with np.errstate(all="ignore"):
            norms = np.zeros((n, S), dtype=F64)
            for s in range(S):       # SC:104-124
                acc = np.zeros(n, dtype=F64)
                for c in range(S):
                    diff = qv[c] - KV[:, (c - s) % S]
                    acc = acc + diff * diff
                norms[:, s] = np.sqrt(acc)
            align = np.zeros(n, dtype=np.int64)
            best = np.full(n, 10000000.0)
            for s in range(S):
                win = norms[:, s] < best
                best = np.where(win, norms[:, s], best)
                align = np.where(win, s, align)
            dist = np.zeros((n, S), dtype=F64)
            for s in range(S):       # SC:80-101 against shifted(k, s)
                total, eff = np.zeros(n, dtype=F64), np.zeros(n, dtype=np.int64)
                for c in range(S):
                    cc = (c - s) % S
                    n1, n2 = qn[c], KN[:, cc]
                    dot = np.zeros(n, dtype=F64)
                    for r in range(R):
                        dot = dot + qd[r, c] * KD[:, r, cc]
                    use = ~((n1 == 0.0) | (n2 == 0.0))
                    total = np.where(use, total + dot / (n1 * n2), total)
                    eff = eff + use
                dist[:, s] = 1.0 - total / eff.astype(F64)
        for k, i in enumerate(todo):
            self._table[(q, i)] = (int(align[k]), dist[k].copy())

    def distance(self, q: int, i: int):
        """distanceBtnScanContext (SC:127-159) -> (distance, shift)"""
        self._score(q, [i])
        a, dist = self._table[(q, i)]
        best, arg, won = 10000000.0, 0, False
        for s in shift_set(a, search_radius(self.p.search_ratio, self.p.num_sector), self.p.num_sector):
            if dist[s] < best:
                best, arg, won = dist[s], s, True
        return (F64(best), arg) if won else (F64(np.nan), 0)

    def detect(self, query_id: int, candidate_ids, top_k: int = 1) -> dict:
        """S3 .. S7 -> dict(loop_id, yaw (fp32), matches: list of (id, shift, distance fp64, ring_d2 fp32, ring_rank))"""
        p = self.p
        none = dict(loop_id=-1, yaw=F32(0.0), matches=[])
        if query_id < p.num_exclude_recent:
            return none
        cand = [int(i) for i in candidate_ids if query_id - int(i) >= p.num_exclude_recent]
        n = len(cand)
        if n == 0:
            return none
        d2 = self.ring_d2(query_id, cand)
        order = sorted(range(n), key=lambda k: (d2[k], k))
        keep = n if (p.num_candidates <= 0 or p.num_candidates >= n) else p.num_candidates
        order = order[:keep]
        self._score(query_id, [cand[k] for k in order])
        recs = []
        for rank, k in enumerate(order):
            dist, shift = self.distance(query_id, cand[k])
            recs.append((cand[k], shift, dist, d2[k], rank))
        recs.sort(key=lambda r: (1, 0.0, r[4]) if np.isnan(r[2]) else (0, r[2], r[4]))
        recs = recs[:top_k]
        first = recs[0]
        loop_id = first[0] if first[2] < p.dist_thresh else -1
        deg = F32(first[1] * ((p.azimuth_max - p.azimuth_min) / p.num_sector))
        yaw = F32(F64(deg) * F64(math.pi) / F64(180.0))
        return dict(loop_id=loop_id, yaw=yaw, matches=recs)


def matches_array(recs, dtype) -> np.ndarray:
    out = np.zeros(len(recs), dtype=dtype)
    for i, r in enumerate(recs):
        out[i] = r
    return out


# ---------------------------------------------------------------------------------------------------------------- test and benchmark inputs
def fov_cloud(rng, n, p=None):
    """n points inside the field of view (|angle| < azimuth_max - 1 deg, range < max_radius - 1 m) with random intensities"""
    p = p or Params()
    ang = np.deg2rad(rng.uniform(p.azimuth_min + 1.0, p.azimuth_max - 1.0, n) + 90.0)   # = atan2(x, y)
    r = rng.uniform(0.5, p.max_radius - 1.0, n)
    c = np.zeros((n, 4), dtype=F32)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = r * np.sin(ang), r * np.cos(ang), rng.normal(size=n), rng.uniform(0.0, 60.0, n)
    return c


def database_descriptors(rng, n, R=40, S=20):
    """n descriptors around 40 'places': a place's descriptor, circularly shifted, with noise, dropped bins and a few empty columns"""
    base = rng.uniform(0.0, 60.0, (40, R, S)) * (rng.uniform(size=(40, R, S)) < 0.6)
    out = []
    for i in range(n):
        d = shifted(base[i % 40], int(rng.integers(0, S))) + rng.normal(size=(R, S)) * 2.0
        d = np.where(rng.uniform(size=(R, S)) < 0.1, 0.0, np.maximum(d, 0.0))
        d[:, rng.uniform(size=S) < 0.1] = 0.0
        out.append(d.astype(F32))
    return out
