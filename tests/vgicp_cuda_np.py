"""Restatement (test infrastructure, NOT product code) of fast_gicp::FastVGICPCuda as include/apdgicp_hip.h pins it down in VC1 .. VC10.
New here: the neighbour covariance as a sequential loop over the ranks (VC2), the regularisation and the planarity filter from
numpy.linalg.eigh (VC3 / VC4), the offset lists (VC6) and the lookup over them.  The voxel map, the cost and the GN / LM loop are those of
tests/vgicp_np.py (V3, V5 .. V7), used as they are: this class hands them the kept clouds and their covariances.

Reference lines, paths under fast_apdgicp/: "CE:" src/fast_gicp/cuda/covariance_estimation.cu, "CR:" .../covariance_regularization.cu,
"VC:" .../fast_vgicp_cuda.cu, "VCI:" include/fast_gicp/gicp/impl/fast_vgicp_cuda_impl.hpp.
"""
from __future__ import annotations

import numpy as np

import apdgicp_np as anp
import vgicp_np as V

K = 20                                                   # VC1 (VCI:38)
DIRECT1, DIRECT7, DIRECT27, DIRECT_RADIUS = 0, 1, 2, 3
MIN_EIG, PLANE, FROBENIUS = 1, 3, 4
MAX_RADIUS = 4
LIM = V.LIM


def neighbor_offsets(method: int, radius: float = 1.5) -> np.ndarray:
    """VC6 (VC:42-95)."""
    if method in (DIRECT1, DIRECT7, DIRECT27):
        return V.neighbor_offsets(method)
    if method != DIRECT_RADIUS:
        raise ValueError("unknown neighbor search method")
    if not (np.isfinite(radius) and 0.0 <= radius <= MAX_RADIUS):
        raise ValueError("radius must be finite with 0 <= r <= 4")
    rng = int(np.ceil(radius))
    out = []
    for i in range(-rng, rng + 1):
        for j in range(-rng, rng + 1):
            for k in range(-rng, rng + 1):                                   # VC:81-87, k fastest
                if np.sqrt(np.float64(i * i + j * j + k * k)) <= np.float64(radius) + 1e-3:
                    out.append((i, j, k))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def neighbours(cloud: np.ndarray) -> np.ndarray:
    """VC1: [n, 20] indices in rank order -- ascending fp32 squared distance, ties by ascending index, the point itself included."""
    cloud = np.ascontiguousarray(cloud, dtype=np.float32)[:, :3]
    if cloud.shape[0] < K:
        raise ValueError("cloud has fewer points than k_correspondences")
    return anp.knn(cloud, K)


def raw_covariances(cloud: np.ndarray, nbrs: np.ndarray) -> np.ndarray:
    """VC2 (CE:26-34): the loop over the ranks, one rank after the other; every point runs the same loop (the vector axis)."""
    P = np.ascontiguousarray(cloud, dtype=np.float32)[:, :3].astype(np.float64)
    n = P.shape[0]
    s1 = np.zeros((n, 3))
    s2 = np.zeros((n, 3, 3))
    for r in range(K):
        p = P[nbrs[:, r]]
        s1 = s1 + p                                   # mean += pt
        s2 = s2 + p[:, :, None] * p[:, None, :]       # cov += pt pt^T : the product is rounded, then added
    mean = s1 / float(K)
    return s2 / float(K) - mean[:, :, None] * mean[:, None, :]


def eigen(raw: np.ndarray):
    """ascending eigenvalues [n, 3] and eigenvectors [n, 3, 3] (columns) of the symmetric raw covariances"""
    return np.linalg.eigh(raw)


def regularize(raw: np.ndarray, method: int):
    """VC3 (CR:91-117): (keep [n] bool, regularised covariances [n, 3, 3] of EVERY point)."""
    n = raw.shape[0]
    if method == FROBENIUS:                                                  # CR:63-71
        C = raw + 1e-3 * np.eye(3)
        Ci = np.linalg.inv(C)
        nf = np.sqrt((Ci * Ci).sum(axis=(1, 2)))
        return np.ones(n, dtype=bool), np.linalg.inv(Ci / nf[:, None, None])
    w, U = eigen(raw)
    if method == PLANE:                                                      # CR:26-31, 96-109
        with np.errstate(invalid="ignore"):
            keep = w[:, 1] > 0.1 * w[:, 2]
        d = np.tile(np.array([1e-3, 1.0, 1.0]), (n, 1))
    elif method == MIN_EIG:                                                  # CR:73-87
        keep = np.ones(n, dtype=bool)
        d = np.maximum(w, 1e-3)
    else:
        raise NotImplementedError("NONE and NORMALIZED_MIN_EIG are not offered")
    return keep, np.einsum("nij,nj,nkj->nik", U, d, U)


def prepare(cloud: np.ndarray, method: int = PLANE) -> dict:
    """VC1 .. VC4 of one cloud."""
    cloud = np.ascontiguousarray(cloud, dtype=np.float32)[:, :3]
    nbrs = neighbours(cloud)
    raw = raw_covariances(cloud, nbrs)
    keep, reg = regularize(raw, method)
    kept = np.nonzero(keep)[0].astype(np.int32)
    return {"neighbours": nbrs, "raw_all": raw, "kept_index": kept, "points": cloud[kept], "raw": raw[kept], "covs": reg[kept]}


def filter_conditions(raw: np.ndarray) -> dict:
    """What the fixtures are chosen by: the distance of every point from the PLANE threshold and the gap below lambda1 of the kept ones,
    both relative to lambda2, and the dropped share."""
    w, _ = eigen(raw)
    keep = w[:, 1] > 0.1 * w[:, 2]
    thr = np.abs(w[:, 1] - 0.1 * w[:, 2]) / w[:, 2]
    gap = (w[keep, 1] - w[keep, 0]) / w[keep, 2]
    return {"threshold_margin": float(thr.min()), "gap_margin": float(gap.min()) if keep.any() else np.inf, "dropped": float(1.0 - keep.mean())}


class FastVGICPCuda(V.FastVGICP):
    """source / target of the base class are the KEPT clouds (VC4); source_full / target_full what the caller set."""

    def __init__(self, params: anp.Params | None = None, resolution: float = 1.0, search: int = DIRECT1, radius: float = 1.5, regularization: int = PLANE):
        super().__init__(params, resolution, search, V.ADDITIVE)
        self.radius, self.regularization = float(radius), regularization
        self.prep = [None, None]
        self.source_full = self.target_full = None

    def setInputSource(self, cloud):
        self.source_full = np.ascontiguousarray(cloud, dtype=np.float32)[:, :3]
        self.prep[0] = prepare(self.source_full, self.regularization)
        super().setInputSource(self.prep[0]["points"])
        self.source_covs = self.prep[0]["covs"]

    def setInputTarget(self, cloud):
        self.target_full = np.ascontiguousarray(cloud, dtype=np.float32)[:, :3]
        self.prep[1] = prepare(self.target_full, self.regularization)
        super().setInputTarget(self.prep[1]["points"])
        self.target_covs = self.prep[1]["covs"]

    def _ensure(self):
        if self.voxelmap is None:
            if len(self.target) == 0:      # VC9: no kept target point, no voxel
                self.voxelmap = {"coords": np.zeros((0, 3), np.int32), "counts": np.zeros(0, np.int32), "means": np.zeros((0, 3)), "covs": np.zeros((0, 3, 3)), "index": {}}
            else:
                self.voxelmap = V.build_voxelmap(self.target, self.target_covs, self.resolution, self.mode)     # VC5

    # VC6 / VC7: V5's lookup over the offset list of this mode
    def update_correspondences(self, T):
        self._ensure()
        T = np.asarray(T, dtype=np.float64)
        offs = neighbor_offsets(self.search, self.radius)
        n, no = self.source.shape[0], len(offs)
        q = self.transform(T, self.source[:, :3]) if n else np.zeros((0, 3))
        t = V.voxel_coord(q, self.resolution)
        # |c| <= 2^20 + 3: beyond that no offset of magnitude <= 4 comes back into the key range, and the sum below is exact in an int64
        usable = np.isfinite(q).all(axis=1) & (np.abs(t) <= LIM + MAX_RADIUS - 1).all(axis=1)
        corr = np.full((n, no), -1, dtype=np.int32)
        index = self.voxelmap["index"]
        rows = np.nonzero(usable)[0]
        cc = t[rows].astype(np.int64)[:, None, :] + offs[None, :, :]
        in_range = (np.abs(cc) < LIM).all(axis=2)          # V2: the range test comes first
        for a, i in enumerate(rows):
            for k in range(no):
                if in_range[a, k]:
                    corr[i, k] = index.get((int(cc[a, k, 0]), int(cc[a, k, 1]), int(cc[a, k, 2])), -1)
        with np.errstate(invalid="ignore"):
            f = q[usable] / self.resolution - 0.5
            self.face_margin = float(np.abs(f - np.round(f)).min()) if usable.any() else np.inf
        self.face_margin_min = min(self.face_margin_min, self.face_margin)
        R = T[:3, :3]
        M = np.zeros((n, no, 3, 3))
        ii, kk = np.nonzero(corr >= 0)
        if len(ii):
            RCR = self.voxelmap["covs"][corr[ii, kk]] + np.einsum("ij,njk,lk->nil", R, self.source_covs[ii], R)
            M[ii, kk] = np.linalg.inv(RCR)
        self.voxel_corr, self.voxel_maha = corr, M
        self.n_matched = int(len(ii))
        self.correspondences = corr
