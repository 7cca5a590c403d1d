"""Restatement (test infrastructure, NOT product code) of fast_gicp::NDTCuda as include/apdgicp_hip.h pins it down in N1 .. N8: a
subclass of the APD-GICP restatement (oracle/apdgicp_np.py) that replaces update_correspondences / linearize / compute_error and
inherits step_lm, step_gn and align.  Vectorised: the voxel map comes from np.unique + np.add.at (which adds in index order, i.e.
in the caller's order), the lookups from np.searchsorted over packed keys; the symmetric eigen-decomposition of N3 is the one
apdgicp_np's covariances use (np.linalg.eigh).  build_map_dict is the independent, point-after-point statement of N1 / N2.

Reference files: fast_apdgicp/src/fast_gicp/cuda/ndt_cuda.cu ("NC:"), ndt_compute_derivatives.cu ("ND:"), gaussian_voxelmap.cu
("GV:"), covariance_regularization.cu ("CR:").
"""
from __future__ import annotations

import numpy as np

import apdgicp_np as anp
from vgicp_np import DIRECT1, DIRECT7, DIRECT27, LIM, neighbor_offsets, voxel_coord  # noqa: F401  (N1 / N5 are V1 .. V3 / V5)

P2D, D2D = 0, 1
MIN_EIG = 1e-3        # N3
MIN_POINTS = 6        # N6: count <= 6 contributes nothing
TRI = ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))   # the six stored entries (r, c), r >= c: xx, yx, zx, yy, zy, zz


def pack_keys(c: np.ndarray) -> np.ndarray:
    """three coordinates biased by 2^20 into 21 bits each, x highest: ascending key = lexicographic (cx, cy, cz)"""
    c = np.asarray(c, dtype=np.int64) + LIM
    return (c[..., 0].astype(np.uint64) << np.uint64(42)) | (c[..., 1].astype(np.uint64) << np.uint64(21)) | c[..., 2].astype(np.uint64)


def _coords_checked(points: np.ndarray, res: float, what: str):
    P = np.asarray(points, dtype=np.float32)[:, :3].astype(np.float64)
    C = voxel_coord(P, res)
    ok = np.isfinite(P).all(axis=1) & (np.abs(C) < LIM).all(axis=1)
    if not ok.all():
        raise ValueError(f"{what} point {int(np.nonzero(~ok)[0][0])} is not finite or outside the voxel key range")
    return P, C.astype(np.int64)


def regularize(raw6: np.ndarray) -> np.ndarray:
    """N3 (CR:73-87): C = V diag(max(lambda, 1e-3)) V^T of the symmetric matrix whose lower triangle is raw6 -> [nv, 3, 3]"""
    nv = raw6.shape[0]
    A = np.zeros((nv, 3, 3))
    for q, (r, c) in enumerate(TRI):
        A[:, r, c] = A[:, c, r] = raw6[:, q]
    w, U = np.linalg.eigh(A)
    return np.einsum("nij,nj,nkj->nik", U, np.maximum(w, MIN_EIG), U)


def _finish(coords, counts, S1, S2):
    n = counts.astype(np.float64)
    means = S1 / n[:, None]
    raw = np.stack([(S2[:, q] - means[:, r] * S1[:, c]) / n for q, (r, c) in enumerate(TRI)], axis=1)   # N2: c_rc = (S2_rc - mean_r S1_c) / n
    return {"coords": coords.astype(np.int32), "counts": counts.astype(np.int32), "means": means, "raw": raw, "covs": regularize(raw),
            "keys": pack_keys(coords)}


def build_map(points: np.ndarray, res: float, what: str = "target") -> dict:
    """N1 .. N3, vectorised: voxels in ascending key order, S1 and S2 summed in the caller's order (np.add.at adds in index order)."""
    P, Ci = _coords_checked(points, res, what)
    coords, inv, counts = np.unique(Ci, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    S1 = np.zeros((len(coords), 3))
    S2 = np.zeros((len(coords), 6))
    np.add.at(S1, inv, P)
    np.add.at(S2, inv, np.stack([P[:, r] * P[:, c] for r, c in TRI], axis=1))
    return _finish(coords, counts, S1, S2)


def build_map_dict(points: np.ndarray, res: float, what: str = "target") -> dict:
    """The same map from a plain dict filled point after point: the independent statement of N1 / N2."""
    P, Ci = _coords_checked(points, res, what)
    vox: dict = {}
    for i in range(P.shape[0]):
        key = (int(Ci[i, 0]), int(Ci[i, 1]), int(Ci[i, 2]))
        v = vox.get(key)
        if v is None:
            v = vox[key] = [0, [0.0, 0.0, 0.0], [0.0] * 6]
        v[0] += 1
        x = (float(P[i, 0]), float(P[i, 1]), float(P[i, 2]))
        for a in range(3):
            v[1][a] += x[a]
        for q, (r, c) in enumerate(TRI):
            v[2][q] += x[r] * x[c]
    keys = sorted(vox)
    nv = len(keys)
    return _finish(np.array(keys, dtype=np.int64).reshape(nv, 3), np.array([vox[k][0] for k in keys]), np.array([vox[k][1] for k in keys]).reshape(nv, 3),
                   np.array([vox[k][2] for k in keys]).reshape(nv, 6))


def map_from_device(v: dict) -> dict:
    """A map as the handle returns it (ndt.NDT.voxels) in this module's form."""
    return {"coords": v["coords"], "counts": v["counts"], "means": v["means"], "raw": v["raw"], "covs": v["covs"], "keys": pack_keys(v["coords"])}


class _Empty(Exception):
    def __init__(self, T):
        self.T = T


class NDT(anp.FastAPDGICP):
    def __init__(self, params: anp.Params | None = None, resolution: float = 1.0, distance_mode: int = D2D, search: int = DIRECT7):
        super().__init__(params)
        self.resolution, self.distance_mode, self.search = float(resolution), distance_mode, search   # NC:15-22
        self.target_map = None
        self.source_map = None
        self.voxel_corr = None      # [n_rows, n_offsets] target voxel index, -1 = miss
        self.voxel_maha = None      # [n_rows, n_offsets, 3, 3]
        self.n_matched = 0
        self.face_margin = np.inf       # of the last linearize
        self.face_margin_min = np.inf   # over everything since the last align() began
        self._in_align = False

    def setInputSource(self, cloud):
        super().setInputSource(cloud)
        self.source_map = None

    def setInputTarget(self, cloud):
        super().setInputTarget(cloud)
        self.target_map = None

    def set_maps(self, target_map: dict, source_map: dict | None = None):
        """Hands over maps built elsewhere (the device's): what is compared is then everything behind them."""
        self.target_map, self.source_map = target_map, source_map

    def _ensure(self):   # N4
        if self.target_map is None:
            self.target_map = build_map(self.target, self.resolution, "target")
        if self.distance_mode == D2D and self.source_map is None:
            self.source_map = build_map(self.source, self.resolution, "source")

    def rows(self) -> np.ndarray:
        """N5: source voxel means in voxel order (D2D) or source points in the caller's order (P2D)"""
        return self.source_map["means"] if self.distance_mode == D2D else self.source[:, :3].astype(np.float64)

    @staticmethod
    def transform(T, a):
        """q_r = ((R_r0 x + R_r1 y) + R_r2 z) + t_r in fp64"""
        T = np.asarray(T, dtype=np.float64)
        a = np.asarray(a, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.stack([((T[r, 0] * a[:, 0] + T[r, 1] * a[:, 1]) + T[r, 2] * a[:, 2]) + T[r, 3] for r in range(3)], axis=1)

    def update_correspondences(self, T):
        self._ensure()
        T = np.asarray(T, dtype=np.float64)
        offs = neighbor_offsets(self.search)
        rows = self.rows()
        n, no = rows.shape[0], len(offs)
        q = self.transform(T, rows)
        t = voxel_coord(q, self.resolution)
        usable = np.isfinite(q).all(axis=1) & (np.abs(t) <= LIM).all(axis=1)
        corr = np.full((n, no), -1, dtype=np.int32)
        keys = self.target_map["keys"]
        ur = np.nonzero(usable)[0]
        if len(ur):
            cc = t[ur].astype(np.int64)[:, None, :] + offs[None, :, :]
            in_range = (np.abs(cc) < LIM).all(axis=2)          # the range test comes first
            k = pack_keys(np.where(in_range[:, :, None], cc, 0))
            pos = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
            hit = in_range & (keys[pos] == k)
            corr[ur] = np.where(hit, pos, -1).astype(np.int32)
        with np.errstate(invalid="ignore"):
            f = q[usable] / self.resolution - 0.5
            self.face_margin = float(np.abs(f - np.round(f)).min()) if usable.any() else np.inf
        self.face_margin_min = min(self.face_margin_min, self.face_margin)
        contributes = (corr >= 0) & (self.target_map["counts"][np.maximum(corr, 0)] > MIN_POINTS)   # N6
        M = np.zeros((n, no, 3, 3))
        ii, kk = np.nonzero(contributes)
        if len(ii):
            CB = self.target_map["covs"][corr[ii, kk]]
            if self.distance_mode == D2D:
                R = T[:3, :3]
                CB = CB + np.einsum("ij,njk,lk->nil", R, self.source_map["covs"][ii], R)   # ND:145-146, R of THIS (the linearize) pose
            M[ii, kk] = np.linalg.inv(CB)
        self.voxel_corr, self.voxel_maha, self._contrib = corr, M, contributes
        self.n_matched = int(len(ii))
        self.correspondences = corr   # (the base class's attribute: not point indices here)

    def _cost_terms(self, T):
        ii, kk = np.nonzero(self._contrib)   # row-major, offset-minor
        v = self.voxel_corr[ii, kk]
        q = self.transform(T, self.rows()[ii])
        e = self.target_map["means"][v] - q                                 # ND:76
        r2 = self.resolution * self.resolution
        w = r2 / (r2 + np.einsum("ni,ni->n", e, e))                         # ND:78, cauchy(resolution, |e|)
        M = self.voxel_maha[ii, kk]
        Me = np.einsum("nij,nj->ni", M, e)
        return q, e, w, M, Me

    def linearize(self, T, want_Hb: bool = True):
        self.trace.n_linearize += 1
        T = np.asarray(T, dtype=np.float64)
        self.update_correspondences(T)
        if self.n_matched == 0:
            if self._in_align:
                raise _Empty(T)    # N8
            return 0.0, (np.zeros((6, 6)) if want_Hb else None), (np.zeros(6) if want_Hb else None)
        q, e, w, M, Me = self._cost_terms(T)
        cost = float(np.sum(w * np.einsum("ni,ni->n", e, Me)))              # ND:79
        if not want_Hb:
            return cost, None, None
        J = np.zeros((len(q), 3, 6))
        J[:, 0, 1], J[:, 0, 2] = -q[:, 2], q[:, 1]
        J[:, 1, 0], J[:, 1, 2] = q[:, 2], -q[:, 0]
        J[:, 2, 0], J[:, 2, 1] = -q[:, 1], q[:, 0]
        J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1.0                         # ND:81-83
        MJ = np.einsum("nij,njk->nik", M, J)
        H = np.einsum("n,nji,njk->ik", w, J, MJ)                            # ND:87
        b = np.einsum("n,nji,nj->i", w, J, Me)                              # ND:88
        return cost, H, b

    def frozen_cost(self, T, w) -> float:
        """The cost over the frozen state with the weights held at `w` (what H and b are the derivatives of)."""
        _, e, _, _, Me = self._cost_terms(np.asarray(T, dtype=np.float64))
        return float(np.sum(w * np.einsum("ni,ni->n", e, Me)))

    # NC:162-177: frozen indices and M; q, e and w of the trial pose
    def compute_error(self, T) -> float:
        self.trace.n_compute_error += 1
        if self.n_matched == 0:
            return 0.0
        _, e, w, _, Me = self._cost_terms(np.asarray(T, dtype=np.float64))
        return float(np.sum(w * np.einsum("ni,ni->n", e, Me)))

    def align(self, guess=None):
        self._ensure()
        self.face_margin_min = np.inf
        self._in_align = True
        if self.source_covs is None:
            self.source_covs = np.zeros((0, 3, 3))   # (the optimiser loop of the base class would compute the k-NN covariances: N4, none here)
        if self.target_covs is None:
            self.target_covs = np.zeros((0, 3, 3))
        try:
            return super().align(guess)
        except _Empty as stop:     # N8: the loop stops, converged = 0, T = the pose so far
            self.converged = False
            self.final_transformation = stop.T.astype(anp.F32)
            return self.final_transformation
        finally:
            self._in_align = False
