"""What tests/test_vgicp_cuda_batch_cpu.py and tests/test_vgicp_cuda_batch.py share (test infrastructure, NOT product code): the batches made
from tests/golden/vgicp_cuda_pair.npz, the searches, which pairs of which search converge in the restatement, and the restatement of one
pair over given prepared clouds."""
from __future__ import annotations

import importlib
import os

import numpy as np

import apdgicp_np as anp
import vgicp_cuda_np as VC
import vgicp_np as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACE_MARGIN = 1e-9
N_TARGET = 2048
TARGET_PREFIXES = (20, 21, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048)       # the block edges: VC_K, the wave, VG_BLK, VC_BLK / SCAN_BLK
SOURCE_SIZES = (2048, 1024, 513, 257, 129, 65, 20)                                   # source k of the batch is source[:SOURCE_SIZES[k]]
KEPT_SOURCE = {2048: 1559, 1024: 724, 513: 410, 257: 221, 129: 125, 65: 65, 20: 20}  # PLANE
KEPT_TARGET = {2048: 1555, 1024: 786}
# (tag, neighbor_search, radius)
SEARCHES = (("d1", VC.DIRECT1, 1.5), ("d7", VC.DIRECT7, 1.5), ("d27", VC.DIRECT27, 1.5), ("r1.5", VC.DIRECT_RADIUS, 1.5))
FIRST_LINEARIZE_SEARCHES = SEARCHES + (("r0", VC.DIRECT_RADIUS, 0.0), ("r4.0", VC.DIRECT_RADIUS, 4.0))
R4_SIZES = (257, 65)                                                                 # radius 4.0 (257 offsets): these sources only
# the source sizes whose pair converges in the restatement, LM and GN alike; the others run to max_iterations
CONVERGING = {
    "d1": (2048, 1024, 257, 20),
    "d7": (2048, 1024, 513, 257, 20),
    "d27": (2048, 513, 257, 129, 65, 20),
    "r1.5": (2048, 1024, 513, 257, 129, 65, 20),
}


def load_pair() -> dict:
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "vgicp_cuda_pair.npz")))


def batch_guesses(pair: dict) -> list:
    """source k starts from make_transform([0.04 k, -0.03 k, 0.01 k], 0.003 k, 0, 0) @ guess, the perturbation of tests/test_vgicp_batch.py"""
    scene = importlib.import_module("riv-slam_amd.scene")
    g = pair["guess"].astype(np.float64)
    return [(scene.make_transform(np.array([0.04 * k, -0.03 * k, 0.01 * k]), 0.003 * k, 0.0, 0.0) @ g).astype(np.float32) for k in range(len(SOURCE_SIZES))]


def batch_clouds(pair: dict):
    """(target, [source k]) of the one batch every align test runs"""
    return pair["target"][:N_TARGET], [pair["source"][:n] for n in SOURCE_SIZES]


def refused_target(pair: dict) -> np.ndarray:
    """The fixture's target with a planar patch at c = 2^20 (the first refused coordinate) behind it, built as
    test_refused_target_point_is_named_by_its_original_index (tests/test_vgicp_cuda.py) builds it: PLANE keeps the patch and has dropped
    points in front of it, so the first refused point's index among the kept points differs from its index in the caller's cloud, 2048."""
    lim = float(1 << 20)
    rng = np.random.default_rng(6)
    patch = np.stack([np.full(30, lim + 0.5), rng.uniform(-3, 3, size=30), rng.uniform(-3, 3, size=30)], axis=1).astype(np.float32)
    return np.concatenate([pair["target"], patch])


def restatement(prep_src: dict, prep_tgt: dict, search: int, radius: float, res: float = 1.0, regularization: int = VC.PLANE, **kw):
    """The restatement of one pair over prepared clouds (dicts with "points" and "covs": VC.prepare's, or the device's own)."""
    o = VC.FastVGICPCuda(anp.Params(**kw), res, search, radius, regularization)
    V.FastVGICP.setInputSource(o, prep_src["points"])
    o.source_covs = prep_src["covs"]
    V.FastVGICP.setInputTarget(o, prep_tgt["points"])
    o.target_covs = prep_tgt["covs"]
    return o
