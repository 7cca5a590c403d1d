"""Targets past 64 super boxes (-m gpu): the search paths that only run for targets beyond 524 288 points.

Large targets carry one more level in front of the group boxes (apd_sort.hpp): the sorted target is cut into groups of
kGroupPts = 128 points, and every kSuperGroups = 64 groups (8192 points) get a super box.  For a target of M points

    ngroups = ceil(M / 128),   nsuper = ceil(ngroups / 64)

and both searches -- nn_search (the 1-NN of every registration tick, k_nn_pruned / k_nn_compact / k_knn_and_search) and
knn_cov_coop_wave (the k-NN behind the covariances) -- walk the super boxes in chunks of 64 (`for (sb0 = 0; sb0 < nsuper;
sb0 += 64)`).  A second chunk exists only for nsuper > 64, i.e. M > 64 * 64 * 128 = 524 288:

    M           nsuper   reaches
    524 288     64       exactly one chunk: the last size one chunk covers
    524 289     65       a second chunk holding ONE super box: the `min(sb0 + lane, nsuper - 1)` clamp and the tail of `smask`
    600 000     74       a second chunk of 10 super boxes: more than eight can pass, so the per-point refinement can run in it
    1 200 000   147      three chunks; the refinement runs in chunks 2 and 3 (sb0 = 64, 128)

The sources:
- one scattered wave: 64 target points drawn uniformly over the whole cloud, each jittered by ~3 cm (source frame = the true
  pose's inverse).  The wave's box is practically the target's box, so in a cold, gated search (radius = the gate) the coarse
  test passes nearly every super box: the per-point refinement (`__popcll(smask) > 8`) runs in every chunk past the first
  (asserted on the host).  The waves' live radii differ there -- in chunk 0 each wave scanned only its own groups (index =
  wid mod W) -- but for random points that rarely changes a mask.
- a diverging wave, built for it (diverging_wave): one point per split W = 2, 4, 8 that lands at the guess on a target of the
  first chunk where the waves' live radii straddle the bound of a super box beyond it, the rest scattered as above.  A host
  model of the device's layout (Layout) shows that with the live radii the W waves would get different masks past the first
  chunk (asserted for every W at 600 000 and 1 200 000 points), i.e. different numbers of block barriers -- the case the
  refinement's START radii (bestR0) exist for.  The model counts exactly the batches the device visits
  (test_the_host_model_of_the_layout_is_the_devices).
- sixteen scattered waves (1000 such points), a realistic 8192-point scan with ~2 % of such outliers mixed in, and at
  M = 1 200 000 a dense 100 000-point source (the engine picks W = 4 for it by itself; one pair with more than 1280 search
  blocks: the blocks report their cost for k_block_order).
The super-box test needs a finite radius: a registration tick searches with the gate as its cap, so the first (cold) tick of every
align in test_registrations_* runs the refinement in every chunk past the first.  A search outside a registration (linearize at a
pose, nearestNeighbours*) has no cap: every super box of every chunk is visited, which covers the chunk loop, the clamp and the
mask tail.

Every case runs under the engine's own wave split and under APDGICP_NN_W = 1, 2, 4, 8 and APDGICP_NN_MODE=brute (k_nn_partial:
no boxes at all); registrations also with neighbour keeping off.  Bars: correspondences, fp32 distances, H, b and cost at a
pose bitwise equal across configurations; correspondences and distances equal to the CPU oracle's, H / b / cost within HB_TOL;
result records of whole registrations byte for byte; gate-free searches bit for bit against the oracle's kd-tree; target
covariances within 1e-10 of the oracle's.
"""
import math
import os
import re

import numpy as np
import pytest

import ref as R
import apdgicp_np as O
from conftest import ROOT, rel_err
from test_hip_parity import HB_TOL, LAUNCH, R_TOL, T_TOL, _handle_with_env, info_of, reg  # noqa: F401 (reg: the module fixture)

pytestmark = pytest.mark.gpu

SIZES = (524_288, 524_289, 600_000, 1_200_000)
NSUPER = {524_288: 64, 524_289: 65, 600_000: 74, 1_200_000: 147}
BIG = SIZES[-1]
SEED = 8_524_289
JITTER = 0.03
SEARCH_ENVS = ({}, {"APDGICP_NN_W": "1"}, {"APDGICP_NN_W": "2"}, {"APDGICP_NN_W": "4"}, {"APDGICP_NN_W": "8"}, {"APDGICP_NN_MODE": "brute"})
# registrations: + neighbour keeping off (with W = 1 that is the one-wave k_nn_pruned instead of k_nn_compact)
ALIGN_ENVS = SEARCH_ENVS + ({"APDGICP_NN_SKIN": "0"}, {"APDGICP_NN_W": "1", "APDGICP_NN_SKIN": "0"})
GN6 = dict(optimizer=1, max_iterations=6, transformation_epsilon=1e-300, rotation_epsilon=1e-300, max_correspondence_distance=2.0,
           azimuth_variance_deg=1.0)
GN6_GATE10 = dict(GN6, max_correspondence_distance=10.0)   # (a larger cap: more super boxes pass, larger start radii)
GATES = (2.0, 10.0)
CAP = 4.0      # the cap of a registration's search under GN6's gate (gate_cap: the smallest float >= 2.0^2)
F32 = np.float32


def _constant(name):
    """a constant of apd_sort.hpp as the kernels see it (a literal, or a product of a literal and an earlier constant)"""
    with open(os.path.join(ROOT, "riv-slam_amd", "csrc", "apd_sort.hpp")) as f:
        expr = re.search(r"constexpr int %s = ([^;]+);" % name, f.read()).group(1).strip()
    m = re.fullmatch(r"(\d+) \* (\w+)", expr)
    return int(m.group(1)) * _constant(m.group(2)) if m else int(expr)


def nsuper_of(m):
    return math.ceil(math.ceil(m / _constant("kGroupPts")) / _constant("kSuperGroups"))


def to_frame(T, p):
    """points p (float64, target frame) into the frame that T maps onto the target's, as float32"""
    Ti = np.linalg.inv(np.asarray(T, dtype=np.float64))
    return (p @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32)


def scattered(rng, tgt, n, T_true):
    """n points within ~JITTER of target points drawn uniformly over the whole cloud: (target frame, source frame)"""
    p = tgt[rng.integers(0, len(tgt), n)].astype(np.float64) + rng.normal(0.0, JITTER, (n, 3))
    return p.astype(F32), to_frame(T_true, p)


# ---- host model of the device's layout of a large target and of the first, cold search of a registration tick


def curve_order(pts):
    """the order of the generic sort (apd_sort.hpp k_morton_keys + bitonic sort, clouds beyond SORT_LDS_MAX_N): the Hilbert code
    of every point in a grid of 2^bits cells per axis over the bounding cube, ties by index -- fp32 like the kernel"""
    n = len(pts)
    np2 = 4096
    while np2 < n:
        np2 <<= 1
    bits = min(21, (64 - max(1, (np2 - 1).bit_length())) // 3)
    lo, hi = pts.min(0), pts.max(0)
    top = F32((1 << bits) - 1)
    scale = F32(top / max(F32(hi[0] - lo[0]), F32(hi[1] - lo[1]), F32(hi[2] - lo[2]), F32(1e-30)))
    X0, X1, X2 = (np.minimum(np.maximum((pts[:, a] - lo[a]) * scale, F32(0)), top).astype(np.uint64) for a in range(3))
    Q = 1 << (bits - 1)
    while Q > 1:   # Skilling's axes-to-transpose transform, as in morton30
        P, q = np.uint64(Q - 1), np.uint64(Q)
        X0 = np.where(X0 & q, X0 ^ P, X0)
        t = (X0 ^ X1) & P
        X0, X1 = np.where(X1 & q, X0 ^ P, X0 ^ t), np.where(X1 & q, X1, X1 ^ t)
        t = (X0 ^ X2) & P
        X0, X2 = np.where(X2 & q, X0 ^ P, X0 ^ t), np.where(X2 & q, X2, X2 ^ t)
        Q >>= 1
    X1 = X1 ^ X0
    X2 = X2 ^ X1
    t = np.zeros_like(X0)
    Q = 1 << (bits - 1)
    while Q > 1:
        t = np.where(X2 & np.uint64(Q), t ^ np.uint64(Q - 1), t)
        Q >>= 1
    code = np.zeros(n, np.uint64)
    for b in range(bits):
        for a, X in enumerate((X0 ^ t, X1 ^ t, X2 ^ t)):
            code |= ((X >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return np.lexsort((np.arange(n), code))


def _boxes(sp, per):
    nb = -(-len(sp) // per)
    a = np.concatenate([sp, np.full((nb * per - len(sp), 3), np.nan, F32)]).reshape(nb, per, 3)
    return np.nanmin(a, 1), np.nanmax(a, 1)


def _lb(lo, hi, plo, phi):
    """lb_point_box (plo = phi = the points) / lb_box_box, fp32 in the kernels' order: [points or boxes, boxes]"""
    g = np.maximum(np.maximum(lo[None] - phi[:, None], plo[:, None] - hi[None]), F32(0))
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


class Layout:
    """the sorted target's group boxes (128 points) and super boxes (64 groups)"""

    def __init__(self, tgt):
        self.sp = tgt[curve_order(tgt)]
        self.glo, self.ghi = _boxes(self.sp, 128)
        self.slo, self.shi = _boxes(self.sp, 128 * 64)
        self.nsuper = len(self.slo)
        self.n0 = min(len(self.sp), 64 * 64 * 128)        # the targets of the first chunk of super boxes

    def radii_after_chunk0(self, p, W, cap, seed=-1):
        """[W, points]: the radius of every point in every wave of a k_nn_pruned<1, W> block once the first chunk is done.  The
        search is exact, so that is the smallest distance to a target of the groups the wave scans there -- index = wid (mod W),
        plus the seed group of a cold start, which every wave scans -- or the cap"""
        grp = np.arange(self.n0) // 128
        r = []
        for w in range(W):
            o = R.RefAPDGICP(R.default_params())
            o.setInputTarget(self.sp[:self.n0][(grp % W == w) | (grp == seed)])
            r.append(np.minimum(o.knn_kdtree_batch("target", p, 1)[1][:, 0], F32(cap)))
        return np.stack(r)

    def cold_chunks(self, p, W, cap):
        """for the wave of the 64 points p (fp32, at the pose) in a cold search with the gate's cap, per chunk past the first:
        (sb0, super boxes passing the coarse test, number of distinct masks the W waves would get from the per-point refinement
        with their LIVE radii).  With the start radii (the cap) the masks are the same in every wave by construction."""
        inside = (_lb(self.glo[:64], self.ghi[:64], p, p) == 0).sum(0)
        r = self.radii_after_chunk0(p, W, cap, int(np.argmax(inside)) if inside.max() > 0 else -1)
        out = []
        for sb0 in range(64, self.nsuper, 64):
            lo, hi = self.slo[sb0:sb0 + 64], self.shi[sb0:sb0 + 64]
            coarse = _lb(lo, hi, p.min(0)[None], p.max(0)[None])[0] <= F32(cap)
            lb = _lb(lo, hi, p, p)
            out.append((sb0, int(coarse.sum()), len({tuple(coarse & (lb <= rw[:, None]).any(0)) for rw in r})))
        return out


def diverging_wave(rng, layout, tgt, guess, cap):
    """64 source points: uniformly scattered ones (the wave's box is the target's, the coarse test passes every super box) and, for
    each of W = 2, 4, 8, one point that lands at `guess` on a target of the first chunk (+ ~1 cm) where the waves' live radii
    straddle the bound of a super box past the first chunk, so that the waves' masks there differ"""
    n_uni = 61
    uni = (tgt[rng.integers(0, len(tgt), n_uni)].astype(np.float64) + rng.normal(0.0, JITTER, (n_uni, 3))).astype(F32)
    cand = (layout.sp[rng.integers(0, layout.n0, 4000)].astype(np.float64) + rng.normal(0.0, 0.01, (4000, 3))).astype(F32)
    # (candidates outside the group boxes of the first batch: the cold start's seed group is then the uniform points' choice)
    cand = cand[(_lb(layout.glo[:64], layout.ghi[:64], cand, cand) > 0).all(1)]
    inside = (_lb(layout.glo[:64], layout.ghi[:64], uni, uni) == 0).sum(0)
    seed = int(np.argmax(inside)) if inside.max() > 0 else -1
    pts = np.concatenate([uni, cand])
    lb = _lb(layout.slo[64:], layout.shi[64:], pts, pts)
    need = {W: lb <= layout.radii_after_chunk0(pts, W, cap, seed)[..., None] for W in (2, 4, 8)}   # [wave, point, super box]

    def diverging(idx):
        return {W: len({tuple(m) for m in need[W][:, idx].any(1)}) > 1 for W in need}

    picks = []
    for c in range(n_uni, len(pts)):   # a point that makes one more split diverge and keeps the others diverging
        have, would = diverging(list(range(n_uni)) + picks), diverging(list(range(n_uni)) + picks + [c])
        if all(would.values()) or (sum(would.values()) > sum(have.values()) and all(would[W] for W in have if have[W])):
            picks.append(c)
        if all(would.values()) or len(picks) == 64 - n_uni:
            break
    uni = np.concatenate([uni, (tgt[rng.integers(0, len(tgt), 64 - n_uni - len(picks))] + F32(0.01))])   # (fewer picks were needed)
    return to_frame(guess, np.concatenate([uni, pts[picks]]).astype(np.float64))


@pytest.fixture(scope="module")
def clouds(scene):
    """per target size: the target (a uniform subset of one 1.2M-point scan), its sources, the guess and T_true"""
    assert (_constant("kGroupPts"), _constant("kSuperGroups")) == (128, 64)
    assert _constant("SORT_LDS_MAX_N") < SIZES[0]                                # (the super-box level is on for every size)
    assert {m: nsuper_of(m) for m in SIZES} == NSUPER                           # the table of the module docstring
    assert NSUPER[SIZES[0]] == 64 < NSUPER[SIZES[1]] and NSUPER[BIG] > 128      # one chunk; two; three
    assert NSUPER[600_000] - 64 > 8                                              # the refinement's popcount bar, in chunk 2
    scan, tgt, T_true, guess = scene.make_pair(8192, BIG, scene.pair_seed(40, 0), "odometry")
    dense, tgt2, T2, _ = scene.make_pair(100_000, BIG, scene.pair_seed(40, 0), "odometry")
    assert np.array_equal(tgt, tgt2) and np.array_equal(T_true, T2)            # (same seed and target size: the same target)
    rng = np.random.default_rng(SEED)
    out = {}
    for m in SIZES:
        t = tgt[:m]
        _, one = scattered(rng, t, 64, T_true)
        q16, sixteen = scattered(rng, t, 1000, T_true)
        _, outl = scattered(rng, t, len(scan) // 50, T_true)
        noisy = np.concatenate([scan, outl])[rng.permutation(len(scan) + len(outl))]
        src = {"one_scattered_wave": one, "sixteen_scattered_waves": sixteen, "scan_with_outliers": noisy}
        lay = None
        if NSUPER[m] - 64 > 8:
            def at_guess(s_):
                return O.transform_points_f32(guess.astype(np.float64), s_)
            # the per-point refinement runs past the first chunk (more than eight super boxes pass the coarse test there) ...
            lay = Layout(t)
            assert all(n > 8 for _, n, _ in lay.cold_chunks(at_guess(one), 8, CAP))
            # ... and with a wave built for it, the waves' live radii would give them different masks (and different numbers of
            # barriers): in some chunk past the first under every wave split
            src["diverging_wave"] = dw = diverging_wave(rng, lay, t, guess, CAP)
            assert len(dw) == 64
            for W in (2, 4, 8):
                assert any(n > 8 and k > 1 for _, n, k in lay.cold_chunks(at_guess(dw), W, CAP)), W
        if m == BIG:
            src["dense"] = dense
        out[m] = dict(tgt=t, src=src, q=q16, scan=scan, guess=guess, T_true=T_true, layout=lay)
    return out


def _fast(reg, env, tgt, **kw):
    h = _handle_with_env(reg, reg.FastAPDGICP, env, **kw)
    h.setInputTarget(tgt)
    return h


@pytest.mark.parametrize("m", SIZES)
def test_search_at_the_guess_is_exact_past_64_super_boxes(reg, clouds, m):
    """linearize at the guess, every source, two gates: correspondences / fp32 distances / H / b / cost bitwise equal across the
    wave splits and the brute-force search, and equal to the oracle's (H, b, cost: HB_TOL).  At 524 289 and 1.2M points the
    target covariances (knn_cov_coop_wave's own chunk loop) are the oracle's within 1e-10."""
    c = clouds[m]
    guess = c["guess"].astype(np.float64)
    hs = [(env, _fast(reg, env, c["tgt"], max_correspondence_distance=GATES[0], azimuth_variance_deg=1.0)) for env in SEARCH_ENVS]
    o = R.RefAPDGICP(R.default_params(max_correspondence_distance=GATES[0], azimuth_variance_deg=1.0))
    o.setInputTarget(c["tgt"])
    if m in (524_289, BIG):
        want = o.covariances("target")
        first = hs[0][1].getTargetCovariances()
        assert np.abs(first[:, :3, :3] - want).max() <= 1e-10
        for env, h in hs[1:]:
            assert np.array_equal(h.getTargetCovariances(), first), env
        del first, want
    for name, src in c["src"].items():
        o.setInputSource(src)
        for _, h in hs:
            h.setInputSource(src)
        for gate in GATES:
            o.set_params(R.default_params(max_correspondence_distance=gate, azimuth_variance_deg=1.0))
            co_, Ho, bo = o.linearize(guess)
            ci, cd = o.correspondences()
            first = None
            for env, h in hs:
                h.setMaxCorrespondenceDistance(gate)
                cost, H, b = h.linearize(guess)
                idx, sqd = h.correspondences()
                got = (cost, H, b, idx, sqd.view(np.uint32))
                first = first or got
                why = (name, gate, env)
                assert np.array_equal(idx, ci) and np.array_equal(sqd.view(np.uint32), cd.view(np.uint32)), why
                assert got[0] == first[0] and all(np.array_equal(x, y) for x, y in zip(got[1:], first[1:])), why
            assert rel_err(first[1], Ho) < HB_TOL and rel_err(first[2], bo) < HB_TOL and abs(first[0] - co_) < HB_TOL * co_, (name, gate)


@pytest.mark.parametrize("m", SIZES)
def test_registrations_agree_across_search_configurations(reg, clouds, m):
    """GN-6 (gates 2 m and 10 m) and LAUNCH LM, every source as a pair of its own and a batch of four pairs sharing the target (the
    engine picks the wave split by load): result records byte for byte under every wave split, the brute-force search and neighbour
    keeping off.  The first tick is a cold search with the gate as its radius; from the second on warm hints and kept neighbours
    feed the radii."""
    c = clouds[m]
    names = list(c["src"])
    cl = [c["tgt"]] + [c["src"][n] for n in names]
    g = c["guess"]
    batch = [(1 + names.index(n), 0) for n in ("scan_with_outliers", "sixteen_scattered_waves", "one_scattered_wave", "scan_with_outliers")]
    want = {}
    for env in ALIGN_ENVS:
        b = _handle_with_env(reg, reg.BatchAPDGICP, env, **GN6)
        b.set_clouds(0, cl)
        for tag, kw in (("gn6", GN6), ("gn6_gate10", GN6_GATE10), ("lm", LAUNCH)):
            b.set_params(reg.default_params(**kw))
            rec = [b.align([(1 + i, 0)], [g]) for i in range(len(names))] + [b.align(batch, [g] * 4)]
            got = b"".join(r.tobytes() for r in rec)
            assert got == want.setdefault(tag, got), (env, tag)
        del b


def test_registration_against_1_2m_points_is_the_oracles(reg, scene, clouds):
    """the 8192-point scan (and the same with ~2 % scattered points) against the 1.2M-point target, GN-6 and LM, fresh handles
    (the first tick is the fused k_knn_and_search): final pose within the north-star tolerance of the oracle's align, equal
    convergence flags and iteration / linearisation / error-evaluation counts"""
    c = clouds[BIG]
    o = R.RefAPDGICP(R.default_params(**GN6))
    o.setInputTarget(c["tgt"])
    for src in (c["scan"], c["src"]["scan_with_outliers"]):
        o.setInputSource(src)
        for kw in (GN6, LAUNCH):
            h = _fast(reg, {}, c["tgt"], **kw)
            h.setInputSource(src)
            o.set_params(R.default_params(**kw))
            T, To = h.align(c["guess"]), o.align(c["guess"])
            te, re_ = scene.pose_error(To, T)
            assert te <= T_TOL and re_ <= R_TOL, (len(src), kw is GN6, te, re_)
            assert info_of(h) == [int(o.converged), o.nr_iterations, o.n_linearize, o.n_compute_error], (len(src), kw is GN6)


@pytest.mark.skipif(os.environ.get("APDGICP_NN_MODE") == "brute",
                    reason="tools/knob_matrix.sh row with the brute-force search: it visits no group boxes for the counters to count")
@pytest.mark.parametrize("m", (600_000, BIG))
def test_the_host_model_of_the_layout_is_the_devices(reg, clouds, m):
    """The diverging wave is built on a host model of the device's layout (Layout: the curve order of the generic sort, the group
    and super boxes, the coarse and per-point super-box tests).  The model must count exactly the batches of group boxes every
    wave visits in the cold first tick of a one-iteration registration (debug counters: waves, batches) -- for the scattered
    and the diverging wave, W = 2 and 8.  A change of the layout or of the super-box tests fails here first: the diverging
    wave has to be rebuilt for it."""
    c = clouds[m]
    lay = c["layout"]
    for name in ("one_scattered_wave", "diverging_wave"):
        p = O.transform_points_f32(c["guess"].astype(np.float64), c["src"][name])
        want = 0
        for sb0 in range(0, lay.nsuper, 64):
            lo, hi = lay.slo[sb0:sb0 + 64], lay.shi[sb0:sb0 + 64]
            mask = _lb(lo, hi, p.min(0)[None], p.max(0)[None])[0] <= F32(CAP)   # (every point starts from the cap)
            if mask.sum() > 8:
                mask &= (_lb(lo, hi, p, p) <= F32(CAP)).any(0)
            want += int(mask.sum())
        for W in (2, 8):
            b = _handle_with_env(reg, reg.BatchAPDGICP, {"APDGICP_NN_W": str(W), "APDGICP_STATS": "1"}, **dict(GN6, max_iterations=1))
            b.set_clouds(0, [c["tgt"], c["src"][name]])
            b.align([(1, 0)], [c["guess"]])
            st = b.debug_stats()
            assert (int(st[3]), int(st[5])) == (W, W * want), (name, W, st[3], st[5], want)
            del b


def test_gate_free_searches_at_1_2m_are_the_kd_trees(reg, clouds):
    """nearestNeighbours(T) and nearestNeighboursOf(q) against the 1.2M-point target (three chunks of super boxes, no gate): index
    and fp32 squared distance bit for bit the oracle's kd-tree (pinned to nanoflann in test_oracle.py), every search configuration"""
    c = clouds[BIG]
    o = R.RefAPDGICP(R.default_params())
    o.setInputTarget(c["tgt"])
    lo, hi = c["tgt"].min(0), c["tgt"].max(0)
    rng = np.random.default_rng(SEED + 1)
    u = rng.uniform(1.0, 300.0, (24, 3))
    far = np.where(rng.random((24, 1)) < 0.5, hi + u, lo - u).astype(np.float32)   # (outside the target's box on every axis)
    q = np.concatenate([c["q"], far, lo[None], hi[None]]).astype(np.float32)
    qi, qd = o.knn_kdtree_batch("target", q, 1)
    checks = []
    for name in ("scan_with_outliers", "sixteen_scattered_waves"):
        src = c["src"][name]
        for T in (c["guess"], c["T_true"].astype(np.float32)):
            pt = O.transform_points_f32(T.astype(np.float64), src)
            checks.append((name, src, T, *o.knn_kdtree_batch("target", pt, 1)))
    for env in SEARCH_ENVS:
        h = _fast(reg, env, c["tgt"])
        idx, sqd = h.nearestNeighboursOf(q)
        assert np.array_equal(idx, qi[:, 0]) and np.array_equal(sqd.view(np.uint32), qd[:, 0].view(np.uint32)), env
        for name, src, T, wi, wd in checks:
            h.setInputSource(src)
            idx, sqd = h.nearestNeighbours(T)
            assert np.array_equal(idx, wi[:, 0]) and np.array_equal(sqd.view(np.uint32), wd[:, 0].view(np.uint32)), (env, name)
        del h
