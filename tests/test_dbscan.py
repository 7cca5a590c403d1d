"""DBSCAN clustering on the device (riv-slam_amd/dbscan.py, csrc/apd_dbscan.hpp): DBSCANSimpleCluster::extract
(radar_graph_slam/include/dbscan/DBSCAN_simple.h).

The expected values come from tests/dbscan_np.py: the reference's literal sequential loop (queue, states, noise marks) over a dense matrix of
radiusSearch's comparison, plus the tie rule of D7.  The device computes connected components, minima and counts instead (D3 - D6 of
include/apdgicp_hip.h); the two meet only in their results.

Bars (GPU): cnt, core flags, roots, primary seeds, final labels, CSR offsets and indices, table seeds / sizes / core counts: identical.  fp32
min / max and Doppler min / max: bit for bit.  Centroid and Doppler mean: within size * 2^-52 * max|value| over the cluster's members per column,
the bound of two fp64 sums of exactly representable terms in any order, each divided by the size.  Every case runs twice on one handle and once
on a fresh one: all outputs byte-equal (the union-find result does not depend on the order the atomics land in).
"""
import importlib

import numpy as np
import pytest

import dbscan_np as D

F32 = np.float32
NEW_SYMBOLS = ["apdgicp_dbscan_default_params", "apdgicp_dbscan_create", "apdgicp_dbscan_destroy", "apdgicp_dbscan_set_params", "apdgicp_dbscan_run", "apdgicp_dbscan_labels",
               "apdgicp_dbscan_copy_labels", "apdgicp_dbscan_clusters", "apdgicp_dbscan_members", "apdgicp_dbscan_debug"]


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration"), importlib.import_module("riv-slam_amd.dbscan")


def line(xs):
    return np.stack([np.asarray(xs, dtype=F32), np.zeros(len(xs), dtype=F32), np.zeros(len(xs), dtype=F32)], axis=1)


D5_X = [0, 0.25, 0.5, 0.75, 1.25, 1.75, 2.0, 2.25, 2.5]        # the seed of the second cluster (index 5, x = 1.75) is adjacent to point 4
D5_TWIN_X = [0, 0.25, 0.5, 0.75, 1.25, 2.0, 1.75, 2.25, 2.5]   # re-indexed: its seed is now x = 2.0, which is not


# ------------------------------------------------------------------ CPU
def test_restatement_on_the_seed_quirk_fixture():
    """D5: point 4 (a border of cluster 1, non-core) is adjacent to the seed of the later cluster and sits in both member lists; point 0 was
    marked noise by the outer loop before cluster 1 took it as a border point"""
    r = D.extract(line(D5_X), 0.5, min_pts=4)
    assert r["cnt"].tolist() == [3, 4, 4, 4, 3, 4, 4, 4, 3] and r["core"].tolist() == [False, True, True, True, False, True, True, True, False]
    assert [c.tolist() for c in r["clusters"]] == [[0, 1, 2, 3, 4], [4, 5, 6, 7, 8]] and r["seeds"].tolist() == [1, 5]
    assert r["primary"].tolist() == [1, 1, 1, 1, 1, 5, 5, 5, 5] and r["labels"].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    t = D.extract(line(D5_TWIN_X), 0.5, min_pts=4)
    assert [c.tolist() for c in t["clusters"]] == [[0, 1, 2, 3, 4], [5, 6, 7, 8]] and t["seeds"].tolist() == [1, 5]
    assert t["primary"].tolist() == [1, 1, 1, 1, 1, 5, 5, 5, 5]


def test_restatement_on_hand_fixtures():
    # D2: the point itself counts -- two points within eps are both core at minPts 2, a lone point is core at minPts 1
    r = D.extract(line([0, 0.4, 5.0]), 0.5, min_pts=2)
    assert r["cnt"].tolist() == [2, 2, 1] and [c.tolist() for c in r["clusters"]] == [[0, 1]] and r["labels"].tolist() == [0, 0, -1]
    r = D.extract(line([0, 0.4, 5.0]), 0.5, min_pts=1)
    assert [c.tolist() for c in r["clusters"]] == [[0, 1], [2]]
    # D1: <= is inclusive, in fp64 on the widened fp32 difference
    assert D.extract(line([0, 0.5]), 0.5, min_pts=2)["labels"].tolist() == [0, 0]
    assert D.extract(line([0, np.nextafter(F32(0.5), F32(1))]), 0.5, min_pts=2)["labels"].tolist() == [-1, -1]
    # D6 / D4: the first cluster is over max_cluster_size and is dropped WITH the border point 4 it took; the later cluster is kept without it
    r = D.extract(line(D5_TWIN_X), 0.5, min_pts=4, max_cluster_size=4)
    assert [c.tolist() for c in r["clusters"]] == [[5, 6, 7, 8]] and r["labels"].tolist() == [-1, -1, -1, -1, -1, 0, 0, 0, 0] and r["primary"][4] == 1
    # D7: larger first, equal sizes by ascending seed
    r = D.extract(line([10, 10.1, 0, 0.1, 0.2, 20, 20.1]), 0.15, min_pts=2)
    assert [c.tolist() for c in r["clusters"]] == [[2, 3, 4], [0, 1], [5, 6]] and r["seeds"].tolist() == [2, 0, 5]
    # a NaN point is adjacent to nothing: a singleton at minPts 1, noise otherwise
    r = D.extract(np.array([[0, 0, 0], [np.nan, 0, 0], [0.1, 0, 0]], dtype=F32), 0.5, min_pts=1)
    assert [c.tolist() for c in r["clusters"]] == [[0, 2], [1]]


def test_symbols_are_exported_and_defaults_are_the_references(mods):
    """fails without the feature: the library exports the apdgicp_dbscan_* entry points; the ABI version stays 6"""
    reg, db = mods
    L = reg.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in reg.SYMBOLS
    assert L.apdgicp_abi_version() == 6
    p = db.default_dbscan_params()   # DBSCAN_simple.h:111-114
    assert (p.eps, p.min_pts, p.min_cluster_size, p.max_cluster_size) == (0.0, 1, 1, 2**31 - 1)


def test_refused_parameters_need_no_device(mods):
    reg, db = mods
    for kw in (dict(min_pts=0), dict(min_cluster_size=0), dict(min_cluster_size=-3), dict(eps=float("nan")), dict(eps=float("inf")), dict(eps=-1.0), dict(max_cluster_size=0)):
        with pytest.raises(reg.ApdgicpError) as e:
            db.DBSCAN(**kw)
        assert e.value.code == -1
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(reg.ApdgicpError):   # no CPU fall-back
            db.DBSCAN(eps=0.5)


# ------------------------------------------------------------------ GPU
def snapshot(h):
    off, idx = h.members()
    dbg = h.debug()
    return dict(labels=h.labels(), off=off, idx=idx, table=h.clusters(), cnt=dbg["cnt"], core=dbg["core"], root=dbg["root"], primary=dbg["primary"])


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in a)


def check(db, xyz, eps, doppler=None, **kw):
    """the device against the restatement, run twice on one handle and once on a fresh one"""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    ref = D.extract(xyz, eps, **kw)
    h = db.DBSCAN(eps=eps, **kw)
    K = h.run(xyz, doppler)
    got = snapshot(h)
    assert h.run(xyz, doppler) == K and same_bytes(got, snapshot(h))
    h2 = db.DBSCAN(eps=eps, **kw)
    assert h2.run(xyz, doppler) == K and same_bytes(got, snapshot(h2))
    n = len(xyz)
    assert K == len(ref["clusters"])
    assert np.array_equal(got["cnt"], ref["cnt"]) and np.array_equal(got["core"], ref["core"])
    assert np.array_equal(got["root"], np.where(ref["core"], ref["primary"], -1)) and np.array_equal(got["primary"], ref["primary"])
    assert np.array_equal(got["labels"], ref["labels"]) and got["labels"].shape == (n,)
    sizes = [len(c) for c in ref["clusters"]]
    assert np.array_equal(got["off"], np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
    assert np.array_equal(got["idx"], np.concatenate(ref["clusters"]) if K else np.zeros(0, dtype=np.int32))
    t, want = got["table"], D.table(xyz, ref, ref["core"], doppler)
    assert np.array_equal(t["seed"], want["seed"]) and np.array_equal(t["size"], want["size"]) and np.array_equal(t["n_core"], want["n_core"])
    assert t["min"].tobytes() == want["min"].tobytes() and t["max"].tobytes() == want["max"].tobytes()
    assert t["doppler_min"].tobytes() == want["doppler_min"].tobytes() and t["doppler_max"].tobytes() == want["doppler_max"].tobytes()
    for r, m in enumerate(ref["clusters"]):
        cols = [(t["centroid"][r, a], want["centroid"][r, a], xyz[m, a]) for a in range(3)]
        if doppler is not None:
            cols.append((t["doppler_mean"][r], want["doppler_mean"][r], np.asarray(doppler, dtype=F32)[m]))
        for g, w, v in cols:
            if np.isfinite(v).all():
                assert abs(g - w) <= len(m) * 2.0**-52 * float(np.abs(v).max())
            else:
                assert np.array_equal(g, w, equal_nan=True)
    if doppler is None:
        assert not t["doppler_mean"].any() and not t["doppler_min"].any() and not t["doppler_max"].any()
    return ref, got


@pytest.mark.gpu
def test_tiny_clouds_and_min_pts_one(mods):
    """n = 0, 1, 2; minPts = 1: every point is core, a NaN point a singleton cluster"""
    _, db = mods
    h = db.DBSCAN(eps=0.5)
    assert h.run(np.zeros((0, 3), dtype=F32)) == 0 and h.labels().shape == (0,) and h.members()[0].tolist() == [0] and len(h.clusters()) == 0
    for mp in (1, 2):
        check(db, line([0.25]), 0.5, min_pts=mp)
        check(db, line([0.25, 0.5]), 0.5, min_pts=mp)
        check(db, line([0.25, 5.0]), 0.5, min_pts=mp)
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [0.1, 0, 0], [0, np.inf, 0], [3, 3, 3], [0, 0, -np.inf]], dtype=F32)
    ref, _ = check(db, pts, 0.5, min_pts=1)
    assert sorted(len(c) for c in ref["clusters"]) == [1, 1, 1, 1, 2]


@pytest.mark.gpu
def test_seed_quirk_and_its_twin(mods):
    """D5: the fixture lists point 4 twice, its twin (the second cluster's seed re-indexed away from point 4) once"""
    _, db = mods
    ref, got = check(db, line(D5_X), 0.5, min_pts=4)
    assert np.count_nonzero(np.concatenate(ref["clusters"]) == 4) == 2 and got["off"].tolist() == [0, 5, 10]
    ref, got = check(db, line(D5_TWIN_X), 0.5, min_pts=4)
    assert np.bincount(np.concatenate(ref["clusters"])).max() == 1 and got["off"].tolist() == [0, 5, 9]
    # the same two in 3-D, turned out of the axes and shifted into negative coordinates
    R = np.linalg.qr(np.random.default_rng(4).normal(size=(3, 3)))[0]
    for xs in (D5_X, D5_TWIN_X):
        check(db, (line(xs).astype(np.float64) @ R.T - 1.0).astype(F32), 0.5001, min_pts=4)


@pytest.mark.gpu
def test_discarded_cluster_keeps_its_border_point(mods):
    """D4 / D6: the first cluster is over max_cluster_size; the border point it took from the later, kept cluster is lost with it"""
    _, db = mods
    ref, got = check(db, line(D5_TWIN_X), 0.5, min_pts=4, max_cluster_size=4)
    assert got["labels"].tolist() == [-1, -1, -1, -1, -1, 0, 0, 0, 0] and got["primary"][4] == 1
    check(db, line(D5_X), 0.5, min_pts=4, max_cluster_size=4)       # both are of size 5: nothing is kept
    check(db, line(D5_X), 0.5, min_pts=4, min_cluster_size=6)
    check(db, line(D5_TWIN_X), 0.5, min_pts=4, min_cluster_size=5)  # only the first


@pytest.mark.gpu
@pytest.mark.parametrize("eps", [0.25, 0.5])
def test_exact_threshold_on_a_lattice(mods, eps):
    """coordinates in multiples of 0.25 (negative ones too): distances exactly equal to eps occur in every direction, duplicates as well"""
    _, db = mods
    rng = np.random.default_rng(7)
    pts = (rng.integers(-6, 7, (700, 3)) * 0.25).astype(F32)
    ref, _ = check(db, pts, eps, min_pts=4)
    a = D.adjacency(pts, eps)
    d = pts[None, :, 0].astype(np.float64) - pts[:, None, 0]
    assert (a & (np.abs(d) == eps)).any() and len(np.unique(pts, axis=0)) < len(pts) and len(ref["clusters"]) >= 1
    check(db, pts, eps, min_pts=7, min_cluster_size=3)


@pytest.mark.gpu
def test_pairs_one_ulp_either_side_of_eps(mods):
    """pairs at eps - 1 ulp, eps, eps + 1 ulp (fp32) along every axis, from bases just below / on / above cell boundaries k * h (h = eps (1 + 2^-20))
    and in negative coordinates; minPts 2 makes every accepted pair a cluster"""
    _, db = mods
    eps = 0.3
    h = eps * (1.0 + 2.0**-20)
    pts = []
    slot = 0
    for k in (0, 1, 7, -1, -8, 1000, -1000):
        for db_ in (-1, 0, 1):
            base = F32(k * h)
            for _ in range(abs(db_)):
                base = np.nextafter(base, F32(np.inf) if db_ > 0 else F32(-np.inf))
            for du in (-1, 0, 1):
                for sign in (1.0, -1.0):
                    other = F32(np.float64(base) + sign * eps)
                    for _ in range(abs(du)):
                        other = np.nextafter(other, F32(np.inf) if du * sign > 0 else F32(-np.inf))
                    for axis in range(3):
                        off = np.zeros(3, dtype=F32)
                        off[(axis + 1) % 3] = F32(10.0 * eps * slot)   # every pair on a line of its own
                        slot += 1
                        a, b = off.copy(), off.copy()
                        a[axis], b[axis] = base, other
                        pts += [a, b]
    pts = np.array(pts, dtype=F32)
    ref, _ = check(db, pts, eps, min_pts=2)
    assert 0 < len(ref["clusters"]) < len(pts) // 2    # some pairs are accepted, some are not


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1025])
def test_many_points_in_one_cell(mods, n):
    """all points inside one grid cell (wave and block edges), some pairs beyond eps; a duplicated point among them"""
    _, db = mods
    rng = np.random.default_rng(n)
    pts = (0.05 + rng.random((n, 3)) * 0.9).astype(F32)   # cell side ~ 1
    pts[n // 2] = pts[0]
    ref, _ = check(db, pts, 1.0, min_pts=int(0.85 * n))   # a point in the middle sees everyone, one in a corner about 72 %
    assert 0 < np.count_nonzero(ref["core"]) < n and len(ref["clusters"]) == 1 and len(ref["clusters"][0]) == n
    check(db, pts, 1.0, min_pts=1)


@pytest.mark.gpu
def test_snake_of_2048_points(mods):
    """one chain at spacing 0.9 eps winding through space, indices shuffled: a single component with a deep union-find tree"""
    _, db = mods
    rng = np.random.default_rng(5)
    eps, n = 0.2, 2048
    s = np.arange(n) * 0.9 * eps
    curve = np.stack([4.0 * np.cos(s / 4.0), 4.0 * np.sin(s / 4.0), s / 12.0], axis=1)   # a helix of radius 4: arc length ~ s, turns 2.1 apart
    pts = curve[rng.permutation(n)].astype(F32)
    ref, got = check(db, pts, eps, min_pts=3)
    assert len(ref["clusters"]) == 1 and len(ref["clusters"][0]) == n and np.count_nonzero(ref["core"]) == n - 2


@pytest.mark.gpu
def test_blobs_with_noise_and_equal_sizes(mods):
    """3 000 points: 20 blobs + uniform noise, with a Doppler lane; then equal-size clusters (D7) from copies of one blob"""
    _, db = mods
    rng = np.random.default_rng(9)
    centres = rng.uniform(-20, 20, (20, 3))
    blobs = [c + 0.3 * rng.normal(size=(int(k), 3)) for c, k in zip(centres, rng.integers(60, 200, 20))]
    pts = np.concatenate(blobs)
    pts = np.concatenate([pts, rng.uniform(-25, 25, (3000 - len(pts), 3))]).astype(F32)
    pts = pts[rng.permutation(len(pts))]
    dop = rng.normal(size=len(pts)).astype(F32) * 5
    ref, _ = check(db, pts, 0.35, doppler=dop, min_pts=5, min_cluster_size=10)
    assert 10 <= len(ref["clusters"]) <= 40 and np.count_nonzero(ref["labels"] < 0) > 100
    one = (0.2 * rng.normal(size=(30, 3))).astype(F32)
    copies = np.concatenate([one + F32(8.0) * np.array(s, dtype=F32) for s in ((2, 0, 0), (0, 0, 0), (-1, 0, 0), (0, -3, 0))])
    ref, got = check(db, copies[rng.permutation(len(copies))], 0.3, min_pts=3)
    sizes = got["table"]["size"]
    assert (np.diff(sizes) <= 0).all() and any(sizes[i] == sizes[i + 1] and got["table"]["seed"][i] < got["table"]["seed"][i + 1] for i in range(len(sizes) - 1))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_blobs_around_one_radix_tile(mods, n):
    """24 blobs of 150 points + uniform noise around 4096 points, the tile of the radix sort: the cell sort and the rank sort run over one tile
    (4095, 4096) or two (4097); the member sort runs over M != n pairs"""
    _, db = mods
    rng = np.random.default_rng(11)
    centres = rng.uniform(-20, 20, (24, 3))
    pts = np.concatenate([c + 0.3 * rng.normal(size=(150, 3)) for c in centres])
    pts = np.concatenate([pts, rng.uniform(-25, 25, (n - len(pts), 3))]).astype(F32)
    pts = pts[rng.permutation(n)]
    ref, got = check(db, pts, 0.4, min_pts=4, min_cluster_size=5, max_cluster_size=400)
    M = len(got["idx"])
    print("clusters:", len(ref["clusters"]), "members:", M)
    assert len(ref["clusters"]) >= 12 and 12 * 100 <= M < n


@pytest.mark.gpu
def test_non_finite_rows_in_the_middle(mods):
    _, db = mods
    rng = np.random.default_rng(13)
    pts = rng.uniform(-2, 2, (500, 3)).astype(F32)
    pts[100, 0], pts[101, 1], pts[250, 2], pts[251] = np.nan, np.inf, -np.inf, np.nan
    ref, _ = check(db, pts, 0.4, min_pts=4)
    assert (ref["labels"][[100, 101, 250, 251]] == -1).all() and len(ref["clusters"]) >= 1
    check(db, pts, 0.4, min_pts=1, min_cluster_size=1)


@pytest.mark.gpu
def test_point_outside_the_grid_is_refused_and_the_handle_stays_usable(mods):
    reg, db = mods
    pts = np.random.default_rng(1).uniform(-1, 1, (300, 3)).astype(F32)
    bad = pts.copy()
    bad[41, 1] = 0.25 * 2**20 * 1.001      # just past 2^20 cells of side ~0.25
    bad[77, 0] = -1e30
    h = db.DBSCAN(eps=0.25, min_pts=3)
    with pytest.raises(reg.ApdgicpError) as e:
        h.run(bad)
    assert e.value.code == -5 and "point 41 " in str(e.value) and h.n == 0 and h.labels().shape == (0,)
    K = h.run(pts)
    ref = D.extract(pts, 0.25, min_pts=3)
    assert K == len(ref["clusters"]) and np.array_equal(h.labels(), ref["labels"])
    inside = pts.copy()
    inside[41, 1] = 0.25 * (2**20 - 2)     # the last cells inside
    assert h.run(inside) == len(D.extract(inside, 0.25, min_pts=3)["clusters"])


@pytest.mark.gpu
def test_device_input_equals_host_input(mods):
    """a [n, 8] device tensor (32-byte rows, Doppler a strided column of it) against contiguous host arrays"""
    import torch
    _, db = mods
    rng = np.random.default_rng(17)
    rows = rng.uniform(-3, 3, (1500, 8)).astype(F32)
    h = db.DBSCAN(eps=0.45, min_pts=5)
    K = h.run(np.ascontiguousarray(rows[:, :3]), np.ascontiguousarray(rows[:, 5]))
    want = snapshot(h)
    t = torch.from_numpy(rows).cuda()
    assert h.run(t, t[:, 5]) == K and same_bytes(want, snapshot(h)) and K >= 1
    assert h.run(rows, rows[:, 5].copy()) == K and same_bytes(want, snapshot(h))   # 32-byte host rows
    ptr, n = h.labels_device()
    assert n == 1500 and ptr != 0


def moving_scan(scene, seed=3):
    """a static scan seen from a moving sensor plus two compact objects with a velocity of their own"""
    base = scene.raw_doppler_scan(3000, seed, moving_share=0.0, outlier_share=0.0)
    rng = np.random.default_rng([seed, 0xDB])
    v_sensor = np.array([2.0, 0.3, -0.1])
    objs = []
    for centre, v_obj in (((12.0, 3.0, 0.5), (6.0, 0.0, 0.0)), ((20.0, -5.0, 0.2), (-8.0, 1.0, 0.0))):
        p = np.asarray(centre) + 0.25 * rng.normal(size=(40, 3))
        u = p / np.linalg.norm(p, axis=1, keepdims=True)
        dop = -(u * (v_sensor + np.asarray(v_obj))).sum(axis=1) + rng.normal(0.0, 0.02, 40)
        objs.append(np.concatenate([p, np.full((40, 1), 30.0), dop[:, None]], axis=1))
    scan = np.concatenate([base.astype(np.float64)] + objs).astype(F32)
    return np.ascontiguousarray(scan[rng.permutation(len(scan))])


@pytest.mark.gpu
def test_cluster_moving_points_from_an_ego_velocity_run(mods, scene):
    """ego velocity -> its outlier cloud (device pointers) -> clusters: labels and table equal the restatement on the copied outlier cloud"""
    _, db = mods
    ev = importlib.import_module("riv-slam_amd.ego_velocity")
    sf = importlib.import_module("riv-slam_amd.scan_filter")
    scan = moving_scan(scene)
    est = ev.EgoVelocityEstimator()
    res = est.run(scan, seed=1)
    out = est.to_numpy("outliers")
    print("ego:", res.success, res.m, res.n_inlier, res.n_outlier)
    assert res.success and res.n_outlier >= 60
    h = db.DBSCAN(eps=0.6, min_pts=5, min_cluster_size=10)
    K = db.cluster_moving_points(est, h)
    ref = D.extract(out["xyzi"][:, :3], 0.6, min_pts=5, min_cluster_size=10)
    want = D.table(out["xyzi"][:, :3], ref, ref["core"], out["doppler"])
    t = h.clusters()
    print("clusters:", K, t["size"], t["doppler_mean"])
    assert K == len(ref["clusters"]) >= 2 and np.array_equal(h.labels(), ref["labels"]) and np.array_equal(t["size"], want["size"])
    assert np.array_equal(h.members()[1], np.concatenate(ref["clusters"]))
    for r in range(K):
        assert abs(t["doppler_mean"][r] - want["doppler_mean"][r]) <= t["size"][r] * 2.0**-52 * np.abs(out["doppler"][ref["clusters"][r]]).max()
    assert t["doppler_min"].tobytes() == want["doppler_min"].tobytes() and t["doppler_max"].tobytes() == want["doppler_max"].tobytes()
    big = t[:2]   # the two objects: 40 points each around (12, 3, 0.5) and (20, -5, 0.2), radial speeds far from the static scene's
    assert (big["size"] >= 30).all() and sorted(np.round(big["centroid"][:, 0]).tolist()) == [12.0, 20.0] and (np.abs(big["doppler_mean"]) > 3.0).all()
    # the radius filter of preprocessing_nodelet.cpp:766-774 in front: the filtered cloud (no Doppler lane) is what gets clustered
    f = sf.ScanFilter(use_distance_filter=0, leaf=None, outlier_method="RADIUS", radius=0.8, min_neighbors=2)
    K2 = db.cluster_moving_points(est, h, scan_filter=f)
    kept = f.to_numpy()
    ref2 = D.extract(kept[:, :3], 0.6, min_pts=5, min_cluster_size=10)
    assert K2 == len(ref2["clusters"]) >= 2 and np.array_equal(h.labels(), ref2["labels"]) and not h.clusters()["doppler_mean"].any()
