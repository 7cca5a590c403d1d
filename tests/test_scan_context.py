"""Scan Context place recognition on the device (riv-slam_amd/scan_context.py, csrc/apd_scan_context.hpp) against radar_graph_slam::SCManager
(radar_graph_slam/src/radar_graph_slam/Scancontext.cpp).

The expected values come from tests/scan_context_np.py, a numpy restatement of include/apdgicp_hip.h's "Scan Context place recognition"
section (S1 .. S8).  Every device comparison is bit for bit: descriptors and ring keys as fp32 bits, sector keys, column norms and distances
as fp64 bits, ids, shifts and ranks as integers.  The one exception is the payload of a NaN distance, which IEEE 754 leaves open.
"""
import importlib
import math

import numpy as np
import pytest

import scan_context_np as snp
from scan_context_np import database_descriptors, fov_cloud

F32, F64 = np.float32, np.float64
NEW_SYMBOLS = ["apdgicp_scan_context_default_params", "apdgicp_scan_context_create", "apdgicp_scan_context_destroy", "apdgicp_scan_context_set_params",
               "apdgicp_scan_context_add", "apdgicp_scan_context_add_descriptor", "apdgicp_scan_context_clear", "apdgicp_scan_context_size",
               "apdgicp_scan_context_detect", "apdgicp_scan_context_detect_batch", "apdgicp_scan_context_descriptors"]
KNOBS = {"reference": dict(num_candidates=3, search_ratio=0.1), "exhaustive": dict(num_candidates=0, search_ratio=1.0)}
# fp32 points whose S1 angle is exactly -56.5 / the fp32 neighbours of +56.5 (atan2f's spacing near 2.56 rad is wider than the angle's, so
# +56.5 itself is not the image of any point on this ray; the exact upper gate is tested with azimuth_max set to a point's own angle)
P_MINUS_56_5 = (float.fromhex("0x1.613d5c0000000p+2"), float.fromhex("0x1.0ad7ec0000000p+3"))


def same_f32(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=F32).view(np.uint32), np.ascontiguousarray(b, dtype=F32).view(np.uint32))


def same_f64(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=F64).view(np.uint64), np.ascontiguousarray(b, dtype=F64).view(np.uint64))


def angle_of(x, y):
    """S1's fp32 angle of one point"""
    a = snp.anp.atan2f_fdlibm(np.array([x], dtype=F32), np.array([y], dtype=F32)).astype(F64)
    return (((a - F64(math.pi / 2)) * F64(180.0)) / F64(math.pi)).astype(F32)[0]


# ---------------------------------------------------------------------------------------------------------------- the restatement (no GPU)
def test_hand_computed_2x3_example():
    """S1: three points, one per bin; S2, S5, S6 on A = [[3, 0, 0], [4, 0, 1]] and B = shifted(A, 1), all by hand"""
    p = snp.Params(num_ring=2, num_sector=3, max_radius=10.0, azimuth_max=60.0, azimuth_min=-60.0)
    # (5, 0): range 5 -> ring 1, angle ~ +2.5e-6 (atan2f's pi/2 is above the double's) -> sector ceil(1.5 + tiny) = 2
    # (5, 5): range 7.07 -> ring 2, angle -45 -> sector ceil(0.375) = 1;  (5, -5): angle +45 -> sector ceil(2.625) = 3
    pts = np.array([[5, 0, 0, 7], [5, 5, 0, 8], [5, -5, 0, 9], [5, -5, 1, 4], [0, 5, 0, 99]], dtype=F32)   # the last: angle -90, outside
    assert np.array_equal(snp.make_descriptor(pts, p), [[0, 7, 0], [8, 0, 9]])
    A = np.array([[3, 0, 0], [4, 0, 1]], dtype=F32)
    rk, sk, cn = snp.keys_of(A)
    assert same_f32(rk, [F32(1.0), F32(F64(5.0) / F64(3.0))]) and same_f64(sk, [3.5, 0.0, 0.5]) and same_f64(cn, [5.0, 0.0, 1.0])
    B = snp.shifted(A, 1)
    assert np.array_equal(B, [[0, 3, 0], [1, 4, 0]])
    db = snp.ScanContextNP(p, search_ratio=1.0, num_exclude_recent=0)
    a, b = db.add_descriptor(A), db.add_descriptor(B)
    db._score(b, [a])
    align, table = db._table[(b, a)]
    # shift 0: only column 0 counts (1 * 5 norms, dot 4): 1 - 4/5; shift 1: columns 0 and 1 are equal: 1 - 2/2; shift 2: column 1: 1 - 4/5
    assert align == 1 and same_f64(table, [1.0 - 4.0 / 5.0, 0.0, 1.0 - 4.0 / 5.0])
    assert db.distance(b, a) == (0.0, 1)
    db.p.search_ratio = 0.0     # radius 0: the aligned shift only
    assert db.distance(b, a) == (0.0, 1)


def test_ring_and_sector_edges():
    p = snp.Params()
    xy = np.array([[80, 0], [2, 0], [0, 0], P_MINUS_56_5, [np.nextafter(F32(80), F32(100)), 0]], dtype=F32)
    keep, ring, sector = snp.bins_of(xy, p)
    assert angle_of(*P_MINUS_56_5) == F32(-56.5)
    # range exactly 80: kept, the last ring; exactly 2.0 = one ring width: the FIRST ring (ceil(1.0)); range 0: angle -90, outside the field of view;
    # angle exactly -56.5: kept (the gate is >), ceil(0) = 0 clamps to sector 1; the float above 80: outside
    assert keep.tolist() == [True, True, False, True, False]
    assert ring[0] == 40 and ring[1] == 1 and sector[3] == 1 and sector[0] == 11
    wide = snp.Params(azimuth_max=100.0, azimuth_min=-100.0)
    keep, ring, sector = snp.bins_of(np.array([[0, 0]], dtype=F32), wide)
    assert keep[0] and ring[0] == 1      # ceil(0) = 0 clamps to ring 1
    # the upper gate, exactly: azimuth_max = the point's own fp32 angle -> kept, sector S; one float below -> the point is outside
    a = float(angle_of(3.0, -4.0))
    assert 30.0 < a < 56.5
    for amax, kept in ((a, True), (float(np.nextafter(F32(a), F32(0))), False)):
        k, _, s = snp.bins_of(np.array([[3.0, -4.0]], dtype=F32), snp.Params(azimuth_max=amax, azimuth_min=-amax))
        assert bool(k[0]) == kept and (not kept or s[0] == 20)


def test_a_shifted_copy_is_found_at_its_shift_with_distance_zero():
    rng = np.random.default_rng(11)
    p = snp.Params(num_exclude_recent=0, num_candidates=0, search_ratio=1.0)
    A = rng.uniform(1.0, 60.0, (p.num_ring, p.num_sector)).astype(F32)
    db = snp.ScanContextNP(p)
    a = db.add_descriptor(A)
    for s in range(p.num_sector):
        q = db.add_descriptor(snp.shifted(A, s))
        dist, shift = db.distance(q, a)
        assert shift == s and abs(dist) <= 1e-15


def test_search_radius_is_c_round():
    assert snp.search_radius(0.1, 20) == 1 and snp.search_radius(1.0, 20) == 10
    assert snp.search_radius(0.1, 5) == 0 and snp.search_radius(0.1, 50) == 3 and round(2.5) == 2   # 0.5 * 0.1 * 50 = 2.5: C rounds it to 3
    assert snp.shift_set(0, 1, 20) == [0, 1, 19] and snp.shift_set(3, 10, 20) == list(range(20))


# ---------------------------------------------------------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def scm():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.scan_context")


def check_detection(scm, det, want):
    """a device Detection against the restatement's dict, bit for bit"""
    w = snp.matches_array(want["matches"], scm.MATCH_DTYPE)
    g = det.matches
    assert len(g) == len(w)
    for f in ("id", "shift", "ring_rank"):
        assert np.array_equal(g[f], w[f]), f
    assert same_f32(g["ring_d2"], w["ring_d2"])
    nan = np.isnan(w["distance"])
    assert np.array_equal(np.isnan(g["distance"]), nan) and same_f64(g["distance"][~nan], w["distance"][~nan])
    assert det.loop_id == want["loop_id"] and same_f32([det.yaw], [want["yaw"]])


def check_descriptors(sc, ref, first=0):
    got = sc.descriptors(first, len(ref) - first)
    assert same_f32(got["desc"], np.stack(ref.desc[first:])) and same_f32(got["ring_key"], np.stack(ref.ring_key[first:]))
    assert same_f64(got["sector_key"], np.stack(ref.sector_key[first:])) and same_f64(got["col_norm"], np.stack(ref.col_norm[first:]))


def edge_cloud(rng, n, p):
    """n points: random ones in and around the field of view, then (n permitting) points on ring and sector edges, on both gates, a NaN
    point, an infinite one, intensities below -1000, negative ones, and two equal intensities in one bin"""
    c = np.zeros((n, 4), dtype=F32)
    ang = np.deg2rad(rng.uniform(-75.0, 75.0, n) + 90.0)
    r = rng.uniform(0.0, 90.0, n)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = r * np.sin(ang), r * np.cos(ang), rng.normal(size=n), rng.uniform(-20.0, 60.0, n)
    w = p.max_radius / p.num_ring
    special = [(p.max_radius, 0.0, 0.0, 5.0), (w, 0.0, 0.0, 6.0), (3 * w, 0.0, 0.0, -7.0), (0.0, 0.0, 0.0, 8.0), (*P_MINUS_56_5, 0.0, 9.0),
               (float(np.nextafter(F32(p.max_radius), F32(1000))), 0.0, 0.0, 50.0), (np.nan, 1.0, 0.0, 70.0), (10.0, 1.0, 0.0, np.nan), (np.inf, 1.0, 0.0, 70.0),
               (20.0, 3.0, 0.0, -1000.0), (20.0, 3.0, 0.1, -2000.0), (33.0, -3.0, 0.0, -1000.5), (41.0, 7.0, 0.0, 12.5), (41.0, 7.0, 1.0, 12.5),
               (41.01, 7.0, 1.0, -0.0), (55.0, -20.0, 0.0, -3.0), (55.0, -20.0, 0.0, -0.0)]
    for sdeg in np.linspace(p.azimuth_min, p.azimuth_max, p.num_sector + 1):   # the sector edges, as close as fp32 gets
        a = math.radians(sdeg + 90.0)
        special.append((30.0 * math.sin(a), 30.0 * math.cos(a), 0.0, 22.0))
    k = min(len(special), max(n - 1, 0))
    if k:
        c[rng.choice(n, k, replace=False)] = np.array(special[:k], dtype=F32)
    return c


@pytest.mark.gpu
def test_new_symbols_are_exported(scm):
    L = scm.load_library()
    assert all(hasattr(L, s) for s in NEW_SYMBOLS)
    p = scm.default_params()
    assert (p.num_ring, p.num_sector, p.max_radius, p.azimuth_max, p.azimuth_min) == (40, 20, 80.0, 56.5, -56.5)
    assert (p.num_exclude_recent, p.num_candidates, p.search_ratio, p.dist_thresh) == (10, 3, 0.1, 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", [(40, 20), (20, 60)])
def test_descriptors_equal_the_restatement(scm, geometry):
    """clouds of 0, 1, 63, 64, 65 and 3000 points with every edge case of S1, host rows of 16 and 32 bytes, a device tensor, a cloud
    outside the field of view"""
    import torch
    R, S = geometry
    rng = np.random.default_rng(100 + R)
    sc = scm.ScanContext(num_ring=R, num_sector=S)
    ref = snp.ScanContextNP(num_ring=R, num_sector=S)
    for n in (0, 1, 63, 64, 65, 3000):
        c = edge_cloud(rng, n, ref.p)
        wide = np.zeros((n, 8), dtype=F32)      # pcl::PointXYZI: 32-byte rows, the intensity at byte 16
        wide[:, :3], wide[:, 4] = c[:, :3], c[:, 3]
        i = ref.add(c)
        assert sc.add(c) == i
        check_descriptors(sc, ref, i)
        others = [(wide, 4)] + ([(torch.from_numpy(c).cuda(), 3), (torch.from_numpy(wide).cuda(), 4)] if n else [(c[:, :3], 3), (wide, None)])
        for other, col in others:
            ref.add(c if n else np.zeros((0, 4), dtype=F32))
            j = sc.add(other, intensity_column=col)
            check_descriptors(sc, ref, j)
    assert len(sc) == len(ref) == 24 and np.count_nonzero(ref.desc[20]) > 50
    outside = fov_cloud(rng, 200, ref.p)
    outside[:, 0] = -outside[:, 0]      # behind the sensor
    i = ref.add(outside)
    assert sc.add(outside) == i and not ref.desc[i].any()
    xyz_only = fov_cloud(rng, 100, ref.p)[:, :3].copy()     # 12-byte rows: intensity 0 everywhere -> the zero descriptor
    i = ref.add(xyz_only)
    assert sc.add(xyz_only) == i and not ref.desc[i].any()
    check_descriptors(sc, ref, len(ref) - 2)
    with pytest.raises(scm.ApdgicpError):
        sc.set_params(num_ring=R + 1)       # S1 parameters are fixed while descriptors exist


@pytest.mark.gpu
def test_geometry_limits_are_refused(scm):
    for kw in (dict(num_ring=0), dict(num_ring=65), dict(num_sector=0), dict(num_sector=65)):
        with pytest.raises(Exception):
            scm.ScanContext(**kw)
    sc = scm.ScanContext(num_ring=64, num_sector=64)
    ref = snp.ScanContextNP(num_ring=64, num_sector=64, num_exclude_recent=0, num_candidates=0, search_ratio=1.0)
    sc.set_params(num_exclude_recent=0, num_candidates=0, search_ratio=1.0)
    rng = np.random.default_rng(64)
    for _ in range(4):
        c = fov_cloud(rng, 2000, ref.p)
        ref.add(c), sc.add(c)
    check_descriptors(sc, ref)
    check_detection(scm, sc.detect(3, [0, 1, 2], 3), ref.detect(3, [0, 1, 2], 3))


@pytest.fixture(scope="module")
def big(scm):
    """a database of 1100 descriptors on the device (it grows across two doublings past 256) and in the restatement; query 1099"""
    rng = np.random.default_rng(2024)
    sc, ref = scm.ScanContext(), snp.ScanContextNP()
    for d in database_descriptors(rng, 1100):
        assert sc.add_descriptor(d) == ref.add_descriptor(d)
    order = rng.permutation(1099)      # candidate lists are drawn from this: not ascending, some inside the 10-keyframe gap
    return sc, ref, order


@pytest.mark.gpu
def test_database_survives_capacity_doublings(big):
    sc, ref, _ = big
    assert len(sc) == 1100
    check_descriptors(sc, ref, 250)     # descriptors on both sides of the 256, 512 and 1024 boundaries


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("n", [1, 2, 3, 4, 63, 64, 65, 257, 1000])
def test_matching_equals_the_restatement(scm, big, knobs, n):
    sc, ref, order = big
    sc.set_params(**KNOBS[knobs])
    ref.p = snp.replace(ref.p, **KNOBS[knobs])
    far = order[order <= 1089]
    cand = np.concatenate([far[:n], order[order > 1089][:3]])     # n candidates that count + three inside the gap, which S3 drops
    cand = cand[np.random.default_rng(n).permutation(len(cand))]
    for top_k in (1, 3, n + 7):
        want = ref.detect(1099, cand, top_k)
        assert len(want["matches"]) == min(top_k, n if KNOBS[knobs]["num_candidates"] == 0 else min(n, 3))
        check_detection(scm, sc.detect(1099, cand, top_k), want)


@pytest.mark.gpu
def test_recent_queries_and_empty_candidate_sets(scm, big):
    sc, ref, _ = big
    sc.set_params(**KNOBS["reference"])
    ref.p = snp.replace(ref.p, **KNOBS["reference"])
    for q, cand in ((9, [0, 1, 2]), (5, []), (1099, [1095, 1090, 1098]), (1099, [])):
        det = sc.detect(q, cand, 3)
        assert det.loop_id == -1 and det.yaw == 0.0 and len(det.matches) == 0
    check_detection(scm, sc.detect(10, [1, 0, 2], 3), ref.detect(10, [1, 0, 2], 3))   # only keyframe 0 is 10 back
    for bad in ([0, 1100], [-1], [3, 4, 3]):
        with pytest.raises(Exception):
            sc.detect(1099, bad, 1)
    with pytest.raises(Exception):
        sc.detect(1100, [0], 1)


@pytest.mark.gpu
def test_crafted_descriptors(scm):
    rng = np.random.default_rng(77)
    R, S = 40, 20
    kw = dict(num_exclude_recent=0, num_candidates=0, search_ratio=1.0)
    sc, ref = scm.ScanContext(**kw), snp.ScanContextNP(**kw)

    def add(d):
        i = ref.add_descriptor(d)
        assert sc.add_descriptor(d) == i
        return i
    A = rng.integers(1, 60, (R, S)).astype(F32)                 # whole numbers: ring keys of permuted columns are EQUAL, not just close
    twin1, twin2 = add(A), add(A)                               # identical candidates: the tie goes to the ring-key rank
    same_key = [add(A[:, rng.permutation(S)]), add(np.sort(A, axis=1))]   # equal ring keys (the same row sums), other descriptors
    zero = add(np.zeros((R, S), dtype=F32))                     # all-zero columns: every shift NaN
    mixed = A.copy()
    mixed[:, ::3] = 0.0
    mixed = add(mixed)                                          # zero and non-zero columns
    period = np.tile(rng.uniform(1.0, 60.0, (R, S // 2)), (1, 2)).astype(F32)
    period = add(period)                                        # period S/2: shifts s and s + S/2 tie in the sector key AND the distance
    negzero = A.copy()
    negzero[3, 4] = -0.0
    negzero = add(negzero)
    shifts = [add(snp.shifted(A, s)) for s in range(S)]         # the query shifted by every s
    q = add(A)
    check_descriptors(sc, ref)
    assert not np.signbit(sc.descriptors(negzero, 1)["desc"]).any()
    cand = [twin2, twin1, *same_key, zero, mixed, period, negzero, *shifts]
    for knobs in KNOBS.values():
        sc.set_params(**knobs), setattr(ref, "p", snp.replace(ref.p, **knobs))
        want = ref.detect(q, cand, len(cand))
        check_detection(scm, sc.detect(q, cand, len(cand)), want)
    by_id = {m[0]: m for m in want["matches"]}                  # (exhaustive)
    assert np.isnan(by_id[zero][2]) and by_id[zero][1] == 0 and want["matches"][-1][0] == zero        # NaN last, shift 0
    assert by_id[twin2][2] == by_id[twin1][2] == 0.0 and by_id[twin2][4] < by_id[twin1][4]            # listed first -> lower rank -> first
    assert [by_id[i][1] for i in shifts] == [(S - s) % S for s in range(S)]                           # candidate = shifted(query, s): shift back
    assert by_id[same_key[0]][3] == by_id[same_key[1]][3] == by_id[twin1][3] == 0.0 and by_id[same_key[0]][2] > 0.01   # d2 ties, by position
    # the periodic descriptor against itself shifted by 3: shifts 3 and 13 tie exactly, the lower wins
    p2 = add(snp.shifted(ref.desc[period], 3))
    want = ref.detect(p2, [period], 1)
    assert want["matches"][0][1] == 3
    check_detection(scm, sc.detect(p2, [period], 1), want)
    # the zero descriptor as the QUERY: every candidate NaN, no loop, records still ranked by ring key
    zq = add(np.zeros((R, S), dtype=F32))
    want = ref.detect(zq, [twin1, mixed, period], 3)
    assert want["loop_id"] == -1 and len(want["matches"]) == 3 and all(np.isnan(m[2]) for m in want["matches"])
    check_detection(scm, sc.detect(zq, [twin1, mixed, period], 3), want)


@pytest.mark.gpu
def test_batch_equals_single_calls_and_a_cleared_handle_starts_again(scm, big):
    sc, ref, order = big
    sc.set_params(**KNOBS["exhaustive"])
    queries = [1099, 700, 5, 1098, 300]
    lists = [order[:70], order[order < 650][:9][::-1], order[:4], np.zeros(0, dtype=np.int32), order[order < 280][:130]]
    batch = sc.detect_batch(queries, lists, 5)
    for q, cand, got in zip(queries, lists, batch):
        one = sc.detect(q, cand, 5)
        assert got.matches.tobytes() == one.matches.tobytes() and got.loop_id == one.loop_id and same_f32([got.yaw], [one.yaw])
    ref.p = snp.replace(ref.p, **KNOBS["exhaustive"])
    check_detection(scm, batch[1], ref.detect(700, lists[1], 5))
    assert len(batch[2].matches) == 0 and len(batch[3].matches) == 0
    # a handle of its own, cleared and refilled with other descriptors (and another geometry, allowed while empty)
    rng = np.random.default_rng(5)
    mine, mref = scm.ScanContext(num_exclude_recent=2), snp.ScanContextNP(num_exclude_recent=2)
    for c in (fov_cloud(rng, 500) for _ in range(6)):
        mine.add(c), mref.add(c)
    check_detection(scm, mine.detect(5, [0, 1, 2, 3], 4), mref.detect(5, [0, 1, 2, 3], 4))
    mine.clear()
    assert len(mine) == 0
    mine.set_params(num_ring=24, num_sector=36)
    mref = snp.ScanContextNP(num_ring=24, num_sector=36, num_exclude_recent=2)
    for c in (fov_cloud(rng, 700) for _ in range(5)):
        assert mine.add(c) == mref.add(c)
    check_descriptors(mine, mref)
    check_detection(scm, mine.detect(4, [2, 0, 1], 4), mref.detect(4, [2, 0, 1], 4))


# ---------------------------------------------------------------------------------------------------------------- end to end
E2E_SEED = 3


def place_clouds(scene, seed=E2E_SEED, n=4096):
    """keyframes 0 .. 29: 24 random places (keyframes 24 .. 29 see places 0 .. 5 from 40 m further on: other views), keyframe 30 revisits
    place 4 within 0.5 m and 2 degrees.  A point's intensity is a smooth random function of where it lies, so that a revisit sees similar
    intensities; plus noise."""
    rng = np.random.default_rng(seed)
    scenes = [scene.Scene(np.random.default_rng(1000 * seed + i)) for i in range(24)]

    def view(i, T):
        pts = scene._observe(rng, scenes[i], T, n)
        ph = np.random.default_rng(77 * seed + i).uniform(0.0, 6.28, 3)
        world = pts.astype(F64) @ T[:3, :3].T + T[:3, 3]
        inten = 30.0 + 12.0 * np.sin(0.25 * world[:, 0] + ph[0]) + 12.0 * np.cos(0.2 * world[:, 1] + ph[1]) + rng.normal(size=n) * 0.5
        return np.concatenate([pts, inten[:, None].astype(F32)], axis=1).astype(F32)
    clouds = [view(i, np.eye(4)) for i in range(24)]
    clouds += [view(i, scene.make_transform([40.0, 5.0, 0.0], 0.4)) for i in range(6)]
    T = scene.make_transform([rng.uniform(-0.35, 0.35), rng.uniform(-0.35, 0.35), 0.0], np.deg2rad(rng.uniform(-2.0, 2.0)))
    assert np.linalg.norm(T[:3, 3]) <= 0.5
    clouds.append(view(4, T))
    return clouds


def restated_places(clouds):
    ref = snp.ScanContextNP()
    for c in clouds:
        ref.add(c)
    out = {}
    for name, knobs in KNOBS.items():
        ref.p = snp.replace(ref.p, **knobs)
        out[name] = ref.detect(30, list(range(30)), 4)
    return ref, out


def test_restatement_finds_the_revisited_place(scene):
    _, out = restated_places(place_clouds(scene))
    for name, det in out.items():
        assert det["loop_id"] == 4 and det["matches"][0][2] < 0.5, (name, det["matches"])


@pytest.mark.gpu
def test_end_to_end_top_k_into_the_loop_verifier(scm, scene):
    import torch
    reg = importlib.import_module("riv-slam_amd.registration")
    lv = importlib.import_module("riv-slam_amd.loop_verifier")
    clouds = place_clouds(scene)
    ref, out = restated_places(clouds)
    for det in out.values():
        assert det["loop_id"] == 4 and det["matches"][0][2] < 0.5
    sc = scm.ScanContext()
    for i, c in enumerate(clouds):
        assert sc.add(torch.from_numpy(c).cuda() if i % 2 else c) == i      # device-resident and host clouds alike
    check_descriptors(sc, ref)
    for name, knobs in KNOBS.items():
        sc.set_params(**knobs)
        check_detection(scm, sc.detect(30, list(range(30)), 4), out[name])
    # exhaustive knobs, top 4 into the batched verifier
    kw = dict(max_correspondence_distance=2.5, azimuth_variance_deg=1.0)
    batch = reg.BatchAPDGICP(reg.default_params(**kw))
    xyz = [np.ascontiguousarray(c[:, :3]) for c in clouds]
    loop, det, scores = scm.detect_and_verify(sc, batch, xyz, xyz[30], 30, list(range(30)), top_k=4, fitness_score_thresh=10.0)
    ids = [m[0] for m in out["exhaustive"]["matches"]]
    assert [int(i) for i in det.matches["id"]] == ids and len(ids) == 4 and len(scores) == 4
    direct, dscores, _ = lv.verify_candidates(reg.BatchAPDGICP(reg.default_params(**kw)), xyz[30], [xyz[i] for i in ids], fitness_score_thresh=10.0)
    print("scan context ids", ids, "fitness scores", scores, "yaw", det.yaw)
    assert loop is not None and loop.candidate == 4 and direct is not None and ids[direct.candidate] == 4
    te, re_ = scene.pose_error(direct.relative_pose, loop.relative_pose)
    assert te <= 1e-3 and re_ <= 1e-4
