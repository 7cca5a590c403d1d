"""Exact k-nearest and radius queries of the target on the device (apdgicp_knn_of, apdgicp_radius_search_of / _rows; Q1 .. Q9 of
include/apdgicp_hip.h) against the numpy restatement tests/search_np.py.  Everything is compared as bytes: indices, the bit patterns of
the distances, row_start, total, n_found.  The restatement computes a row from the whole target at once, so nothing here follows the
order the kernels visit the target in.

Sizes: targets of 1, 15, 16, 17 (one chunk and its edges), 127, 128, 129 (one group and its edges), 2 049 (the first size of the tiled
cloud sort) and 20 000 points (the generic sort: super boxes); 1, 63, 64, 65, 129 and 3 000 queries (one wave and its edges, several
blocks), which is more queries than most of the targets have points.  The reference of a (target, query set) pair is computed once,
for k = 64, and its row prefixes serve every smaller k and every prefix of the query set (Q8)."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_np as S  # noqa: E402

gpu = pytest.mark.gpu
F32 = np.float32
INVALID_ARG, NO_INPUT, UNSUPPORTED = -1, -3, -5
TARGET_SIZES = (1, 15, 16, 17, 127, 128, 129, 2049, 20000)
QUERY_COUNTS = (1, 63, 64, 65, 129, 3000)
KS = (1, 2, 5, 20, 63, 64)
LM = dict(max_correspondence_distance=2.0, transformation_epsilon=0.1, azimuth_variance_deg=1.0)


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def make_target(m, seed=7):
    """m points in a 20 x 20 x 4 m slab (a scan's shape), float32"""
    return (np.random.default_rng(seed + m).random((m, 3)) * np.array([20.0, 20.0, 4.0])).astype(F32)


def make_queries(t, n=3000, seed=99):
    """inside the target's box, 1 000 m outside it, on target points (d2 = 0), duplicated -- shuffled, so that every prefix holds every kind"""
    rng = np.random.default_rng(seed)
    inside = (rng.random((n, 3)) * np.array([20.0, 20.0, 4.0])).astype(F32)
    k = max(n // 10, 1)
    far = (inside[:k] + F32(1000.0) * rng.choice([-1.0, 1.0], (k, 3))).astype(F32)
    on = t[rng.integers(0, len(t), k)]
    q = np.concatenate([inside[: n - 4 * k], far, on, inside[:k], inside[:k]]).astype(F32)
    return q[rng.permutation(len(q))]


_REF = {}


def knn_ref(m):
    """(target, queries, restatement at k = 64) of target size m, computed once"""
    if m not in _REF:
        t = make_target(m)
        q = make_queries(t)
        _REF[m] = (t, q, S.knn(q, t, 64))
    return _REF[m]


def handle(reg, tgt, **kw):
    g = reg.FastAPDGICP(reg.default_params(**kw))
    g.setInputTarget(tgt)
    return g


def check_knn(g, q, t, k, ref):
    """device rows of q at k against the k = 64 reference rows of the same queries"""
    ri, rd, _ = ref
    idx, sqd = g.nearestKSearchOf(q, k)
    nf = min(k, len(t))
    assert g.last_n_found == nf
    want_i = np.full((len(q), k), -1, dtype=np.int32)
    want_d = np.full((len(q), k), np.inf, dtype=F32)
    want_i[:, :nf], want_d[:, :nf] = ri[: len(q), :nf], rd[: len(q), :nf]
    assert same(sqd.view(np.uint32), want_d.view(np.uint32)), (len(t), len(q), k)
    assert same(idx, want_i), (len(t), len(q), k)


# ------------------------------------------------------------------------------------------------------------------------ k nearest
@gpu
@pytest.mark.parametrize("m", TARGET_SIZES)
def test_knn_of_every_size_and_k(reg, m):
    """Q2: every target size x every query count x every k, tails of -1 / +Inf where k > M, n_found = min(k, M)"""
    t, q, ref = knn_ref(m)
    g = handle(reg, t)
    for nq in QUERY_COUNTS:
        for k in KS:
            check_knn(g, q[:nq], t, k, ref)
    on = t[np.arange(0, m, max(m // 50, 1))]
    idx, sqd = g.nearestKSearchOf(on, 1)
    assert (sqd == 0).all()                                   # queries on target points
    assert same(t[idx[:, 0]], on)


@gpu
def test_knn_of_16_byte_stride_and_q9_k1(reg):
    """Q3: 16-byte rows (the fourth float is not a coordinate, not even a NaN there); Q9: k = 1 is nearestNeighboursOf, byte for byte"""
    t, q, ref = knn_ref(2049)
    g = handle(reg, t)
    q16 = np.full((len(q), 4), np.nan, dtype=F32)
    q16[:, :3] = q
    i12, d12 = g.nearestKSearchOf(q, 5)
    i16, d16 = g.nearestKSearchOf(q16, 5)
    assert same(i12, i16) and same(d12.view(np.uint32), d16.view(np.uint32))
    check_knn(g, q, t, 5, ref)
    for m in (17, 2049, 20000):
        t, q, _ = knn_ref(m)
        g = handle(reg, t)
        i1, d1 = g.nearestNeighboursOf(q)
        ik, dk = g.nearestKSearchOf(q, 1)
        assert same(ik[:, 0], i1) and same(dk[:, 0].view(np.uint32), d1.view(np.uint32))


def lattice(nx, ny, nz):
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F32)


@gpu
@pytest.mark.parametrize("which", ["lattice", "tripled"])
def test_knn_and_radius_with_ties(reg, which):
    """An integer lattice (12 x 12 x 6: every distance an integer or a multiple of 1/4, shared by many points) and a cloud with every
    point stored three times at shuffled indices (2 100 points): what a non-strict skip or a wrong tie rule gets wrong.  Queries on
    lattice points, at cell centres and at face centres."""
    rng = np.random.default_rng(5)
    if which == "lattice":
        t = lattice(12, 12, 6)
        q = np.concatenate([t[::7], t[::11] + F32(0.5), t[::13] + np.array([0.5, 0.0, 0.0], dtype=F32)])
    else:
        base = make_target(700, seed=3)
        t = np.concatenate([base, base, base])[rng.permutation(2100)]
        q = np.concatenate([base[::3], make_queries(base, 300, seed=4)])
    g = handle(reg, t)
    ref = S.knn(q, t, 64)
    for k in KS:
        check_knn(g, q, t, k, ref)
    for radius, max_nn in ((1.0, 0), (1.5, 0), (1.5, 7), (2.0, 64), (0.5, 0), (1.0, 1)):
        got = g.radiusSearchOf(q, radius, max_nn)
        want = S.radius_search(q, t, radius, max_nn)
        assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[2].view(np.uint32), want[2].view(np.uint32)), (radius, max_nn)


# ------------------------------------------------------------------------------------------------------------------------ radius
def check_radius(g, q, t, radius, max_nn):
    got = g.radiusSearchOf(q, radius, max_nn)
    want = S.radius_search(q, t, radius, max_nn)
    assert same(got[0], want[0]), (len(t), len(q), radius, max_nn)
    assert same(got[1], want[1]) and same(got[2].view(np.uint32), want[2].view(np.uint32)), (len(t), len(q), radius, max_nn)
    return got


_RREF = {}


def radius_rows_ref(m, radius):
    """the restatement's full rows (max_nn = 0) of target size m's query set, computed once"""
    if (m, radius) not in _RREF:
        t, q, _ = knn_ref(m)
        _RREF[(m, radius)] = S.radius_search(q, t, radius, 0)
    return _RREF[(m, radius)]


def cut_rows(ref, nq, max_nn, m):
    """Q5 / Q8 applied to restated full rows: the first nq rows, each cut to its max_nn smallest while 0 < max_nn < M"""
    rs, idx, dist = ref
    lim = max_nn if 0 < max_nn < m else 1 << 62
    pieces = [(idx[a:min(b, a + lim)], dist[a:min(b, a + lim)]) for a, b in zip(rs[:nq], rs[1:nq + 1])]
    out = np.zeros(nq + 1, dtype=np.int64)
    out[1:] = np.cumsum([len(p[0]) for p in pieces])
    return out, np.concatenate([p[0] for p in pieces]), np.concatenate([p[1] for p in pieces])


@gpu
@pytest.mark.parametrize("m", TARGET_SIZES)
def test_radius_search_every_size(reg, m):
    """Q4 / Q5 / Q6 at every target size: r = 0 (no hit, not even on a target point), a radius with short rows and empty rows (the
    far queries), max_nn = 0, 1, 7, 64 and one above 64 and below M, every query count"""
    t, q, _ = knn_ref(m)
    g = handle(reg, t)
    on = t[:: max(m // 20, 1)]
    rs, idx, sqd = g.radiusSearchOf(on, 0.0)
    assert not rs.any() and len(idx) == 0 and len(sqd) == 0
    ref = radius_rows_ref(m, 1.2)
    assert same(cut_rows(ref, 65, 7, m)[1], S.radius_search(q[:65], t, 1.2, 7)[1])      # (the cut is the restatement's own)
    for nq in QUERY_COUNTS:
        for max_nn in (0, 1, 7, 64, 100):
            got = g.radiusSearchOf(q[:nq], 1.2, max_nn)
            want = cut_rows(ref, nq, max_nn, m)
            assert same(got[0], want[0]), (m, nq, max_nn)
            assert same(got[1], want[1]) and same(got[2].view(np.uint32), want[2].view(np.uint32)), (m, nq, max_nn)
        if nq >= 63:
            assert (np.diff(got[0]) == 0).any()               # rows of length 0 among them
    far = q[:64] + F32(5000.0)
    rs, idx, sqd = g.radiusSearchOf(far, 3.0)                 # total = 0
    assert same(rs, np.zeros(65, dtype=np.int64)) and len(idx) == 0


def _one_ulp_inside(r2):
    """(x, y) float32 with fl(fl(x x) + fl(y y)) == the float just below r2"""
    want = np.nextafter(F32(r2), F32(0))
    x0 = np.sqrt(F32(r2))
    for i in range(1, 64):
        x = x0
        for _ in range(i):
            x = np.nextafter(x, F32(0))
        gap = np.float64(want) - np.float64(F32(x * x))
        if gap < 0:
            continue
        y0 = F32(np.sqrt(gap))
        for y in (y0, np.nextafter(y0, F32(0)), np.nextafter(y0, F32(1)), F32(0)):
            if F32(F32(x * x) + F32(y * y)) == want:
                return x, y
    raise AssertionError("no representable pair found")


@gpu
def test_radius_boundary_is_strict(reg):
    """Q4: a target point at exactly d2 == r2 is excluded, one a single ulp inside is included; r2 is the float of the double square.
    The coordinates are representable and the distances are checked here with the restatement's arithmetic before the device is asked."""
    radius = 0.5
    r2 = S.r2_of(radius)
    assert r2 == F32(0.25)
    x, y = _one_ulp_inside(r2)
    filler = make_target(300, seed=21) + F32(50.0)            # (other groups, far away)
    t = np.concatenate([[[0.5, 0.0, 0.0]], [[x, y, 0.0]], [[0.0, -0.5, 0.0]], filler]).astype(F32)
    q = np.zeros((1, 3), dtype=F32)
    d = S.sqdist_f32(q, t)[0]
    assert d[0] == r2 and d[2] == r2 and d[1] == np.nextafter(r2, F32(0))
    g = handle(reg, t)
    rs, idx, sqd = check_radius(g, q, t, radius, 0)
    assert rs.tolist() == [0, 1] and idx.tolist() == [1] and sqd[0] == np.nextafter(r2, F32(0))
    rs, idx, _ = check_radius(g, q, t, radius, 5)           # the bounded kernel takes the same decision
    assert rs.tolist() == [0, 1] and idx.tolist() == [1]
    # a radius whose double square is not a float: 0.3 -> r2 = float(0.09)
    check_radius(g, t[:50] + F32(0.01), t, 0.3, 0)
    # one float up, the two boundary points are inside
    rs, idx, _ = check_radius(g, q, t, float(np.sqrt(np.float64(np.nextafter(r2, F32(1))))) + 1e-9, 0)
    assert sorted(idx.tolist()) == [0, 1, 2]


@gpu
@pytest.mark.parametrize("m,nq", [(129, 65), (2049, 65), (20000, 3)])
def test_radius_covering_the_whole_target(reg, m, nq):
    """max_nn = 0 (and max_nn >= M) with a radius that covers everything: every row is all M points in key order"""
    t, q, _ = knn_ref(m)
    q = q[:nq]
    g = handle(reg, t)
    for max_nn in (0, m, m + 5):
        rs, idx, sqd = g.radiusSearchOf(q, 5000.0, max_nn)
        assert same(rs, np.arange(nq + 1, dtype=np.int64) * m)
        ky = np.sort(S.keys(q, t), axis=1)
        wi, wd = S._split(ky.ravel())
        assert same(idx, wi) and same(sqd.view(np.uint32), wd.view(np.uint32))


@gpu
@pytest.mark.parametrize("max_nn", [1, 7, 64])
def test_q9_bounded_radius_is_the_head_of_knn(reg, max_nn):
    """Q9 on the device's own answers: radius rows with 0 < max_nn <= 64 are the entries of knn_of(k = max_nn) that pass Q4"""
    t, q, _ = knn_ref(2049)
    g = handle(reg, t)
    ki, kd = g.nearestKSearchOf(q, max_nn)
    for radius in (0.4, 1.2):
        rs, ri, rd = g.radiusSearchOf(q, radius, max_nn)
        keep = kd < S.r2_of(radius)
        assert same(np.diff(rs), keep.sum(1).astype(np.int64))
        assert same(ri, ki[keep]) and same(rd.view(np.uint32), kd[keep].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------ Q8
@gpu
def test_q8_rows_do_not_depend_on_the_other_queries(reg):
    """The query set shuffled, then split in two calls; duplicated queries have equal rows"""
    t, q, _ = knn_ref(20000)
    q = q[:1000]
    g = handle(reg, t)
    perm = np.random.default_rng(8).permutation(len(q))
    for k in (5, 64):
        i0, d0 = g.nearestKSearchOf(q, k)
        i1, d1 = g.nearestKSearchOf(q[perm], k)
        assert same(i1, i0[perm]) and same(d1.view(np.uint32), d0[perm].view(np.uint32))
        ia, da = g.nearestKSearchOf(q[:333], k)
        ib, db = g.nearestKSearchOf(q[333:], k)
        assert same(np.concatenate([ia, ib]), i0) and same(np.concatenate([da, db]).view(np.uint32), d0.view(np.uint32))
    dup = np.concatenate([q[:100], q[:100], q[50:60]])
    i, d = g.nearestKSearchOf(dup, 20)
    assert same(i[:100], i[100:200]) and same(d[:100].view(np.uint32), d[100:200].view(np.uint32)) and same(i[200:], i[50:60])
    for max_nn in (0, 20):
        r0 = g.radiusSearchOf(q, 1.0, max_nn)
        r1 = g.radiusSearchOf(q[perm], 1.0, max_nn)
        rows0 = [(r0[1][a:b].tobytes(), r0[2][a:b].tobytes()) for a, b in zip(r0[0][:-1], r0[0][1:])]
        rows1 = [(r1[1][a:b].tobytes(), r1[2][a:b].tobytes()) for a, b in zip(r1[0][:-1], r1[0][1:])]
        assert rows1 == [rows0[j] for j in perm]
        ra, rb = g.radiusSearchOf(q[:333], 1.0, max_nn), g.radiusSearchOf(q[333:], 1.0, max_nn)
        assert same(np.concatenate([ra[1], rb[1]]), r0[1]) and same(np.concatenate([ra[0][:-1], rb[0] + ra[0][-1]]), r0[0])


# ------------------------------------------------------------------------------------------------------------------------ Q6 / Q7
def _rows_rc(reg, g, n=16):
    idx, sqd = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=F32)
    return g.L.apdgicp_radius_search_rows(g.h, idx.ctypes.data_as(C.c_void_p), sqd.ctypes.data_as(C.c_void_p))


@gpu
def test_q6_rows_need_a_search_of_the_current_target(reg):
    t, q, _ = knn_ref(129)
    g = handle(reg, t)
    assert _rows_rc(reg, g) == NO_INPUT                       # no search yet
    g.nearestKSearchOf(q[:10], 3)
    assert _rows_rc(reg, g) == NO_INPUT                       # a k-nearest call keeps no rows
    rs, idx, sqd = g.radiusSearchOf(q[:64], 1.2)
    again_i, again_d = np.empty_like(idx), np.empty_like(sqd)
    assert g.L.apdgicp_radius_search_rows(g.h, again_i.ctypes.data_as(C.c_void_p), again_d.ctypes.data_as(C.c_void_p)) == 0
    assert same(again_i, idx) and same(again_d.view(np.uint32), sqd.view(np.uint32))     # the rows can be read twice
    g.setInputTarget(t.copy())
    assert _rows_rc(reg, g, len(idx) + 1) == NO_INPUT         # the target was set again
    g.radiusSearchOf(q[:64], 1.2)
    g.clearTarget()
    assert _rows_rc(reg, g, len(idx) + 1) == NO_INPUT
    with pytest.raises(reg.ApdgicpError) as e:
        g.radiusSearchOf(q[:64], 1.2)                          # no target
    assert e.value.code == NO_INPUT
    with pytest.raises(reg.ApdgicpError) as e:
        g.nearestKSearchOf(q[:64], 5)
    assert e.value.code == NO_INPUT
    g.setInputTarget(t)
    with pytest.raises(reg.ApdgicpError) as e:
        g.nearestKSearchOf(q[:64], 65)
    assert e.value.code == UNSUPPORTED
    bad = q[:64].copy()
    bad[17, 1] = np.nan
    with pytest.raises(reg.ApdgicpError, match="query 17 ") as e:
        g.radiusSearchOf(bad, 1.2)
    assert e.value.code == INVALID_ARG
    assert _rows_rc(reg, g, len(idx) + 1) == NO_INPUT         # (nothing was searched since the target was set)
    check_radius(g, q[:64], t, 1.2, 0)                        # ... and the handle is usable


@gpu
def test_q7_the_handles_own_work_is_undisturbed(reg, scene):
    """align before and after the queries returns the same bytes; getPoints unchanged; covariances kept"""
    src, tgt, _, guess = scene.make_pair(1500, 3000, scene.pair_seed(3, 0), "odometry")
    g = reg.FastAPDGICP(reg.default_params(**LM))
    g.setInputSource(src)
    g.setInputTarget(tgt)
    T0 = g.align(guess).copy()
    cov0 = g.getTargetCovariances()
    q = make_queries(tgt[:, :3].astype(F32), 500, seed=31)
    t3 = np.ascontiguousarray(tgt[:, :3], dtype=F32)
    ref = S.knn(q, t3, 64)
    check_knn(g, q, t3, 20, ref)
    assert same(g.align(guess), T0)
    check_radius(g, q, t3, 0.8, 0)
    assert same(g.align(guess), T0)
    check_radius(g, q, t3, 0.8, 20)
    assert same(g.getPoints(reg.TARGET), t3) and same(g.getPoints(reg.SOURCE), np.ascontiguousarray(src[:, :3], dtype=F32))
    assert same(g.getTargetCovariances(), cov0)
    assert same(g.align(guess), T0)
    i1, d1 = g.nearestNeighboursOf(q)                         # the 1-NN path after the k-nearest one, on the same scratch slot
    assert same(i1, ref[0][:, 0]) and same(d1.view(np.uint32), ref[1][:, 0].view(np.uint32))


@gpu
def test_q7_device_resident_target_and_vgicp_cuda_mode(reg, scene):
    """Q1: the target is the cloud as set, device-resident too, and in the FAST_VGICP_CUDA mode of the handle (whose prepared clouds drop
    points: the queries see the whole target); the mode's align is the same before and after"""
    import torch
    vc = importlib.import_module("riv-slam_amd.vgicp_cuda")
    src, tgt, _, guess = scene.make_pair(1500, 3000, scene.pair_seed(3, 1), "odometry")
    t3 = np.ascontiguousarray(tgt[:, :3], dtype=F32)
    q = make_queries(t3, 400, seed=32)
    ref = S.knn(q, t3, 64)
    g = reg.FastAPDGICP(reg.default_params(**LM))
    g.setInputTarget(torch.from_numpy(t3).cuda())
    check_knn(g, q, t3, 5, ref)
    check_radius(g, q, t3, 0.8, 0)
    h = vc.FastVGICPCuda(reg.default_params(**LM))
    h.setInputSource(torch.from_numpy(np.ascontiguousarray(src[:, :3], dtype=F32)).cuda())
    h.setInputTarget(torch.from_numpy(t3).cuda())
    assert h.enabled()
    T0 = h.align(guess).copy()
    builds = h.build_count()
    check_knn(h, q, t3, 64, ref)
    check_radius(h, q, t3, 0.8, 7)
    check_radius(h, q, t3, 0.8, 0)
    assert same(h.align(guess), T0)
    assert h.build_count() == builds                            # cached maps untouched
    assert same(h.getPoints(reg.TARGET), t3)


@gpu
def test_q7_a_handle_reused_across_three_targets(reg):
    """buffers grow and shrink with the target and the query set; nothing of an earlier target is left in a later answer"""
    g = reg.FastAPDGICP(reg.default_params())
    for m, nq, k in ((20000, 3000, 64), (17, 129, 20), (2049, 65, 5), (20000, 64, 1)):
        t, q, ref = knn_ref(m)
        g.setInputTarget(t)
        check_knn(g, q[:nq], t, k, ref)
        check_radius(g, q[: min(nq, 300)], t, 1.0, 0)
        check_radius(g, q[: min(nq, 300)], t, 1.0, 7)
    a, b = g.searchGroupStats()
    assert 0 < a <= b
