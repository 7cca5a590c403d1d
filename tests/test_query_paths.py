"""The query side of the neighbour search: getFitnessScore, inlierFraction, the batched fitness of loop candidates, nearestNeighbours /
nearestNeighboursOf and transformSource, in every search regime and at the sizes where a launch changes shape.

k_fitness reads the search's partial minima (Work::nnpart) directly -- it takes the minimum over the target splits itself and never goes
through k_linearize's settle pass -- so nothing that pins the search through linearize / align says anything about it.

References (plain, independent): oracle/apdgicp_np.py's brute-force fp32 search (FLANN's accumulation order, the lowest original index on
ties) for indices and distances, compared bit for bit; from its fp32 squared distances d, widened to float64,
    fitness(r)        = fsum(d[d <= r]) / count, or DBL_MAX with count 0      (r is compared with the SQUARED distance, as PCL does)
    inlierFraction(c) = float32(count(d < c * c)) / float32(n_src)            (c * c formed in float64)
Counts, indices and distances are compared exactly.  A score is compared either with `==` (the lattice fixture below: every distance and
every partial sum is a multiple of 1/64, exact in float64 in any order of addition) or within a DERIVED bound: every term is
non-negative, so any order of float64 additions of n terms is within (n - 1) 2^-53 relative of the exact sum, fsum is within 2^-53 of it,
and both divisions add half an ulp each:  |got - want| <= n 2^-52 want,  n = the inlier count."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import apdgicp_np as O
from test_search_runner_up import ENVS, handle_with_env

gpu = pytest.mark.gpu
DBL_MAX = float(np.finfo(np.float64).max)
NO_INPUT, INVALID_ARG = -3, -1
LM = dict(max_correspondence_distance=2.0, transformation_epsilon=0.1, azimuth_variance_deg=1.0)
GN = dict(optimizer=1, max_iterations=5, transformation_epsilon=1e-300, rotation_epsilon=1e-300, max_correspondence_distance=2.0, azimuth_variance_deg=1.0)


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


# ---------------------------------------------------------------------------------------------------------------- references
def ref_nn(src, tgt, T, linear_chain=False):
    return O.nn1(O.transform_points_f32(np.asarray(T, dtype=np.float32).astype(np.float64), src, linear_chain), tgt)


def ref_fitness(d32, r):
    d = d32.astype(np.float64)
    sel = d <= r
    n = int(sel.sum())
    return (math.fsum(d[sel]) / n if n else DBL_MAX), n


def ref_inliers(d32, c, n_src):
    n = int((d32.astype(np.float64) < np.float64(c) * np.float64(c)).sum())
    return float(np.float32(n) / np.float32(n_src)), n


def assert_score(got, got_n, want, want_n, what=None):
    """counts exactly; the score within n 2^-52 relative (module docstring), DBL_MAX exactly when nothing is in range"""
    assert got_n == want_n, (what, got_n, want_n)
    if want_n == 0:
        assert got == DBL_MAX, (what, got)
    else:
        assert abs(got - want) <= want_n * 2.0 ** -52 * want, (what, got, want)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the lattice
LATTICE_SIZES = (1, 17, 255, 256, 257, 320)
ROT = np.array([[0, -1, 0, 7], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)   # turn 90 degrees about z, then move by (7, 0, 0)
EYE = np.eye(4, dtype=np.float32)


def lattice_target():
    """the integer lattice 0..7 x 0..7 x 0..4 (320 points), index = 40 x + 5 y + z"""
    x, y, z = np.meshgrid(np.arange(8), np.arange(8), np.arange(5), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)


def lattice_source(offsets=(0.0, 0.125, 0.25, 0.375), seed=20262):
    """(source, a): source i = lattice point i + a_i along an axis drawn per point, a_i cycling over `offsets` (all < 0.5: target i is the
    unique nearest neighbour, d_i = a_i^2 exactly in fp32)"""
    t = lattice_target()
    a = np.asarray(offsets, dtype=np.float32)[np.arange(len(t)) % len(offsets)]
    axis = np.random.default_rng(seed).integers(0, 3, len(t))
    s = t.copy()
    s[np.arange(len(t)), axis] += a
    return s, a


def lattice_tie_source():
    """the lattice points with x <= 6 moved by half a cell along x: exactly between target i and target i + 40, d = 0.25 to both"""
    t = lattice_target()
    keep = np.flatnonzero(t[:, 0] <= 6)
    s = t[keep].copy()
    s[:, 0] += np.float32(0.5)
    return s, keep.astype(np.int32)


def under_rot(points):
    """ROT^-1 applied exactly: (X, Y, Z) -> (Y, 7 - X, Z), so that ROT * result == points bit for bit under both transform orders"""
    return np.stack([points[:, 1], np.float32(7.0) - points[:, 0], points[:, 2]], axis=1).astype(np.float32)


def hand_fitness(a, r):
    d = a.astype(np.float64) ** 2
    sel = d <= r
    n = int(sel.sum())
    return (float(d[sel].sum()) / n if n else DBL_MAX), n     # (multiples of 1/64 below 2^53 / 64: the sum is exact in any order)


def hand_inliers(a, c, n_src):
    n = int((a.astype(np.float64) ** 2 < c * c).sum())
    return float(np.float32(n) / np.float32(n_src)), n


def test_lattice_fixture_is_exact():
    """CPU: the fixture's claims, checked with the oracle so that it cannot drift.  The transformed clouds are bit-equal to the intended
    ones under both transform orders, the neighbours are arange(n), the distances a * a, the counts at 1/16 the ones worked out by hand."""
    tgt = lattice_target()
    src, a = lattice_source()
    assert tgt.shape == (320, 3) and np.array_equal(tgt[41], [1, 0, 1])
    rot_src = under_rot(src)
    for lin in (False, True):
        assert np.array_equal(bits(O.transform_points_f32(EYE.astype(np.float64), src, lin)), bits(src))
        assert np.array_equal(bits(O.transform_points_f32(ROT.astype(np.float64), rot_src, lin)), bits(src))
        for s, T in ((src, EYE), (rot_src, ROT)):
            idx, d = ref_nn(s, tgt, T, lin)
            assert np.array_equal(idx, np.arange(320)) and np.array_equal(bits(d), bits(a * a))
    d = a * a
    inclusive, strict = (1, 13, 192, 192, 193, 240), (1, 9, 128, 128, 129, 160)
    for n, ni, ns in zip(LATTICE_SIZES, inclusive, strict):
        assert ref_fitness(d[:n], 1.0 / 16) == hand_fitness(a[:n], 1.0 / 16) and hand_fitness(a[:n], 1.0 / 16)[1] == ni
        assert ref_inliers(d[:n], 0.25, n) == hand_inliers(a[:n], 0.25, n) and hand_inliers(a[:n], 0.25, n)[1] == ns
        assert all((64.0 * np.cumsum(d[:n].astype(np.float64))) % 1.0 == 0.0)          # every partial sum is a multiple of 1/64
    assert hand_fitness(a, 1.0 / 16)[0] == 6.25 / 240 and hand_fitness(a, DBL_MAX) == (80 * 14 / 64 / 320, 320)
    # the tie source: two targets at exactly 0.25, the oracle keeps the lower original index (the point's own lattice point)
    tie, keep = lattice_tie_source()
    assert len(tie) == 280
    idx, dd = ref_nn(tie, tgt, EYE)
    assert np.array_equal(idx, keep) and (dd == np.float32(0.25)).all()
    assert (O.sqdist_f32(tie, tgt)[np.arange(280), keep + 40] == np.float32(0.25)).all()
    idx, dd = ref_nn(under_rot(tie), tgt, ROT)
    assert np.array_equal(idx, keep) and (dd == np.float32(0.25)).all()
    # the source without a zero offset: nothing within 1/128, nothing strictly inside 0.125
    nz, a_nz = lattice_source((0.125, 0.25, 0.375))
    idx, dd = ref_nn(nz, tgt, EYE)
    assert np.array_equal(idx, np.arange(320)) and np.array_equal(bits(dd), bits(a_nz * a_nz))
    assert ref_fitness(dd, 1.0 / 128) == (DBL_MAX, 0) and ref_inliers(dd, 0.125, 320) == (0.0, 0)
    assert ref_fitness(dd, 1.0 / 64)[1] == 107                                         # (`<=`: the points at exactly 1/64 count)


# ---------------------------------------------------------------------------------------------------------------- handles
def fast_handle(reg, src, tgt, env=None, **kw):
    """A FastAPDGICP with both clouds set; a cloud below k_correspondences points gets identity covariances injected (the handle refuses to
    compute covariances of such a cloud, and nothing here reads them)."""
    env = {k: v for k, v in (env or {}).items() if k != "ONE_GROUP"}   # (pair groups are a batch handle's; a single handle with W = 1 is k_nn_compact)
    g = handle_with_env(reg, reg.FastAPDGICP, env, **kw)
    set_clouds(reg, g, src, tgt)
    return g


def set_clouds(reg, g, src=None, tgt=None):
    if src is not None:
        g.setInputSource(src)
    if tgt is not None:
        g.setInputTarget(tgt)
    k = g.params.k_correspondences
    if src is not None and len(src) < k:
        g.setSourceCovariances(np.tile(np.eye(3), (len(src), 1, 1)))
    if tgt is not None and len(tgt) < k:
        g.setTargetCovariances(np.tile(np.eye(3), (len(tgt), 1, 1)))


def check_lattice_on(g, n, T, a, what):
    """fitness and inlier results of the first n lattice source points on handle g, `==` the hand values"""
    for r in (DBL_MAX, 1.0 / 16, 9.0 / 64, 0.0):
        got = g.getFitnessScore(r, T)
        assert (got, g.last_inliers) == hand_fitness(a[:n], r), (what, n, r, got, g.last_inliers)
    for c in (0.5, 0.25, 0.125):
        got = g.inlierFraction(c, T)
        assert (got, g.last_inliers) == hand_inliers(a[:n], c, n), (what, n, c, got, g.last_inliers)


# ---------------------------------------------------------------------------------------------------------------- 1. sizes at the edges
@pytest.fixture(scope="module")
def big_pair(scene):
    src, tgt, _, guess = scene.make_pair(1025, 16385, scene.pair_seed(61, 0), "odometry")
    return src, tgt, guess


# every listed source size (1, 2, 16, 17, 63, 64, 65, 255, 256, 257, 1025) and every listed target size (1, 2, 15, 16, 17, 127, 128, 129,
# 1025, 16385: past SORT_LDS_MAX_N, the generic sort) at least once on its side; 16385 once
SIZE_PAIRS = ((1025, 16385), (1, 1), (2, 2), (16, 15), (17, 16), (63, 17), (64, 127), (65, 128), (255, 129), (256, 1025), (257, 1), (1025, 17))


@gpu
@pytest.mark.parametrize("n,m", SIZE_PAIRS)
def test_sizes_at_the_edges(reg, big_pair, n, m):
    """Slices of one random pair, at the pair's guess, under both transform orders: neighbours (of the source, and of foreign queries)
    bit for bit; fitness at DBL_MAX, at the median distance (an exact threshold: `<=` must count it), below the minimum and at 0;
    inlierFraction at thresholds checked with the same float64 c * c."""
    src, tgt, guess = big_pair[0][:n], big_pair[1][:m], big_pair[2]
    g = fast_handle(reg, src, tgt)
    far = (tgt[:3] + np.float32(1000.0) * np.array([[1, 1, 1], [-1, 1, -1], [1, -1, -1]], dtype=np.float32)[:len(tgt[:3])]).astype(np.float32)
    for lin in (False, True):
        g.setTransformOrder(lin)
        want_i, want_d = ref_nn(src, tgt, guess, lin)
        idx, sqd = g.nearestNeighbours(guess)
        assert np.array_equal(idx, want_i) and np.array_equal(bits(sqd), bits(want_d)), lin
        q = np.concatenate([O.transform_points_f32(guess.astype(np.float64), src, lin), far])
        qi, qd = O.nn1(q, tgt)
        idx, sqd = g.nearestNeighboursOf(q)
        assert np.array_equal(idx, qi) and np.array_equal(bits(sqd), bits(qd)), lin
        assert np.array_equal(bits(qd[:n]), bits(want_d))       # (the same points: the two entries must agree with each other too)
        median = float(np.sort(want_d)[n // 2])
        assert float(want_d.min()) > 0.0
        for r in (DBL_MAX, median, 0.5 * float(want_d.min()), 0.0):
            want, want_n = ref_fitness(want_d, r)
            got = g.getFitnessScore(r, guess)
            assert_score(got, g.last_inliers, want, want_n, (lin, r))
        assert ref_fitness(want_d, median)[1] == int((want_d < np.float32(median)).sum()) + int((want_d == np.float32(median)).sum()) >= 1
        for c in (float(np.sqrt(np.float64(median))), 0.5, 2.0, 1e-9):
            want, want_n = ref_inliers(want_d, c, n)
            got = g.inlierFraction(c, guess)
            assert (got, g.last_inliers) == (want, want_n), (lin, c)


@gpu
def test_lattice_sizes_single_handle(reg):
    """The lattice at 1 / 17 / 255 / 256 / 257 / 320 source points, under T = I and under the exact quarter turn, both transform orders:
    score, count and fraction `==` the hand values; the tie source resolves to the lower original index; nothing in range gives DBL_MAX."""
    tgt = lattice_target()
    src, a = lattice_source()
    tie, keep = lattice_tie_source()
    nz, a_nz = lattice_source((0.125, 0.25, 0.375))
    g = fast_handle(reg, src, tgt)
    for lin in (False, True):
        g.setTransformOrder(lin)
        for n in LATTICE_SIZES:
            for s, T in ((src, EYE), (under_rot(src), ROT)):
                set_clouds(reg, g, src=s[:n])
                check_lattice_on(g, n, T, a, ("single", lin))
                idx, sqd = g.nearestNeighbours(T)
                assert np.array_equal(idx, np.arange(n)) and np.array_equal(bits(sqd), bits((a * a)[:n]))
        for s, T in ((tie, EYE), (under_rot(tie), ROT)):
            set_clouds(reg, g, src=s)
            idx, sqd = g.nearestNeighbours(T)
            assert np.array_equal(idx, keep) and (sqd == np.float32(0.25)).all()
            idx, sqd = g.nearestNeighboursOf(tie)
            assert np.array_equal(idx, keep) and (sqd == np.float32(0.25)).all()
            assert (g.getFitnessScore(0.25, T), g.last_inliers) == (0.25, 280)
            assert (g.inlierFraction(0.5, T), g.last_inliers) == (0.0, 0)
        set_clouds(reg, g, src=nz)
        assert (g.getFitnessScore(1.0 / 128, EYE), g.last_inliers) == (DBL_MAX, 0)
        assert (g.inlierFraction(0.125, EYE), g.last_inliers) == (0.0, 0)
        assert (g.getFitnessScore(1.0 / 64, EYE), g.last_inliers) == (1.0 / 64, 107)


# ---------------------------------------------------------------------------------------------------------------- 2. every search regime
@pytest.fixture(scope="module")
def regime_pair(scene):
    """one random pair of 700 x 2100 points: 700 x 900 for every regime, 300 x 2100 for the brute-force batch; references computed once"""
    src, tgt, _, guess = scene.make_pair(700, 2100, scene.pair_seed(62, 0), "odometry")
    _, d = ref_nn(src, tgt[:900], guess)
    _, d2 = ref_nn(src[:300], tgt, guess)
    return src, tgt, guess, d, d2


def lattice_batch_cases():
    """clouds and (source, pose, a or None) of the lattice cases of a batch; the target is the last cloud"""
    src, a = lattice_source()
    tie, _ = lattice_tie_source()
    nz, a_nz = lattice_source((0.125, 0.25, 0.375))
    clouds = [src[:257], src, under_rot(src), tie, under_rot(tie), nz, lattice_target()]
    half = np.full(280, 0.5, dtype=np.float32)
    cases = [(0, EYE, a[:257]), (1, EYE, a), (2, ROT, a), (3, EYE, half), (4, ROT, half), (5, EYE, a_nz)]
    return clouds, cases


@gpu
@pytest.mark.parametrize("env", ENVS, ids=lambda e: "-".join(f"{k[-6:]}{v}" for k, v in e.items()) or "default")
def test_every_search_regime(reg, regime_pair, env):
    """default, keeping off, brute force (T > 1 target splits: the split loop of k_fitness), W = 1 / 2 / 4 / 8, one pair group with
    k_nn_compact and its point-serial path off / at 5 / everywhere: a FastAPDGICP and a BatchAPDGICP created under the regime give the hand
    values on the lattice (hence the same in every regime) and the reference's on a random 700 x 900 pair."""
    rs, rt, guess, d, d2 = regime_pair
    tgt = lattice_target()
    src, a = lattice_source()
    tie, keep = lattice_tie_source()
    nz, a_nz = lattice_source((0.125, 0.25, 0.375))
    g = fast_handle(reg, src, tgt, env)
    for n in (257, 320):
        for s, T in ((src, EYE), (under_rot(src), ROT)):
            set_clouds(reg, g, src=s[:n])
            check_lattice_on(g, n, T, a, env)
    set_clouds(reg, g, src=tie)
    idx, sqd = g.nearestNeighbours(EYE)
    assert np.array_equal(idx, keep) and (sqd == np.float32(0.25)).all()
    assert (g.getFitnessScore(DBL_MAX, EYE), g.last_inliers) == (0.25, 280)
    set_clouds(reg, g, src=nz)
    assert (g.getFitnessScore(1.0 / 128, EYE), g.last_inliers) == (DBL_MAX, 0)
    assert (g.inlierFraction(0.125, EYE), g.last_inliers) == (0.0, 0)
    set_clouds(reg, g, src=rs, tgt=rt[:900])
    median = float(np.sort(d)[350])
    for r in (DBL_MAX, median, 1.0 / 16):
        got = g.getFitnessScore(r, guess)
        assert_score(got, g.last_inliers, *ref_fitness(d, r), (env, r))
    for c in (float(np.sqrt(np.float64(median))), 0.5):
        assert (g.inlierFraction(c, guess), g.last_inliers) == ref_inliers(d, c, 700), (env, c)

    clouds, cases = lattice_batch_cases()
    b = handle_with_env(reg, reg.BatchAPDGICP, env)
    b.set_clouds(0, clouds + [rs, rt[:900]])
    nt = len(clouds) - 1
    pairs = [(ci, nt) for ci, _, _ in cases] + [(nt + 1, nt + 2)]
    poses = np.stack([T for _, T, _ in cases] + [guess])
    for r in (DBL_MAX, 1.0 / 16, 1.0 / 128, median):
        scores, inl = b.fitness(pairs, poses, r)
        for k, (_, _, ak) in enumerate(cases):
            assert (float(scores[k]), int(inl[k])) == hand_fitness(ak, r), (env, r, k)
        assert_score(float(scores[-1]), int(inl[-1]), *ref_fitness(d, r), (env, r))
    if env.get("APDGICP_NN_MODE") == "brute":
        # one pair of 300 x 2100: S = 2, one source block, T = min(64, ceil(512 / (1 * 1))) = 64 target splits (setup_pairs)
        b.set_clouds(0, [rs[:300], rt])
        for r in (DBL_MAX, float(np.sort(d2)[150]), 1.0 / 16):
            scores, inl = b.fitness([(0, 1)], guess[None], r)
            assert b.last_ticks()[2] == 64                       # (nn_target_splits: the split loop of k_fitness really runs)
            assert_score(float(scores[0]), int(inl[0]), *ref_fitness(d2, r), ("brute T = 64", r))


# ---------------------------------------------------------------------------------------------------------------- 3. unequal batches
@pytest.fixture(scope="module")
def unequal_batch(scene):
    """Clouds of 20, 255, 256, 257, 700 and 2049 points (slices of one pair) and a pair list in which the 2049-point source sets nblk_max
    and nstride (2304), the 20-point source leaves all but the first block to the early return, cloud 2 is a target in two pairs and a
    source in a third, and pair 4 is a cloud against itself.  (source, target, pose) and the reference (score inputs) per pair."""
    s, t, _, guess = scene.make_pair(2049, 2049, scene.pair_seed(63, 0), "odometry")
    back = np.linalg.inv(guess.astype(np.float64)).astype(np.float32)
    clouds = [t[:20], s[:255], t[:256], s[300:557], t[300:1000], s]
    assert [len(c) for c in clouds] == [20, 255, 256, 257, 700, 2049]
    pairs = [(5, 4, guess), (0, 2, EYE), (1, 2, guess), (2, 4, EYE), (3, 3, EYE), (4, 5, back), (1, 0, guess)]
    dists = [ref_nn(clouds[a], clouds[b], T)[1] for a, b, T in pairs]
    assert not dists[4].any()
    return clouds, pairs, dists


@gpu
@pytest.mark.parametrize("env", ({}, {"ONE_GROUP": "1", "APDGICP_NN_W": "1"}), ids=("default", "one_group"))
def test_batches_of_unequal_pairs(reg, unequal_batch, env):
    clouds, pairs, dists = unequal_batch
    b = handle_with_env(reg, reg.BatchAPDGICP, env)
    b.set_clouds(0, clouds)
    ids = [(a, c) for a, c, _ in pairs]
    poses = np.stack([T for _, _, T in pairs])
    for r in (DBL_MAX, 4.0, float(np.sort(dists[0])[1024])):
        scores, inl = b.fitness(ids, poses, r)
        for k, d in enumerate(dists):
            assert_score(float(scores[k]), int(inl[k]), *ref_fitness(d, r), (env, r, k))
        assert (float(scores[4]), int(inl[4])) == (0.0, 257)
        # the same list backwards: a record must not depend on its slot (counts and, pair by pair, scores within the bound)
        rs, ri = b.fitness(ids[::-1], poses[::-1], r)
        assert np.array_equal(ri[::-1], inl)
        for k, d in enumerate(dists):
            assert_score(float(rs[::-1][k]), int(ri[::-1][k]), *ref_fitness(d, r), (env, r, k, "reversed"))


# ---------------------------------------------------------------------------------------------------------------- 4. T == NULL and handle state
@pytest.fixture(scope="module")
def mixed_pairs(scene):
    """three easy odometry pairs and three loop pairs (guess = identity, up to 3 m / 20 degrees away), sources of at most 512 points: two
    blocks of k_fitness per pair, so the float64 sum of the two block partials is the same number in either order of the atomicAdds and
    two calls at the same poses must agree to the bit"""
    clouds, guesses = [], []
    for p in range(6):
        s, t, _, g = scene.make_pair(500 - 7 * p, 600, scene.pair_seed(64, p), "odometry" if p < 3 else "loop")
        clouds += [s, t]
        guesses.append(g)
    return clouds, [(2 * p, 2 * p + 1) for p in range(6)], guesses


def records_poses(reg, recs):
    return np.stack([reg.result_matrix(r) for r in recs])


def assert_no_input(reg, fn):
    with pytest.raises(reg.ApdgicpError) as ei:
        fn()
    assert ei.value.code == NO_INPUT, ei.value


def check_null_poses(reg, b, mixed, align, iterations_must_differ):
    """`align()` runs the pair list on b and returns its records.  T == NULL scores the poses of that align -- exactly what the explicit
    call at the records' poses gives, counts included -- and nothing else: another pair list, a replaced cloud or poses somebody else has
    written since are refused with NO_INPUT and no numbers, and the next explicit-pose call on the handle is right."""
    clouds, pairs, _ = mixed
    recs = align()
    if iterations_must_differ:
        assert len(set(int(x) for x in recs["iterations"])) > 1      # the pairs end at different ticks, or the case proves nothing
    T = records_poses(reg, recs)
    ranges = (DBL_MAX, 4.0, 0.25)
    null = [b.fitness(pairs, None, r) for r in ranges]
    assert_no_input(reg, lambda: b.fitness(pairs[:-1], None, 4.0))                         # another list: shorter,
    assert_no_input(reg, lambda: b.fitness([pairs[1], pairs[0]] + pairs[2:], None, 4.0))   # in another order
    again = b.fitness(pairs, None, 4.0)                                                    # (the refusals changed nothing)
    assert np.array_equal(again[0], null[1][0]) and np.array_equal(again[1], null[1][1])
    for r, (scores, inl) in zip(ranges, null):
        es, ei = b.fitness(pairs, T, r)
        assert np.array_equal(scores, es) and np.array_equal(inl, ei), r
    for k, (s, t) in enumerate(pairs):
        _, d = ref_nn(clouds[s], clouds[t], T[k])
        assert_score(float(null[1][0][k]), int(null[1][1][k]), *ref_fitness(d, 4.0), k)
    # explicit poses that are NOT the align's: T == NULL must not score those
    other = np.stack([EYE] * len(pairs))
    b.fitness(pairs, other, 4.0)
    assert_no_input(reg, lambda: b.fitness(pairs, None, 4.0))
    # the same align again, then a replaced cloud (a larger one: its buffers move) -- refused at once, and still refused after the
    # covariances have been computed, which uploads the descriptor table again without setting the pairs up
    assert align().tobytes() == recs.tobytes()
    new_src = np.ascontiguousarray(np.concatenate([clouds[0][::-1], clouds[2][:150]]))
    assert len(new_src) > len(clouds[0])
    b.set_cloud(0, new_src)
    assert_no_input(reg, lambda: b.fitness(pairs, None, 4.0))
    b.compute_covariances()
    assert_no_input(reg, lambda: b.fitness(pairs, None, 4.0))
    scores, inl = b.fitness(pairs, T, 4.0)
    for k, (s, t) in enumerate(pairs):
        _, d = ref_nn(new_src if s == 0 else clouds[s], clouds[t], T[k])
        assert_score(float(scores[k]), int(inl[k]), *ref_fitness(d, 4.0), k)
    assert_no_input(reg, lambda: b.fitness(pairs, None, 4.0))


@gpu
def test_null_poses_after_gauss_newton(reg, mixed_pairs):
    clouds, pairs, guesses = mixed_pairs
    b = reg.BatchAPDGICP(reg.default_params(**GN))
    b.set_clouds(0, clouds)
    check_null_poses(reg, b, mixed_pairs, lambda: b.align(pairs, guesses), False)


@gpu
def test_null_poses_after_lm_that_shrinks_to_its_slow_pairs(reg, mixed_pairs, monkeypatch):
    """the host-polled LM loop (APDGICP_LM_POOL=0) launches over the pairs still running (Work::active): the poses of ALL pairs must be there
    afterwards, in their own slots"""
    clouds, pairs, guesses = mixed_pairs
    b = reg.BatchAPDGICP(reg.default_params(**LM))
    b.set_clouds(0, clouds)

    def align():
        with monkeypatch.context() as m:
            m.setenv("APDGICP_LM_POOL", "0")
            return b.align(pairs, guesses)
    check_null_poses(reg, b, mixed_pairs, align, True)


@gpu
def test_null_poses_after_a_pooled_batch(reg, mixed_pairs):
    """LM with the pair pool on, enqueue / collect: the first T == NULL call takes the poses from the batch's records (pool.last_lane) and
    leaves the pool; the later ones find them in the handle's state"""
    clouds, pairs, guesses = mixed_pairs
    b = reg.BatchAPDGICP(reg.default_params(**LM))
    b.set_clouds(0, clouds)
    check_null_poses(reg, b, mixed_pairs, lambda: b.align_collect(b.align_enqueue(pairs, guesses)), True)
    pooled = lambda pr, gs: b.align_collect(b.align_enqueue(pr, gs))
    # a cloud replaced straight behind the collect, the pool still on: the batch's records no longer describe the handle's clouds
    b.set_clouds(0, clouds)
    recs = pooled(pairs, guesses)
    b.set_cloud(1, np.ascontiguousarray(clouds[1][:500]))
    assert_no_input(reg, lambda: b.fitness(pairs, None, 4.0))
    # the poses in the handle's state (a T == NULL call has copied them there and left the pool), a cloud replaced, then a pooled batch
    # of ANOTHER list, which uploads the descriptor table again: still refused
    b.set_clouds(0, clouds)
    assert pooled(pairs, guesses).tobytes() == recs.tobytes()
    b.fitness(pairs, None, 4.0)
    b.set_cloud(1, np.ascontiguousarray(clouds[1][:500]))
    recs2 = pooled(pairs[1:], guesses[1:])                                    # (a batch that does not read the replaced slot)
    assert recs2.tobytes() == recs[1:].tobytes()
    assert_no_input(reg, lambda: b.fitness(pairs, None, 4.0))
    scores, inl = b.fitness(pairs[1:], None, 4.0)
    es, ei = b.fitness(pairs[1:], records_poses(reg, recs2), 4.0)
    assert np.array_equal(scores, es) and np.array_equal(inl, ei)
    # no cloud written at all, but the last align is another list's: its poses are not this list's
    assert pooled(pairs[1:], guesses[1:]).tobytes() == recs2.tobytes()
    b.fitness(pairs[1:], None, 4.0)
    pooled(pairs[2:], guesses[2:])
    assert_no_input(reg, lambda: b.fitness(pairs[1:], None, 4.0))
    scores, inl = b.fitness(pairs[1:], records_poses(reg, recs2), 4.0)      # (explicit poses on the state's list while the pool is on)
    assert np.array_equal(scores, es) and np.array_equal(inl, ei)


@gpu
def test_queries_leave_no_trace_on_a_single_handle(reg, scene):
    """getFitnessScore / inlierFraction / nearestNeighboursOf at pose A in front of align(guess) and linearize(T): bit-equal to a fresh
    handle's (the queries run cold, nothing of theirs seeds the next search); correspondences() after a fitness call is the documented
    error, never the other pose's data."""
    src, tgt, T_true, guess = scene.make_pair(700, 900, scene.pair_seed(65, 0), "odometry")
    A = scene.make_transform([1.5, -0.7, 0.1], yaw=0.1).astype(np.float32)
    kw = dict(max_correspondence_distance=2.0, azimuth_variance_deg=1.0)
    fresh = fast_handle(reg, src, tgt, **kw)
    want_T = fresh.align(guess).copy()
    want_rec, want_corr = bytes(fresh.result), [x.copy() for x in fresh.correspondences()]
    fresh2 = fast_handle(reg, src, tgt, **kw)
    want_lin = fresh2.linearize(T_true)
    want_lin_corr = [x.copy() for x in fresh2.correspondences()]

    def queries(g):
        _, d = ref_nn(src, tgt, A)
        assert_score(g.getFitnessScore(4.0, A), g.last_inliers, *ref_fitness(d, 4.0))
        assert (g.inlierFraction(0.5, A), g.last_inliers) == ref_inliers(d, 0.5, len(src))
        q = O.transform_points_f32(A.astype(np.float64), src)[:333]
        idx, sqd = g.nearestNeighboursOf(q)
        wi, wd = O.nn1(q, tgt)
        assert np.array_equal(idx, wi) and np.array_equal(bits(sqd), bits(wd))

    g = fast_handle(reg, src, tgt, **kw)
    queries(g)
    assert np.array_equal(g.align(guess), want_T) and bytes(g.result) == want_rec
    for x, y in zip(g.correspondences(), want_corr):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    queries(g)
    got_lin = g.linearize(T_true)
    assert got_lin[0] == want_lin[0] and np.array_equal(got_lin[1], want_lin[1]) and np.array_equal(got_lin[2], want_lin[2])
    for x, y in zip(g.correspondences(), want_lin_corr):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    g.getFitnessScore(4.0, A)
    assert_no_input(reg, g.correspondences)                      # (the partials were overwritten at pose A: no correspondences, not A's)
    g.inlierFraction(0.5, A)
    assert_no_input(reg, g.correspondences)
    g.linearize(T_true)
    for x, y in zip(g.correspondences(), want_lin_corr):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # nearestNeighbours(A) leaves the handle as linearize(A) would: its correspondences are A's, ungated
    idx, sqd = g.nearestNeighbours(A)
    fresh2.linearize(A.astype(np.float64))
    for x, y in zip(g.correspondences(), fresh2.correspondences()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 5. poses that leave the floats
@gpu
def test_a_pose_that_overflows_the_distances(reg, scene):
    """A translation of 3e38: every transformed point is finite, every squared distance +inf.  inf <= DBL_MAX is false: 0 inliers, DBL_MAX,
    no error, and the handle works afterwards."""
    src, tgt, _, guess = scene.make_pair(300, 400, scene.pair_seed(66, 0), "odometry")
    away = np.eye(4, dtype=np.float32)
    away[0, 3] = np.float32(3e38)
    with np.errstate(over="ignore"):
        _, d = ref_nn(src, tgt, away)
    assert np.isinf(d).all() and ref_fitness(d, DBL_MAX) == (DBL_MAX, 0)
    _, dg = ref_nn(src, tgt, guess)
    g = fast_handle(reg, src, tgt)
    for r in (DBL_MAX, 4.0):
        assert (g.getFitnessScore(r, away), g.last_inliers) == (DBL_MAX, 0), r
    assert (g.inlierFraction(0.5, away), g.last_inliers) == (0.0, 0)
    assert_score(g.getFitnessScore(4.0, guess), g.last_inliers, *ref_fitness(dg, 4.0))
    for env in ({}, {"APDGICP_NN_MODE": "brute"}, {"ONE_GROUP": "1", "APDGICP_NN_W": "1"}):
        b = handle_with_env(reg, reg.BatchAPDGICP, env)
        b.set_clouds(0, [src, tgt])
        for r in (DBL_MAX, 4.0):
            scores, inl = b.fitness([(0, 1), (0, 1)], np.stack([away, guess]), r)
            assert (float(scores[0]), int(inl[0])) == (DBL_MAX, 0), (env, r)
            assert_score(float(scores[1]), int(inl[1]), *ref_fitness(dg, r), (env, r))


# ---------------------------------------------------------------------------------------------------------------- 6. transformSource
def xf_left_to_right(T, p):
    """((T00 x + T01 y) + T02 z) + T03 in float32, operation by operation (the library is built with -ffp-contract=off)"""
    T = np.asarray(T, dtype=np.float32)
    x, y, z = (np.ascontiguousarray(p[:, k], dtype=np.float32) for k in range(3))
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


@gpu
@pytest.mark.parametrize("n", (1, 255, 256, 257, 1025))
def test_transform_source(reg, big_pair, scene, n):
    src, guess = big_pair[0][:n], big_pair[2]
    T2 = scene.make_transform([-3.25, 11.5, 0.7], yaw=-0.9, pitch=0.2, roll=-0.1).astype(np.float32)
    g = reg.FastAPDGICP(reg.default_params(max_correspondence_distance=2.0, azimuth_variance_deg=1.0))
    g.setInputSource(src)
    for T in (guess, T2, EYE):
        assert np.array_equal(bits(g.transformSource(T)), bits(xf_left_to_right(T, src)))
    Tc = np.asfortranarray(T2)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    want = bits(xf_left_to_right(T2, src))
    for stride in (16, 32):
        out = np.full((n, stride // 4), 0xDEADBEEF, dtype=np.uint32)
        assert g.L.apdgicp_transform_source(g.h, ptr(Tc), ptr(out), n, stride) == 0
        assert np.array_equal(out[:, :3], want) and (out[:, 3:] == 0xDEADBEEF).all(), stride
    out = np.full((n + 1, 8), 0xDEADBEEF, dtype=np.uint32)
    for bad_n, stride in ((n + 1, 12), (n - 1, 12), (n, 8), (n, 14)):
        assert g.L.apdgicp_transform_source(g.h, ptr(Tc), ptr(out), bad_n, stride) == INVALID_ARG, (bad_n, stride)
    assert (out == 0xDEADBEEF).all()
    if n >= 257:   # align(want_output=True): the source under the final pose
        g.setInputTarget(big_pair[1][:1025])
        cloud = g.align(guess, want_output=True)
        assert np.array_equal(bits(cloud), bits(xf_left_to_right(g.getFinalTransformation(), src)))
