"""The keep record of the neighbour search (nn_finish: nnaux.w = min(second smallest scanned distance, pruning radius)) when the chunk
scans track only chunk MINIMA and the runner-up inside the winner's chunk comes from nn_finish's re-scan of that chunk.

A bound that forgets the in-chunk runner-up is too LARGE: the next tick keeps a neighbour that should have flipped to its chunk mate.
Nothing else notices -- the search itself still returns exact neighbours -- so the scenes here are built to make that flip common
(case 1), to put the winner into partial and lone chunks (case 2), and the keep / scan counters are pinned to recorded values (case 3)."""
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GN = dict(optimizer=1, transformation_epsilon=1e-300, rotation_epsilon=1e-300, max_correspondence_distance=2.0, azimuth_variance_deg=1.0)

# every regime of the search: keeping off, brute force, each wave split of k_nn_pruned, and one pair group per handle with one-wave
# blocks = k_nn_compact (ONE_GROUP is this file's own key, not the engine's) with its point-serial path off, at 5 and for every block
ENVS = ({}, {"APDGICP_NN_SKIN": "0"}, {"APDGICP_NN_MODE": "brute"}, {"APDGICP_NN_W": "1"}, {"APDGICP_NN_W": "2"}, {"APDGICP_NN_W": "4"},
        {"APDGICP_NN_W": "8"}, {"ONE_GROUP": "1", "APDGICP_NN_W": "1", "APDGICP_NN_SPARSE": "0"},
        {"ONE_GROUP": "1", "APDGICP_NN_W": "1", "APDGICP_NN_SPARSE": "5"}, {"ONE_GROUP": "1", "APDGICP_NN_W": "1", "APDGICP_NN_SPARSE": "64"})


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


def handle_with_env(reg, cls, env, **kw):
    """A handle created under `env` (the engine reads its switches when a handle is made); the process environment is put back."""
    env = dict(env)
    one_group = env.pop("ONE_GROUP", None)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h = cls(reg.default_params(**kw))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if one_group:
        h.set_pair_groups(1)
    return h


def assert_records_equal_in_every_regime(reg, clouds, pairs, guesses, **kw):
    want = None
    for env in ENVS:
        b = handle_with_env(reg, reg.BatchAPDGICP, env, **kw)
        b.set_clouds(0, clouds)
        got = b.align(pairs, guesses).tobytes()
        want = want or got
        assert got == want, env


def assert_single_handle_equal(reg, src, tgt, guess, **kw):
    out = []
    for env in ({}, {"APDGICP_NN_SKIN": "0"}):
        h = handle_with_env(reg, reg.FastAPDGICP, env, **kw)
        h.setInputSource(src), h.setInputTarget(tgt)
        T = h.align(guess)
        c, q = h.correspondences()
        out.append((T, c, q.view(np.uint32)))
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def rigid(t, w):
    """exp of the rotation vector w, translation t"""
    th = float(np.linalg.norm(w))
    k = np.asarray(w, dtype=np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = t
    return T


# ---------------------------------------------------------------------------------------------------------------- case 1
def mate_scene(seed=20261, guess_t=0.025, guess_r=5e-4):
    """N = M = 2048.  The target is 1024 tight pairs: mate B = mate A + (2 cm +- 2 mm) along a random axis, the pairs one per cell of
    a 32 x 16 x 2 grid of 1 m cells (centre jittered by +- 0.2 m: pairs >= 0.6 m apart, 3 - 36 m from the sensor), in shuffled order.
    Two source points per pair, on the pair's axis at U(-1 cm, 1 cm) from its mid-plane (and up to 3 mm beside the axis), seen from a
    pose 0.5 m / 1 degree away; the guess is that pose moved by `guess_t` metres and turned by `guess_r` radians (1 mrad is 3 cm at
    30 m).  Gauss-Newton closes in on the pose by about a factor of two per iteration here (the residual of a point jumps from -x to
    +x at its mid-plane), and every step carries the points nearest their mid-plane over to the other mate.
    Returns source, target, guess and mate[j] = index of target j's partner."""
    rng = np.random.default_rng(seed)
    gx, gy, gz = np.meshgrid(np.arange(32), np.arange(16), np.arange(2), indexing="ij")
    centre = np.stack([3.5 + gx.ravel(), -7.5 + gy.ravel(), -0.5 + gz.ravel()], axis=1) + rng.uniform(-0.2, 0.2, size=(1024, 3))
    u = rng.normal(size=(1024, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    half = 0.5 * (0.02 + rng.uniform(-0.002, 0.002, size=(1024, 1)))
    order = rng.permutation(2048)
    target = np.concatenate([centre - half * u, centre + half * u])[order]
    pos = np.argsort(order)                      # where each of the 2048 built points went
    mate = np.empty(2048, dtype=np.int64)
    mate[pos[:1024]], mate[pos[1024:]] = pos[1024:], pos[:1024]
    c2, u2 = np.repeat(centre, 2, axis=0), np.repeat(u, 2, axis=0)
    side = np.cross(u2, rng.normal(size=(2048, 3)))
    side *= rng.uniform(0.0, 0.003, size=(2048, 1)) / np.linalg.norm(side, axis=1, keepdims=True)
    world = c2 + rng.uniform(-0.01, 0.01, size=(2048, 1)) * u2 + side
    T_true = rigid([0.5, 0.05, -0.02], [0.0, 0.0, np.deg2rad(1.0)])
    Ti = np.linalg.inv(T_true)
    source = (world @ Ti[:3, :3].T + Ti[:3, 3])[rng.permutation(2048)]
    dt, dw = rng.normal(size=3), rng.normal(size=3)
    guess = rigid(guess_t * dt / np.linalg.norm(dt), guess_r * dw / np.linalg.norm(dw)) @ T_true
    return source.astype(np.float32), target.astype(np.float32), guess.astype(np.float32), mate


def switch_shares(corr, mate):
    """corr[t]: the correspondences of the t-th linearize, t = 2 .. 8.  Share of the source points that go from one mate of a pair to
    the other between linearize t and t + 1, for t = 2 .. 7."""
    out = []
    for t in range(2, 8):
        a, b = corr[t], corr[t + 1]
        ok = (a >= 0) & (b >= 0)
        out.append(float(np.mean(ok & (b == mate[np.maximum(a, 0)]))))
    return out


def test_runner_up_in_the_winners_chunk(reg):
    """A source point between two mates that share a chunk: its keep bound is the distance to the OTHER mate, which only the re-scan
    of the winner's chunk sees.  Byte-equal records in every regime, equal correspondences with and without keeping -- on a scene in
    which (asserted) points really do change mates from the third iteration on."""
    src, tgt, guess, mate = mate_scene()
    kw = dict(GN, max_iterations=8)
    # the precondition, on the searches WITHOUT keeping: correspondences after t and t + 1 iterations
    # The numpy oracle alone (oracle/apdgicp_np.py, same parameters) on this scene: 7.6 %, 4.9 %, 1.5 %, 0.2 %, 0.1 %, 0.0 % for t = 2 .. 7,
    # so the 2 % asked for is met almost four times over between the second and the third iteration and more than twice between the
    # third and the fourth.  (A guess 4 mm / 0.2 mrad off gave 2.6 % and 1.3 %, 8 mm / 0.5 mrad 4.1 % and 1.2 %, 15 mm / 1 mrad 10.1 %
    # and 1.9 %: the guess is 25 mm / 0.5 mrad off for the margin at the later iteration.)
    corr = {}
    for t in range(2, 9):
        h = handle_with_env(reg, reg.FastAPDGICP, {"APDGICP_NN_SKIN": "0"}, **dict(GN, max_iterations=t))
        h.setInputSource(src), h.setInputTarget(tgt)
        h.align(guess)
        corr[t] = h.correspondences()[0].astype(np.int64)
    shares = switch_shares(corr, mate)
    print("share of points that change mates between iterations t and t + 1, t = 2 .. 7:", shares)
    assert max(shares) >= 0.02, shares
    assert_records_equal_in_every_regime(reg, [src, tgt], [(0, 1)], [guess], **kw)
    assert_single_handle_equal(reg, src, tgt, guess, **kw)


# ---------------------------------------------------------------------------------------------------------------- case 2
def edge_scene(M, seed):
    """A target of M points and 300 source points, source i beside target i mod M: for M <= 300 EVERY target -- hence every chunk, the
    last, partial one included -- is some point's neighbour.  For M = 2049 (a last chunk of one point) the first eight targets are the
    corners of the cloud's bounding cube: the space-filling curve of the sort ends in a corner cell, so one of them is the last point."""
    rng = np.random.default_rng(seed)
    target = np.stack([rng.uniform(8, 20, M), rng.uniform(-6, 6, M), rng.uniform(-1.5, 1.5, M)], axis=1)
    if M > 300:
        target[:8] = np.array([[14 + 7 * sx, 7 * sy, 7 * sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    world = target[np.arange(300) % M] + rng.normal(scale=0.03, size=(300, 3))
    T_true = rigid([0.4, -0.05, 0.02], [0.0, 0.0, np.deg2rad(-1.0)])
    Ti = np.linalg.inv(T_true)
    source = world @ Ti[:3, :3].T + Ti[:3, 3]
    guess = rigid(rng.normal(size=3) * 0.01, rng.normal(size=3) * 5e-4) @ T_true
    return source.astype(np.float32), target.astype(np.float32), guess.astype(np.float32)


@pytest.mark.parametrize("M", (5, 16, 17, 127, 129, 2049))
def test_winner_in_the_last_chunk(reg, M):
    """A lone partial chunk (5), exactly one chunk (16), a last chunk of one point (17, 2049), the group boundary (127, 129: a group is
    128 points): the re-scan counts what lies beyond the cloud as +inf, like the scan's LDS tile."""
    src, tgt, guess = edge_scene(M, 7000 + M)
    kw = dict(GN, max_iterations=8, k_correspondences=min(20, M))   # (a cloud needs k_correspondences points)
    assert_records_equal_in_every_regime(reg, [src, tgt], [(0, 1)], [guess], **kw)
    assert_single_handle_equal(reg, src, tgt, guess, **kw)


# ---------------------------------------------------------------------------------------------------------------- case 3
COUNTER_CASES = (("odometry", 2048, 2148, 20), ("loop", 3000, 3100, 20), ("odometry", 6000, 20_000, 4))   # (the last: the super-box level)
COUNTER_REGIMES = (("default", {}), ("one_group", {"ONE_GROUP": "1", "APDGICP_NN_W": "1"}))


def keep_counters(reg, scene):
    """{(case, regime): (points kept, chunks scanned)} -- debug_stats()[6] and [2], summed over the run by the kernels themselves"""
    out = {}
    for ci, (kind, n, m, iters) in enumerate(COUNTER_CASES):
        src, tgt, _, guess = scene.make_pair(n, m, scene.pair_seed(33, ci), kind)
        for name, env in COUNTER_REGIMES:
            b = handle_with_env(reg, reg.BatchAPDGICP, dict(env, APDGICP_STATS="1"), **dict(GN, max_iterations=iters))
            b.set_clouds(0, [src, tgt])
            b.align([(0, 1)], [guess])
            st = b.debug_stats()
            out[(ci, name)] = (int(st[6]), int(st[2]))
    return out


# Recorded on an MI355X from the library built from the commit BEFORE this file's (chunk scans that track a runner-up each), by calling
# keep_counters() above with that library loaded in place of the tree's.  Integer sums of deterministic counters: equal, no margin.
PARENT_COUNTERS = {
    (0, "default"): (31796, 4440), (0, "one_group"): (31796, 2143),
    (1, "default"): (22602, 13876), (1, "one_group"): (22691, 9744),
    (2, "default"): (4140, 14527), (2, "one_group"): (4108, 11358),
}


def test_keep_and_scan_counters_are_the_parents(reg, scene):
    """The stored bound is the same NUMBER as before, so the same points are kept and the same chunks scanned, tick for tick."""
    got = keep_counters(reg, scene)
    print(got)
    assert got == PARENT_COUNTERS
