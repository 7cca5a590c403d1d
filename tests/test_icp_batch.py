"""Point-to-point ICP as a mode of the BATCH handle: include/apdgicp_hip.h IC11 .. IC16, riv-slam_amd/csrc/apd_icp_batch.hpp,
riv-slam_amd/icp.py (BatchICP), against the single handle (tests/test_icp.py checks that one against the restatement) and the restatement
tests/icp_np.py itself.

CPU part: exports, the Python class, the refusals that need no handle, and the margins of every align fixture used below.
GPU part (-m gpu): batches against the single handle and the restatement, sizes, purity (IC14), chunk lengths, every convergence state
inside a batch, non-finite points, the brute reciprocal search, the mode rules (IC16), launch and wait counts.

Bars.  Batch against single handle and batch against batch: bytes -- the record, the state, every trace entry (T_k, n_corr, mse, similar),
the last correspondences and the final W.  Against the restatement: state, iteration count, n_matched and converged equal, the pose
within 1e-3 m / 1e-4 rad, the bars of tests/test_icp.py, asserted where the restatement alone shows a margin (no convergence quantity
within 1e-3 relative of its threshold, no best and second-best distance within 4 fp32 ulps).

How the fixtures become batches: a batch handle has ONE set of parameters, so each of the batches A .. D is six pairs against one target:
prefixes of 700, 350, 257, 256, 65 and 23 points of one source, each from its own perturbed guess, so that pairs of different sizes stop
after different numbers of iterations and idle beside running ones.
"""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import icp_np as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apdgicp_batch_set_icp", "apdgicp_batch_get_icp", "apdgicp_batch_icp_states", "apdgicp_batch_icp_get_correspondences",
               "apdgicp_batch_icp_get_working_cloud", "apdgicp_batch_icp_get_trace", "apdgicp_batch_icp_debug_counts")
GATE = 2.5
ROT_EPS = 0.99   # explicit: with the default the cosine test compares 1.0 with 1 - eps, and the restatement's relative margin reads 1e-6
DBL_MAX = float(np.finfo(np.float64).max)
f32 = np.float32
SIZES = (700, 350, 257, 256, 65, 23)
# name: (k of pair_seed(73, k), reciprocal, transformation_epsilon)
BATCHES = {"A": (0, False, 1e-5), "B": (1, True, 1e-5), "C": (1, False, 1e-6), "D": (0, True, 1e-4)}
_CPU_RUNS = {}


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


@pytest.fixture(scope="module")
def icp(reg):
    return importlib.import_module("riv-slam_amd.icp")


def batch_fixture(scene, name):
    """(target, [(source prefix, guess)], reciprocal, transformation_epsilon) of one of the batches A .. D."""
    k, recip, eps = BATCHES[name]
    src, tgt, _, guess = scene.make_pair(700, 600, scene.pair_seed(73, k), "odometry")
    pairs = []
    for j, m in enumerate(SIZES):
        P = scene.make_transform(np.array([0.04 * j, -0.03 * j, 0.01 * j]), 0.003 * j, 0.0, 0.0)
        pairs.append((src[:m], (P @ guess.astype(np.float64)).astype(f32)))
    return tgt, pairs, recip, eps


def cpu_runs(scene, name):
    """The restatement's align of every pair of a batch, computed once per session."""
    if name not in _CPU_RUNS:
        tgt, pairs, recip, eps = batch_fixture(scene, name)
        _CPU_RUNS[name] = [I.align(s, tgt, g, max_iterations=10, transformation_epsilon=eps, max_dist=GATE, reciprocal=recip, rotation_epsilon=ROT_EPS, want_second=True)
                           for s, g in pairs]
    return _CPU_RUNS[name]


# ====================================================================== CPU
def test_new_symbols_are_exported_and_the_class_imports(reg, icp):
    L = reg.load_library()
    header = open(os.path.join(ROOT, "include", "apdgicp_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in reg.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
    for i in range(11, 17):
        assert re.search(r"\bIC%d\. " % i, header), f"IC{i} is missing from the header"
    assert "Not built: batch handles" not in header
    assert L.apdgicp_abi_version() == 6
    assert issubclass(icp.BatchICP, reg.BatchAPDGICP)
    for m in ("setUseReciprocalCorrespondences", "setEuclideanFitnessEpsilon", "setTransformationRotationEpsilon", "setMinCorrespondences",
              "setMaximumIterationsSimilarTransforms", "setAbsoluteMSE", "setMaximumIterations", "setTransformationEpsilon", "setMaxCorrespondenceDistance",
              "states", "correspondences", "working_cloud", "trace", "debug_counts", "enable", "disable", "enabled", "get_icp",
              "align", "align_async", "synchronize", "fitness", "set_clouds"):
        assert callable(getattr(icp.BatchICP, m)), m


def test_set_icp_checks_its_parameters_before_the_handle(reg, icp):
    """Valid parameters reach the handle check (INVALID_ARG: the handle is null); bad ones are refused as INVALID_ARG whatever the handle."""
    L = reg.load_library()
    p = icp.default_icp_params()
    assert L.apdgicp_batch_set_icp(None, ctypes.byref(p)) == -1 and b"null" in L.apdgicp_last_error()
    p.min_correspondences = 0
    assert L.apdgicp_batch_set_icp(None, ctypes.byref(p)) == -1 and b"min_correspondences" in L.apdgicp_last_error()
    p = icp.default_icp_params()
    p.max_similar_transforms = -1
    assert L.apdgicp_batch_set_icp(None, ctypes.byref(p)) == -1 and b"max_similar_transforms" in L.apdgicp_last_error()
    p = icp.default_icp_params()
    p.rotation_epsilon = float("nan")
    assert L.apdgicp_batch_set_icp(None, ctypes.byref(p)) == -1 and b"not a number" in L.apdgicp_last_error()
    n = ctypes.c_int64()
    assert L.apdgicp_batch_get_icp(None, None, None) == -1
    assert L.apdgicp_batch_icp_states(None, None, 0) == -1
    assert L.apdgicp_batch_icp_get_correspondences(None, 0, None, None, 0) == -1
    assert L.apdgicp_batch_icp_get_working_cloud(None, 0, None, 0) == -1
    assert L.apdgicp_batch_icp_get_trace(None, 0, 0, None, None, None, None, ctypes.byref(n)) == -1
    assert L.apdgicp_batch_icp_debug_counts(None, None, None, None) == -1


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_fixture_margins_from_the_restatement_alone(scene, name):
    """The conditions of tests/test_icp.py for every pair, and pairs that stop after at least three different iteration counts."""
    runs = cpu_runs(scene, name)
    for j, want in enumerate(runs):
        assert min(want["margins"]) > 1e-3, (name, j, min(want["margins"]))
        assert want["min_gap_ulps"] > 4, (name, j, want["min_gap_ulps"])
    assert len({w["iterations"] for w in runs}) >= 3, [w["iterations"] for w in runs]


# ====================================================================== GPU
def params(icp, eps, max_iterations=10, **kw):
    return icp.pcl_params(max_correspondence_distance=GATE, transformation_epsilon=eps, max_iterations=max_iterations, **kw)


def configure(g, recip=False, rot_eps=ROT_EPS, linear=False, **setters):
    """The same setters on an ICP and on a BatchICP (linear: the single handle's setTransformOrder; a batch takes the flag with its parameters)."""
    g.setUseReciprocalCorrespondences(recip)
    g.setTransformationRotationEpsilon(rot_eps)
    for name, v in setters.items():
        getattr(g, name)(v)
    if linear:
        g.setTransformOrder(True)


def snap_single(g):
    tr = g.trace()
    m, s = g.correspondences()
    return (bytes(g.result), g.convergence_state(), tr["T_k"].tobytes(), tr["n_corr"].tobytes(), tr["mse"].tobytes(), tr["similar"].tobytes(), m.tobytes(), s.tobytes(),
            g.working_cloud().tobytes())


def snap_batch(b, res, i, states=None):
    tr = b.trace(i)
    m, s = b.correspondences(i)
    st = b.states() if states is None else states
    return (res[i].tobytes(), int(st[i]), tr["T_k"].tobytes(), tr["n_corr"].tobytes(), tr["mse"].tobytes(), tr["similar"].tobytes(), m.tobytes(), s.tobytes(),
            b.working_cloud(i).tobytes())


FIELDS = ("record", "state", "T_k", "n_corr", "mse", "similar", "match", "sq_dist", "W")


def assert_same(got, want, what):
    for f, a, b_ in zip(FIELDS, got, want):
        assert a == b_, (what, f)


def single_loop(icp, prm, tgt, pairs, **cfg):
    """One ICP handle, one pair after the other: the snapshots the batch is compared with."""
    g = icp.ICP(prm, device=0)
    configure(g, **cfg)
    out = []
    for s, guess in pairs:
        g.setInputSource(s)
        g.setInputTarget(tgt if not isinstance(tgt, list) else tgt[len(out)])
        g.align(guess)
        out.append(snap_single(g))
    g.close()
    return out


def batch_run(b, tgt, pairs, order=None):
    """clouds: the target in slot 0, the sources behind it; returns the snapshots in the order of `pairs`."""
    b.clear()
    b.set_clouds(0, [tgt, *[s for s, _ in pairs]])
    order = list(range(len(pairs))) if order is None else list(order)
    res = b.align([(1 + i, 0) for i in order], [pairs[i][1] for i in order])
    st = b.states()
    snaps = [None] * len(pairs)
    for pos, i in enumerate(order):
        snaps[i] = snap_batch(b, res, pos, st)
    return snaps, res


def make_batch(icp, reg, eps, recip=False, linear=False, max_iterations=10, rot_eps=ROT_EPS, **setters):
    prm = params(icp, eps, max_iterations)
    if linear:
        prm.flags |= reg.FLAG_XF_LINEAR_CHAIN
    b = icp.BatchICP(prm, device=0)
    configure(b, recip, rot_eps, **setters)
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("linear", (False, True))
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_batches_against_the_single_handle(reg, icp, scene, name, linear):
    """IC13, traps 1 and 2: T_k applied once per iteration (the final W), the search cold (every trace entry)."""
    tgt, pairs, recip, eps = batch_fixture(scene, name)
    want = single_loop(icp, params(icp, eps), tgt, pairs, recip=recip, linear=linear)
    b = make_batch(icp, reg, eps, recip, linear)
    got, res = batch_run(b, tgt, pairs)
    for i in range(len(pairs)):
        assert_same(got[i], want[i], (name, linear, i))
    assert len({int(r["iterations"]) for r in res}) >= 3
    assert b.last_ticks()[0] == b.debug_counts()[2] <= 10
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_batches_against_the_restatement(reg, icp, scene, name):
    tgt, pairs, recip, eps = batch_fixture(scene, name)
    runs = cpu_runs(scene, name)
    b = make_batch(icp, reg, eps, recip)
    _, res = batch_run(b, tgt, pairs)
    st = b.states()
    for i, want in enumerate(runs):
        assert min(want["margins"]) > 1e-3 and want["min_gap_ulps"] > 4
        assert (int(st[i]), int(res[i]["iterations"]), int(res[i]["n_matched"]), bool(res[i]["converged"])) == \
            (want["state"], want["iterations"], want["n_matched"], want["converged"]), (name, i)
        te, re_ = scene.pose_error(want["T"], reg.result_matrix(res[i]))
        assert te <= 1e-3 and re_ <= 1e-4, (name, i, te, re_)
    b.close()


@pytest.mark.gpu
def test_sizes(reg, icp, scene):
    """Sources of 1 .. 2 048 points in one batch (blocks that are not full, more than one block, pairs without three matches), then 65
    pairs in one align (the one-lane-per-pair kernels cover 64 pairs per block)."""
    src, tgt, _, guess = scene.make_pair(2048, 2048, 20241023, "odometry")
    guess = guess.astype(f32)
    for recip in (False, True):
        pairs = [(src[:n], guess) for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 2048)]
        want = single_loop(icp, params(icp, 1e-5), tgt, pairs, recip=recip)
        b = make_batch(icp, reg, 1e-5, recip)
        got, _ = batch_run(b, tgt, pairs)
        for i in range(len(pairs)):
            assert_same(got[i], want[i], (recip, len(pairs[i][0])))
        b.close()
    pairs = [(src[7 * i:7 * i + 23 + i], guess) for i in range(65)]
    want = single_loop(icp, params(icp, 1e-5), tgt[:600], pairs)
    b = make_batch(icp, reg, 1e-5)
    got, _ = batch_run(b, tgt[:600], pairs)
    for i in range(65):
        assert_same(got[i], want[i], ("65 pairs", i))
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("A", "D"))
def test_a_pair_gives_the_same_bytes_wherever_it_runs(reg, icp, scene, name):
    """IC14, trap 3 (the stale rows of an earlier, larger align)."""
    tgt, pairs, recip, eps = batch_fixture(scene, name)
    b = make_batch(icp, reg, eps, recip)
    base, _ = batch_run(b, tgt, pairs)
    again, _ = batch_run(b, tgt, pairs)                       # the batch repeated on the same handle
    rev, _ = batch_run(b, tgt, pairs, order=range(len(pairs) - 1, -1, -1))
    for i in range(len(pairs)):
        assert_same(again[i], base[i], ("repeated", i))
        assert_same(rev[i], base[i], ("reversed", i))
    for i in range(len(pairs)):                                # each pair alone, on the reused handle and on a fresh one
        alone, _ = batch_run(b, tgt, pairs[i:i + 1])
        assert_same(alone[0], base[i], ("alone", i))
    fresh = make_batch(icp, reg, eps, recip)
    alone, _ = batch_run(fresh, tgt, pairs[5:6])
    assert_same(alone[0], base[5], "alone on a fresh handle")
    # after an align of fewer and smaller pairs, and after one of more and larger pairs
    big_src, big_tgt, _, big_guess = scene.make_pair(2048, 900, scene.pair_seed(73, 5), "odometry")
    batch_run(fresh, tgt, pairs[4:6])
    after_small, _ = batch_run(fresh, tgt, pairs)
    batch_run(fresh, big_tgt, [(big_src[:n], big_guess.astype(f32)) for n in (2048, 1500, 1025, 1024, 700, 512, 300, 77)])
    after_big, _ = batch_run(fresh, tgt, pairs)
    for i in range(len(pairs)):
        assert_same(after_small[i], base[i], ("after a smaller align", i))
        assert_same(after_big[i], base[i], ("after a larger align", i))
    fresh.close()
    # two pairs sharing source and target slot with different guesses; a pair whose source and target are one slot
    b.clear()
    b.set_clouds(0, [tgt, pairs[0][0]])
    guesses = [pairs[0][1], pairs[3][1], np.eye(4, dtype=f32), pairs[1][1]]
    res = b.align([(1, 0), (1, 0), (0, 0), (1, 1)], guesses)
    st = b.states()
    shared = [snap_batch(b, res, i, st) for i in range(4)]
    assert_same(shared[0], base[0], "shared slots, the first guess")
    other = single_loop(icp, params(icp, eps), [tgt, tgt, tgt, pairs[0][0]], [(pairs[0][0], guesses[1]), (pairs[0][0], guesses[1]), (tgt, guesses[2]), (pairs[0][0], guesses[3])],
                        recip=recip)
    for i in (1, 2, 3):
        assert_same(shared[i], other[i], ("shared slots", i))
    assert np.array_equal(b.correspondences(2)[0], np.arange(len(tgt)))   # a cloud against itself: every point its own match
    b.close()


CHILD = r"""
import hashlib, importlib, json, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import test_icp_batch as T
scene = importlib.import_module("riv-slam_amd.scene")
reg = importlib.import_module("riv-slam_amd.registration")
icp = importlib.import_module("riv-slam_amd.icp")
out = {}
for name in %(names)r:
    tgt, pairs, recip, eps = T.batch_fixture(scene, name)
    b = T.make_batch(icp, reg, eps, recip)
    snaps, _ = T.batch_run(b, tgt, pairs)
    launches, waits, ticks = b.debug_counts()
    out[name] = dict(digest=[hashlib.sha256(repr(s).encode()).hexdigest() for s in snaps], launches=launches, waits=waits, ticks=ticks)
    b.close()
print("RESULT " + json.dumps(out))
"""


def run_child(names, env):
    e = dict(os.environ)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, names=tuple(names))], env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    import json
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])


def digests(snaps):
    import hashlib
    return [hashlib.sha256(repr(s).encode()).hexdigest() for s in snaps]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", (1, 16))
def test_chunk_length_changes_nothing(reg, icp, scene, chunk):
    """APDGICP_VGB_CHUNK = 1 and a value beyond max_iterations, each in a process of its own: the same bytes, ticks within the bound."""
    got = run_child(("A", "B"), {"APDGICP_VGB_CHUNK": str(chunk)})
    for name in ("A", "B"):
        tgt, pairs, recip, eps = batch_fixture(scene, name)
        b = make_batch(icp, reg, eps, recip)
        snaps, _ = batch_run(b, tgt, pairs)
        b.close()
        assert got[name]["digest"] == digests(snaps), name
        assert 1 <= got[name]["ticks"] <= 10
        assert got[name]["waits"] <= -(-got[name]["ticks"] // chunk) + 2
        assert got[name]["launches"] == 2 + got[name]["ticks"] * (10 if recip else 7)


@pytest.mark.gpu
def test_brute_reciprocal_search_gives_the_same_records(reg, icp, scene):
    got = run_child(("B", "D"), {"APDGICP_ICP_RECIP_MODE": "brute"})
    for name in ("B", "D"):
        tgt, pairs, recip, eps = batch_fixture(scene, name)
        b = make_batch(icp, reg, eps, recip)
        snaps, _ = batch_run(b, tgt, pairs)
        b.close()
        assert got[name]["digest"] == digests(snaps), name
        assert got[name]["launches"] == 2 + got[name]["ticks"] * 8


def rigid_copy(scene, n, seed, t=(0.05, -0.02, 0.01), ypr=(0.004, -0.002, 0.003)):
    """tests/test_icp.py's: a noise-free rigid copy at a small motion."""
    rng = np.random.default_rng(seed)
    src = (rng.uniform(-1, 1, size=(n, 3)) * [30, 30, 4]).astype(f32)
    T = scene.make_transform(t, *ypr)
    tgt = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(f32)
    return src, tgt, T


def run_with_targets(b, clouds, pair_slots, guesses):
    b.clear()
    b.set_clouds(0, clouds)
    res = b.align(pair_slots, guesses)
    st = b.states()
    return [snap_batch(b, res, i, st) for i in range(len(pair_slots))], res, st


@pytest.mark.gpu
def test_every_convergence_state_inside_a_batch(reg, icp, scene):
    """The fixtures of tests/test_icp.py::test_every_convergence_state, one batch per parameter set; every batch also holds a pair from a
    far guess that runs longer.  Each pair against the single handle as bytes, the states as that test asserts them."""
    src, tgt, _, guess = scene.make_pair(2048, 2048, 20241023, "odometry")
    src, tgt, guess = src[:800], tgt[:1000], guess.astype(f32)
    far = (scene.make_transform(np.array([0.6, -0.5, 0.1]), 0.03, 0.0, 0.0) @ guess.astype(np.float64)).astype(f32)
    s2, t2, _ = rigid_copy(scene, 400, 9)
    eye = np.eye(4, dtype=f32)
    clouds = [tgt, src, src[:500], t2, s2]
    slots = [(1, 0), (2, 0), (4, 3)]
    guesses = [guess, far, eye]
    tgts = [tgt, tgt, t2]
    srcs = [src, src[:500], s2]
    # (eps, max_iterations, rot_eps, setters, the pair the expectation is about, state, iterations)
    cases = (
        (0.01, 10, 0.0, {}, 0, icp.TRANSFORM, 1),
        (0.01, 10, 0.0, {"setMaximumIterationsSimilarTransforms": 2}, 0, icp.TRANSFORM, 3),
        (1e-8, 5, 0.0, {}, 0, icp.ITERATIONS, 5),
        (1e-8, 50, 2.0, {"setEuclideanFitnessEpsilon": 0.5}, 0, icp.REL_MSE, 2),
        (1e-8, 50, 2.0, {}, 2, icp.ABS_MSE, None),
        (1e-8, 0, 0.0, {}, 0, icp.ITERATIONS, 1),
        (1e-8, 1, 0.0, {}, 0, icp.ITERATIONS, 1),
    )
    for eps, max_it, rot, setters, which, state, iters in cases:
        what = (eps, max_it, rot, tuple(setters))
        want = single_loop(icp, params(icp, eps, max_it), tgts, list(zip(srcs, guesses)), rot_eps=rot, **setters)
        b = make_batch(icp, reg, eps, max_iterations=max_it, rot_eps=rot, **setters)
        got, res, st = run_with_targets(b, clouds, slots, guesses)
        for i in range(3):
            assert_same(got[i], want[i], (what, i))
        assert int(st[which]) == state and bool(res[which]["converged"]), what
        if iters is not None:
            assert int(res[which]["iterations"]) == iters, what
        else:
            assert 2 <= int(res[which]["iterations"]) < 50, what
        if max_it >= 5:   # the pair from the far guess is still running when the expected one stops (or every pair runs to the bound)
            assert int(res[1]["iterations"]) >= int(res[which]["iterations"]) or which == 2, what
        if setters.get("setMaximumIterationsSimilarTransforms") == 2:
            assert b.trace(0)["similar"].tolist() == [1, 2, 2]
        assert b.debug_counts()[2] <= max(1, max_it)
        b.close()
    # NO_CORRESPONDENCES with 2 matches at the first iteration (trap 4), beside 3 matches and beside a pair that runs on
    s3 = np.array([[0, 0, 0], [0, 0, 100], [0, 50, 200]], dtype=f32)
    t3a = s3 + np.array([[0.5, 0, 0], [0.5, 0, 0], [3.0, 0, 0]], dtype=f32)
    t3b = s3 + np.array([[0.5, 0, 0], [0.5, 0, 0], [2.0, 0, 0]], dtype=f32)
    gs = scene.make_transform([0.01, 0, 0]).astype(f32)
    for eps in (0.5, 1e-8):
        clouds = [s3, t3a, t3b, src, tgt]
        slots = [(3, 4), (0, 1), (0, 2), (3, 4)]
        guesses = [far, gs, gs, guess]
        want = single_loop(icp, params(icp, eps, 4), [tgt, t3a, t3b, tgt], [(src, far), (s3, gs), (s3, gs), (src, guess)], rot_eps=0.0)
        b = make_batch(icp, reg, eps, max_iterations=4, rot_eps=0.0)
        got, res, st = run_with_targets(b, clouds, slots, guesses)
        for i in range(4):
            assert_same(got[i], want[i], (eps, i))
        assert int(st[1]) == icp.NO_CORRESPONDENCES and not res[1]["converged"] and int(res[1]["iterations"]) == 0 and int(res[1]["n_matched"]) == 2
        assert np.asarray(res[1]["T"], dtype=f32).tobytes() == np.ascontiguousarray(gs.T).tobytes()      # T = guess
        assert int(res[2]["n_matched"]) == 3 and bool(res[2]["converged"]) and int(res[2]["iterations"]) >= 1
        if eps == 0.5:
            assert int(st[2]) == icp.TRANSFORM
        else:
            assert int(res[0]["iterations"]) == 4 and int(res[3]["iterations"]) == 4      # the neighbours ran on to the bound
        assert len(b.trace(1)["n_corr"]) == 1
        b.close()


@pytest.mark.gpu
def test_non_finite_source_points_in_one_pair(reg, icp, scene):
    tgt, pairs, recip, eps = batch_fixture(scene, "A")
    b = make_batch(icp, reg, eps, recip)
    base, _ = batch_run(b, tgt, pairs)
    bad = pairs[1][0].copy()
    bad[5] = np.nan
    bad[300, 1] = np.inf
    dirty = list(pairs)
    dirty[1] = (bad, pairs[1][1])
    got, res = batch_run(b, tgt, dirty)
    for i in (0, 2, 3, 4, 5):
        assert_same(got[i], base[i], ("beside a pair with non-finite points", i))
    W = b.working_cloud(1)
    m, sq = b.correspondences(1)
    for r in (5, 300):
        assert np.all(np.isnan(W[r])) and m[r] == -1 and np.isnan(sq[r])
    assert np.all(np.isfinite(np.delete(W, (5, 300), axis=0)))
    want = single_loop(icp, params(icp, eps), tgt, [dirty[1]], recip=recip)
    assert_same(got[1], want[0], "the pair itself")
    b.close()


@pytest.mark.gpu
def test_mode_rules(reg, icp, scene):
    L = reg.load_library()
    vg = importlib.import_module("riv-slam_amd.vgicp")
    nd = importlib.import_module("riv-slam_amd.ndt")
    lv = importlib.import_module("riv-slam_amd.loop_verifier")
    src, tgt, _, guess = scene.make_pair(2048, 2048, 20241023, "odometry")
    src, tgt, guess = src[:600], tgt[:800], guess.astype(f32)
    kw = dict(max_correspondence_distance=2.0, transformation_epsilon=0.01)
    fresh = reg.BatchAPDGICP(reg.default_params(**kw), device=0)
    fresh.set_clouds(0, [tgt, src, src[:300]])
    rec_apd = fresh.align([(1, 0), (2, 0)], [guess, guess]).tobytes()
    fresh.close()
    b = icp.BatchICP(reg.default_params(**kw), device=0)
    assert b.enabled() and b.get_icp()[0].min_correspondences == 3
    # exclusivity with batch VGICP and NDT, both ways
    on = ctypes.c_int()
    assert L.apdgicp_batch_set_vgicp(b.b, ctypes.byref(vg.default_vgicp_params())) == 0
    assert not b.enabled() and L.apdgicp_batch_get_vgicp(b.b, None, ctypes.byref(on)) == 0 and on.value == 1
    b.enable()
    assert b.enabled() and L.apdgicp_batch_get_vgicp(b.b, None, ctypes.byref(on)) == 0 and on.value == 0
    assert L.apdgicp_batch_set_ndt(b.b, ctypes.byref(nd.default_ndt_params())) == 0
    assert not b.enabled() and L.apdgicp_batch_get_ndt(b.b, None, ctypes.byref(on)) == 0 and on.value == 1
    b.enable()
    assert b.enabled() and L.apdgicp_batch_get_ndt(b.b, None, ctypes.byref(on)) == 0 and on.value == 0
    # the pool calls
    b.set_clouds(0, [tgt, src, src[:300]])
    pairs = b.make_pairs([(1, 0), (2, 0)], [guess, guess])
    ticket = ctypes.c_uint64()
    assert L.apdgicp_batch_align_enqueue(b.b, pairs, 2, ctypes.byref(ticket)) == -5
    assert L.apdgicp_batch_pump(b.b) == -5
    assert L.apdgicp_batch_align_collect(b.b, 1, None, None) == -5
    assert L.apdgicp_batch_is_pooled(b.b) == 0
    b.set_pair_groups(1)      # accepted, no effect
    with pytest.raises(reg.ApdgicpError) as ei:
        b.states()            # nothing aligned yet
    assert ei.value.code == -3
    # an ICP align; fitness(T=None) scores the records' T
    res = b.align(pairs)
    assert np.all(res["converged"] == 1) and np.all(b.states() == icp.TRANSFORM)
    s_none, i_none = b.fitness(pairs, None, 4.0)
    s_T, i_T = b.fitness(pairs, np.stack([reg.result_matrix(r) for r in res]), 4.0)
    assert s_none.tobytes() == s_T.tobytes() and i_none.tobytes() == i_T.tobytes() and np.all(i_none > 100)
    s_g, _ = b.fitness(pairs, np.stack([guess, guess]), 4.0)
    assert np.all(s_none < s_g)       # (the aligned poses, not the guesses or the identity)
    # with the mode off again: the bytes of a handle that never had it on
    b.disable()
    assert not b.enabled()
    assert b.align(pairs).tobytes() == rec_apd
    with pytest.raises(reg.ApdgicpError):
        b.states()
    # clouds smaller than k_correspondences align
    b.enable()
    s5, t5, T5 = rigid_copy(scene, 5, 12)
    b.clear()
    b.set_clouds(0, [t5, s5])
    b.setMaxCorrespondenceDistance(1.0)
    b.setTransformationEpsilon(1e-10)
    b.setMaximumIterations(3)
    r5 = b.align([(1, 0)])
    assert int(r5[0]["n_matched"]) == 5 and np.abs(reg.result_matrix(r5[0]).astype(np.float64) - T5).max() <= 1e-5
    with pytest.raises(reg.ApdgicpError) as ei:
        b.working_cloud(1)    # not a pair of the last align
    assert ei.value.code == -1
    b.set_cloud(1, s5)
    with pytest.raises(reg.ApdgicpError) as ei:
        b.working_cloud(0)    # a slot was set since
    assert ei.value.code == -3
    b.close()
    # loop verification: the candidate the single-handle loop picks
    cands, guesses = [], []
    for k in range(4):
        cs, _, _, cg = scene.make_pair(600, 800, scene.pair_seed(74, k), "odometry")
        cands.append(cs if k != 2 else src)
        guesses.append(cg.astype(f32) if k != 2 else guess)
    prm = icp.pcl_params(max_correspondence_distance=GATE, transformation_epsilon=1e-5)
    b = icp.BatchICP(prm, device=0)
    loop, scores, results = lv.verify_candidates(b, tgt, cands, guesses, fitness_score_thresh=1e9)
    g = icp.ICP(prm, device=0)
    best, best_score = -1, DBL_MAX
    for k in range(4):
        g.setInputSource(cands[k])
        g.setInputTarget(tgt)
        T = g.align(guesses[k])
        assert bytes(g.result) == results[k].tobytes()
        s = g.getFitnessScore(T=T)
        assert abs(s - scores[k]) <= 1e-9 * s
        if g.hasConverged() and s <= best_score:
            best, best_score = k, s
    assert loop is not None and loop.candidate == best == 2
    g.close()
    b.close()


@pytest.mark.gpu
def test_launches_per_tick_do_not_depend_on_the_batch(reg, icp, scene, monkeypatch):
    monkeypatch.delenv("APDGICP_VGB_CHUNK", raising=False)
    monkeypatch.delenv("APDGICP_ICP_RECIP_MODE", raising=False)
    tgt, pairs, _, eps = batch_fixture(scene, "A")
    for recip, per_tick in ((False, 7), (True, 10)):
        counts = []
        for n in (1, 32):
            b = make_batch(icp, reg, eps, recip)
            batch_run(b, tgt, [pairs[i % 6] for i in range(n)])
            launches, waits, ticks = b.debug_counts()
            assert 1 <= ticks <= 10 and b.last_ticks()[0] == ticks
            assert (launches - 2) % ticks == 0
            assert waits <= -(-ticks // 4) + 2      # (chunks of 4 ticks by default)
            counts.append((launches - 2) // ticks)
            b.close()
        assert counts == [per_tick, per_tick], (recip, counts)
