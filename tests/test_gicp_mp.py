"""FastGICPMultiPoints on the device (MP1 .. MP11 of include/apdgicp_hip.h; kernels: riv-slam_amd/csrc/apd_gicp_mp.hpp) against the literal
restatement tests/gicp_mp_np.py and against the public radius query of the same handle.  The covariances are the device's own (read back
through getSourceCovariances / getTargetCovariances) or stored ones: the restatement restates what the mode does with them.

Bars: rows byte for byte; sum_w / mean_B / cov_B 1e-12 relative; H / g / cost 1e-10 relative (the project's bar), n_matched exact; traces
teacher-forced (cost 1e-10, n_matched exact, delta 1e-10, the restatement's update of a traced pose by the traced delta gives the next
traced pose within 1e-12); end states equal to the free-running restatement on the fixtures of tests/gicp_mp_cases.py.

Measured on an MI355X (the tests print the figures before they assert): sum_w / mean_B / cov_B differ from the restatement by 0.0 on both
pairs (rows up to 66 entries long) -- the order is written and contraction is off; H 1.8e-16, g 1.9e-16, cost 0.0 relative at the guess
(numpy sums the points pairwise, the device in lane / wave / block order); over the traced iterations cost at most 4.0e-16, delta at most
8.9e-12 (the solve amplifies the difference of the sums by the condition of H), the next pose 0.0."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gicp_mp_cases as cases  # noqa: E402
import gicp_mp_np as rnp  # noqa: E402

gpu = pytest.mark.gpu
STATES = ("NOT_CONVERGED", "CONVERGED", "TOO_FEW_ROWS", "SINGULAR")
UNSUPPORTED, TOO_FEW = -5, -4


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


@pytest.fixture(scope="module")
def gmp(reg):
    return importlib.import_module("riv-slam_amd.gicp_mp")


@pytest.fixture(scope="module")
def pairs():
    return {name: cases.scene_pair(name) for name in cases.PAIRS}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def handle(gmp, src, tgt, radius, linear=False, **kw):
    g = gmp.FastGICPMultiPoints(gmp.class_params(**kw))
    if linear:
        g.setTransformOrder(True)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    g.setNeighborSearchRadius(radius)
    return g


def same_rows(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def lin_bytes(g, T):
    cost, H, b = g.linearize(T)
    return np.float64(cost).tobytes() + H.tobytes() + b.tobytes() + b"".join(x.tobytes() for x in g.rows()) + b"".join(x.tobytes() for x in g.fused().values())


# ---------------------------------------------------------------------- rows
SIZES = [(20, 20), (63, 700), (64, 1700), (65, 700), (255, 1700), (256, 20), (257, 700), (1500, 1700)]


@gpu
@pytest.mark.parametrize("ns, nt", SIZES, ids=[f"{a}x{b}" for a, b in SIZES])
def test_rows_are_the_radius_query_of_the_transformed_source(gmp, pairs, ns, nt):
    src, tgt, guess, _ = pairs["converged_r2.0"]
    src, tgt, r = src[:ns], tgt[:nt], 2.0
    g = handle(gmp, src, tgt, r)
    g.linearize(guess.astype(np.float64))
    got = g.rows()
    q = rnp.queries(guess, src)
    assert same_rows(got, rnp.rows(q, tgt, r))
    assert same_rows(got, g.radiusSearchOf(q, r))
    assert same_rows(got, g.rows())   # Q7 / MP9: the Q call in between changed nothing of the mode's rows
    g.close()


@pytest.fixture(scope="module")
def crafted():
    """source and target with: an empty row (0), a row of one (1), a row of 70 (2), duplicated target points (3), the d2 == r2 point (4: the
    source point is the origin, the target point (0.5, 0, 0), r = 0.5), and 40 scattered points each so that both clouds have k points"""
    rng = np.random.default_rng(7)
    src = np.concatenate([np.array([[50, 50, 50], [10, 0, 0], [20, 0, 0], [30, 0, 0], [0, 0, 0]], dtype=np.float32),
                          rng.uniform(-40, -20, (40, 3)).astype(np.float32)])
    tgt = np.concatenate([np.array([[10.2, 0, 0]], dtype=np.float32),
                          (np.array([20, 0, 0]) + rng.uniform(-0.1, 0.1, (70, 3))).astype(np.float32),
                          np.repeat(np.array([[30.1, 0.1, 0]], dtype=np.float32), 3, axis=0), np.array([[30.1, 0.1, 0.2]], dtype=np.float32),
                          np.array([[0.5, 0, 0]], dtype=np.float32),
                          rng.uniform(-40, -20, (40, 3)).astype(np.float32)])
    return src, tgt


@gpu
@pytest.mark.parametrize("linear", [False, True], ids=["pairwise", "linear_chain"])
def test_rows_of_the_crafted_cases(gmp, crafted, pairs, linear):
    src, tgt = crafted
    g = handle(gmp, src, tgt, 0.5, linear)
    g.linearize(np.eye(4))
    rs, idx, d2 = got = g.rows()
    lens = np.diff(rs)
    assert lens[0] == 0 and lens[1] == 1 and lens[2] == 70 and lens[3] == 4 and lens[4] == 0
    assert idx[rs[3]:rs[3] + 3].tolist() == [71, 72, 73]   # ties: ascending index
    assert same_rows(got, rnp.rows(rnp.queries(np.eye(4), src, linear), tgt, 0.5))
    g.close()
    # both transform orders at a pose that is not the identity
    s2, t2, guess, _ = pairs["converged_r2.0"]
    g = handle(gmp, s2[:257], t2[:700], 2.0, linear)
    g.linearize(guess.astype(np.float64))
    assert same_rows(g.rows(), rnp.rows(rnp.queries(guess, s2[:257], linear), t2[:700], 2.0))
    g.close()


@gpu
def test_a_non_finite_source_point_has_an_empty_row(gmp, pairs):
    src, tgt, guess, _ = pairs["converged_r2.0"]
    src, tgt = src[:257].copy(), tgt[:700]
    src[5] = (np.nan, 0, 0)
    src[64] = (1.0, np.inf, 0)
    src[200] = (0, 0, -np.inf)
    cs, ct = cases.spd_covs(257, 1), cases.spd_covs(700, 2)
    g = handle(gmp, src, tgt, 2.0)
    g.setSourceCovariances(cs), g.setTargetCovariances(ct)
    T = guess.astype(np.float64)
    cost, H, b = g.linearize(T)
    got = g.rows()
    lens = np.diff(got[0])
    assert lens[5] == 0 and lens[64] == 0 and lens[200] == 0 and lens.sum() > 0
    assert same_rows(got, rnp.rows(rnp.queries(guess, src), tgt, 2.0))
    want = rnp.linearize(T, src, tgt, cs, ct, 2.0)
    assert np.isfinite(H).all() and rel(H, want["H"]) <= 1e-10 and rel(b, want["g"]) <= 1e-10 and rel(cost, want["cost"]) <= 1e-10
    g.close()


# ---------------------------------------------------------------------- fused terms, H, g, cost
@gpu
@pytest.mark.parametrize("name", ["converged_r2.0", "max_iterations"])
def test_fused_terms_and_sums(gmp, pairs, name):
    src, tgt, guess, r = pairs[name]
    g = handle(gmp, src, tgt, r)
    cs, ct = g.getSourceCovariances()[:, :3, :3], g.getTargetCovariances()[:, :3, :3]
    T = guess.astype(np.float64)
    cost, H, b = g.linearize(T)
    f = g.fused()
    want = rnp.linearize(T, src, tgt, cs, ct, r)
    e = {k: rel(f[k], want[k]) for k in ("sum_w", "mean_B", "cov_B")}
    eH, eg, ec = rel(H, want["H"]), rel(b, want["g"]), rel(cost, want["cost"])
    print(f"{name}: rows up to {np.diff(g.rows()[0]).max()} long; fused {e}; H {eH:.3e} g {eg:.3e} cost {ec:.3e}")
    assert same_rows(g.rows(), want["rows"])
    assert max(e.values()) <= 1e-12
    assert eH <= 1e-10 and eg <= 1e-10 and ec <= 1e-10
    assert np.array_equal(H, H.T) and g.getFinalHessian().tobytes() == H.tobytes()   # MP9: the last H
    g.setMaximumIterations(1)   # n_matched of that pose: the record and the trace of an align of one iteration
    g.align(guess)
    assert g.result.n_matched == want["n_matched"] and g.trace()["n_matched"].tolist() == [want["n_matched"]]
    g.close()


# ---------------------------------------------------------------------- traces and end states
@gpu
@pytest.mark.parametrize("name", list(cases.PAIRS))
def test_trace_teacher_forced_and_end_state_free_running(gmp, pairs, name):
    src, tgt, guess, r = pairs[name]
    g = handle(gmp, src, tgt, r)
    cs, ct = g.getSourceCovariances()[:, :3, :3], g.getTargetCovariances()[:, :3, :3]
    T = g.align(guess)
    tr = g.trace()
    k = len(tr["cost"])
    assert k == g.result.iterations + 1 == g.result.n_linearize and g.result.n_compute_error == 0 and g.result.lm_failed == 0
    assert tr["poses"][0].tobytes() == guess.astype(np.float64).tobytes()
    worst = {"cost": 0.0, "delta": 0.0, "pose": 0.0}
    for i in range(k):   # teacher-forced: every traced pose on its own
        lin = rnp.linearize(tr["poses"][i], src, tgt, cs, ct, r)
        assert lin["n_matched"] == tr["n_matched"][i]
        worst["cost"] = max(worst["cost"], rel(tr["cost"][i], lin["cost"]))
        worst["delta"] = max(worst["delta"], rel(tr["delta"][i], rnp.solve(lin["H"], lin["g"])))
        nxt = rnp.update(tr["poses"][i], tr["delta"][i])   # the restatement's update of the traced pose by the traced delta
        if i + 1 < k:
            worst["pose"] = max(worst["pose"], rel(tr["poses"][i + 1], nxt))
        else:
            assert T.tobytes() == nxt.astype(np.float32).tobytes() or rel(T, nxt) <= 2.0 ** -23   # the record's T is the fp32 pose
    print(name, "iterations", k, worst)
    assert worst["cost"] <= 1e-10 and worst["delta"] <= 1e-10 and worst["pose"] <= 1e-12
    assert g.result.final_cost == tr["cost"][-1] and g.result.n_matched == tr["n_matched"][-1]
    # free running
    out = rnp.align(src, tgt, cs, ct, r, guess, cases.MAX_ITERATIONS, cases.ROT_EPS, cases.TRANS_EPS)
    cases.check_margins(out, cases.PAIRS[name][4], STATES)
    assert (STATES[g.state()], g.result.iterations, bool(g.result.converged), g.result.n_matched) == (STATES[out["state"]], out["iterations"], out["converged"], out["n_matched"])
    assert g.hasConverged() == out["converged"]
    launches, waits = g.debug_counts()
    assert waits == 2 * k and launches <= 10 * k + 1
    g.close()


@gpu
def test_too_few_rows_and_singular(gmp, pairs):
    src, tgt, guess, r = cases.far_pair()
    g = handle(gmp, src, tgt, r)
    T = g.align(guess)
    assert (STATES[g.state()], g.result.iterations, g.result.n_matched, g.result.converged, g.result.n_linearize) == ("TOO_FEW_ROWS", 0, 0, 0, 1)
    assert T.tobytes() == guess.tobytes()
    assert g.rows()[0].tolist() == [0] * (len(src) + 1)
    g.close()
    src, tgt, guess, r = cases.one_hit_pair()
    g = handle(gmp, src, tgt, r)
    T = g.align(guess)
    assert (STATES[g.state()], g.result.iterations, g.result.n_matched, g.result.converged) == ("TOO_FEW_ROWS", 0, 1, 0)
    assert T.tobytes() == guess.tobytes() and g.rows()[1].tolist() == [7] and np.diff(g.rows()[0])[3] == 1
    g.close()
    src, tgt, guess, r = pairs["converged_r2.0"]
    src, tgt = src[:257], tgt[:700]
    g = handle(gmp, src, tgt, r)
    ct = g.getTargetCovariances()
    ct[:, 0, 0] = np.inf
    g.setTargetCovariances(ct)
    T = g.align(guess)
    assert (STATES[g.state()], g.result.iterations, g.result.converged) == ("SINGULAR", 0, 0) and g.result.n_matched >= 2
    assert T.tobytes() == guess.tobytes()
    out = rnp.align(src, tgt, g.getSourceCovariances()[:, :3, :3], ct[:, :3, :3], r, guess)
    assert (STATES[out["state"]], out["iterations"], out["n_matched"]) == ("SINGULAR", 0, g.result.n_matched)
    g.close()


# ---------------------------------------------------------------------- covariances and refusals
@gpu
def test_stored_covariances_are_the_ones_used_and_normalized_min_eig_runs(reg, gmp, pairs):
    src, tgt, guess, r = pairs["converged_r2.0"]
    src, tgt, T = src[:257], tgt[:700], guess.astype(np.float64)
    cs, ct = cases.spd_covs(257, 5), cases.spd_covs(700, 6)
    g = handle(gmp, src, tgt, r)
    own = g.linearize(T)
    g.setSourceCovariances(cs), g.setTargetCovariances(ct)
    cost, H, b = g.linearize(T)
    want = rnp.linearize(T, src, tgt, cs, ct, r)
    assert rel(H, want["H"]) <= 1e-10 and rel(b, want["g"]) <= 1e-10 and rel(cost, want["cost"]) <= 1e-10 and cost != own[0]
    assert max(rel(g.fused()[k], want[k]) for k in ("sum_w", "mean_B", "cov_B")) <= 1e-12
    g.close()
    g = handle(gmp, src, tgt, r, regularization=reg.REG_NORMALIZED_MIN_EIG)
    cost, H, b = g.linearize(T)
    want = rnp.linearize(T, src, tgt, g.getSourceCovariances()[:, :3, :3], g.getTargetCovariances()[:, :3, :3], r)
    assert rel(H, want["H"]) <= 1e-10 and rel(b, want["g"]) <= 1e-10 and rel(cost, want["cost"]) <= 1e-10 and cost != own[0]
    g.close()


@gpu
@pytest.mark.parametrize("method", ["REG_MIN_EIG", "REG_FROBENIUS", "REG_NONE"])
def test_regularizations_on_the_undivided_scatter_are_refused(reg, gmp, pairs, method):
    src, tgt, guess, r = pairs["converged_r2.0"]
    src, tgt, T = src[:257], tgt[:700], guess.astype(np.float64)
    m = getattr(reg, method)
    # switching the mode on is refused, and the handle stays what it was: an APD-GICP handle
    a = reg.FastAPDGICP(reg.default_params(regularization=m, max_iterations=2))
    a.setInputSource(src), a.setInputTarget(tgt)
    before = a.linearize(T)
    p, on = gmp.default_gicp_mp_params(), C.c_int32(-1)
    assert a.L.apdgicp_set_gicp_mp(a.h, C.byref(p)) == UNSUPPORTED
    assert a.L.apdgicp_get_gicp_mp(a.h, None, C.byref(on)) == 0 and on.value == 0
    after = a.linearize(T)
    assert before[0] == after[0] and before[1].tobytes() == after[1].tobytes()
    a.close()
    # with the mode on, the first linearize / align after the parameter change is refused and the mode stays on
    g = handle(gmp, src, tgt, r)
    good = lin_bytes(g, T)
    g.setRegularizationMethod(m)
    assert g.L.apdgicp_linearize(g.h, np.asfortranarray(T).ctypes.data_as(C.c_void_p), None, None, C.byref(C.c_double())) == UNSUPPORTED
    assert g.L.apdgicp_align(g.h, None, C.byref(type(g.result)())) == UNSUPPORTED
    assert g.enabled()
    g.setRegularizationMethod(reg.REG_PLANE)
    assert lin_bytes(g, T) == good
    g.close()


@gpu
def test_a_cloud_of_19_points_is_refused(gmp, pairs):
    src, tgt, guess, r = pairs["converged_r2.0"]
    T = np.asfortranarray(guess.astype(np.float64))
    for s, t in ((src[:19], tgt[:700]), (src[:257], tgt[:19])):
        g = handle(gmp, s, t, r)
        assert g.L.apdgicp_linearize(g.h, T.ctypes.data_as(C.c_void_p), None, None, C.byref(C.c_double())) == TOO_FEW
        assert g.L.apdgicp_align(g.h, None, C.byref(type(g.result)())) == TOO_FEW
        g.close()


@gpu
def test_unsupported_calls_and_the_calls_that_keep_working(gmp, pairs):
    src, tgt, guess, r = pairs["converged_r2.0"]
    src, tgt, T = src[:257], tgt[:700], guess.astype(np.float64)
    g = handle(gmp, src, tgt, r)
    good = lin_bytes(g, T)
    with pytest.raises(Exception, match="-5"):
        g.compute_error(T)
    with pytest.raises(Exception, match="-5"):
        g.correspondences()
    with pytest.raises(Exception, match="-5"):
        g.mahalanobis()
    assert np.isfinite(g.getFitnessScore(T=guess)) and 0.0 <= g.inlierFraction(0.5, T=guess) <= 1.0
    assert g.nearestNeighbours(guess)[0].shape == (257,) and g.transformSource(guess).shape == (257, 3)
    assert g.nearestKSearchOf(src[:5], 3)[0].shape == (5, 3)
    assert lin_bytes(g, T) == good
    T1 = g.align(guess)
    T2 = g.align(guess, host_loop=True)   # MP9: the same loop
    assert T1.tobytes() == T2.tobytes()
    g.close()


# ---------------------------------------------------------------------- reused handles, determinism
@gpu
def test_a_reused_handle_gives_the_bytes_of_a_fresh_one(gmp, pairs):
    src, tgt, guess, _ = pairs["converged_r2.0"]
    src, tgt, tgt2, T = src[:257], tgt[:700], tgt[700:1500], guess.astype(np.float64)

    def fresh(s, t, r):
        g = handle(gmp, s, t, r)
        out = lin_bytes(g, T)
        g.close()
        return out

    g = handle(gmp, src, tgt, 2.0)
    assert lin_bytes(g, T) == fresh(src, tgt, 2.0)
    g.setNeighborSearchRadius(0.5)
    assert lin_bytes(g, T) == fresh(src, tgt, 0.5)
    g.setNeighborSearchRadius(2.0)
    g.setInputTarget(tgt2)
    assert lin_bytes(g, T) == fresh(src, tgt2, 2.0)
    g.swapSourceAndTarget()
    assert lin_bytes(g, T) == fresh(tgt2, src, 2.0)
    g.swapSourceAndTarget()
    g.linearize(T)
    g.radiusSearchOf(src[:50] + np.float32(0.3), 1.0)
    assert lin_bytes(g, T) == fresh(src, tgt2, 2.0)
    g.close()


@gpu
def test_the_same_bytes_on_two_runs(gmp, pairs):
    src, tgt, guess, r = pairs["converged_r0.5"]
    runs = []
    for _ in range(2):
        g = handle(gmp, src, tgt, r)
        g.align(guess)
        tr = g.trace()
        runs.append(bytes(g.result) + b"".join(v.tobytes() for v in tr.values()) + g.getFinalHessian().tobytes() + b"".join(x.tobytes() for x in g.rows()))
        g.close()
    assert runs[0] == runs[1]
