"""CPU tests (-m "not gpu"): the two oracle restatements against the committed golden vectors and
against each other.  The reference holds no fixture for FastAPDGICP (parity unpinned)."""
import os

import numpy as np
import pytest

import apdgicp_np as O
import ref as R
from conftest import rel_err
from trace_util import golden_trace, trace_close

LAUNCH = dict(max_correspondence_distance=2.0, transformation_epsilon=0.1, azimuth_variance_deg=1.0)
REGS = (("none", 0), ("min_eig", 1), ("norm_min_eig", 2), ("plane", 3), ("frobenius", 4))


@pytest.mark.parametrize("name,reg", REGS)
def test_cov_golden_cpp(golden, name, reg):
    r = R.RefAPDGICP(R.default_params(regularization=reg))
    r.setInputSource(golden["cov_cloud"])
    assert np.abs(r.covariances("source") - golden[f"cov_{name}"]).max() <= 1e-12


@pytest.mark.parametrize("name,reg", REGS)
def test_cov_golden_numpy(golden, name, reg):
    c = O.calculate_covariances(golden["cov_cloud"], 20, reg)
    assert np.abs(c - golden[f"cov_{name}"]).max() <= 1e-12 * max(1.0, np.abs(c).max())


def test_plane_cov_structure(golden):
    """PLANE regularisation == I - (1-1e-3) n n^T: eigenvalues {1, 1, 1e-3} (fast_apdgicp_impl.hpp:344-357)."""
    w = np.linalg.eigvalsh(golden["cov_plane"])
    assert np.allclose(w, [1e-3, 1.0, 1.0], atol=1e-12)


def test_kdtree_equals_bruteforce(golden):
    cloud = golden["lin_target"]
    r = R.RefAPDGICP()
    r.setInputTarget(cloud)
    rng = np.random.default_rng(3)
    qs = np.concatenate([cloud[rng.integers(0, len(cloud), 64)], rng.uniform(-5, 100, size=(64, 3)).astype(np.float32)])
    d = O.sqdist_f32(qs, cloud)
    for k in (1, 20, 70, 200):   # (k > 64: the product's selection kernel is held against this)
        want = np.argsort(d, axis=1, kind="stable")[:, :k]
        for i, q in enumerate(qs):
            idx, dist = r.knn_kdtree("target", q, k)
            assert np.array_equal(idx, want[i])
            assert np.array_equal(dist, d[i, want[i]])


def test_kdtree_ties_pick_lowest_index():
    pts = np.zeros((64, 3), dtype=np.float32)
    pts[:, 0] = np.repeat(np.arange(8), 8)  # 8 copies of each of 8 points
    r = R.RefAPDGICP()
    r.setInputTarget(pts)
    idx, _ = r.knn_kdtree("target", np.array([3.0, 0, 0], dtype=np.float32), 3)
    assert list(idx) == [24, 25, 26]


def _nanoflann_cases(golden):
    """(name, target cloud, queries): the golden pair at its guess and two 8k bench pairs at theirs, the source transformed in fp32 under
    BOTH orders Eigen can give T * p (A:137,149), plus the target against itself (the covariance k-NN, A:318)."""
    import importlib
    scene = importlib.import_module("riv-slam_amd.scene")
    cases = []
    pairs = [("golden", golden["lin_source"], golden["lin_target"], golden["lin_guess"])]
    for p in (0, 1):
        s, t, _, g = scene.make_pair(8192, 8192, scene.pair_seed(2, p), "odometry")
        pairs.append((f"bench{p}", s, t, g))
    for name, s, t, g in pairs:
        for lin in (False, True):
            cases.append((f"{name}/{'linear' if lin else 'pairwise'}", t, O.transform_points_f32(np.asarray(g, dtype=np.float32), s, lin)))
        cases.append((f"{name}/self", t, t))
    return cases


NANOFLANN_KS, NANOFLANN_LEAVES, NANOFLANN_QUERIES = (1, 20), (10, 15), 256


def test_kdtree_against_the_reference_trees_own_nanoflann(golden):
    """VERDICT r05 item 6.  The reference tree holds ONE exact nearest-neighbour implementation that compiles in this image:
    radar_graph_slam/include/scan_context/nanoflann.hpp with L2_Simple_Adaptor<float> (:423-446) -- FLANN's L2_Simple accumulation
    order.  The oracle's kd-tree (the piece SURVEY 7 hard-part 2 calls the parity risk) must return the same fp32 distances BIT FOR
    BIT for 1-NN and 20-NN, and the same indices wherever the distance is unique among the cloud's points (ties: FLANN's order is
    unspecified, the oracle's is the lowest index).  It is ScanContext's tree, not the path's FLANN: the cap "parity unpinned" stays.
    nanoflann's answers are stored vectors (tests/golden/nanoflann_knn.npz, tests/golden/make_nanoflann_golden.py): a seeded sample of
    NANOFLANN_QUERIES queries per case, the target clouds regenerated here and checked against the stored hashes."""
    import hashlib
    nf = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nanoflann_knn.npz"))
    for name, tgt, q in _nanoflann_cases(golden):
        key = name.replace("/", "_")
        sel = nf[f"{key}__sel"]
        q = np.ascontiguousarray(q[sel], dtype=np.float32)
        assert np.array_equal(q.view(np.uint32), nf[f"{key}__q"].view(np.uint32)), name      # the same queries ...
        sha = hashlib.sha256(np.ascontiguousarray(tgt, dtype=np.float32).tobytes()).digest()
        assert sha == nf[f"{key}__tgt_sha"].tobytes(), name                                 # ... against the same cloud
        r = R.RefAPDGICP()
        r.setInputTarget(tgt)
        for k in NANOFLANN_KS:
            for leaf in NANOFLANN_LEAVES:   # nanoflann's default leaf size and the one PCL's FLANN index is built with: exact either way
                ni, nd = nf[f"{key}__idx_k{k}_l{leaf}"], nf[f"{key}__d_k{k}_l{leaf}"]
                oi, od = r.knn_kdtree_batch("target", q, k)
                assert np.array_equal(nd.view(np.uint32), od.view(np.uint32)), (name, k, leaf)
                # a distance is unique for its query when its neighbours in the sorted list differ and nothing BEHIND the list equals the last entry
                uniq = np.ones_like(od, dtype=bool)
                uniq[:, 1:] &= od[:, 1:] != od[:, :-1]
                uniq[:, :-1] &= od[:, :-1] != od[:, 1:]
                ki, kd = r.knn_kdtree_batch("target", q, k + 1)
                uniq[:, -1] &= kd[:, k] != od[:, -1]
                assert np.array_equal(ni[uniq], oi[uniq]), (name, k, leaf)
                assert uniq.mean() > 0.98, (name, k, float(uniq.mean()))


def test_algebraic_sensor_model_checker(golden):
    """flags bit 3 of both restatements is the checker of the product's opt-in APDGICP_FLAG_ALGEBRAIC_APD (NOT the reference's arithmetic):
    the two writings agree with each other, and the mode differs from the reference's arithmetic only by the fp32 rounding of its angles."""
    src, tgt, T0 = golden["lin_source"], golden["lin_target"], golden["lin_guess"].astype(np.float64)
    r0, r8 = R.RefAPDGICP(R.default_params(**LAUNCH)), R.RefAPDGICP(R.default_params(flags=8, **LAUNCH))
    n8 = O.FastAPDGICP(O.Params(flags=8, **LAUNCH))
    for x in (r0, r8, n8):
        x.setInputSource(src)
        x.setInputTarget(tgt)
    n8.source_covs, n8.target_covs = golden["lin_source_cov"], golden["lin_target_cov"]   # (the numpy writing's covariances take minutes)
    c0, H0, b0 = r0.linearize(T0)
    c8, H8, b8 = r8.linearize(T0)
    cn, Hn, bn = n8.linearize(T0)
    assert np.array_equal(r0.correspondences()[0], r8.correspondences()[0])
    assert rel_err(H8, Hn) < 1e-12 and rel_err(b8, bn) < 1e-11 and abs(c8 - cn) < 1e-12 * cn
    assert 1e-12 < rel_err(H8, H0) < 1e-5 and abs(c8 - c0) < 1e-5 * c0
    Ta, Tb = r0.align(golden["lin_guess"]), r8.align(golden["lin_guess"])
    assert np.abs(Ta - Tb).max() < 1e-6


# fp32 summation order of T * p (A:149): pairwise (Eigen >= 3.3, default) | linear chain (Eigen 3.2, flags bit 1)
XF = (pytest.param("", 0, id="xf_pairwise"), pytest.param("_xflin", 2, id="xf_linear"))


@pytest.mark.parametrize("sfx,flags", XF)
@pytest.mark.parametrize("tag,kw", (("default", {}), ("launch", LAUNCH)))
def test_linearize_golden_cpp(golden, tag, kw, sfx, flags):
    r = R.RefAPDGICP(R.default_params(flags=flags, **kw))
    tag = tag + sfx
    r.setInputSource(golden["lin_source"])
    r.setInputTarget(golden["lin_target"])
    for k in range(3):
        cost, H, b = r.linearize(golden[f"lin_{tag}_{k}_T"])
        corr, sqd = r.correspondences()
        assert np.array_equal(corr, golden[f"lin_{tag}_{k}_corr"])
        assert np.array_equal(sqd, golden[f"lin_{tag}_{k}_sqd"])
        assert rel_err(H, golden[f"lin_{tag}_{k}_H"]) < 1e-10
        assert rel_err(b, golden[f"lin_{tag}_{k}_b"]) < 1e-10
        assert abs(cost - golden[f"lin_{tag}_{k}_cost"]) < 1e-10 * cost
        assert rel_err(r.mahalanobis()[:128], golden[f"lin_{tag}_{k}_maha128"]) < 1e-12
        err = r.compute_error(golden[f"lin_{tag}_{k}_errT"])
        assert abs(err - golden[f"lin_{tag}_{k}_err"]) < 1e-10 * err
        cost_only, _, _ = r.linearize(golden[f"lin_{tag}_{k}_T"], want_Hb=False)
        assert abs(cost_only - cost) < 1e-12 * cost


@pytest.mark.parametrize("sfx,flags", XF)
def test_linearize_golden_numpy(golden, sfx, flags):
    """Independent restatement: exact on the discrete outputs, 1e-10 on the smooth ones (both evaluate the fp32 angles with the
    C library's atan2f algorithm: include/apd_atan2f.h and apdgicp_np.atan2f_fdlibm)."""
    n = O.FastAPDGICP(O.Params(flags=flags, **LAUNCH))
    n.setInputSource(golden["lin_source"])
    n.setInputTarget(golden["lin_target"])
    n.source_covs, n.target_covs = golden["lin_source_cov"], golden["lin_target_cov"]
    k = 1
    cost, H, b = n.linearize(golden[f"lin_launch{sfx}_{k}_T"])
    assert np.array_equal(n.correspondences, golden[f"lin_launch{sfx}_{k}_corr"])
    assert np.array_equal(n.sq_distances, golden[f"lin_launch{sfx}_{k}_sqd"])
    assert rel_err(H, golden[f"lin_launch{sfx}_{k}_H"]) < 1e-10
    assert rel_err(b, golden[f"lin_launch{sfx}_{k}_b"]) < 1e-10
    assert abs(cost - golden[f"lin_launch{sfx}_{k}_cost"]) < 1e-10 * cost


def test_transform_orders_by_hand():
    """The two orders on a case small enough to evaluate by hand in fp32: pairwise (a + b) + (c + t), chain ((a + b) + c) + t."""
    f = np.float32
    T = np.eye(4)
    T[0, :] = [1.0, 2.0 ** -12, 2.0 ** -24, 2.0 ** -24]
    p = np.array([[1.0, 1.0, 1.0]], dtype=f)
    # row 0: a = 1, b = 2^-12, c = 2^-24, t = 2^-24:  (a + b) = 1 + 2^-12 exactly; + c rounds back (half an ulp of 2^-23, ties to
    # even), + t again -> 1 + 2^-12; pairwise: c + t = 2^-23 = one ulp -> 1 + 2^-12 + 2^-23
    chain = O.transform_points_f32(T, p, True)[0, 0]
    pair = O.transform_points_f32(T, p, False)[0, 0]
    assert chain == f(1.0) + f(2.0 ** -12) and pair == f(f(1.0) + f(2.0 ** -12)) + f(2.0 ** -23) and pair != chain
    for flags, want in ((0, pair), (2, chain)):  # the C++ restatement evaluates the same two values
        r = R.RefAPDGICP(R.default_params(flags=flags, k_correspondences=1))
        tgt = np.array([[0.0, 1.0, 1.0]], dtype=f)
        r.setInputSource(p), r.setInputTarget(tgt)
        r.linearize(T)
        d = r.correspondences()[1][0]
        assert d == f(want * want)   # (dy = dz = 0: the squared distance is the transformed x, squared)


def test_serial_and_threaded_sums_agree(golden):
    a, b = R.RefAPDGICP(num_threads=1), R.RefAPDGICP(num_threads=4)
    for r in (a, b):
        r.setInputSource(golden["lin_source"])
        r.setInputTarget(golden["lin_target"])
    ca, Ha, ba = a.linearize(golden["lin_default_1_T"])
    cb, Hb, bb = b.linearize(golden["lin_default_1_T"])
    assert rel_err(Ha, Hb) < 1e-12 and rel_err(ba, bb) < 1e-11 and abs(ca - cb) < 1e-12 * ca


RUNS = {
    "lm_default": {},
    "lm_launch": LAUNCH,
    "gn20": dict(optimizer=1, max_iterations=20, transformation_epsilon=1e-300, rotation_epsilon=1e-300),
    "lm_loop": dict(max_correspondence_distance=2.5),
}


@pytest.mark.parametrize("sfx,flags", XF)
@pytest.mark.parametrize("tag", list(RUNS))
def test_align_golden_cpp(golden, scene, tag, sfx, flags):
    r = R.RefAPDGICP(R.default_params(flags=flags, **RUNS[tag]))
    pre = "lm_loop" if tag == "lm_loop" else "lin"
    r.setInputSource(golden[f"{pre}_source"])
    r.setInputTarget(golden[f"{pre}_target"])
    T = r.align(golden[f"{pre}_guess"])
    tag = tag + sfx
    info = golden[f"{tag}_info"]
    assert [int(r.converged), r.nr_iterations, r.n_linearize, r.n_compute_error] == list(info)
    te, re_ = scene.pose_error(golden[f"{tag}_T"], T)
    assert te < 1e-7 and re_ < 1e-7
    assert rel_err(r.final_hessian(), golden[f"{tag}_final_hessian"]) < 1e-9
    d = trace_close(r.trace(), golden_trace(golden, tag))   # KAT-lm: lambda, rho, costs per trial, pose per outer iteration
    assert max(d.values()) < 1.0, d


@pytest.mark.parametrize("sfx,flags", XF)
def test_align_golden_numpy_launch(golden, scene, sfx, flags):
    n = O.FastAPDGICP(O.Params(flags=flags, **LAUNCH))
    n.setInputSource(golden["lin_source"])
    n.setInputTarget(golden["lin_target"])
    T = n.align(golden["lin_guess"])
    assert [int(n.converged), n.nr_iterations, n.trace.n_linearize, n.trace.n_compute_error] == list(golden[f"lm_launch{sfx}_info"])
    te, re_ = scene.pose_error(golden[f"lm_launch{sfx}_T"], T)
    assert te < 1e-7 and re_ < 1e-7
    tn = {"lambda": np.array(n.trace.lambdas), "rho": np.array(n.trace.rhos), "y0": np.array(n.trace.y0s), "yi": np.array(n.trace.yis),
          "poses": np.array(n.trace.poses)}
    d = trace_close(tn, golden_trace(golden, f"lm_launch{sfx}"))
    assert max(d.values()) < 1.0, d


@pytest.mark.parametrize("sfx,flags", XF)
def test_degenerate_golden_cpp(golden, sfx, flags):
    r = R.RefAPDGICP(R.default_params(max_correspondence_distance=2.0, flags=flags))
    r.setInputSource(golden["deg_source"])
    r.setInputTarget(golden["deg_target"])
    cost, H, b = r.linearize(golden["deg_T"])
    corr, sqd = r.correspondences()
    assert np.array_equal(corr, golden[f"deg_moved{sfx}_corr"]) and np.array_equal(sqd, golden[f"deg_moved{sfx}_sqd"])
    assert rel_err(H, golden[f"deg_moved{sfx}_H"]) < 1e-10
    cost, H, b = r.linearize(np.eye(4))
    corr, sqd = r.correspondences()
    assert np.array_equal(corr, golden[f"deg{sfx}_corr"]) and corr[2] == -1
    assert rel_err(H, golden[f"deg{sfx}_H"]) < 1e-10 and rel_err(b, golden[f"deg{sfx}_b"]) < 1e-10
    M = r.mahalanobis()
    assert np.all(M[2] == 0)
    # +x-axis point: APD sigma_y,z ~ dist*sin(var)/cos(AoA) is huge -> tiny information in y/z
    assert M[0][1, 1] < 1e-3 * M[0][0, 0] or M[0][1, 1] < 1e-2


@pytest.mark.parametrize("sfx,flags", XF)
@pytest.mark.parametrize("tag,kw", (("rej", {}), ("fail", dict(lm_max_iterations=1))))
def test_lm_rejection_paths_cpp(golden, scene, tag, kw, sfx, flags):
    r = R.RefAPDGICP(R.default_params(flags=flags, **kw))
    r.setInputSource(golden["rej_source"])
    r.setInputTarget(golden["rej_target"])
    T = r.align(None)
    assert [int(r.converged), r.nr_iterations, r.n_linearize, r.n_compute_error] == list(golden[f"{tag}{sfx}_info"])
    assert (golden[f"{tag}{sfx}_trace_rho"] < 0).any()
    te, re_ = scene.pose_error(golden[f"{tag}{sfx}_T"], T)
    assert te < 1e-6 and re_ < 1e-8
    d = trace_close(r.trace(), golden_trace(golden, tag + sfx))
    assert max(d.values()) < 1.0, d
    if tag == "fail":
        assert not r.converged and r.nr_iterations < 63


def test_too_few_points_is_an_error():
    r = R.RefAPDGICP()
    r.setInputSource(np.zeros((5, 3), dtype=np.float32))
    with pytest.raises(RuntimeError):
        r.covariances("source")


def test_scene_is_deterministic(scene):
    a = scene.make_pair(512, 640, scene.pair_seed(9, 3), "odometry")
    b = scene.make_pair(512, 640, scene.pair_seed(9, 3), "odometry")
    assert a[0].shape == (512, 3) and a[1].shape == (640, 3) and a[0].dtype == np.float32
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    r = np.linalg.norm(a[0], axis=1)
    assert r.min() > 1.5 and r.max() < 103


def test_plain_gicp_mode_restatements_agree(golden):
    """flags bit 0 = upstream FastGICP cost (cov_dist dropped, fast_gicp_impl.hpp): both restatements, and
    the difference to the APD cost is real."""
    src, tgt = golden["lin_source"][:700], golden["lin_target"][:700]
    kw = dict(max_correspondence_distance=2.5, flags=1)
    r = R.RefAPDGICP(R.default_params(**kw))
    n = O.FastAPDGICP(O.Params(**kw))
    a = R.RefAPDGICP(R.default_params(max_correspondence_distance=2.5))
    for o in (r, n, a):
        o.setInputSource(src)
        o.setInputTarget(tgt)
    n.source_covs, n.target_covs = r.covariances("source"), r.covariances("target")
    T = golden["lin_guess"].astype(np.float64)
    cr, Hr, br = r.linearize(T)
    cn, Hn, bn = n.linearize(T)
    ca, Ha, ba = a.linearize(T)
    assert rel_err(Hr, Hn) < 1e-10 and rel_err(br, bn) < 1e-9 and abs(cr - cn) < 1e-10 * cr   # no atan2f in this mode
    assert rel_err(Ha, Hr) > 1e-2                                                            # APD term matters
    assert np.array_equal(r.correspondences()[0], a.correspondences()[0])                    # same nearest neighbours
