"""Scan ingest and deskew on the device (riv-slam_amd/scan_ingest.py, csrc/apd_ingest.hpp): the two ends of
PreprocessingNodelet::cloud_callback (preprocessing_nodelet.cpp:667-697, :792-810, :914-975).

The expected values come from tests/scan_ingest_np.py, the literal numpy restatement of I1 .. I7 of include/apdgicp_hip.h.  Bars (GPU):
n_out, the rows, the index array and the deskewed cloud are the restatement's BYTES.  The one thing bytes cannot pin is a NaN that
arithmetic produces from a non-finite coordinate (inf - inf, 0 * inf): IEEE 754 leaves its sign and payload to the machine, and the host
and the device choose differently.  So the clouds of the byte comparisons that reach arithmetic (a pre-transform, the deskew, the frame
transform) keep such products out -- the transform used has no zero in its rotation, the deskewed clouds are finite -- and
test_non_finite_points_through_the_deskew compares non-finite points on their own: a NaN where the restatement has one, the same bits
everywhere else.  The chain test compares every stage of preprocess_scan with the chain of restatements (scan_ingest_np ->
ego_velocity_np -> scan_ingest_np -> scan_filter_np) under the bars the stages' own tests use.
"""
import ctypes
import importlib

import numpy as np
import pytest

import ego_velocity_np as E
import ref as R
import scan_ingest_np as S
from scan_filter_np import knn_d2_kdtree, np_range_gate

F32 = np.float32
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049]
NEW_SYMBOLS = ["apdgicp_scan_ingest_default_params", "apdgicp_scan_ingest_create", "apdgicp_scan_ingest_destroy", "apdgicp_scan_ingest_set_params",
               "apdgicp_scan_ingest_run", "apdgicp_scan_ingest_points", "apdgicp_scan_ingest_copy", "apdgicp_scan_ingest_deskew", "apdgicp_scan_ingest_deskewed",
               "apdgicp_scan_ingest_deskewed_copy", "apdgicp_scan_ingest_synchronize", "apdgicp_scan_ingest_stats"]
OMEGA = (0.31, -0.22, 0.47)
THR = F32(5.0)


def transform(scene):
    """a rigid transform whose rotation has no zero entry (see the module docstring)"""
    T = scene.make_transform([0.3, -0.1, 1.2], 0.4, -0.25, 0.15).astype(F32)
    assert (T[:3, :3] != 0).all()
    return T


# ------------------------------------------------------------------ CPU: the restatement against itself
def test_one_point_deskews_to_itself():
    """n = 1: dt = 0, q = (+-0, +-0, +-0, 1), so out = (v + 1 * 0) + 0 = v -- except that -0.0 + 0.0 is +0.0"""
    c = np.array([[1.5, -2.25, 0.75, 9.0]], dtype=F32)
    for linear in (False, True):
        assert S.deskew(c, OMEGA, 0.1, None, linear).tobytes() == c.tobytes()
    z = np.array([[-0.0, 3.0, -0.0, 1.0]], dtype=F32)
    out = S.deskew(z, OMEGA)
    assert np.array_equal(out, z) and not np.signbit(out[0, [0, 2]]).any() and np.signbit(z[0, [0, 2]]).all()
    assert S.deskew(z, None).tobytes() == z.tobytes()      # no IMU message: the cloud itself


def test_zero_rate_deskews_to_the_input():
    rng = np.random.default_rng(3)
    c = rng.uniform(-50, 50, (257, 4)).astype(F32)
    c[5, 1] = -0.0
    for linear in (False, True):
        out = S.deskew(c, (0.0, 0.0, 0.0), 0.1, None, linear)
        assert np.array_equal(out, c) and not np.signbit(out[5, 1])
        keep = np.ones(c.shape, dtype=bool)
        keep[5, 1] = False
        assert np.array_equal(out.view(np.uint32)[keep], c.view(np.uint32)[keep])


def test_a_nan_rate_gives_eigens_zero_quaternion():
    c = np.random.default_rng(4).uniform(-50, 50, (64, 4)).astype(F32)
    out = S.deskew(c, (np.nan, 0.1, 0.2))
    assert np.array_equal(out, c)                          # c = 0, cw = 0: (v + 0) + 0


def test_both_squared_norm_orders_agree_where_they_must():
    """(xx + yy) + (zz + 1) and ((xx + yy) + zz) + 1 are the same sum when zz = 0; they differ where zz is lost against 1 on its own but
    not beside xx + yy"""
    rng = np.random.default_rng(5)
    q = rng.uniform(-0.01, 0.01, (3, 4096)).astype(F32)
    one, zero = np.ones(4096, dtype=F32), np.zeros(4096, dtype=F32)
    assert np.array_equal(S.squared_norm(q[0], q[1], zero, one, False), S.squared_norm(q[0], q[1], zero, one, True))
    a, b = S.squared_norm(F32(2.0**-12), F32(0), F32(2.0**-13), F32(1), False), S.squared_norm(F32(2.0**-12), F32(0), F32(2.0**-13), F32(1), True)
    assert a == F32(1.0) and b == F32(1.0) + F32(2.0**-23)
    c = rng.uniform(-50, 50, (1025, 4)).astype(F32)
    w = (0.31, -0.22, 0.0)
    assert S.deskew(c, w, 0.1, None, False).tobytes() == S.deskew(c, w, 0.1, None, True).tobytes()
    d = S.deskew(c, OMEGA, 0.1)                            # a rotation by at most |w| * 0.1 rad: the norm moves by rounding only
    assert np.abs(np.linalg.norm(d[:, :3].astype(np.float64), axis=1) / np.linalg.norm(c[:, :3].astype(np.float64), axis=1) - 1).max() < 1e-3
    assert np.abs(d[:, :3] - c[:, :3]).max() > 1e-3


def test_the_gate_of_the_restatement():
    xyz = np.ones((6, 3), dtype=F32)
    power = np.array([5.0, np.nan, 20.0, 20.0, 20.0, 5.000001], dtype=F32)
    xyz[2, 0], xyz[3, 1], xyz[4, 2] = np.nan, np.inf, -np.inf
    rows, idx, keep = S.ingest(xyz, power, np.arange(6, dtype=F32), THR)
    assert keep.tolist() == [False, False, True, False, True, True] and idx.tolist() == [2, 4, 5]
    assert rows.shape == (3, 8) and rows[:, 4].tolist() == [2.0, 4.0, 5.0] and (rows[:, 5:] == 0).all()
    assert S.ingest(xyz, power, np.arange(6, dtype=F32), THR, gate=0)[1].tolist() == list(range(6))


def test_select_imu():
    assert S.select_imu([], 1.0) == (-1, 0)                              # an empty queue
    assert S.select_imu([0.1, 0.2, 0.3], 1.0) == (2, 3)                  # all earlier: the last one, everything erased
    assert S.select_imu([1.1, 1.2, 1.3], 1.0) == (0, 0)                  # all later: the first one, nothing erased
    assert S.select_imu([0.9, 1.0, 1.1, 1.2], 1.0) == (2, 2)             # a stamp equal to the scan's is not "later"
    assert S.select_imu([1.0], 1.0) == (0, 1)
    ing = importlib.import_module("riv-slam_amd.scan_ingest")
    rng = np.random.default_rng(6)
    for _ in range(200):
        stamps = np.sort(rng.integers(0, 12, rng.integers(0, 8))).astype(np.float64).tolist()
        t = float(rng.integers(-1, 13))
        assert ing.select_imu(stamps, t) == S.select_imu(stamps, t)


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    return tuple(importlib.import_module("riv-slam_amd." + m) for m in ("registration", "scan_ingest", "ego_velocity", "scan_filter"))


def test_symbols_are_exported_and_the_defaults_are_the_nodelets(mods):
    reg, ing = mods[:2]
    L = reg.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in reg.SYMBOLS
    p = ing.default_ingest_params()
    assert (p.power_threshold, p.gate, p.flags, p.reserved) == (0.0, 1, 0, 0) and ctypes.sizeof(ing.ScanIngestParams) == 16
    assert L.apdgicp_abi_version() == 6 and S.MAX_N == ing.MAX_POINTS == 1 << 24


# ------------------------------------------------------------------ GPU
def message(n, seed, planted=True):
    """xyz [n, 3], power [n], doppler [n] with the planted points of I2 (n >= 5: all five; n = 1: `planted` names the one)"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-60, 60, (n, 3)).astype(F32)
    power = rng.uniform(0, 40, n).astype(F32)
    dop = rng.normal(0, 3, n).astype(F32)
    kinds = []
    if planted is True and n >= 5:
        kinds = [(k, (k * n) // 5) for k in range(5)]
    elif planted is not True and planted is not False and n >= 1:
        kinds = [(planted, 0)]
    for k, i in kinds:
        power[i] = F32(20.0)
        if k == 0:
            power[i] = THR                  # exactly at the threshold: dropped
        elif k == 1:
            power[i] = np.nan               # dropped
        elif k == 2:
            xyz[i, 0] = np.nan              # kept
        elif k == 3:
            xyz[i, 1] = np.inf              # dropped
        else:
            xyz[i, 2] = -np.inf             # kept
    return xyz, power, dop


def layouts(xyz, power, dop):
    """the three layouts of I1 as (name, buffers, views(buffers) -> xyz, intensity, doppler)"""
    n = len(xyz)
    junk = np.random.default_rng(1).uniform(1e3, 2e3, (n, 12)).astype(F32)
    a32 = junk[:, :8].copy()
    a32[:, :3], a32[:, 3], a32[:, 4] = xyz, power, dop
    a48 = junk.copy()                        # a PointCloud2 with the fields out of order: doppler, xyz, intensity
    a48[:, 1], a48[:, 5:8], a48[:, 10] = dop, xyz, power
    return [("12/4/4", [xyz.copy(), power.copy(), dop.copy()], lambda b: (b[0], b[1], b[2])),
            ("aos32", [a32], lambda b: (b[0][:, :3], b[0][:, 3], b[0][:, 4])),
            ("aos48", [a48], lambda b: (b[0][:, 5:8], b[0][:, 10], b[0][:, 1]))]


def run_layouts(ing_mod, obj, msg, **kw):
    """every layout from host and from device memory against the restatement; returns the restatement's (rows, index, keep)"""
    import torch
    xyz, power, dop = msg
    lin = bool(obj.params.flags & ing_mod.FLAG_XF_LINEAR_CHAIN)
    rows, index, keep = S.ingest(xyz, power, dop, obj.params.power_threshold, obj.params.gate, kw.get("pre_transform"), lin)
    for name, bufs, views in layouts(xyz, power, dop):
        for where in ("host", "device"):
            b = bufs if where == "host" else [torch.from_numpy(a).cuda() for a in bufs]
            n_out = obj.run(*views(b), **kw)
            got = obj.to_numpy()
            tag = f"n={len(xyz)} {name} {where} gate={obj.params.gate} thr={obj.params.power_threshold} xf={'pre_transform' in kw} linear={lin}"
            assert n_out == len(rows) == obj.points().n, tag
            assert np.array_equal(got["index"], index), tag
            assert got["rows"].tobytes() == rows.tobytes(), tag
            assert (obj.points().ptr != 0) == (n_out > 0) and obj.points().stride_bytes == 32
            assert obj.stats() == (dict(launches=3, waits=1) if len(xyz) else dict(launches=0, waits=0))
    return rows, index, keep


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_ingest(mods, scene, n):
    _, ing = mods[:2]
    T = transform(scene)
    obj = ing.ScanIngest(power_threshold=float(THR))
    msgs = [message(n, 100 + n)] if n != 1 else [message(1, 101, planted=k) for k in range(5)]
    for msg in msgs:
        obj.set_params(power_threshold=float(THR), gate=1, flags=0)
        rows, index, keep = run_layouts(ing, obj, msg)
        if n >= 5:
            assert 0 < len(rows) < n and not np.isfinite(rows[:, :3]).all() and not keep[np.isnan(msg[1])].any()
            assert keep[np.isnan(msg[0][:, 0])].all() and keep[msg[0][:, 2] == -np.inf].all() and not keep[msg[0][:, 1] == np.inf].any() and not keep[msg[1] == THR].any()
        run_layouts(ing, obj, msg, pre_transform=T)                               # pairwise
        obj.set_params(flags=ing.FLAG_XF_LINEAR_CHAIN)
        lin = run_layouts(ing, obj, msg, pre_transform=T)[0]
        obj.set_params(flags=0, gate=0)                                            # the hugin callback: everything is kept
        assert len(run_layouts(ing, obj, msg)[0]) == n
        assert len(run_layouts(ing, obj, msg, pre_transform=T)[0]) == n
        obj.set_params(gate=1, power_threshold=1e9)                                # all points dropped
        assert len(run_layouts(ing, obj, msg)[0]) == 0
    clean = message(n, 200 + n, planted=False)
    obj.set_params(gate=1, power_threshold=-1.0)                                   # all points kept
    assert len(run_layouts(ing, obj, clean)[0]) == n
    if n >= 1023:   # the two orders are different sums: somewhere among a thousand points a last bit differs
        obj.set_params(power_threshold=float(THR))
        pair = S.ingest(*message(n, 100 + n), THR, 1, T, False)[0]
        assert pair.tobytes() != lin.tobytes()


@pytest.mark.gpu
def test_a_smaller_second_run_leaves_nothing_of_the_first(mods):
    _, ing = mods[:2]
    obj = ing.ScanIngest(power_threshold=float(THR))
    big, small = message(2049, 7), message(63, 8)
    run_layouts(ing, obj, big)
    rows, index, _ = run_layouts(ing, obj, small)
    got = obj.to_numpy()
    assert obj.n == len(rows) < 63 and got["rows"].shape == (len(rows), 8) and got["index"].max() < 63
    assert obj.run(np.zeros((0, 3), dtype=F32), np.zeros(0, dtype=F32), np.zeros(0, dtype=F32)) == 0
    assert obj.points().n == 0 and obj.points().ptr == 0 and obj.to_numpy()["rows"].shape == (0, 8)


def deskew_inputs(c):
    """the cloud as device rows 16 and 32 bytes apart and as a host cloud"""
    import torch
    wide = np.random.default_rng(2).uniform(1e3, 2e3, (len(c), 8)).astype(F32)
    wide[:, :4] = c
    return [("device16", torch.from_numpy(c).cuda()), ("device32", torch.from_numpy(wide).cuda()), ("host16", c)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_deskew(mods, scene, n):
    _, ing = mods[:2]
    T = transform(scene)
    c = np.random.default_rng(300 + n).uniform(-60, 60, (n, 4)).astype(F32)
    if n > 2:
        c[1, 0], c[2, 2] = -0.0, 0.0
    obj = ing.ScanIngest()
    for flags in (0, ing.FLAG_XF_LINEAR_CHAIN):
        obj.set_params(flags=flags)
        for w in (OMEGA, (0.0, 0.0, 0.0), (0.3, np.nan, -0.1), None):
            for Tm in (None, T):
                want = S.deskew(c, w, 0.1, Tm, bool(flags))
                for name, cloud in deskew_inputs(c):
                    assert obj.deskew(cloud, w, 0.1, Tm) == n
                    got = obj.to_numpy("deskewed")
                    assert got.tobytes() == want.tobytes(), f"n={n} {name} flags={flags} w={w} T={Tm is not None}"
                    dp = obj.deskewed()
                    assert dp.n == n and dp.stride_bytes == 16 and (dp.ptr != 0) == (n > 0)
                    assert obj.stats() == (dict(launches=1, waits=0) if n else dict(launches=0, waits=0))
                if w is None and Tm is None:
                    assert want.tobytes() == c.tobytes()                           # NULL / NULL: the input, bit for bit
    if n >= 1023:   # (on the restatement alone) the cases above are different computations
        a, b = S.deskew(c, OMEGA, 0.1, None, False), S.deskew(c, OMEGA, 0.1, T, False)
        assert a.tobytes() != c.tobytes() and a.tobytes() != b.tobytes() and b.tobytes() != S.deskew(c, OMEGA, 0.1, T, True).tobytes()


@pytest.mark.gpu
def test_deskew_of_the_objects_own_rows_and_without_an_intensity(mods, scene):
    """I7: legal on the rows the same object's run produced (32-byte rows, read in place); a cloud without an intensity column gets 0"""
    _, ing = mods[:2]
    obj = ing.ScanIngest(power_threshold=float(THR))
    xyz, power, dop = message(1025, 9, planted=False)
    rows = S.ingest(xyz, power, dop, THR)[0]
    assert obj.run(xyz, power, dop) == len(rows)
    assert obj.deskew(obj.points(), OMEGA, 0.1, transform(scene)) == len(rows)
    assert obj.to_numpy("deskewed").tobytes() == S.deskew(rows, OMEGA, 0.1, transform(scene)).tobytes()
    assert obj.to_numpy()["rows"].tobytes() == rows.tobytes()                      # the rows are still there
    assert obj.deskew(np.ascontiguousarray(xyz), OMEGA, 0.1) == 1025
    assert obj.to_numpy("deskewed").tobytes() == S.deskew(xyz, OMEGA, 0.1).tobytes()


@pytest.mark.gpu
def test_non_finite_points_through_the_deskew(mods, scene):
    """NaN, +inf and -inf coordinates through the deskew and the transform: a NaN wherever the restatement has one, the restatement's bits
    everywhere else (the sign and payload of a NaN that inf - inf or 0 * inf produces are the machine's)"""
    _, ing = mods[:2]
    c = np.random.default_rng(10).uniform(-60, 60, (130, 4)).astype(F32)
    c[3, 0], c[64, 1], c[65, 2], c[129, 0], c[129, 1] = np.nan, np.inf, -np.inf, np.inf, np.nan
    obj = ing.ScanIngest()
    for w in (OMEGA, (0.0, 0.0, 0.0), (np.nan, 0.0, 0.0), None):
        for Tm in (None, transform(scene)):
            want = S.deskew(c, w, 0.1, Tm)
            obj.deskew(c, w, 0.1, Tm)
            got = obj.to_numpy("deskewed")
            nan = np.isnan(want)
            print(f"w={w} T={Tm is not None}: {nan.sum()} NaN, bytes equal: {got.tobytes() == want.tobytes()}")
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
            if w is None and Tm is None:
                assert got.tobytes() == c.tobytes()


@pytest.mark.gpu
def test_argument_errors_leave_the_handle_usable(mods):
    reg, ing = mods[:2]
    L = reg.load_library()
    obj = ing.ScanIngest(power_threshold=float(THR))
    xyz, power, dop = message(65, 11, planted=False)           # (finite: usable() deskews the rows and compares bytes)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n_out = ctypes.c_int64(-7)

    def run(x, n, sx, i, si, d, sd):
        rc = L.apdgicp_scan_ingest_run(obj.h, x, n, sx, i, si, d, sd, 0, None, ctypes.byref(n_out))
        return rc, L.apdgicp_last_error().decode()

    def usable():
        rows = S.ingest(xyz, power, dop, THR)[0]
        assert obj.run(xyz, power, dop) == len(rows) and obj.to_numpy()["rows"].tobytes() == rows.tobytes()
        assert obj.deskew(rows, OMEGA) == len(rows) and obj.to_numpy("deskewed").tobytes() == S.deskew(rows, OMEGA).tobytes()

    for args, status, word in (((None, 65, 12, p(power), 4, p(dop), 4), -1, "null"), ((p(xyz), 65, 12, None, 4, p(dop), 4), -1, "null"),
                               ((p(xyz), 65, 12, p(power), 4, None, 4), -1, "null"), ((p(xyz), -1, 12, p(power), 4, p(dop), 4), -1, "negative"),
                               ((p(xyz), 65, 8, p(power), 4, p(dop), 4), -1, "stride"), ((p(xyz), 65, 12, p(power), 0, p(dop), 4), -1, "stride"),
                               ((p(xyz), 65, 12, p(power), 4, p(dop), 2), -1, "stride"), ((p(xyz), 65, 14, p(power), 4, p(dop), 4), -1, "stride"),
                               ((p(xyz), S.MAX_N + 1, 12, p(power), 4, p(dop), 4), -5, "2^24")):
        rc, msg = run(*args)
        assert rc == status and word in msg and n_out.value == 0, (args, rc, msg)
        assert obj.points().n == 0
        usable()
    w = (ctypes.c_double * 3)(*OMEGA)
    for args, status, word in (((None, 65, 16, 12), -1, "null"), ((p(xyz), -1, 12, -1), -1, "negative"), ((p(xyz), 65, 8, -1), -1, "stride"),
                               ((p(xyz), 65, 12, 12), -1, "offset"), ((p(xyz), S.MAX_N + 1, 12, -1), -5, "2^24")):
        rc = L.apdgicp_scan_ingest_deskew(obj.h, args[0], args[1], args[2], args[3], 0, w, 0.1, None)
        msg = L.apdgicp_last_error().decode()
        assert rc == status and word in msg and obj.deskewed().n == 0, (args, rc, msg)
        usable()
    bad = ing.ScanIngestParams(0.0, 2, 0, 0)
    assert L.apdgicp_scan_ingest_set_params(obj.h, ctypes.byref(bad)) == -1 and obj.params.gate == 1
    with pytest.raises(reg.ApdgicpError):
        obj.set_params(flags=1)
    with pytest.raises(ValueError):
        import torch
        obj.run(torch.from_numpy(xyz).cuda(), power, dop)                          # lanes in two memory spaces
    usable()


class RecordingRegistration:
    def __init__(self):
        self.sources = []

    def setInputSource(self, cloud):
        self.sources.append(cloud)


def first_words(scan, cfg, cond, K, S_):
    for seed in range(64):
        w = np.random.default_rng(seed).integers(0, 2**32, (K, S_), dtype=np.uint32)
        if cond(E.estimate(scan, cfg, w)):
            return w
    raise AssertionError("no word table with the wanted property among 64 seeds")


@pytest.mark.gpu
@pytest.mark.parametrize("removal", (True, False), ids=("inliers", "raw"))
def test_the_whole_callback(mods, scene, removal):
    """preprocess_scan on one 2 000-point scan (scene.raw_doppler_scan: the structured scene, near and far returns, clutter, ~2 % movers;
    its five non-finite rows made finite, see the module docstring; 40 powers below the threshold, one on it, one NaN) against the chain
    of restatements: identical masks and counts at every stage, the deskewed cloud byte-equal, the filtered cloud under the bars of
    tests/test_scan_filter.py (gate mask exact; voxel grid: sizes equal, one-point voxels exact, centroids within the fp32 sum bound of
    tests/test_submap.py; STATISTICAL: scores bit for bit on the device's voxel cloud, mean / stddev / thr within 1e-9 relative, the mask
    identical after the restatement alone showed no score within 1e-9 thr of thr, the output = the kept rows)."""
    from test_scan_filter import bits, centroids_close, statistical_expected
    reg, ing, ev, sf = mods
    raw = scene.raw_doppler_scan(2000, 31, (2.0, 0.3, -0.1), 0.02)
    raw[~np.isfinite(raw[:, :3]).all(axis=1), :3] = F32(1.25)
    rng = np.random.default_rng(32)
    low = rng.choice(2000, 42, replace=False)
    thr = F32(2.5)
    raw[low[:40], 3], raw[low[40], 3], raw[low[41], 3] = rng.uniform(0, 2.4, 40).astype(F32), thr, np.nan
    T, w = transform(scene), OMEGA
    cfg = E.Config()
    # the chain of restatements
    rows, index, keep = S.ingest(raw[:, :3], raw[:, 3], raw[:, 4], thr)
    assert len(rows) <= 2000 - 42 and not keep[low].any()
    scan5 = np.ascontiguousarray(rows[:, :5])
    words = first_words(scan5, cfg, lambda e: not e.merged and len(e.outlier_rows) > 0, 3, 5)
    est = E.estimate(scan5, cfg, words)
    assert est.success and 0 < len(est.outlier_rows) and 0.9 * est.m <= len(est.inlier_rows) < est.m
    src = est.cloud(scan5, "in")[0] if removal else np.ascontiguousarray(rows[:, :4])
    desk = S.deskew(src, w, 0.1, T)
    gate = np_range_gate(desk)
    exp, idx, cnt = R.submap_assemble([desk[gate]], None, 0.1)
    assert (idx >= 0).all()
    # the device
    a48 = np.random.default_rng(33).uniform(1e3, 2e3, (2000, 12)).astype(F32)       # the message as a PointCloud2: doppler, xyz, intensity
    a48[:, 1], a48[:, 5:8], a48[:, 10] = raw[:, 4], raw[:, :3], raw[:, 3]
    obj, est_dev, flt, g = ing.ScanIngest(power_threshold=float(thr)), ev.EgoVelocityEstimator(), sf.ScanFilter(), RecordingRegistration()
    out = ing.preprocess_scan(obj, est_dev, flt, a48[:, 5:8], a48[:, 10], a48[:, 1], registration=g, enable_dynamic_object_removal=removal, ang_vel=w,
                              scan_period=0.1, T=T, words=words)
    got = obj.to_numpy()
    assert out["n_ingest"] == len(rows) and np.array_equal(got["index"], index) and got["rows"].tobytes() == rows.tobytes()
    r = out["ego"]
    assert (r.m, r.n_inlier, r.n_outlier, r.best_in, r.best_out) == (est.m, len(est.inlier_rows), len(est.outlier_rows), est.best_in, est.best_out)
    assert np.array_equal(est_dev.debug()["valid"], est.valid) and np.array_equal(est_dev.to_numpy("inliers")["index"], est.cloud(scan5, "in")[2])
    assert out["n_source"] == len(src) == obj.n_deskewed and obj.to_numpy("deskewed").tobytes() == desk.tobytes()
    counts = flt.stage_counts()
    assert counts[:3] == (len(desk), gate.sum(), len(exp)) and out["n_filtered"] == counts[3] == flt.n > 0
    s2f = sf.ScanFilter(outlier_method="NONE")
    assert s2f.run(desk) == len(exp)
    s2 = s2f.to_numpy()
    assert np.array_equal(s2[cnt == 1], exp[cnt == 1]) and centroids_close(s2, exp, cnt)
    score, mean, stddev, t, kept, gap = statistical_expected(knn_d2_kdtree(s2, 21), 20, 1.0)
    sc = flt.scores()
    rel = max(abs(sc["mean"] - mean) / mean, abs(sc["stddev"] - stddev) / stddev, abs(sc["thr"] - t) / t)
    print(f"removal {removal}: {len(raw)} -> {len(rows)} -> {len(src)} -> {gate.sum()} -> {len(exp)} -> {kept.sum()}; sums rel diff {rel:.2e}, nearest score {gap / t:.2e} thr away")
    assert np.array_equal(bits(sc["stat"]), bits(score)) and rel <= 1e-9
    assert np.array_equal(sc["kept"], kept) and out["n_filtered"] == kept.sum() and np.array_equal(bits(flt.to_numpy()), bits(s2[kept]))
    assert len(g.sources) == 1 and g.sources[0].ptr == flt.points().ptr != 0 and g.sources[0].n == out["n_filtered"] and g.sources[0].stride_bytes == 16


@pytest.mark.gpu
def test_an_empty_source_cloud_returns_before_the_deskew(mods):
    _, ing, ev, sf = mods
    obj, est_dev, flt, g = ing.ScanIngest(power_threshold=1e9), ev.EgoVelocityEstimator(), sf.ScanFilter(), RecordingRegistration()
    xyz, power, dop = message(300, 12)
    obj.deskew(xyz, OMEGA)
    out = ing.preprocess_scan(obj, est_dev, flt, xyz, power, dop, registration=g, ang_vel=OMEGA)
    assert (out["n_ingest"], out["n_source"], out["n_filtered"], out["ego"].success) == (0, 0, 0, 0) and not g.sources
    assert obj.n_deskewed == 300                                                   # the earlier deskew: no new one ran
