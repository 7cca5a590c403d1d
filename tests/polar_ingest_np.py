"""numpy restatement of the polar ingest and the distance histogram (riv-slam_amd/csrc/apd_ingest.hpp: k_ing_polar, k_ing_hist), statement by
statement as include/apdgicp_hip.h writes them down (PI1 .. PI5, H1 .. H4; "P:" = radar_graph_slam/apps/preprocessing_nodelet.cpp): the
expected values of tests/test_polar_ingest.py and tests/test_polar_ingest_cpu.py.  Every operation is on np.float32 / np.float64 arrays of
the stated type, so nothing is promoted on the way."""
from __future__ import annotations

import ctypes

import numpy as np

F32, F64 = np.float32, np.float64
BINS = 100
TARGET_FLOATS = 19    # a msgs_radar/RadarTargetExtended: range, azimuth, elevation, velocity, snr and 14 more float32


def f32(a):
    a = np.asarray(a)
    assert a.dtype == F32, a.dtype
    return a


def _rows(rng_, ce, se, ca, sa, snr, velocity):
    """P:333-337 from the four factors: every product rounded to fp32 on its own, left to right"""
    with np.errstate(all="ignore"):
        rc = f32(rng_ * ce)
        x, y, z = f32(rc * ca), f32(rc * sa), f32(f32(-rng_) * se)
    rows = np.zeros((len(rng_), 8), dtype=F32)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = x, y, z, snr, velocity
    return rows


def _lanes(range_, azimuth, elevation, snr, velocity):
    return tuple(np.ascontiguousarray(a, dtype=F32).reshape(-1) for a in (range_, azimuth, elevation, snr, velocity))


def polar_rows(range_, azimuth, elevation, snr, velocity):
    """PI3 / PI4 -> (rows [n, 8] float32, index [n] int32): each factor is the fp64 sine / cosine rounded once to fp32"""
    r, az, el, s, v = _lanes(range_, azimuth, elevation, snr, velocity)
    with np.errstate(invalid="ignore"):
        ce, se = np.cos(el.astype(F64)).astype(F32), np.sin(el.astype(F64)).astype(F32)
        ca, sa = np.cos(az.astype(F64)).astype(F32), np.sin(az.astype(F64)).astype(F32)
    return _rows(r, ce, se, ca, sa, s, v), np.arange(len(r), dtype=np.int32)


_libm = None


def _libm_f(name, a):
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL("libm.so.6")
        for f in ("cosf", "sinf"):
            getattr(_libm, f).argtypes, getattr(_libm, f).restype = [ctypes.c_float], ctypes.c_float
    fn = getattr(_libm, name)
    return np.fromiter(map(fn, a.tolist()), dtype=F32, count=len(a))


def polar_rows_libm(range_, azimuth, elevation, snr, velocity):
    """the reference's literal form (P:333-335 under `using namespace std`): the running C library's own cosf / sinf"""
    r, az, el, s, v = _lanes(range_, azimuth, elevation, snr, velocity)
    return _rows(r, _libm_f("cosf", el), _libm_f("sinf", el), _libm_f("cosf", az), _libm_f("sinf", az), s, v), np.arange(len(r), dtype=np.int32)


def targets(range_, azimuth, elevation, snr, velocity, fill=None):
    """the five lanes as [n, 19] float32 records of a RadarTargetExtended[] (76 bytes; the other 14 floats: `fill` or junk)"""
    r, az, el, s, v = _lanes(range_, azimuth, elevation, snr, velocity)
    t = np.random.default_rng(1).uniform(1e3, 2e3, (len(r), TARGET_FLOATS)).astype(F32) if fill is None else np.full((len(r), TARGET_FLOATS), fill, dtype=F32)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4] = r, az, el, v, s
    return t


def fixture(n, seed):
    """n targets as the GPU tests make them: range 2 .. 100 m, azimuth +-0.986 rad, elevation +-0.262 rad, snr 0 .. 40, velocity N(0, 3)
    -> (range, azimuth, elevation, snr, velocity), float32 each"""
    rng = np.random.default_rng([seed, 0x90])
    return (rng.uniform(2.0, 100.0, n).astype(F32), rng.uniform(-0.986, 0.986, n).astype(F32), rng.uniform(-0.262, 0.262, n).astype(F32),
            rng.uniform(0.0, 40.0, n).astype(F32), rng.normal(0.0, 3.0, n).astype(F32))


def histogram(cloud):
    """H1 -> [100] int32: d = sqrtf((x x + y y) + z z) in fp32, bin (int)floorf(d), counted iff d is finite and the bin is < 100"""
    cloud = np.asarray(cloud, dtype=F32)
    x, y, z = (np.ascontiguousarray(cloud[:, q]) for q in range(3))
    with np.errstate(all="ignore"):
        d = f32(np.sqrt(f32(f32(f32(x * x) + f32(y * y)) + f32(z * z))))
    ok = np.isfinite(d) & (d < F32(BINS))
    return np.bincount(np.floor(d[ok]).astype(np.int64), minlength=BINS).astype(np.int32)


def _near_fp32_midpoint(v):
    """true where the fp64 value v lies within 2 fp64 ulps of the midpoint of two neighbouring fp32 values"""
    v = np.asarray(v, dtype=F64)
    with np.errstate(all="ignore"):
        f = v.astype(F32)
        other = np.where(f.astype(F64) <= v, np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf)))
        mid = (f.astype(F64) + other.astype(F64)) / 2.0              # exact: two neighbouring floats
        out = np.abs(v - mid) <= 2.0 * np.spacing(np.abs(v))
    return out & np.isfinite(v)


def excused(angle):
    """true where the fp64 sine or cosine of the (fp32) angle lies within 2 fp64 ulps of the midpoint of two neighbouring fp32 values: the
    only places where two fp64 implementations that are each within one ulp can round to different floats"""
    a = np.asarray(angle, dtype=F32).astype(F64)
    with np.errstate(invalid="ignore"):
        return _near_fp32_midpoint(np.sin(a)) | _near_fp32_midpoint(np.cos(a))


def ulp_diff(a, b):
    """|a - b| in fp32 ulps through the ordered-integer view (finite inputs)"""
    def key(v):
        i = np.ascontiguousarray(v, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
