"""CPU tests of the exact k-nearest / radius queries (Q1 .. Q9 of include/apdgicp_hip.h): the numpy restatement (tests/search_np.py)
against its literal second form on clouds full of ties, and the argument checks of the three entry points through the loaded
library -- everything the library decides before it needs a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_np as S  # noqa: E402

F32 = np.float32
ERR_INVALID_ARG, ERR_HIP, ERR_NO_INPUT, ERR_UNSUPPORTED = -1, -2, -3, -5   # include/apdgicp_hip.h


@pytest.fixture(scope="module")
def reg(pkg):
    import importlib
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


def lattice(n):
    g = np.arange(n, dtype=F32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("k", [1, 2, 5, 20, 64])
def test_knn_restatement_equals_the_literal_sort_on_lattices(k):
    """An integer lattice (every distance a small integer: ties everywhere) and the same lattice stored three times (every key's distance
    shared by three indices): the matrix form and the sort of Python tuples give the same bytes, tail included (k > M)."""
    rng = np.random.default_rng(11)
    t = lattice(3)                                   # 27 points
    t3 = np.concatenate([t, t, t])[rng.permutation(81)]
    q = np.concatenate([t[:5], t[:5] + F32(0.5), rng.random((6, 3)).astype(F32) * 4 - 1])
    for tgt in (t, t3, t[:1]):
        a, b = S.knn(q, tgt, k), S.knn_literal(q, tgt, k)
        assert same(a[0], b[0]) and same(a[1], b[1]) and a[2] == b[2] == min(k, len(tgt))
        assert (a[0][:, a[2]:] == -1).all() and np.isposinf(a[1][:, a[2]:]).all()
        # ascending keys, ties by ascending index
        d, i = a[1][:, :a[2]].astype(np.float64), a[0][:, :a[2]].astype(np.int64)
        assert ((d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (i[:, 1:] > i[:, :-1]))).all()


def test_knn_k1_is_the_oracles_nearest_neighbour():
    import apdgicp_np as O
    rng = np.random.default_rng(12)
    t = np.concatenate([lattice(4), lattice(4)])
    q = (rng.random((200, 3)) * 5 - 1).astype(F32)
    i1, d1 = O.nn1(q, t)
    i, d, nf = S.knn(q, t, 1)
    assert nf == 1 and same(i[:, 0].copy(), i1) and same(d[:, 0].copy(), d1)


@pytest.mark.parametrize("max_nn", [0, 1, 7, 64, 1000])
def test_radius_restatement_equals_the_literal_scan(max_nn):
    """Q4 / Q5: strict `<` against the float r2, rows cut to max_nn only while max_nn < M; r = 0 and a radius that covers everything."""
    rng = np.random.default_rng(13)
    t = lattice(4)
    t3 = np.concatenate([t, t, t])[rng.permutation(192)]
    q = np.concatenate([t[:4], rng.random((5, 3)).astype(F32) * 3])
    for tgt in (t, t3):
        for radius in (0.0, 1.0, 1.5, float(np.sqrt(2.0)), 100.0):
            a, b = S.radius_search(q, tgt, radius, max_nn), S.radius_search_literal(q, tgt, radius, max_nn)
            assert all(same(x, y) for x, y in zip(a, b))
            if radius == 0.0:
                assert a[0][-1] == 0
            if radius == 100.0 and not (0 < max_nn < len(tgt)):
                assert (np.diff(a[0]) == len(tgt)).all()
    # a lattice neighbour at exactly d2 == r2 is excluded: radius 1 around a lattice point holds the point alone
    rs, idx, _ = S.radius_search(t[21:22], t, 1.0)
    assert rs[-1] == 1 and idx[0] == 21


def test_radius_row_is_the_head_of_the_knn_row_that_passes():
    """Q9 in the restatement itself"""
    rng = np.random.default_rng(14)
    t = (rng.random((300, 3)) * 4).astype(F32)
    q = (rng.random((40, 3)) * 4).astype(F32)
    for max_nn in (1, 7, 64):
        ki, kd, _ = S.knn(q, t, max_nn)
        rs, ri, rd = S.radius_search(q, t, 0.7, max_nn)
        for i in range(len(q)):
            keep = kd[i] < S.r2_of(0.7)
            assert same(ri[rs[i]:rs[i + 1]], ki[i][keep]) and same(rd[rs[i]:rs[i + 1]], kd[i][keep])


# ---- the argument checks, through the library (no device: the handle is NULL, which is the LAST thing a call looks at)
def _err(reg, rc):
    return rc, reg.load_library().apdgicp_last_error().decode()


def test_knn_of_argument_checks(reg):
    L = reg.load_library()
    q = np.zeros((4, 3), dtype=F32)
    idx, sqd, nf = np.zeros((4, 64), dtype=np.int32), np.zeros((4, 64), dtype=F32), C.c_int32()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda qq, n, stride, k: L.apdgicp_knn_of(None, p(qq) if qq is not None else None, n, stride, k, p(idx), p(sqd), C.byref(nf))  # noqa: E731
    for k in (0, -3):
        rc, msg = _err(reg, call(q, 4, 12, k))
        assert rc == ERR_INVALID_ARG and "k must be" in msg
    for k in (65, 1000):
        rc, msg = _err(reg, call(q, 4, 12, k))
        assert rc == ERR_UNSUPPORTED and "64" in msg
    assert call(q, 0, 12, 5) == ERR_INVALID_ARG and call(q, -1, 12, 5) == ERR_INVALID_ARG
    assert call(None, 4, 12, 5) == ERR_INVALID_ARG
    for stride in (8, 0, 13):
        rc, msg = _err(reg, call(q, 4, stride, 5))
        assert rc == ERR_INVALID_ARG and "stride" in msg
    for bad in (np.nan, np.inf, -np.inf):
        qq = q.copy()
        qq[3, 0], qq[2, 1] = bad, bad                     # (the first such query is named)
        rc, msg = _err(reg, call(qq, 4, 12, 5))
        assert rc == ERR_INVALID_ARG and "query 2 " in msg
    q16 = np.zeros((4, 4), dtype=F32)
    q16[:, 3] = np.nan                                   # (16-byte rows: the fourth float is not a coordinate)
    rc, msg = _err(reg, call(q16, 4, 16, 5))
    assert rc == ERR_INVALID_ARG and "null" in msg   # every check of the queries passed: what is left is the NULL handle
    for k in (1, 64):
        rc, msg = _err(reg, call(q, 4, 12, k))
        assert rc == ERR_INVALID_ARG and "null" in msg


def test_radius_search_argument_checks(reg):
    L = reg.load_library()
    q = np.zeros((4, 3), dtype=F32)
    rs, total = np.zeros(5, dtype=np.int64), C.c_int64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda qq, n, stride, r, m: L.apdgicp_radius_search_of(None, p(qq), n, stride, r, m, p(rs), C.byref(total))  # noqa: E731
    for r in (-1.0, -1e-30, np.nan, np.inf):
        rc, msg = _err(reg, call(q, 4, 12, r, 0))
        assert rc == ERR_INVALID_ARG and "radius" in msg
    rc, msg = _err(reg, call(q, 4, 12, 1.0, -1))
    assert rc == ERR_INVALID_ARG and "max_nn" in msg
    assert call(q, 0, 12, 1.0, 0) == ERR_INVALID_ARG
    rc, msg = _err(reg, call(q, 4, 8, 1.0, 0))
    assert rc == ERR_INVALID_ARG and "stride" in msg
    qq = q.copy()
    qq[1, 2] = np.nan
    rc, msg = _err(reg, call(qq, 4, 12, 1.0, 0))
    assert rc == ERR_INVALID_ARG and "query 1 " in msg
    for r, m in ((0.0, 0), (2.0, 20), (2.0, 1 << 30)):   # accepted values: only the NULL handle is left to refuse
        rc, msg = _err(reg, call(q, 4, 12, r, m))
        assert rc == ERR_INVALID_ARG and "null" in msg
    # Q6: the rows of no handle
    assert L.apdgicp_radius_search_rows(None, None, None) == ERR_INVALID_ARG
    a, b = C.c_int64(), C.c_int64()
    assert L.apdgicp_search_group_stats(None, C.byref(a), C.byref(b)) == ERR_INVALID_ARG
