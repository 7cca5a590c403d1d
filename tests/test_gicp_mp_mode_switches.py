"""Switching a single handle between FastGICPMultiPoints and each of its five other pipelines -- APD-GICP (none), voxelized GICP,
FAST_VGICP_CUDA, NDT, point-to-point ICP -- in the manner of tests/test_mode_switches.py (the transition table: DESIGN.md, "Mode
transitions").  For every existing mode X: X -> this mode gives the bytes of a handle that was only ever in this mode, and this mode -> X
gives X's fresh bytes -- the align's record with its pose, and the final Hessian; exactly the flag of the mode that is on is set; the
mode's own getters answer APDGICP_ERR_NO_INPUT while it is off.  Both sides run the same kernels on the same clouds, so the bar is equality.

Clouds: pair["source"][:257] and pair["target"][:700] of tests/golden/vgicp_cuda_pair.npz, max_iterations = 3, as there."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("apd", "vgicp", "vgicp_cuda", "ndt", "icp")
MODES = OTHERS + ("gicp_mp",)
NO_INPUT = -3
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def reg():
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("riv-slam_amd.registration")


@pytest.fixture(scope="module")
def mode_params(reg):
    mod = lambda name: importlib.import_module("riv-slam_amd." + name)
    return {"vgicp": mod("vgicp").default_vgicp_params(), "vgicp_cuda": mod("vgicp_cuda").default_vgicp_cuda_params(), "ndt": mod("ndt").default_ndt_params(),
            "icp": mod("icp").default_icp_params(), "gicp_mp": mod("gicp_mp").default_gicp_mp_params()}


@pytest.fixture(scope="module")
def pair():
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "vgicp_cuda_pair.npz")))
    return {"source": d["source"][:257], "target": d["target"][:700], "guess": d["guess"]}


def _switch(L, h, a, b, mode_params):
    """to B through B's setter; to APD through A's setter with NULL"""
    rc = getattr(L, "apdgicp_set_" + a)(h, None) if b == "apd" else getattr(L, "apdgicp_set_" + b)(h, C.byref(mode_params[b]))
    assert rc == 0, L.apdgicp_last_error().decode()


def _flags(L, h):
    out = {}
    for m in MODES[1:]:
        on = C.c_int32(-1)
        assert getattr(L, "apdgicp_get_" + m)(h, None, C.byref(on)) == 0
        out[m] = on.value
    return out


def _handle(reg, pair):
    g = reg.FastAPDGICP(reg.default_params(max_iterations=3))
    g.setInputSource(pair["source"])
    g.setInputTarget(pair["target"])
    return g


def _align(g, pair):
    guess = np.ascontiguousarray(pair["guess"].T, dtype=np.float32)
    res = type(g.result)()
    rc = g.L.apdgicp_align(g.h, guess.ctypes.data_as(C.c_void_p), C.byref(res))
    H = np.full(36, -7.0)
    rh = g.L.apdgicp_get_final_hessian(g.h, H.ctypes.data_as(C.c_void_p))
    return rc, bytes(res), (rh, H.tobytes())


def _mp_getters(g):
    """the return codes of the getters only this mode answers"""
    L, n, s = g.L, C.c_int64(), C.c_int32()
    buf = np.zeros(g.n_src * g.n_tgt + g.n_src + 1)   # (room for every row entry there can be)
    p = buf.ctypes.data_as(C.c_void_p)
    return [L.apdgicp_gicp_mp_get_rows(g.h, p, g.n_src, C.byref(n)), L.apdgicp_gicp_mp_get_row_entries(g.h, p, p), L.apdgicp_gicp_mp_get_fused(g.h, p, None, None, g.n_src),
            L.apdgicp_gicp_mp_get_trace(g.h, 0, None, None, None, None, C.byref(n)), L.apdgicp_gicp_mp_state(g.h, C.byref(s)), L.apdgicp_gicp_mp_debug_counts(g.h, C.byref(n), C.byref(n))]


@pytest.fixture(scope="module")
def fresh(reg, pair, mode_params):
    """per mode: what a handle that was only ever in it returns"""
    out = {}
    for b in MODES:
        g = _handle(reg, pair)
        if b != "apd":
            _switch(g.L, g.h, "apd", b, mode_params)
        out[b] = _align(g, pair)
        assert out[b][0] == 0, (b, g.L.apdgicp_last_error().decode())
        g.close()
    return out


@gpu
@pytest.mark.parametrize("x", OTHERS)
def test_into_the_mode(reg, pair, mode_params, fresh, x):
    g = _handle(reg, pair)
    L = g.L
    if x != "apd":
        _switch(L, g.h, "apd", x, mode_params)
    assert _mp_getters(g) == [NO_INPUT] * 6
    assert _align(g, pair)[0] == 0, L.apdgicp_last_error().decode()
    if x != "icp":
        g.linearize(np.eye(4))
    _switch(L, g.h, x, "gicp_mp", mode_params)
    assert _flags(L, g.h) == {m: int(m == "gicp_mp") for m in MODES[1:]}   # the four existing getters report 0
    assert _mp_getters(g)[:3] == [NO_INPUT] * 3   # (no linearize in the mode yet)
    rc, rec, hess = _align(g, pair)
    assert rc == 0, L.apdgicp_last_error().decode()
    assert rec == fresh["gicp_mp"][1] and hess == fresh["gicp_mp"][2]
    assert _mp_getters(g) == [0] * 6
    g.close()


@gpu
@pytest.mark.parametrize("x", OTHERS)
def test_out_of_the_mode(reg, pair, mode_params, fresh, x):
    g = _handle(reg, pair)
    L = g.L
    _switch(L, g.h, "apd", "gicp_mp", mode_params)
    assert _align(g, pair)[0] == 0, L.apdgicp_last_error().decode()
    g.linearize(np.eye(4))
    _switch(L, g.h, "gicp_mp", x, mode_params)
    assert _flags(L, g.h) == {m: int(m == x) for m in MODES[1:]}
    assert _mp_getters(g) == [NO_INPUT] * 6
    rc, rec, hess = _align(g, pair)
    assert rc == 0, L.apdgicp_last_error().decode()
    assert rec == fresh[x][1] and hess == fresh[x][2]   # x = apd: an APD align after a visit equals that of a handle that never had the mode
    g.close()


@gpu
def test_enable_zero_and_null_switch_off_and_are_no_ops_elsewhere(reg, pair, mode_params):
    g = _handle(reg, pair)
    L = g.L
    _switch(L, g.h, "apd", "ndt", mode_params)
    assert L.apdgicp_set_gicp_mp(g.h, None) == 0 and _flags(L, g.h)["ndt"] == 1   # a no-op while another mode is on
    _switch(L, g.h, "ndt", "gicp_mp", mode_params)
    off = type(mode_params["gicp_mp"])(0, 0, 0.75)
    assert L.apdgicp_set_gicp_mp(g.h, C.byref(off)) == 0
    assert _flags(L, g.h) == {m: 0 for m in MODES[1:]}
    got = type(off)()
    assert L.apdgicp_get_gicp_mp(g.h, C.byref(got), None) == 0 and (got.enable, got.neighbor_search_radius) == (0, 0.75)   # stored
    g.close()
