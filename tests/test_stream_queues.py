"""GPU tests: the main streams of four batch handles run side by side, whatever else the process created first.

Two HIP streams that share a hardware queue run their work one behind the other.  One spin kernel of T1 milliseconds on each of
four streams therefore takes about T1 when every stream has a queue of its own and at least 2 T1 when any two share; the tests
assert the midpoint, 1.5 T1.  The engine's streams come from the registry of riv-slam_amd/csrc/apd_streams.hpp, which places
them in a priority class of their own (its queues are not the ones the null stream, torch and RCCL use)."""
import ctypes as C
import os

import pytest

pytestmark = pytest.mark.gpu

N_HANDLES = 4


@pytest.fixture(scope="module")
def gpu():
    import importlib

    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    reg = importlib.import_module("riv-slam_amd.registration")
    L = reg.load_library()
    hip = C.CDLL(_loaded_hip_runtime())
    lo, hi = C.c_int(0), C.c_int(0)
    assert hip.hipDeviceGetStreamPriorityRange(C.byref(lo), C.byref(hi)) == 0
    if lo.value == hi.value:
        pytest.skip("the device reports a single stream priority level: nothing to place")
    torch.cuda.set_device(0)
    cycles, t1 = _calibrate(torch)
    print(f"priority range {lo.value} .. {hi.value}; GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}; "
          f"_sleep({cycles}) = T1 = {t1:.3f} ms")
    return torch, reg, cycles, t1


def _loaded_hip_runtime() -> str:
    """The copy of libamdhip64 this process already runs on (torch wheels bundle their own)."""
    with open("/proc/self/maps") as fh:
        for line in fh:
            if "libamdhip64" in line:
                return line.split()[-1]
    return "libamdhip64.so"


def _timed_sleeps(torch, streams, cycles) -> float:
    """Milliseconds from before the first to behind the last of one _sleep per stream (the GPU idle before and all streams released together)."""
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    cur = torch.cuda.current_stream()
    e0.record(cur)
    for s in streams:
        s.wait_event(e0)
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
    for s in streams:
        done = torch.cuda.Event()
        done.record(s)
        cur.wait_event(done)
    e1.record(cur)
    e1.synchronize()
    return e0.elapsed_time(e1)


def _calibrate(torch):
    """A cycle count for which one _sleep lasts 2 - 5 ms, and the time T1 it takes (best of three: an upper bound on T1 only loosens the check's lower side)."""
    cur = [torch.cuda.current_stream()]
    cycles = 1_000_000
    _timed_sleeps(torch, cur, cycles)   # (loads the kernel)
    t = min(_timed_sleeps(torch, cur, cycles) for _ in range(3))
    cycles = int(cycles * 3.5 / max(t, 1e-3))
    t1 = min(_timed_sleeps(torch, cur, cycles) for _ in range(3))
    assert 2.0 <= t1 <= 5.0, f"calibration: _sleep({cycles}) took {t1:.3f} ms"
    return cycles, t1


def _handles(reg, n):
    return [reg.BatchAPDGICP(reg.default_params(), device=0) for _ in range(n)]


def _check_side_by_side(torch, handles, cycles, t1, what):
    streams = [torch.cuda.ExternalStream(h.stream_ptr(), device=0) for h in handles]
    assert len({h.stream_ptr() for h in handles}) == len(handles)
    _timed_sleeps(torch, streams, cycles)   # (first use of each stream)
    t4 = min(_timed_sleeps(torch, streams, cycles) for _ in range(3))
    print(f"{what}: T4 = {t4:.3f} ms, T1 = {t1:.3f} ms, T4 / T1 = {t4 / t1:.2f}")
    assert t4 < 1.5 * t1, f"{what}: four handle streams took {t4:.3f} ms for {t1:.3f} ms of work each: two of them share a hardware queue"


def test_four_handles_each_on_a_queue_of_their_own(gpu):
    torch, reg, cycles, t1 = gpu
    hs = _handles(reg, N_HANDLES)
    try:
        _check_side_by_side(torch, hs, cycles, t1, "four handles")
    finally:
        for h in hs:
            h.close()


def test_streams_created_before_the_handles_do_not_matter(gpu):
    """Three torch streams, created AND used, occupy queues of the normal class before the first handle exists."""
    torch, reg, cycles, t1 = gpu
    others = [torch.cuda.Stream() for _ in range(3)]
    for s in others:
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    hs = _handles(reg, N_HANDLES)
    try:
        _check_side_by_side(torch, hs, cycles, t1, "four handles behind three torch streams")
    finally:
        for h in hs:
            h.close()
    del others


def test_slots_of_closed_handles_are_reused(gpu):
    torch, reg, cycles, t1 = gpu
    hs = _handles(reg, N_HANDLES)
    try:
        _check_side_by_side(torch, hs, cycles, t1, "four handles")
        for h in hs[:2]:
            h.close()
        hs[:2] = _handles(reg, 2)
        _check_side_by_side(torch, hs, cycles, t1, "two of four handles closed and created again")
    finally:
        for h in hs:
            h.close()
