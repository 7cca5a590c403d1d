"""CPU tests (-m "not gpu"): the product's HOST-side thread logic under ThreadSanitizer and AddressSanitizer / UBSan.

No sanitizer runs on the GPU box (not available there); what can race or overrun on the host is plain C++ around hip* / nccl* /
apdgicp_* calls, so a test-only, link-time fake of those three call families (tests/cpp/fake/, never shipped) lets the real
`ShardedBatchAlignerHip` -- worker threads, queues, slots, late gathers, abort_all -- run the schedule of tests/cpp/test_multi_device.cpp on
four fake devices; the engine's own host code that needs no HIP at all (riv-slam_amd/csrc/apd_hostpack.hpp: packing host clouds, the
process-wide thread pool; riv-slam_amd/csrc/apd_devbuf.hpp: the owners of device and pinned memory) is compiled as it is.  Also: the sanitizer build of the ORACLE (oracle/Makefile) runs a registration."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "cpp", "fake")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"   # has the sanitizer runtimes and intercepts pthread_cond_clockwait; g++ 11's libtsan does not


def _compile(sources, exe, san, includes, need_clang=False):
    os.makedirs(OUT, exist_ok=True)
    cxx = CLANG if os.path.exists(CLANG) else ("g++" if not need_clang else None)
    if cxx is None:
        pytest.skip("needs clang++ (vector extensions of apd_hostpack.hpp)")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-pthread", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    if cxx == "g++" and san == "thread":
        cmd += ["-include", os.path.join(FAKE, "tsan_prelude.h")]   # (see that file: libstdc++'s wait_for and GCC 11's libtsan)
    for inc in includes:
        cmd += ["-I", inc]
    cmd += sources + ["-o", exe]
    subprocess.check_call(cmd)
    return exe


def _run(exe, env_extra):
    env = dict(os.environ, **env_extra)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    report = out.stdout + out.stderr
    assert "ThreadSanitizer" not in report and "AddressSanitizer" not in report and "runtime error" not in report, report[-4000:]
    assert out.returncode == 0 and "ok 1" in out.stdout, report[-2000:]
    return report


@pytest.mark.parametrize("san", ("thread", "address,undefined"))
def test_sharded_aligner_host_logic_under_sanitizers(san):
    """riv-slam_amd/cpp/sharded_batch_hip.hpp on four fake devices: batches twice, three times as many batches as slots with in_flight - 1
    uncollected, the Gauss-Newton form collected out of order, a poisoned cloud failing ONE rank mid-batch with a good batch right behind it,
    a failed record allocation (fallback buffers), a block too large for the fallback (abort_all: every collect returns) -- five runs each."""
    exe = _compile([os.path.join(FAKE, "test_sharded_fake.cpp"), os.path.join(FAKE, "fake_backend.cpp")], os.path.join(OUT, "sharded_fake_" + san.split(",")[0]), san,
                   [os.path.join(FAKE, "include"), os.path.join(ROOT, "include"), os.path.join(ROOT, "riv-slam_amd", "cpp")])
    for _ in range(5):
        rep = _run(exe, {"TSAN_OPTIONS": "halt_on_error=1", "ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
        assert "live_allocations 0" in rep


@pytest.mark.parametrize("san", ("thread", "address,undefined"))
def test_host_cloud_packing_and_the_host_pool_under_sanitizers(san):
    """apd_hostpack.hpp as the engine compiles it: pack_staged_host from heap blocks of exactly n x stride bytes (its 16-byte loads must never
    reach behind the last point), NaN coordinates, strides 12 / 16 / 32; the shared pool with three callers at once."""
    exe = _compile([os.path.join(FAKE, "test_hostpack.cpp")], os.path.join(OUT, "hostpack_" + san.split(",")[0]), san,
                   [os.path.join(ROOT, "riv-slam_amd", "csrc")], need_clang=True)
    _run(exe, {"TSAN_OPTIONS": "halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})


def test_buffer_owners_under_sanitizers():
    """riv-slam_amd/csrc/apd_devbuf.hpp as the library compiles it, against the fake runtime (its hipMalloc is malloc, so a double free or a use
    after free is a report and fake_live_allocations() counts leaks): DevBuf, PinnedBuf and CachedTable::dev through ensure / release / moves /
    std::swap, a vector of owners resized up and down, the four-buffer growth of the scan-context database with an allocation failing half way."""
    exe = _compile([os.path.join(FAKE, "test_devbuf.cpp"), os.path.join(FAKE, "fake_backend.cpp")], os.path.join(OUT, "devbuf_address"), "address,undefined",
                   [os.path.join(FAKE, "include"), os.path.join(ROOT, "include"), os.path.join(ROOT, "riv-slam_amd", "csrc")])
    rep = _run(exe, {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert "live_allocations 0 device 0 pinned 0" in rep


def test_the_oracle_runs_clean_under_address_sanitizer(tmp_path):
    """oracle/Makefile's sanitizer build of the CHECKER (_build/libapdgicp_ref_asan.so), loaded in a child interpreter with libasan preloaded:
    kd-tree build, 20-NN covariances, an LM registration from the golden guess and a batch of kd-tree queries on the golden clouds."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "_build/libapdgicp_ref_asan.so"])
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan.so not found")
    code = f"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, {os.path.join(ROOT, "oracle")!r})
import ref as R
R._LIB_PATH = {os.path.join(ROOT, "oracle", "_build", "libapdgicp_ref_asan.so")!r}
R.build = lambda force=False: R._LIB_PATH
g = dict(np.load({os.path.join(ROOT, "tests", "golden", "apdgicp_golden.npz")!r}))
o = R.RefAPDGICP(R.default_params(max_correspondence_distance=2.0, transformation_epsilon=0.1, azimuth_variance_deg=1.0))
o.setInputSource(g["lin_source"]); o.setInputTarget(g["lin_target"])
T = o.align(g["lin_guess"])
assert [int(o.converged), o.nr_iterations, o.n_linearize, o.n_compute_error] == list(g["lm_launch_info"]), "counts"
idx, d = o.knn_kdtree_batch("target", g["lin_source"][:300], 20)
assert idx.shape == (300, 20) and (np.diff(d, axis=1) >= 0).all()
print("asan-ok")
"""
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", OMP_NUM_THREADS="4")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert out.returncode == 0 and "asan-ok" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])
