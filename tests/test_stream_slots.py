"""CPU tests (-m "not gpu"): the policy of the engine's stream registry (riv-slam_amd/csrc/apd_streams.hpp) as the library compiles it,
in the stand-alone program tests/cpp/test_stream_slots.cpp under ThreadSanitizer and under AddressSanitizer / UBSan.  The policy has
no HIP in it (creation and destruction are injected), so the program needs neither a GPU nor the fake runtime."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.parametrize("san", ("thread", "address,undefined"))
def test_stream_registry_policy_under_sanitizers(san):
    """Fill to Q, overflow to the normal class, release and reuse, Q from an unset / garbage / zero environment value, a device with one
    priority level, eight threads acquiring and releasing -- three runs each."""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "stream_slots_" + san.split(",")[0])
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", f"-fsanitize={san}", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "riv-slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_stream_slots.cpp"), "-o", exe])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for _ in range(3):
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        report = out.stdout + out.stderr
        assert "ThreadSanitizer" not in report and "AddressSanitizer" not in report and "runtime error" not in report, report[-4000:]
        assert out.returncode == 0 and "ok 1" in out.stdout, report[-2000:]
