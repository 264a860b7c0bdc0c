"""ThreadSanitizer gate for the engine's shared concurrency primitives
(BoundedQueue between pipeline stages, Profiler): compiles
tests/cpp/tsan_concurrency.cpp with -fsanitize=thread (plain g++ — the
primitives are HIP-free C++) and requires zero TSAN reports. The reference
ships no race detection at all."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_aslr():
    """Command prefix that turns address-space randomisation off for the
    child. libtsan only accepts a fixed set of address ranges and exits
    with "FATAL: ThreadSanitizer: unexpected memory mapping" where the
    kernel randomises more bits than it expects (vm.mmap_rnd_bits = 32)."""
    import platform
    import shutil
    setarch = shutil.which("setarch")
    if setarch:
        prefix = [setarch, platform.machine(), "-R"]
        probe = subprocess.run(prefix + ["true"], capture_output=True)
        if probe.returncode == 0:
            return prefix
    return []


def test_tsan_queue_profiler(tmp_path):
    src = os.path.join(REPO, "tests", "cpp", "tsan_concurrency.cpp")
    binp = str(tmp_path / "tsan_test")
    r = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-pthread",
         src, "-o", binp],
        capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        pytest.fail(f"tsan build failed:\n{r.stderr[-2000:]}")
    env = dict(os.environ)
    env["TSAN_OPTIONS"] = "halt_on_error=1 exitcode=66"
    run = subprocess.run(_no_aslr() + [binp], capture_output=True, text=True,
                         env=env, timeout=300)
    out = run.stdout + run.stderr
    assert run.returncode == 0, f"tsan reported races:\n{out[-3000:]}"
    assert "OK" in out
    assert "WARNING: ThreadSanitizer" not in out
