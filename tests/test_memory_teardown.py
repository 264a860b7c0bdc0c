"""Allocator teardown with a CPU pool (runs in a child process: a regression
here is a crash of the interpreter, not an exception)."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_destroy_memory_with_cpu_pool():
    """The CPU pool returns its slab through the system allocator, which
    therefore has to outlive it; init -> destroy -> init must also work."""
    code = ("from scanner_amd import _core\n"
            "_core.init_memory(1 << 20, 0, [])\n"
            "_core.destroy_memory()\n"
            "_core.init_memory(1 << 20, 0, [])\n"
            "_core.destroy_memory()\n"
            "print('teardown ok')\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-c", code], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-500:]
    assert "teardown ok" in p.stdout
