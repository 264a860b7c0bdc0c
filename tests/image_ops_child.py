"""Child process of test_image_ops_gpu.py: the rows-per-thread optical-flow
case under SCANNER_LK_PY=4, which the library reads once per process.

    SCANNER_LK_PY=4 python image_ops_child.py

Exits non-zero at the first failed check.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import image_ops_cases as C  # noqa: E402
from scanner_amd import _core  # noqa: E402

if __name__ == "__main__":
    assert _core.have_gpu()
    assert os.environ.get("SCANNER_LK_PY") == "4"
    worst = C.check_flow_rows(C.GPU, "PY=4")
    print(f"worst err/tol PY=4: {worst:.3f}")
    print("child OK")
