"""Child process of test_svc_decode_gpu.py: the launch-to-launch handover of
the SVC GPU decoder under SCANNER_SVC_BATCH, which the library reads once per
process.

    SCANNER_SVC_BATCH=1 python svc_decode_child.py

At 1 every delta frame is a launch of its own that starts from `prev` in
HBM. Exits non-zero at the first failed check.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import svc_cases as C  # noqa: E402
from scanner_amd import _core  # noqa: E402

GEOMS = [(5, 7, 3), (1, 2049, 1), (37, 45, 3)]
CONTENTS = ["smooth", "noise", "widths", "overwide_random"]
WANTS = [C.ALL, (39,), (15, 16)]

if __name__ == "__main__":
    assert _core.have_gpu()
    batch = int(os.environ["SCANNER_SVC_BATCH"])
    assert batch in (1, 5)
    calls = handovers = scratch = 0
    for keys in C.FEW_KEYS:
        for want in WANTS:
            for la in C.launches(keys, want, batch):
                assert len(la["frames"]) <= batch
                handovers += la["continues"]
                scratch += la["continues"] and not la["last_wanted"]
            for geom in GEOMS:
                for content in CONTENTS:
                    C.check_gpu(geom, content, keys, C.N, want,
                                ("host", "resident0"))
                    calls += 2
    # per geometry and content: the launches that hand a frame on, and how
    # many of them through the scratch frame
    assert handovers > 0 and scratch > 0
    print(f"batch {batch}: {calls} calls exact, {handovers} handovers "
          f"({scratch} through the scratch frame) per clip")
    print("child OK")
