"""The SVC GPU decoder (kernels/svc_codec.hip) called directly through
_core.svc_gpu_decode on the case list of svc_cases.py: chains longer than a
launch, sparse wants that keep frames in registers only, resident streams
with an offset, packets wider than the encoder would write, launches cut by
SCANNER_SVC_BATCH, four threads at once. The codec is lossless: every
comparison is equality with the source frames, which test_svc_decode_cpu.py
ties to the format and to both CPU readers. Only streams written by
svc_ref.write_stream reach the device: the kernel does not validate widths or
offsets (ROADMAP.md), so no corrupt stream is sent to it."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import svc_cases as C
from scanner_amd import _core

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = C.cases()


@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_decode_matches_source(case):
    """Every want of the case on the host path (stream_offset at the span's
    first frame), resident from byte 0 and resident from the span's key."""
    for want in case.wants:
        C.check_gpu(case.geom, case.content, case.keys, case.n, want)


@pytest.mark.parametrize("batch", [1, 5])
def test_decode_batch_limit(batch):
    """SCANNER_SVC_BATCH is read once per process: a fresh child."""
    out = subprocess.run(
        [sys.executable, os.path.join(HERE, "svc_decode_child.py")],
        env=dict(os.environ, SCANNER_SVC_BATCH=str(batch)),
        capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, \
        f"child exited {out.returncode}:\n{out.stdout[-2000:]}\n" \
        f"{out.stderr[-4000:]}"
    assert "child OK" in out.stdout


BIG_SMOOTH = (C.BIG_GEOM, "smooth", (0,), C.BIG_N)
NOISE_IRREGULAR = ((37, 45, 3), "noise", C.IRREGULAR, C.N)


@pytest.mark.parametrize("clip", [BIG_SMOOTH, NOISE_IRREGULAR],
                         ids=["1mb-smooth", "37x45x3-noise"])
def test_decode_deterministic(clip):
    want = tuple(range(clip[3]))
    for path in C.PATHS:
        runs = [C.gpu_decode(*clip, want, path) for _ in range(3)]
        np.testing.assert_array_equal(runs[0], C.frames(*clip))
        for r in runs[1:]:
            np.testing.assert_array_equal(r, runs[0])


def test_decode_four_threads():
    """What the benchmark does with 4-6 pipeline instances, as an equality
    test: four threads, each five calls on its own clip, host and resident
    paths mixed; a fixed 20 calls, every result exact."""
    clips = [
        (NOISE_IRREGULAR, [C.ALL, (17, 33)]),
        (((5, 7, 3), "widths", (0,), C.N), [C.ALL, (39,)]),
        (((1, 2049, 1), "smooth", tuple(range(C.N)), C.N),
         [C.ALL, (2, 23, 38)]),
        (BIG_SMOOTH, [tuple(range(C.BIG_N)), (17,)]),
    ]
    for clip, _ in clips:   # frames and streams built before any thread
        C.frames(*clip), C.stream(*clip)
    paths = list(C.PATHS)
    errors = []
    done = [0] * len(clips)
    start = threading.Barrier(len(clips))

    def work(t):
        clip, wants = clips[t]
        try:
            start.wait(timeout=60)
            for i in range(5):
                C.check_gpu(*clip, wants[i % 2], (paths[(i + t) % 3],))
                done[t] += 1
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append((t, repr(e)[:2000]))

    threads = [threading.Thread(target=work, args=(t,))
               for t in range(len(clips))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert done == [5] * len(clips)


SMALL = ((5, 7, 3), "noise", (0,), C.N)


def rejected_calls():
    """Each must raise by name before anything reaches the device."""
    data, sizes = C.stream(*SMALL)
    geom = SMALL[0]

    def call(want, resident, first=0, keys=(0,)):
        return _core.svc_gpu_decode(data, sizes, *geom, list(keys),
                                    list(want), resident=resident,
                                    first=first)

    for resident in (False, True):
        with pytest.raises(Exception, match="frame beyond stream"):
            call([C.N], resident)
        with pytest.raises(Exception, match="frame beyond stream"):
            call([3, C.N + 7], resident)
        with pytest.raises(Exception, match="not all frames produced"):
            call([5, 5], resident)
        with pytest.raises(Exception, match="no keyframe before frame"):
            call([3], resident, keys=(5,))
    with pytest.raises(Exception,
                       match="device stream range does not cover span"):
        call([5], True, first=3)
    with pytest.raises(Exception,
                       match="stream range does not cover decode span"):
        call([5], False, first=3)
    with pytest.raises(Exception, match="first beyond stream"):
        call([5], True, first=C.N)


def test_rejections_by_name():
    rejected_calls()
    data, sizes = C.stream(*SMALL)
    for resident in (False, True):
        got = _core.svc_gpu_decode(data, sizes, *SMALL[0], [0], [],
                                   resident=resident)
        assert got.shape == (0,) + SMALL[0] and got.dtype == np.uint8
    # the decoder still works after the rejected calls
    C.check_gpu(*SMALL, C.ALL)


def test_memory_is_returned():
    """mem_stats of the GPU and of the CPU pool unchanged across a dense
    call, a sparse call whose handover goes through the scratch frame, and
    every rejected call."""
    sparse = (17, 33)
    la = C.launches(SMALL[2], sparse)
    assert la[0]["continues"] and not la[0]["last_wanted"]

    def calls():
        C.check_gpu(*SMALL, C.ALL)
        C.check_gpu(*SMALL, sparse)
        rejected_calls()

    calls()  # the peak settles
    before = (_core.mem_stats(0), _core.mem_stats(-1))
    calls()
    assert (_core.mem_stats(0), _core.mem_stats(-1)) == before
