"""Host side of the SVC sink encoder: the worst-case packet bound that sizes
the GPU encoder's staging, checked against the CPU encoder (no GPU
needed)."""
import numpy as np
import pytest

from scanner_amd import _core


def bound_formula(nbytes):
    ngroups = (nbytes + 31) // 32
    nsuper = (ngroups + 127) // 128
    pad4 = (ngroups + 3) // 4 * 4
    return 20 + 4 * nsuper + pad4 + 32 * ngroups


@pytest.mark.parametrize(
    "nbytes", [1, 9, 32, 33, 4095, 4096, 4097, 1920 * 1080 * 3])
def test_packet_bound_formula(nbytes):
    assert _core.svc_packet_bound(nbytes) == bound_formula(nbytes)


@pytest.mark.parametrize("shape", [(3, 1, 3, 3), (4, 5, 7, 3), (3, 37, 45, 3),
                                   (2, 32, 128, 1)])
def test_noise_packets_within_bound(shape):
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, size=shape).astype(np.uint8)
    stream, sizes = _core.svc_cpu_encode(frames, 2)
    bound = _core.svc_packet_bound(int(np.prod(shape[1:])))
    assert len(sizes) == shape[0]
    assert sum(sizes) == len(stream)
    assert all(s <= bound for s in sizes)


@pytest.mark.parametrize("shape", [(1, 1, 3, 3), (1, 5, 7, 3), (1, 37, 45, 3),
                                   (1, 32, 128, 1)])
def test_zero_keyframe_hits_bound(shape):
    """An all-zero keyframe is the worst case: every group's first residual
    is 0 - 128 = -128, which zigzags to 255 and needs width 8."""
    frames = np.zeros(shape, np.uint8)
    stream, sizes = _core.svc_cpu_encode(frames, 16)
    bound = _core.svc_packet_bound(int(np.prod(shape[1:])))
    assert sizes == [bound]
    assert len(stream) == bound


def test_cpu_decode_binding_roundtrip():
    rng = np.random.RandomState(5)
    frames = rng.randint(0, 256, size=(7, 5, 7, 3)).astype(np.uint8)
    stream, sizes = _core.svc_cpu_encode(frames, 3)
    got = _core.svc_cpu_decode(stream, sizes, 5, 7, 3, 3)
    np.testing.assert_array_equal(got, frames)
