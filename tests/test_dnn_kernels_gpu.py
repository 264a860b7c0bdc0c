"""Direct GPU tests of every GEMM / convolution dispatch path and of the DNN
helper kernels, each against a float64 CPU reference computed from the
bf16-rounded inputs.

The shape table, the reference, the derived tolerance and the mutation
check live in dnn_ref.py (its docstring derives the tolerance);
test_gemm_plan.py pins the table on the CPU. Every test here first asserts
that its shape takes the path it is meant to cover, then that the
comparator flags seeded bugs on these very inputs (from the reference
alone), and only then trusts the kernel's pass. Every element is compared;
the worst err/tol per case is printed (`pytest -rP` shows it).

Worst err/tol measured on an MI355X is tabulated in docs/testing.md
(0.58-0.99 over all paths); it is informational, tol is not tuned from it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dnn_ref as R
from scanner_amd import _core

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _ids(c):
    return c["id"] + ("" if c["scratch"] in (0, R.AMPLE)
                      else f"-scratch{c['scratch']}")


# ---- GEMM paths ----

def _run_gemm(case, inp, epi, **kw):
    return _core.gemm_bf16_test(inp["A"], inp["B"],
                                splitk_scratch_bytes=case["scratch"],
                                **R.pick(inp, epi), **kw)


@pytest.mark.parametrize("case", R.GEMM_CASES, ids=_ids)
def test_gemm_path(case):
    M, N, K = case["M"], case["N"], case["K"]
    assert R.plan_of(_core, M, N, K, case["scratch"]) == case["plan"]
    inp = R.gemm_inputs(case)
    R.assert_mutations_flagged(inp["A"], inp["B"], inp, K, case["id"])
    worst = 0.0
    for name, epi in R.EPILOGUES.items():
        ref, mag = R.gemm_ref(inp["A"], inp["B"], **R.pick(inp, epi))
        got = _run_gemm(case, inp, epi)
        worst = max(worst, R.assert_within(got, ref, R.tolerance(ref, mag, K),
                                           f"{case['id']} {name}"))
        if case["plan"]["kernel"] == "splitk":
            # the partials + ordered reduce claim run-to-run determinism
            again = _run_gemm(case, inp, epi)
            assert np.array_equal(got, again), f"{case['id']} {name}"
    print(f"worst err/tol {_ids(case)}: {worst:.3f}")


@pytest.mark.parametrize("case", R.GEMM_CASES, ids=_ids)
def test_gemm_path_exact(case):
    assert R.plan_of(_core, case["M"], case["N"], case["K"],
                     case["scratch"]) == case["plan"]
    inp = R.gemm_exact_inputs(case)
    for epi in (R.FULL_NO_RELU, R.EPILOGUES["scale+bias+residual+relu"]):
        ref, _ = R.gemm_ref(inp["A"], inp["B"], **R.pick(inp, epi))
        R.assert_exact_reference(ref)
        got = _run_gemm(case, inp, epi)
        bad = np.argwhere(got != ref.astype(np.float32))
        assert bad.size == 0, (f"{len(bad)} elements differ, first at "
                               f"{bad[0]}: {got[tuple(bad[0])]} vs "
                               f"{ref[tuple(bad[0])]}")


def test_gemm_positional_call_unchanged():
    """gemm_bf16_test(A, B, relu) as the older tests call it."""
    case = R.GEMM_CASES[3]
    inp = R.gemm_inputs(case)
    ref, mag = R.gemm_ref(inp["A"], inp["B"], relu=True)
    got = _core.gemm_bf16_test(inp["A"], inp["B"], True)
    R.assert_within(got, ref, R.tolerance(ref, mag, case["K"]), "positional")


# ---- convolutions ----

def _run_conv(case, inp, epi, implicit, **kw):
    return _core.conv_bf16_test(
        inp["x"], inp["w"], case["r"], case["s"], case["stride"], case["pad"],
        splitk_scratch_bytes=case["scratch"], implicit=implicit,
        **R.pick(inp, epi), **kw)


@pytest.mark.parametrize("implicit", [True, False],
                         ids=["implicit", "im2col"])
@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c["id"])
def test_conv_path(case, implicit):
    M, N, kp = case["M"], case["N"], case["kp"]
    rsc = case["r"] * case["s"] * case["c"]
    assert R.plan_of(_core, M, N, kp, case["scratch"], implicit) \
        == case["plan"]
    inp = R.conv_inputs(case)
    cols_ref = R.im2col_ref(inp["x"], case["r"], case["s"], case["stride"],
                            case["pad"], kp)
    R.assert_mutations_flagged(cols_ref, inp["w"], inp, rsc, case["id"])
    worst = 0.0
    for name, epi in R.EPILOGUES.items():
        what = f"{case['id']} {name}"
        ref, mag = R.conv_ref(case, inp, **R.pick(inp, epi))
        got, cols = _run_conv(case, inp, epi, implicit)
        assert np.array_equal(cols, cols_ref), f"{what}: im2col differs"
        worst = max(worst, R.assert_within(
            got, ref, R.tolerance(ref, mag, rsc), what))
        if case["plan"]["kernel"] == "splitk":
            again, _ = _run_conv(case, inp, epi, implicit)
            assert np.array_equal(got, again), what
    print(f"worst err/tol conv {case['id']} "
          f"{'implicit' if implicit else 'im2col'}: {worst:.3f}")

    inp = R.conv_exact_inputs(case)
    ref, _ = R.conv_ref(case, inp, **R.pick(inp, R.FULL_NO_RELU))
    R.assert_exact_reference(ref)
    got, _ = _run_conv(case, inp, R.FULL_NO_RELU, implicit)
    assert np.array_equal(got, ref.astype(np.float32)), \
        f"{case['id']}: exact case differs"


# ---- variants chosen by environment variables: one fresh child each ----

_child_failed = []


def _run_child(env, *args):
    if _child_failed:
        pytest.fail(f"not started: child {_child_failed[0]} failed earlier")
    out = subprocess.run(
        [sys.executable, os.path.join(HERE, "dnn_child.py")] + list(args),
        env=dict(os.environ, **env), capture_output=True, text=True,
        timeout=120)
    print(out.stdout)
    if out.returncode != 0:
        _child_failed.append(args[0])
        pytest.fail(f"child {args[0]} exited {out.returncode}:\n"
                    f"{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    assert "child OK" in out.stdout


@pytest.fixture(scope="module")
def default_path_npz(tmp_path_factory):
    """What the default split-K path (partials + reduce kernel) computes,
    for the children to compare with bit for bit."""
    arrays = {}
    for case in R.SPLITK_CASES:
        inp = R.gemm_inputs(case)
        for name, epi in R.EPILOGUES.items():
            arrays[f"gemm/{case['id']}/{name}"] = _run_gemm(case, inp, epi)
    (case,) = [c for c in R.CONV_CASES if c["plan"]["kernel"] == "splitk"]
    inp = R.conv_inputs(case)
    rsc = case["r"] * case["s"] * case["c"]
    for name, epi in R.EPILOGUES.items():
        ref, mag = R.conv_ref(case, inp, **R.pick(inp, epi))
        arrays[f"conv/ref/{name}"] = ref
        arrays[f"conv/tol/{name}"] = R.tolerance(ref, mag, rsc)
        arrays[f"conv/out/{name}"] = _run_conv(case, inp, epi, True)[0]
    path = str(tmp_path_factory.mktemp("splitk") / "default_path.npz")
    np.savez(path, **arrays)
    return path


def test_smallk_multi_tile_walk():
    """tiles_per_wg > 1: the double-buffered cross-tile A prefetch, with a
    lone and a partial last tile."""
    _run_child({"SCANNER_SMALLK_WGS": "256"}, "smallk-walk")


def test_splitk_fused_bit_equal_and_repeatable(default_path_npz):
    _run_child({"SCANNER_SPLITK_FUSED": "1"}, "fused", default_path_npz)


def test_splitk_atomic_within_tolerance(default_path_npz):
    _run_child({"SCANNER_SPLITK_ATOMIC": "1"}, "atomic", default_path_npz)


# ---- helper kernels ----

@pytest.mark.parametrize("shape", [(2, 15, 13, 64), (1, 7, 9, 20),
                                   (1, 5, 5, 3)], ids=str)
def test_maxpool(shape):
    """c % 8 == 0 takes the vector kernel, the others the scalar one."""
    rng = np.random.RandomState(shape[3])
    x = R.bf16_round(rng.randn(*shape))
    for name, xx in (("mixed", x), ("all-negative", -np.abs(x) - 1.0)):
        xx = R.bf16_round(xx)
        got = _core.maxpool3x3s2_bf16_test(xx)
        ref = R.maxpool_ref(xx)
        assert got.shape == ref.shape
        assert np.array_equal(got, ref.astype(np.float32)), name
    assert got.max() < 0  # the -1e30 start value never leaks out


def test_avgpool():
    rng = np.random.RandomState(7)
    x = R.bf16_round(rng.randn(2, 7, 7, 72) + 0.5)
    ref, tol = R.avgpool_ref(x)
    got = _core.global_avgpool_bf16_test(x)
    print(f"worst err/tol avgpool: "
          f"{R.assert_within(got, ref, tol, 'avgpool'):.3f}")
    # exact case: integers whose sum is a multiple of hw
    xi = np.zeros((2, 7, 7, 72), np.float32)
    xi += rng.randint(-100, 101, (2, 1, 1, 72))
    xi[:, 0, 0] += 49
    xi[:, 3, 4] -= 49
    got = _core.global_avgpool_bf16_test(xi)
    assert np.array_equal(got, xi.astype(np.float64).mean(axis=(1, 2)))


def test_bf16_rows_to_f32_padded_stride():
    rng = np.random.RandomState(8)
    x = R.bf16_round(rng.randn(3, 1024) * 100)
    got = _core.bf16_rows_to_f32_test(x, 1000)
    assert got.dtype == np.float32 and got.shape == (3, 1000)
    assert np.array_equal(got, x[:, :1000])


def test_concat3_pose_geometry():
    rng = np.random.RandomState(9)
    npix = 50
    a = R.bf16_round(rng.randn(npix, 128))
    b = R.bf16_round(rng.randn(npix, 64))
    c = R.bf16_round(rng.randn(npix, 64))
    b[:, 38:] = 7.0   # source pad columns must not be copied
    c[:, 19:] = -7.0
    got = _core.concat3_bf16_test(a, 128, b, 38, c, 19, 192)
    ref = np.zeros((npix, 192), np.float32)
    ref[:, :128] = a
    ref[:, 128:166] = b[:, :38]
    ref[:, 166:185] = c[:, :19]
    assert np.array_equal(got, ref)
    assert not got[:, 185:].any()


def _distinct_bf16(rng, n):
    """n distinct positive bf16 values in random order."""
    bits = (np.arange(0x3000, 0x3000 + n, dtype=np.uint32) << 16)
    return rng.permutation(bits.view(np.float32))


def _argmax_expect(maps, nch):
    n, h, w, _ = maps.shape
    exp = np.zeros((n, nch, 3), np.float32)
    for f in range(n):
        for ch in range(nch):
            m = maps[f, :, :, ch].reshape(-1)
            i = int(np.argmax(m))  # first occurrence in flat order
            exp[f, ch] = (i % w, i // w, m[i])
    return exp


HEATMAP_TIES = {
    "distinct": None,
    # thread 44 owns index 300, thread 45 owns 45: the wave shuffle must
    # keep the lower index, not the lower lane
    "peak-at-45-and-300": (45, 300),
    # thread 10 (wave 0) owns 266, thread 200 (wave 3) owns 200: the same
    # in the cross-wave stage
    "peak-at-200-and-266": (200, 266),
    "all-equal": "flat",
}


@pytest.mark.parametrize("tie", HEATMAP_TIES, ids=str)
def test_heatmap_argmax(tie):
    rng = np.random.RandomState(10)
    n, hw, cs, nch = 2, 46, 64, 19
    maps = np.zeros((n, hw * hw, cs), np.float32)
    for f in range(n):
        for ch in range(cs):
            maps[f, :, ch] = _distinct_bf16(rng, hw * hw)
    # the pad channels hold larger values that no channel may pick up
    maps[:, :, nch:] *= 4
    spec = HEATMAP_TIES[tie]
    if spec == "flat":
        maps[:, :, :nch] = 0.25
    elif spec is not None:
        peak = maps.max() * 2  # still exact in bf16
        for i in spec:
            maps[:, i, :nch] = peak
    maps = maps.reshape(n, hw, hw, cs)
    assert np.array_equal(R.bf16_round(maps), maps)
    got = _core.heatmap_argmax_test(maps, nch)
    exp = _argmax_expect(maps, nch)
    if spec not in (None, "flat"):
        assert (exp[..., 0] == spec[0] % hw).all()
        assert (exp[..., 1] == spec[0] // hw).all()
    bad = np.argwhere((got != exp).any(axis=2))
    assert bad.size == 0, (
        f"{len(bad)} maps differ, first (frame, ch) {bad[0]}: got "
        f"{got[tuple(bad[0])]} (flat index "
        f"{int(got[tuple(bad[0])][1] * hw + got[tuple(bad[0])][0])}) "
        f"expected {exp[tuple(bad[0])]}")


@pytest.mark.parametrize("geom", [(37, 53, 32, 8), (20, 24, 48, 3)], ids=str)
def test_preprocess(geom):
    ih, iw, ohw, oc = geom
    rng = np.random.RandomState(ih)
    frames = rng.randint(0, 256, (2, ih, iw, 3)).astype(np.uint8)
    mean, std = R.PRE_MEAN, R.PRE_STD
    got = _core.preprocess_frames_bf16_test(frames, ohw, oc, mean, std)
    assert got.shape == (2, ohw, ohw, oc)
    ref = R.preprocess_ref(frames, ohw, mean, std)
    tol = R.preprocess_tolerance(ref, ih, iw, std)
    worst = R.assert_within(got[..., :3], ref, tol, f"preprocess {geom}")
    print(f"worst err/tol preprocess {geom}: {worst:.3f}")
    assert not got[..., 3:].any()  # pad channels exactly zero
