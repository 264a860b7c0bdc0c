"""GPU tests of the GEMM hot-path code that the stock path table in
dnn_ref.py does not reach: the implicit-conv staging routine shared by the
tile and split-K kernels (its c % 64 == 0 fast path with more than one
M-tile, a non-power-of-two c, a strided 1x1 and a strided 3x3 on the 128
tile, and a split-K conv whose incremental state starts mid-K), and the
epilogues with only some of scale / bias / residual present.

Every test asserts its plan first, then checks random inputs against
dnn_ref.tolerance and exact integer inputs for bit equality. References are
computed once per case and shared; nothing here is tuned from kernel
output.
"""
import functools

import numpy as np
import pytest

import dnn_ref as R
from scanner_amd import _core

gpu = pytest.mark.gpu

# The smallest shapes at which the staging code can still go wrong.
CONV_CASES = [
    # two M-tiles (m0 != 0), partial last tile, an image boundary inside a
    # tile, the (r, s) cell changes every 2nd K step
    R._conv("3x3s1p1-c128-2tiles", 3, 3, 1, 1, 128, 2, 9, 9, 128, 0,
            "tile128", 2),
    # the same as split-K: several tiles, 18 k-steps as 5, 5, 5, 3 — the
    # splits start their incremental state at k = 320, 640, 960
    R._conv("3x3s1p1-c128-2tiles-splitk", 3, 3, 1, 1, 128, 2, 9, 9, 128,
            R.AMPLE, "splitk", 8, splits=4, kps=5),
    # c a multiple of 64 but no power of two: the cell changes every 3rd step
    R._conv("3x3s1p1-c192", 3, 3, 1, 1, 192, 1, 5, 6, 64, 0, "tile64", 1),
    # strided 1x1: two K steps inside the one cell
    R._conv("1x1s2p0-c128", 1, 1, 2, 0, 128, 2, 13, 11, 128, 0, "tile128", 1),
    # stride 2 with odd extents on the 128 tile
    R._conv("3x3s2p1-c64-odd", 3, 3, 2, 1, 64, 3, 11, 9, 128, 0, "tile128",
            1),
]

EXPECT_SHAPE = {
    "3x3s1p1-c128-2tiles": (162, 1152),
    "3x3s1p1-c128-2tiles-splitk": (162, 1152),
    "3x3s1p1-c192": (30, 1728),
    "1x1s2p0-c128": (84, 128),
    "3x3s2p1-c64-odd": (90, 576),
}

# Epilogue operand combinations the stock EPILOGUES table does not contain.
NULL_COMBOS = {
    "scale-only": dict(scale=True, bias=False, residual=False, relu=False),
    "bias+relu": dict(scale=False, bias=True, residual=False, relu=True),
    "bias+residual": dict(scale=False, bias=True, residual=True, relu=False),
}

# one shape per kernel, taken from the pinned path table
NULL_COMBO_SHAPES = ["tile64-63x192x128", "tile128-384x256x192",
                     "smallk-1025x256x64", "splitk-uneven-200x256x1088"]


def _gemm_case(case_id):
    (case,) = [c for c in R.GEMM_CASES if c["id"] == case_id]
    return case


def _assert_conv_plan(case):
    assert (case["M"], case["kp"]) == EXPECT_SHAPE[case["id"]]
    for is_conv in (True, False):
        assert R.plan_of(_core, case["M"], case["N"], case["kp"],
                         case["scratch"], is_conv) == case["plan"], is_conv


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c["id"])
def test_hotpath_conv_plans(case):
    """No GPU needed: implicit and im2col dispatch agree on these plans."""
    _assert_conv_plan(case)


@pytest.mark.parametrize("case_id", NULL_COMBO_SHAPES)
def test_hotpath_gemm_plans(case_id):
    case = _gemm_case(case_id)
    assert R.plan_of(_core, case["M"], case["N"], case["K"],
                     case["scratch"]) == case["plan"]


# ---- references: once per case, shared, never modified ----

@functools.lru_cache(maxsize=None)
def _conv_data(case_id, exact):
    (case,) = [c for c in CONV_CASES if c["id"] == case_id]
    inp = (R.conv_exact_inputs if exact else R.conv_inputs)(case)
    refs = {name: R.conv_ref(case, inp, **R.pick(inp, epi))
            for name, epi in R.EPILOGUES.items()}
    for ref, mag in refs.values():
        ref.setflags(write=False)
        mag.setflags(write=False)
    return inp, refs


def _run_conv(case, inp, epi, implicit):
    return _core.conv_bf16_test(
        inp["x"], inp["w"], case["r"], case["s"], case["stride"], case["pad"],
        splitk_scratch_bytes=case["scratch"], implicit=implicit,
        **R.pick(inp, epi))


@gpu
@pytest.mark.parametrize("implicit", [True, False],
                         ids=["implicit", "im2col"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c["id"])
def test_hotpath_conv(case, implicit):
    _assert_conv_plan(case)
    rsc = case["r"] * case["s"] * case["c"]
    splitk = case["plan"]["kernel"] == "splitk"

    inp, refs = _conv_data(case["id"], False)
    cols_ref = R.im2col_ref(inp["x"], case["r"], case["s"], case["stride"],
                            case["pad"], case["kp"])
    R.assert_mutations_flagged(cols_ref, inp["w"], inp, rsc, case["id"])
    worst = 0.0
    for name, epi in R.EPILOGUES.items():
        what = f"{case['id']} {name}"
        ref, mag = refs[name]
        got, cols = _run_conv(case, inp, epi, implicit)
        assert np.array_equal(cols, cols_ref), f"{what}: im2col differs"
        worst = max(worst, R.assert_within(
            got, ref, R.tolerance(ref, mag, rsc), what))
        if splitk:
            again, _ = _run_conv(case, inp, epi, implicit)
            assert np.array_equal(got, again), f"{what}: not repeatable"
    print(f"worst err/tol conv {case['id']} "
          f"{'implicit' if implicit else 'im2col'}: {worst:.3f}")

    inp, refs = _conv_data(case["id"], True)
    for name, epi in R.EPILOGUES.items():
        ref, _ = refs[name]
        R.assert_exact_reference(ref)
        got, _ = _run_conv(case, inp, epi, implicit)
        bad = np.argwhere(got != ref.astype(np.float32))
        assert bad.size == 0, (
            f"{case['id']} {name} exact: {len(bad)} elements differ, first "
            f"at {bad[0]}: {got[tuple(bad[0])]} vs {ref[tuple(bad[0])]}")


@gpu
@pytest.mark.parametrize("case_id", NULL_COMBO_SHAPES)
def test_hotpath_epilogue_null_combinations(case_id):
    case = _gemm_case(case_id)
    assert R.plan_of(_core, case["M"], case["N"], case["K"],
                     case["scratch"]) == case["plan"]
    inp = R.gemm_exact_inputs(case)
    for name, epi in NULL_COMBOS.items():
        ref, _ = R.gemm_ref(inp["A"], inp["B"], **R.pick(inp, epi))
        R.assert_exact_reference(ref)
        got = _core.gemm_bf16_test(inp["A"], inp["B"],
                                   splitk_scratch_bytes=case["scratch"],
                                   **R.pick(inp, epi))
        bad = np.argwhere(got != ref.astype(np.float32))
        assert bad.size == 0, (
            f"{case_id} {name}: {len(bad)} elements differ, first at "
            f"{bad[0]}: {got[tuple(bad[0])]} vs {ref[tuple(bad[0])]}")
        if case["plan"]["kernel"] == "splitk":
            again = _core.gemm_bf16_test(
                inp["A"], inp["B"], splitk_scratch_bytes=case["scratch"],
                **R.pick(inp, epi))
            assert np.array_equal(got, again), f"{case_id} {name}"
