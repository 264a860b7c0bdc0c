"""CPU tests for the GEMM/conv dispatch plan and for the comparator the GPU
kernel tests rely on.

The path table (dnn_ref.GEMM_CASES / CONV_CASES) names, for every shape the
GPU tests run, the kernel, split count, tiles per workgroup and grid that
shape must get. If a heuristic in gemm_plan changes, this file fails first
and test_dnn_kernels_gpu.py does not silently lose a path.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dnn_ref as R
from scanner_amd import _core

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("case", R.GEMM_CASES, ids=lambda c: c["id"])
def test_gemm_path_table(case):
    got = R.plan_of(_core, case["M"], case["N"], case["K"], case["scratch"])
    assert got == case["plan"]


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c["id"])
def test_conv_path_table(case):
    # the implicit path and the im2col + gemm path must both land on it
    for is_conv in (True, False):
        got = R.plan_of(_core, case["M"], case["N"], case["kp"],
                        case["scratch"], is_conv)
        assert got == case["plan"], f"is_conv={is_conv}"


def test_path_table_covers_every_kernel_and_swizzle_state():
    kernels = {c["plan"]["kernel"] for c in R.GEMM_CASES}
    assert kernels == {"smallk", "splitk", "tile128", "tile64"}
    multi_n = [c for c in R.GEMM_CASES
               if c["plan"]["kernel"] == "tile128" and c["N"] > 128]
    assert {c["plan"]["swizzle"] for c in multi_n} == {True, False}
    # an uneven last split: ksteps not a multiple of ksteps_per_split
    assert any((c["K"] // 64) % c["plan"]["ksteps_per_split"]
               for c in R.SPLITK_CASES)


def test_plan_geometry_is_consistent():
    """Properties every plan must have, over a sweep of shapes."""
    for M in (1, 64, 65, 128, 130, 1000, 1024, 5000, 50176):
        for N in (64, 128, 192, 256, 1024):
            for K in (64, 128, 960, 1024, 2112, 4608):
                for scratch in (0, 4096, 1 << 20, 64 << 20):
                    p = R.plan_of(_core, M, N, K, scratch)
                    ksteps = K // 64
                    if p["kernel"] == "splitk":
                        kps, sp = p["ksteps_per_split"], p["splits"]
                        assert 2 <= sp <= 6 and K >= 1024 and N % 128 == 0
                        # every split has work and together they cover K
                        assert (sp - 1) * kps < ksteps <= sp * kps
                        assert sp * M * N * 4 + 4096 <= scratch
                        tiles = -(-M // 128) * (N // 128)
                        assert p["grid"] == tiles * sp and tiles < 256
                    elif p["kernel"] == "smallk":
                        assert K == 64 and N % 128 == 0 and M >= 1024
                        strips = p["grid"] // (N // 128)
                        assert strips * p["tiles_per_wg"] >= -(-M // 128)
                        assert (strips - 1) * p["tiles_per_wg"] < -(-M // 128)
                    else:
                        bt = 128 if p["kernel"] == "tile128" else 64
                        assert N % bt == 0
                        assert p["grid"] == -(-M // bt) * (N // bt)
                        assert p["swizzle"] == (p["grid"] % 8 == 0)
                        assert p["splits"] == 1
                        assert p["ksteps_per_split"] == ksteps


def test_conv_plan_ignores_the_gemm_only_branches():
    # no small-K kernel and no M > 64 condition on the implicit path
    assert R.plan_of(_core, 4096, 128, 64, 0, True)["kernel"] == "tile128"
    assert R.plan_of(_core, 4096, 128, 64, 0, False)["kernel"] == "smallk"
    assert R.plan_of(_core, 49, 128, 576, 0, True)["kernel"] == "tile128"
    assert R.plan_of(_core, 49, 128, 576, 0, False)["kernel"] == "tile64"


def test_plan_rejects_unpadded_shapes():
    with pytest.raises(Exception):
        _core.gemm_plan(8, 64, 100)
    with pytest.raises(Exception):
        _core.gemm_plan(8, 100, 64)


def _plan_in_child(env, *shape):
    """The env knobs are read once per process: ask a fresh interpreter."""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); "
            "from scanner_amd import _core; "
            "print(dict(_core.gemm_plan(*map(int, sys.argv[2:]))))")
    out = subprocess.run(
        [sys.executable, "-c", code, os.path.dirname(HERE)] +
        [str(v) for v in shape], env=dict(os.environ, **env),
        capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return eval(out.stdout)


def test_env_knobs_reach_the_plan():
    for case in R.SMALLK_WALK_CASES:
        got = _plan_in_child({"SCANNER_SMALLK_WGS": "256"}, case["M"],
                             case["N"], case["K"])
        assert got == case["plan"]
    c = R.SPLITK_CASES[-1]
    shape = (c["M"], c["N"], c["K"], c["scratch"])
    got = _plan_in_child({"SCANNER_SPLITK_FUSED": "1"}, *shape)
    assert got == dict(c["plan"], fused=True)
    got = _plan_in_child({"SCANNER_SPLITK_ATOMIC": "1",
                          "SCANNER_SPLITK_FUSED": "1"}, *shape)
    assert got == dict(c["plan"], atomic=True)  # atomic wins over fused
    got = _plan_in_child({"SCANNER_SPLITK_OFF": "1"}, *shape)
    assert got["kernel"] == "tile128" and got["splits"] == 1


# ---- the comparator, against mutated references (no kernel involved) ----

COMPARATOR_SHAPES = [(65, 128, 128), (200, 256, 1088), (130, 128, 2112),
                     (4, 1024, 2048)]


def _case_for(shape):
    (case,) = [c for c in R.GEMM_CASES
               if (c["M"], c["N"], c["K"]) == shape and c["scratch"] in
               (0, R.AMPLE)]
    return case


def test_comparator_shapes_are_in_the_table():
    for shape in COMPARATOR_SHAPES:
        _case_for(shape)


@pytest.mark.parametrize("case", R.GEMM_CASES + R.SMALLK_WALK_CASES,
                         ids=lambda c: f"{c['id']}-{c['scratch']}")
def test_comparator_flags_mutated_references(case):
    """Zero one 8-wide K chunk of A, drop the residual, shift the columns
    by one, zero one column's bias: each must be flagged on at least 10 %
    of the elements it changes, with and without ReLU, on the inputs of
    every GPU case (COMPARATOR_SHAPES among them)."""
    inp = R.gemm_inputs(case)
    rates = R.assert_mutations_flagged(inp["A"], inp["B"], inp, case["K"],
                                       case["id"])
    print(case["id"], {k: round(v, 3) for k, v in rates.items()})


def _fp32_gemm_in_splits(A, B, splits):
    """Emulate fp32 accumulation: K split into `splits` runs, each summed
    one product at a time in float32, the partials then summed in order."""
    K = A.shape[1]
    kps = -(-(K // 64) // splits) * 64
    total = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for k0 in range(0, K, kps):
        part = np.zeros_like(total)
        for k in range(k0, min(k0 + kps, K)):
            part += A[:, k, None] * B[None, :, k]
        total += part
    return total


@pytest.mark.parametrize("shape", COMPARATOR_SHAPES, ids=str)
def test_tolerance_admits_fp32_accumulation(shape):
    """The bound must not be so tight that a correct fp32 kernel fails it:
    a float32 emulation in 1, 4 and 6 splits, with the full fp32 epilogue
    and one bf16 rounding, stays inside tol."""
    case = _case_for(shape)
    inp = R.gemm_inputs(case)
    ep = R.pick(inp, R.FULL_NO_RELU)
    ref, mag = R.gemm_ref(inp["A"], inp["B"], **ep)
    tol = R.tolerance(ref, mag, case["K"])
    for splits in (1, 4, 6):
        acc = _fp32_gemm_in_splits(inp["A"], inp["B"], splits)
        out = R.bf16_round(acc * inp["scale"] + inp["bias"] +
                           inp["residual"])
        worst = R.assert_within(out, ref, tol, f"{case['id']} x{splits}")
        print(case["id"], "splits", splits, "worst err/tol", round(worst, 3))


def test_exact_inputs_are_exact():
    for case in R.GEMM_CASES:
        inp = R.gemm_exact_inputs(case)
        assert (inp["A"] != 0).sum(axis=1).max() <= 128
        ref, _ = R.gemm_ref(inp["A"], inp["B"], **R.pick(inp, R.FULL_NO_RELU))
        R.assert_exact_reference(ref)
        assert np.abs(ref).max() > 32  # not a trivially small problem


def test_im2col_reference_matches_conv2d():
    """The numpy im2col the GPU tests compare against bit for bit is itself
    checked against torch conv2d, and the pad columns of the weights must
    not reach it."""
    for case in R.CONV_CASES:
        inp = R.conv_inputs(case)
        cols = R.im2col_ref(inp["x"], case["r"], case["s"], case["stride"],
                            case["pad"], case["kp"])
        assert cols.shape == (case["M"], case["kp"])
        rsc = case["r"] * case["s"] * case["c"]
        assert not cols[:, rsc:].any() and inp["w"][:, rsc:].all()
        ref, mag = R.conv_ref(case, inp)
        via_cols, mag_cols = R.gemm_ref(cols, inp["w"])
        np.testing.assert_allclose(via_cols, ref, rtol=0, atol=1e-9)
        np.testing.assert_allclose(mag_cols, mag, rtol=0, atol=1e-9)
        # the comparator must also see seeded bugs on the conv inputs
        R.assert_mutations_flagged(cols, inp["w"], inp, rsc, case["id"])
