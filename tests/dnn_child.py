"""Child process of test_dnn_kernels_gpu.py for the GEMM variants chosen by
environment variables, which the library reads once per process:

    python dnn_child.py smallk-walk            (SCANNER_SMALLK_WGS=256)
    python dnn_child.py fused  parent.npz      (SCANNER_SPLITK_FUSED=1)
    python dnn_child.py atomic parent.npz      (SCANNER_SPLITK_ATOMIC=1)

parent.npz holds what the parent computed with the default path: the
outputs `gemm/<case>/<epilogue>` and, for the split-K conv, the inputs'
reference, tolerance and output. Exits non-zero at the first failed check.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dnn_ref as R  # noqa: E402
from scanner_amd import _core  # noqa: E402


def smallk_walk():
    assert os.environ.get("SCANNER_SMALLK_WGS") == "256"
    for case in R.SMALLK_WALK_CASES:
        M, N, K = case["M"], case["N"], case["K"]
        assert R.plan_of(_core, M, N, K) == case["plan"], case["id"]
        inp = R.gemm_inputs(case)
        worst = 0.0
        for name, epi in R.EPILOGUES.items():
            ep = R.pick(inp, epi)
            ref, mag = R.gemm_ref(inp["A"], inp["B"], **ep)
            got = _core.gemm_bf16_test(inp["A"], inp["B"], **ep)
            worst = max(worst, R.assert_within(
                got, ref, R.tolerance(ref, mag, K), f"{case['id']} {name}"))
        print(f"worst err/tol {case['id']} tiles_per_wg="
              f"{case['plan']['tiles_per_wg']}: {worst:.3f}")
        # exact data: bit-equal whatever the tile walk does
        inp = R.gemm_exact_inputs(case)
        ep = R.pick(inp, R.FULL_NO_RELU)
        ref, _ = R.gemm_ref(inp["A"], inp["B"], **ep)
        R.assert_exact_reference(ref)
        got = _core.gemm_bf16_test(inp["A"], inp["B"], **ep)
        assert np.array_equal(got, ref.astype(np.float32)), case["id"]


def splitk_variant(flag, npz_path):
    parent = np.load(npz_path)
    fused = flag == "fused"
    worst = 0.0
    for case in R.SPLITK_CASES:
        M, N, K = case["M"], case["N"], case["K"]
        want = dict(case["plan"], fused=fused, atomic=not fused)
        assert R.plan_of(_core, M, N, K, case["scratch"]) == want, case["id"]
        inp = R.gemm_inputs(case)
        for name, epi in R.EPILOGUES.items():
            what = f"{flag} {case['id']} {name}"
            ep = R.pick(inp, epi)
            ref, mag = R.gemm_ref(inp["A"], inp["B"], **ep)
            tol = R.tolerance(ref, mag, K)
            got = _core.gemm_bf16_test(
                inp["A"], inp["B"], splitk_scratch_bytes=case["scratch"],
                repeat=3, **ep)
            for rep in range(3):
                worst = max(worst, R.assert_within(got[rep], ref, tol, what))
            if fused:
                # the counters restore themselves: later launches on the
                # same scratch reduce the same way
                assert np.array_equal(got[0], got[1]), what
                assert np.array_equal(got[0], got[2]), what
                key = f"gemm/{case['id']}/{name}"
                assert np.array_equal(got[0], parent[key]), \
                    f"{what}: fused differs from the default reduce"
    print(f"worst err/tol splitk-{flag} gemm: {worst:.3f}")

    (case,) = [c for c in R.CONV_CASES if c["plan"]["kernel"] == "splitk"]
    want = dict(case["plan"], fused=fused, atomic=not fused)
    assert R.plan_of(_core, case["M"], case["N"], case["kp"],
                     case["scratch"], True) == want
    inp = R.conv_inputs(case)
    worst = 0.0
    for name, epi in R.EPILOGUES.items():
        what = f"{flag} conv {case['id']} {name}"
        got, _ = _core.conv_bf16_test(
            inp["x"], inp["w"], case["r"], case["s"], case["stride"],
            case["pad"], splitk_scratch_bytes=case["scratch"], implicit=True,
            repeat=3, **R.pick(inp, epi))
        ref, tol = parent[f"conv/ref/{name}"], parent[f"conv/tol/{name}"]
        for rep in range(3):
            worst = max(worst, R.assert_within(got[rep], ref, tol, what))
        if fused:
            assert np.array_equal(got[0], got[1]), what
            assert np.array_equal(got[0], got[2]), what
            assert np.array_equal(got[0], parent[f"conv/out/{name}"]), \
                f"{what}: fused differs from the default reduce"
    print(f"worst err/tol splitk-{flag} conv: {worst:.3f}")


if __name__ == "__main__":
    assert _core.have_gpu()
    if sys.argv[1] == "smallk-walk":
        smallk_walk()
    else:
        assert os.environ.get(
            "SCANNER_SPLITK_" + sys.argv[1].upper()) == "1"
        splitk_variant(sys.argv[1], sys.argv[2])
    print("child OK")
