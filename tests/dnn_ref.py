"""Shared reference code for the GEMM / conv / DNN-helper kernel tests
(test_gemm_plan.py on the CPU, test_dnn_kernels_gpu.py and its child
processes on the GPU): the shape table with the dispatch path each shape
must take, deterministic inputs, the float64 reference, the derived
tolerance and the mutation-sensitivity check. numpy only; torch is imported
where a torch reference is asked for.

Tolerance (elementwise, nothing tuned):

    mag = |scale| * (|A| @ |B|^T) + |bias| + |residual|
    E   = (K + 4) * 2^-23 * mag
    tol = 2^-8 * |ref| + (1 + 2^-8) * E

2^-8 is the unit roundoff of bf16 round-to-nearest (the one final store).
fp32 accumulation of K products in any order errs by at most
(K-1) * 2^-24 * sum|a||b| to first order; the factor 2 over that covers the
MFMA's internal summation, whose per-add rounding is unspecified, and the
+4 covers the epilogue's fp32 multiply and adds. ReLU is 1-Lipschitz, so
the bound survives the activation.
"""
import numpy as np

U_BF16 = 2.0 ** -8


def bf16_round(x):
    """float -> nearest bf16 (ties to even), returned as float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


# ---- the path table ----

AMPLE = 16 << 20                   # split-K scratch that never limits
PER_SPLIT_130x128 = 130 * 128 * 4  # one f32 partial of the (130,128,*) shape
CTR = 4096                         # tile-counter tail of the scratch


def plan(kernel, grid, K, splits=1, kps=None, tpw=1, swizzle=False):
    return dict(kernel=kernel, grid=grid, splits=splits,
                ksteps_per_split=K // 64 if kps is None else kps,
                tiles_per_wg=tpw, swizzle=swizzle, atomic=False, fused=False)


def _case(path, M, N, K, scratch, expect):
    return dict(id=f"{path}-{M}x{N}x{K}", path=path, M=M, N=N, K=K,
                scratch=scratch, plan=expect)


# (path, shape, scratch bytes, the plan that shape must get). The smallest
# shapes that still reach each branch of gemm_plan.
GEMM_CASES = [
    _case("tile64", 1, 64, 64, 0, plan("tile64", 1, 64)),
    _case("tile64", 63, 192, 128, 0, plan("tile64", 3, 128)),
    _case("tile64", 64, 128, 64, 0, plan("tile64", 2, 64)),
    _case("tile128", 65, 128, 128, 0, plan("tile128", 1, 128)),
    _case("tile128", 384, 256, 192, 0, plan("tile128", 6, 192)),
    _case("tile128-swizzled", 512, 256, 128, 0,
          plan("tile128", 8, 128, swizzle=True)),
    _case("tile128-swizzled", 1000, 512, 576, 0,
          plan("tile128", 32, 576, swizzle=True)),
    _case("smallk", 1024, 128, 64, 0, plan("smallk", 8, 64)),
    _case("smallk", 1025, 256, 64, 0, plan("smallk", 18, 64)),
    # 16 k-steps in 4 splits of 4
    _case("splitk", 1, 128, 1024, AMPLE,
          plan("splitk", 4, 1024, splits=4, kps=4)),
    # the FC shape: 32 k-steps in 6 splits of 6, 6, 6, 6, 6, 2
    _case("splitk", 4, 1024, 2048, AMPLE,
          plan("splitk", 48, 2048, splits=6, kps=6)),
    # 17 k-steps: 5, 5, 5, 2
    _case("splitk-uneven", 200, 256, 1088, AMPLE,
          plan("splitk", 16, 1088, splits=4, kps=5)),
    # 33 k-steps: 6 x 5 + 3
    _case("splitk-uneven", 130, 128, 2112, AMPLE,
          plan("splitk", 12, 2112, splits=6, kps=6)),
    # scratch holds exactly two partials: fit == 2 < want == 6 -> 17 + 16
    _case("splitk-scratch-limited", 130, 128, 2112,
          CTR + 2 * PER_SPLIT_130x128,
          plan("splitk", 4, 2112, splits=2, kps=17)),
    # scratch holds one partial: fit < 2 -> the tile kernel
    _case("splitk-fallback", 130, 128, 2112, CTR + PER_SPLIT_130x128,
          plan("tile128", 2, 2112)),
    # K < 1024: never split, however much scratch
    _case("nosplit", 130, 128, 960, AMPLE, plan("tile128", 2, 960)),
]

# Multi-tile small-K walk: only reachable with SCANNER_SMALLK_WGS=256 in a
# fresh process; N = 1024 is 8 N-tiles, so 256 / 8 = 32 strips at the most.
SMALLK_WALK_CASES = [
    # 34 M-tiles -> 17 strips of 2; the last tile is partial (5 rows)
    _case("smallk-walk", 4229, 1024, 64, 0,
          plan("smallk", 17 * 8, 64, tpw=2)),
    # 33 M-tiles -> 17 strips of 2; the last strip is a lone, partial tile
    _case("smallk-walk", 4101, 1024, 64, 0,
          plan("smallk", 17 * 8, 64, tpw=2)),
    # 32 M-tiles fit the 32 strips exactly: one tile per workgroup, grid 256
    _case("smallk-walk", 4096, 1024, 64, 0,
          plan("smallk", 32 * 8, 64, tpw=1)),
]

SPLITK_CASES = [c for c in GEMM_CASES if c["plan"]["kernel"] == "splitk"]


def _conv(name, r, s, stride, pad, c, n, h, w, N, scratch, expect_kernel,
          grid, splits=1, kps=None):
    oh = (h + 2 * pad - r) // stride + 1
    ow = (w + 2 * pad - s) // stride + 1
    kp = -(-r * s * c // 64) * 64
    return dict(id=name, r=r, s=s, stride=stride, pad=pad, c=c, n=n, h=h,
                w=w, N=N, oh=oh, ow=ow, M=n * oh * ow, kp=kp, scratch=scratch,
                plan=plan(expect_kernel, grid, kp, splits=splits, kps=kps))


# Both gemm_plan(is_conv=True) (implicit) and gemm_plan(is_conv=False)
# (im2col + gemm) give these plans for these shapes.
CONV_CASES = [
    # K 392 padded to 448: the last step is all zero lanes; c = 8
    _conv("7x7s2p3-c8", 7, 7, 2, 3, 8, 2, 20, 20, 64, 0, "tile64", 4),
    _conv("3x3s1p1-c64", 3, 3, 1, 1, 64, 1, 9, 11, 128, 0, "tile128", 1),
    _conv("3x3s2p1-c64", 3, 3, 2, 1, 64, 2, 15, 13, 64, 0, "tile64", 2),
    _conv("1x1s2p0-c64", 1, 1, 2, 0, 64, 2, 14, 14, 128, 0, "tile128", 1),
    # K 216 padded to 256; cells straddle the 64-wide step
    _conv("3x3s1p1-c24", 3, 3, 1, 1, 24, 1, 8, 8, 64, 0, "tile64", 1),
    # K 1152 with scratch: split-K conv, 18 k-steps as 5, 5, 5, 3
    _conv("3x3s1p1-c128-splitk", 3, 3, 1, 1, 128, 1, 7, 7, 128, AMPLE,
          "splitk", 4, splits=4, kps=5),
]

EPILOGUES = {
    "none": dict(scale=False, bias=False, residual=False, relu=False),
    "scale+bias": dict(scale=True, bias=True, residual=False, relu=False),
    "scale+bias+relu": dict(scale=True, bias=True, residual=False, relu=True),
    "residual": dict(scale=False, bias=False, residual=True, relu=False),
    "scale+bias+residual+relu": dict(scale=True, bias=True, residual=True,
                                     relu=True),
}
FULL_NO_RELU = dict(scale=True, bias=True, residual=True, relu=False)


def plan_of(_core, M, N, K, scratch=0, is_conv=False):
    return dict(_core.gemm_plan(M, N, K, scratch, is_conv))


# ---- inputs ----

def case_seed(case):
    return (case["M"] * 1000003 + case["N"] * 1009 + case.get("K", 0)) % 2**31


def epilogue_operands(rng, M, N):
    """Asymmetric per-column scale and bias of either sign, bf16 residual."""
    scale = (rng.uniform(0.5, 1.5, N) * rng.choice([-1.0, 1.0], N))
    bias = (rng.uniform(1.0, 3.0, N) * rng.choice([-1.0, 1.0], N))
    residual = bf16_round(rng.randn(M, N) * 2.0)
    return scale.astype(np.float32), bias.astype(np.float32), residual


def gemm_inputs(case):
    """N(0,1) operands rounded to bf16; B is asymmetric by construction."""
    rng = np.random.RandomState(case_seed(case))
    M, N, K = case["M"], case["N"], case["K"]
    A = bf16_round(rng.randn(M, K))
    B = bf16_round(rng.randn(N, K))
    scale, bias, residual = epilogue_operands(rng, M, N)
    return dict(A=A, B=B, scale=scale, bias=bias, residual=residual)


def exact_epilogue_operands(rng, M, N):
    scale = rng.choice([1.0, 2.0], N).astype(np.float32)
    bias = rng.randint(-32, 33, N).astype(np.float32)
    residual = rng.randint(-64, 65, (M, N)).astype(np.float32)
    return scale, bias, residual


def gemm_exact_inputs(case):
    """Integer data: A in {-1,0,1} with <= 64 non-zeros per row, B in
    {-1,1}, scale in {1,2}, |bias| <= 32, |residual| <= 64. Every partial
    sum in any order is an integer of magnitude <= 64, and every result an
    integer of magnitude <= 2*64 + 32 + 64 = 224 <= 256: exact in fp32 and
    in bf16, so the kernel must return the reference bit for bit."""
    rng = np.random.RandomState(case_seed(case) ^ 0x5EED)
    M, N, K = case["M"], case["N"], case["K"]
    A = np.zeros((M, K), np.float32)
    nz = min(K, 64)
    for i in range(M):
        cols = rng.choice(K, nz, replace=False)
        A[i, cols] = rng.choice([-1.0, 1.0], nz)
    B = rng.choice([-1.0, 1.0], (N, K)).astype(np.float32)
    scale, bias, residual = exact_epilogue_operands(rng, M, N)
    return dict(A=A, B=B, scale=scale, bias=bias, residual=residual)


def conv_inputs(case):
    rng = np.random.RandomState(case_seed(case) + case["c"])
    rsc = case["r"] * case["s"] * case["c"]
    x = bf16_round(rng.randn(case["n"], case["h"], case["w"], case["c"]))
    # weight columns past r*s*c are non-zero on purpose: the kernel must
    # zero the A side there, so they must not reach the output
    w = bf16_round(rng.randn(case["N"], case["kp"]))
    w[:, rsc:] = 3.0
    scale, bias, residual = epilogue_operands(rng, case["M"], case["N"])
    return dict(x=x, w=w, scale=scale, bias=bias, residual=residual)


def conv_exact_inputs(case):
    """x in {-1,0,1}; each filter has <= 64 non-zero taps in {-1,1}, so
    every partial sum is an integer of magnitude <= 64 (see
    gemm_exact_inputs for the rest of the bound)."""
    rng = np.random.RandomState(case_seed(case) + case["c"] + 77)
    rsc = case["r"] * case["s"] * case["c"]
    x = rng.choice([-1.0, 0.0, 1.0],
                   (case["n"], case["h"], case["w"], case["c"]))
    w = np.zeros((case["N"], case["kp"]), np.float32)
    nz = min(rsc, 64)
    for j in range(case["N"]):
        cols = rng.choice(rsc, nz, replace=False)
        w[j, cols] = rng.choice([-1.0, 1.0], nz)
    w[:, rsc:] = 3.0
    scale, bias, residual = exact_epilogue_operands(rng, case["M"], case["N"])
    return dict(x=x.astype(np.float32), w=w, scale=scale, bias=bias,
                residual=residual)


def pick(inp, epi):
    """The optional epilogue operands an epilogue uses, as kwargs."""
    return dict(scale=inp["scale"] if epi["scale"] else None,
                bias=inp["bias"] if epi["bias"] else None,
                residual=inp["residual"] if epi["residual"] else None,
                relu=epi["relu"])


# ---- reference and tolerance ----

def epilogue_ref(acc, mag, scale=None, bias=None, residual=None, relu=False):
    """float64 epilogue on a float64 accumulator and its magnitude sum."""
    ref = acc.copy()
    mag = mag.copy()
    if scale is not None:
        ref *= scale.astype(np.float64)
        mag *= np.abs(scale.astype(np.float64))
    if bias is not None:
        ref += bias.astype(np.float64)
        mag += np.abs(bias.astype(np.float64))
    if residual is not None:
        ref += residual.astype(np.float64)
        mag += np.abs(residual.astype(np.float64))
    if relu:
        ref = np.maximum(ref, 0.0)
    return ref, mag


def gemm_ref(A, B, **ep):
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    return epilogue_ref(A64 @ B64.T, np.abs(A64) @ np.abs(B64).T, **ep)


def tolerance(ref, mag, K):
    E = (K + 4) * 2.0 ** -23 * mag
    return U_BF16 * np.abs(ref) + (1 + U_BF16) * E


def err_over_tol(got, ref, tol):
    """Elementwise err/tol; inf where tol is zero and the error is not, or
    where the kernel left a NaN."""
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(ratio), np.inf, ratio)


def assert_within(got, ref, tol, what):
    """Every element within tol; returns the worst err/tol."""
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    ratio = err_over_tol(got, ref, tol)
    worst = float(ratio.max())
    bad = int((ratio > 1.0).sum())
    if bad:
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError(
            f"{what}: {bad}/{ratio.size} elements outside tol, worst "
            f"err/tol {worst:.3g} at {i}: got {got[i]!r} ref {ref[i]!r} "
            f"tol {tol[i]!r}")
    return worst


def assert_exact_reference(ref):
    """The property the exact cases rest on, asserted on the reference."""
    assert np.all(ref == np.round(ref)) and np.abs(ref).max() <= 256
    assert np.array_equal(bf16_round(ref), ref.astype(np.float32))


# ---- mutation sensitivity of the comparator ----

def mutation_rates(A, B, scale, bias, residual, K, relu=False):
    """Seed four bugs into the *reference* (no kernel involved) and return,
    per mutation, the fraction of the elements it changes that the
    comparator flags. A/B are the GEMM operands ([M][K], [N][K])."""
    ep = dict(scale=scale, bias=bias, residual=residual, relu=relu)
    ref, mag = gemm_ref(A, B, **ep)
    tol = tolerance(ref, mag, K)
    mutated = {}
    k0 = (K // 8 // 2) * 8
    A_m = A.copy()
    A_m[:, k0:k0 + 8] = 0
    mutated["zero-k-chunk"] = gemm_ref(A_m, B, **ep)[0]
    mutated["drop-residual"] = gemm_ref(A, B, **dict(ep, residual=None))[0]
    mutated["shift-columns"] = np.roll(ref, 1, axis=1)
    # the first column from N/3 on whose bias the activation lets through
    # (with one row and ReLU, a column can be zero with and without it)
    for j in range(B.shape[0] // 3, B.shape[0]):
        col = gemm_ref(A, B[j:j + 1], scale=scale[j:j + 1],
                       residual=residual[:, j:j + 1], relu=relu)[0]
        if np.any(col[:, 0] != ref[:, j]):
            break
    mutated["zero-one-bias"] = ref.copy()
    mutated["zero-one-bias"][:, j] = col[:, 0]
    rates = {}
    for name, m in mutated.items():
        affected = m != ref
        assert affected.any(), f"mutation {name} changed nothing"
        flagged = err_over_tol(m, ref, tol) > 1.0
        rates[name] = float((flagged & affected).sum() / affected.sum())
    return rates


def assert_mutations_flagged(A, B, inp, K, what):
    for relu in (False, True):
        rates = mutation_rates(A, B, inp["scale"], inp["bias"],
                               inp["residual"], K, relu=relu)
        for name, rate in rates.items():
            assert rate >= 0.10, (
                f"{what}: comparator flags only {rate:.1%} of the elements "
                f"that mutation {name} (relu={relu}) changes")
    return rates


# ---- preprocess (resize + normalise) ----

PRE_MEAN = np.array([0.485, 0.456, 0.406], np.float32)
PRE_STD = np.array([0.229, 0.224, 0.225], np.float32)


def preprocess_ref(frames, ohw, mean=PRE_MEAN, std=PRE_STD):
    """float64 bilinear resize (half-pixel centres) of u8 [n][h][w][3]
    frames to ohw x ohw, then (y / 255 - mean) / std."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(frames.astype(np.float64)).permute(0, 3, 1, 2)
    y = F.interpolate(t, size=(ohw, ohw), mode="bilinear",
                      align_corners=False).permute(0, 2, 3, 1).numpy()
    return (y / 255.0 - mean.astype(np.float64)) / std.astype(np.float64)


def preprocess_tolerance(ref, ih, iw, std=PRE_STD):
    return (U_BF16 * np.abs(ref) +
            (2.0 ** -22 * max(ih, iw) + 2.0 ** -20) / float(std.min()))


# ---- convolution ----

def im2col_ref(x, r, s, stride, pad, kp):
    """numpy im2col of an NHWC tensor: rows [n*oh*ow][kp], k = (dr*s+ds)*c
    + cj, zero past r*s*c and outside the image."""
    n, h, w, c = x.shape
    oh = (h + 2 * pad - r) // stride + 1
    ow = (w + 2 * pad - s) // stride + 1
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, c), x.dtype)
    xp[:, pad:pad + h, pad:pad + w] = x
    out = np.zeros((n, oh, ow, kp), x.dtype)
    for dr in range(r):
        for ds in range(s):
            k = (dr * s + ds) * c
            out[..., k:k + c] = xp[:, dr:dr + (oh - 1) * stride + 1:stride,
                                   ds:ds + (ow - 1) * stride + 1:stride]
    return out.reshape(n * oh * ow, kp)


def conv_ref(case, inp, **ep):
    """float64 torch conv2d reference (and magnitude sum) as [M][N]."""
    import torch
    import torch.nn.functional as F
    r, s, c = case["r"], case["s"], case["c"]
    x = torch.from_numpy(inp["x"].astype(np.float64)).permute(0, 3, 1, 2)
    w = inp["w"][:, :r * s * c].astype(np.float64)
    w = torch.from_numpy(w.reshape(case["N"], r, s, c)).permute(0, 3, 1, 2)

    def run(xx, ww):
        y = F.conv2d(xx, ww, stride=case["stride"], padding=case["pad"])
        return y.permute(0, 2, 3, 1).reshape(case["M"], case["N"]).numpy()

    return epilogue_ref(run(x, w), run(x.abs(), w.abs()), **ep)


# ---- pools ----

def maxpool_ref(x, pad_value=None):
    """3 x 3 stride-2 pad-1 max of an NHWC tensor as float64; the border is
    padded with -inf, or with pad_value where one is given."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    if pad_value is None:
        y = F.max_pool2d(t, kernel_size=3, stride=2, padding=1)
    else:
        y = F.max_pool2d(F.pad(t, (1, 1, 1, 1), value=float(pad_value)),
                         kernel_size=3, stride=2)
    return y.permute(0, 2, 3, 1).numpy()


def avgpool_ref(x, divisor=None):
    """(ref, tol) of the global average of an NHWC bf16-exact tensor, as
    [n][c] float64: hw fp32 adds and one multiply on the magnitude sum, then
    the bf16 store."""
    n, h, w, c = x.shape
    hw = h * w
    x64 = x.astype(np.float64).reshape(n, hw, c)
    ref = x64.mean(axis=1)
    if divisor is not None:  # a seeded bug of the comparator test
        ref = ref * hw / divisor
    tol = (U_BF16 * np.abs(ref) + (1 + U_BF16) * (hw + 2) * 2.0 ** -24 *
           np.abs(x64).mean(axis=1) * hw)
    return ref, tol
