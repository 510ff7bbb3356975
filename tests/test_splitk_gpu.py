"""Split-K of the GEMM / implicit-GEMM convolution kernels (kernels/gemm.hip) at forced factors and slice edges.

Every kernel family - the symmetric gemm_kernel, the loader kernel gemm_ldr_kernel, the producer / consumer gemm_ws_kernel - carries its own
copy of the slice arithmetic (per = ceil(nk_all / split), kt_lo / kt_hi, the mid-K first-tile decode, the one all-zero step of an empty
slice) and splitk_epilogue re-implements bias, c0, residual and activation.  The planner only ever picks a handful of (tile, factor) pairs,
so these tests force the factor (Engine.tune_force(cfg, split)) on every family:

1. on integer data, where fp32 accumulation is exact in any order, the sliced result equals the unsliced one and the integer reference
   bit for bit, run after run;
2. on fp16-rounded Gaussian data with the full epilogue, against fp64 at TOL and against the unsliced output at one fp16 spacing;
3. where split-K must step aside (GEGLU, the statistics epilogue) it does;
4. every branch of gemm_plan that returns a factor > 1 is reached by a small shape and computes the right thing."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import TOL, rnd
from util import assert_close, conv_f64, h16, where_differ as _where

pytestmark = pytest.mark.gpu

SPLITS = (2, 3, 5, 8, 24)       # the planner's range (2 .. 24) and its uneven cases: see _exact_problems


# ---------------------------------------------------------------------------------------------------
# 1. Exact-integer screen.  A, W, x, w in {-1, 0, 1}, bias in [-2, 2], residual in [-8, 8], c0 = c1 = 1, no activation: every product and every
# partial sum is an integer below 2^24, so the fp32 accumulation is exact whatever the order, and |result| <= K + 2 + 8 < 2048 is an exact fp16
# integer.  A K tile dropped or doubled at a slice boundary, a K-tail mask on the wrong slice, a stale partial of an empty slice or an epilogue term
# applied per slice changes the sum by a non-zero integer.  Shapes: those of test_tile_configs_bitwise_identical_small_ragged (every addressing path).
#   dense 2049 x 640, K = 1344: nk_all = 21 K tiles - split 5 leaves a last slice of one tile, split 8 an empty slice 7 (per = 3), split 24 three empty
#     slices; buffer-addressed form of the loader and producer / consumer kernels.  K = 1352: nk_all = 22 with an 8-column K tail - split 8 makes the
#     ragged tile a slice of its own; flat-address fall-back of 35 / 39 / 54 / 59 / 63.  85 tiles of 128 x 128 for a persistent grid of
#     max(8, 256 / split) workgroups: each walks several tiles, each starting mid-K.
#   dense 77 x 128: one tile, more workgroups than tiles.
#   two-source 3x3 conv (K = 1728, nk_all = 27), temporal conv (K = 384, nk_all = 6: split 5 -> slices 3 and 4 empty, 8 and 24 mostly empty),
#   stride-2 conv in both padding variants, and the conv on the nearest-2x source (nk_all = 18): the only single-tap form on flat addresses, where
#   an empty slice's tap decode ran past the last channel chunk and read through the absent second source until it was masked (gemm_kernel: a_mask).
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_problems():
    rng = np.random.default_rng(20240)

    def tri(*shape):
        return rng.integers(-1, 2, shape).astype(np.float32)

    def ints(lim, *shape):
        return rng.integers(-lim, lim + 1, shape).astype(np.float32)

    probs = []
    for (M, K, N) in [(2049, 1344, 640), (2049, 1352, 640), (77, 1344, 128)]:
        A, W, b, R = tri(M, K), tri(N, K), ints(2, N), ints(8, M, N)
        ref = A.astype(np.float64) @ W.astype(np.float64).T + b + R
        probs.append((f"dense {M}x{N}x{K}", lambda e, A=A, W=W, b=b, R=R: e.op_linear(A, W, b, R1=R), ref))
    x, x1 = tri(5, 20, 28, 128), tri(5, 20, 28, 64)
    w, wt, bc = tri(192, 192, 1, 3, 3), tri(192, 128, 3, 1, 1), ints(2, 192)
    w128 = np.ascontiguousarray(w[:, :128])
    probs += [
        ("two-source conv3x3", lambda e: e.op_conv(x, w, bc, x1=x1), conv_f64(x, w, bc, x1=x1)),
        ("temporal conv", lambda e: e.op_conv(x, wt, bc, kt=3, k=1, pad_t=0, pad_l=0), conv_f64(x, wt, bc, kt=3, k=1, pad_t=0, pad_l=0)),
        ("stride-2 conv pad 1", lambda e: e.op_conv(x, w128, bc, stride=2), conv_f64(x, w128, bc, stride=2)),
        ("stride-2 conv pad (0,1,0,1)", lambda e: e.op_conv(x, w128, bc, stride=2, pad_t=0, pad_l=0), conv_f64(x, w128, bc, stride=2, pad_t=0, pad_l=0)),
        ("conv3x3 on the nearest-2x source", lambda e: e.op_conv(x, w128, bc, ups=2), conv_f64(x, w128, bc, ups=2)),
    ]
    out = []
    for name, run, ref in probs:
        ri = np.rint(ref).astype(np.int64)
        assert np.array_equal(ri, ref)                    # the fp64 evaluation is itself exact: an integer matmul / conv
        out.append((name, run, ri))
    return tuple(out)


# symmetric kernel: 0, 3, 12, 14, 19, 61; loader kernel: 35, 39; producer / consumer kernel: 54, 59, 63; -1: the planner's tile with a forced factor (the
# halo-staged and streaming kernels only take split == 1 launches: launch_gemm)
@pytest.mark.parametrize("cfg", [-1, 0, 3, 12, 14, 19, 35, 39, 54, 59, 61, 63])
def test_splitk_exact_integer_screen(engine, cfg):
    try:
        for name, run, ref in _exact_problems():
            assert np.abs(ref).max() < 2048, f"{name}: the reference leaves the exact fp16 integers"
            engine.tune_force(cfg, 1)
            base = run(engine)
            assert np.array_equal(base, ref), f"cfg {cfg} {name} unsliced vs integer reference: {_where(base, ref)}"
            for sp in SPLITS:
                engine.tune_force(cfg, sp)
                for rep in range(2):
                    got = run(engine)
                    assert np.array_equal(got, ref), f"cfg {cfg} split {sp} {name} run {rep} vs integer reference: {_where(got, ref)}"
                    assert np.array_equal(got, base), f"cfg {cfg} split {sp} {name} run {rep} vs split 1: {_where(got, base)}"
    finally:
        engine.tune_force(-1, -1)


# ---------------------------------------------------------------------------------------------------
# 2. Rounded inputs and the full epilogue.  The exact screen cannot see a mis-scaled epilogue (c0 = c1 = 1) and says nothing about real-valued data.
# Against fp64 at TOL; against the unsliced output of the same tile at 2^-10 max|ref|: the two differ only in the order of the fp32 summation (relative
# 1e-6 or so) before ONE rounding to fp16, so they are the same fp16 number or neighbours, and the spacing of fp16 at x is at most 2^-10 |x|.
# ---------------------------------------------------------------------------------------------------
def _act64(y, act):
    y = torch.from_numpy(y)
    return (F.silu(y) if act == 1 else F.gelu(y) if act == 2 else y).numpy()


@pytest.mark.parametrize("cfg", [0, 3, 59, 63])
def test_splitk_full_epilogue_against_fp64_and_unsliced(engine, cfg):
    rng = np.random.default_rng(300 + cfg)
    M, K, N = 260, 1352, 320
    A, W, b, R = rnd(rng, M, K), rnd(rng, N, K, scale=K ** -0.5), rnd(rng, N), rnd(rng, M, N)
    lin64 = 0.3 * (A.astype(np.float64) @ W.astype(np.float64).T + b) + 0.7 * R
    x, x1 = rnd(rng, 5, 20, 28, 128), rnd(rng, 5, 20, 28, 64)
    w, bc = rnd(rng, 192, 192, 1, 3, 3, scale=(9 * 192) ** -0.5), rnd(rng, 192)
    conv64 = conv_f64(x, w, bc, x1=x1)
    xr, wr, br, rr = rnd(rng, 3, 20, 24, 64), rnd(rng, 64, 64, 1, 3, 3, scale=(9 * 64) ** -0.5), rnd(rng, 64), rnd(rng, 3, 20, 24, 64)
    gamma, beta = h16(1.0 + 0.2 * rng.standard_normal(64)), h16(0.1 * rng.standard_normal(64))
    res64 = conv_f64(xr, wr, br) + rr
    Wz = rnd(rng, N, K)
    cases = [(f"linear act={act}", lambda act=act: engine.op_linear(A, W, b, R1=R, c0=0.3, c1=0.7, act=act), _act64(lin64, act)) for act in (0, 1, 2)]
    cases.append(("two-source conv3x3", lambda: engine.op_conv(x, w, bc, x1=x1), conv64))
    cases.append(("conv3x3 + residual", lambda: engine.op_conv_gn(xr, wr, br, 32, 1e-5, gamma, beta, res=rr)[0], res64))
    try:
        for name, run, ref in cases:
            engine.tune_force(cfg, 1)
            base = run()
            assert_close(base, ref, TOL, f"cfg {cfg} unsliced {name}")
            for sp in (2, 5, 8):
                engine.tune_force(cfg, sp)
                got = run()
                assert_close(got, ref, TOL, f"cfg {cfg} split {sp} {name}")
                d = float(np.abs(got - base).max())
                assert d <= 2.0 ** -10 * np.abs(ref).max(), f"cfg {cfg} split {sp} {name}: {d} from the unsliced output, more than one fp16 spacing at {np.abs(ref).max()}"
        # epilogue terms once, not per slice: zero A, bias 100, residual 100 -> exactly 200
        for sp in (1, 2, 5, 8):
            engine.tune_force(cfg, sp)
            got = engine.op_linear(np.zeros((M, K), np.float32), Wz, np.full(N, 100.0, np.float32), R1=np.full((M, N), 100.0, np.float32))
            assert np.array_equal(got, np.full((M, N), 200.0, np.float32)), f"cfg {cfg} split {sp}: bias + residual on zero A: {_where(got, np.full((M, N), 200.0, np.float32))}"
    finally:
        engine.tune_force(-1, -1)


# ---------------------------------------------------------------------------------------------------
# 3. Where split-K must not happen: gemm_plan's plain_epi turns a forced factor off for GEGLU (and for the engine's sub-pixel upsample convolution,
# GemmP::up_phase: tests/test_conv_bound_gpu.py); launch_gemm declines the statistics epilogue for a sliced launch.
# op_conv(ups=2) is the OTHER upsample form - the nearest-2x mapping inside the im2col address (GemmP::ups) - and it IS sliced under a forced factor:
# its outputs are compared on integer data, where sliced and unsliced agree bit for bit either way (and the exact screen above runs it at every factor).
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [0, 35, 54, 64])
def test_forced_split_is_ignored_for_geglu(engine, cfg):
    rng = np.random.default_rng(400 + cfg)
    M, K, inner = 260, 1344, 320
    A, W, b = rnd(rng, M, K), rnd(rng, 2 * inner, K, scale=K ** -0.5), rnd(rng, 2 * inner)
    try:
        engine.tune_force(cfg, 1)
        base = engine.op_linear(A, W, b, geglu=True)
        engine.tune_force(cfg, 8)
        got = engine.op_linear(A, W, b, geglu=True)
    finally:
        engine.tune_force(-1, -1)
    assert np.array_equal(got, base), f"cfg {cfg}: a forced split changed a GEGLU launch: {_where(got, base)}"
    y = torch.from_numpy(A.astype(np.float64) @ W.astype(np.float64).T + b)
    h, g = y.chunk(2, dim=-1)
    assert_close(got, (h * F.gelu(g)).numpy(), TOL, f"cfg {cfg} geglu under a forced split")


@pytest.mark.parametrize("cfg", [0, 59])
def test_forced_split_on_upsample_conv_equals_unsliced(engine, cfg):
    name, run, ref = _exact_problems()[-1]
    assert name == "conv3x3 on the nearest-2x source" and np.abs(ref).max() < 2048
    try:
        engine.tune_force(cfg, 1)
        base = run(engine)
        engine.tune_force(cfg, 8)
        got = run(engine)
    finally:
        engine.tune_force(-1, -1)
    assert np.array_equal(got, base), f"cfg {cfg}: op_conv(ups=2) split 8 vs split 1: {_where(got, base)}"
    assert np.array_equal(got, ref), f"cfg {cfg}: op_conv(ups=2) split 8 vs integer reference: {_where(got, ref)}"


def test_forced_split_declines_the_statistics_epilogue(engine):
    """The smallest case of test_groupnorm_statistics_from_conv_epilogue that reports statistics blocks (rb = 48 on the planner's halo tile): under a
    forced factor the launch is sliced on an im2col tile, must report rb == 0 (nothing consumed: y_epi is the statistics-pass result) and the
    convolution must still be right."""
    rng = np.random.default_rng(500)
    T, H, W, C = 2, 96, 128, 128
    x, w, b = rnd(rng, T, H, W, C), rnd(rng, C, C, 1, 3, 3, scale=(9 * C) ** -0.5), rnd(rng, C)
    gamma, beta = h16(1.0 + 0.2 * rng.standard_normal(C)), h16(0.1 * rng.standard_normal(C))
    try:
        co1, _, _, rb1 = engine.op_conv_gn(x, w, b, 32, 1e-5, gamma, beta)
        engine.tune_force(-1, 8)
        co, y_pass, y_epi, rb = engine.op_conv_gn(x, w, b, 32, 1e-5, gamma, beta)
    finally:
        engine.tune_force(-1, -1)
    assert rb1 == 48, f"unsliced: rows per statistics block {rb1}, expected 48"
    assert rb == 0, f"a sliced launch reported statistics blocks of {rb} rows"
    assert np.array_equal(y_epi, y_pass)
    ref = conv_f64(x, w, b)
    assert_close(co, ref, TOL, "conv under a forced split, statistics requested")
    assert np.abs(co - co1).max() <= 2.0 ** -10 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------
# 4. The planner's own split branches, unforced: one small shape per branch of gemm_plan that returns a factor > 1 (shapes from its comments, K trimmed to
# the branch's threshold), the whole output against fp64, and Engine.bench_gemm(same shape, cfg=-1, split=0) as the proof that the branch was taken.
# dense: (M, K, N); conv: (T, H, W, C, O, kt, k, ups).  Two of them carry an empty slice of the planner's own making (nk_all = 72 in 10 slices of 8).
# Not reachable without a knob: the im2col arm of the "nk >= 128" loop and the few-tile im2col rule on buffer-addressable sources - the round-3
# rules (config 63 / M <= 128) override both whenever gemm_can_bufa holds; the few-tile rule is reached here through the nearest-2x source instead.
# conv320@72x72 itself gets 160 / 81 = 1 slice from the under-filled rule; the 48 x 48 shape below takes the same arm with four.
# ---------------------------------------------------------------------------------------------------
PLANNER_BRANCHES = [
    ("latency corner, nk >= 128: largest factor of the 128x128 tile", "dense", (1200, 8192, 640), (0, 8)),
    ("latency corner, nk >= 48: two slices of the 128x64 tile", "dense", (1200, 3072, 640), (3, 2)),
    ("few-tile dense (81 rows)", "dense", (81, 1024, 320), (3, 3)),
    ("few-tile im2col (nearest-2x source, 324 rows)", "conv", (1, 9, 9, 512, 512, 1, 3, 2), (0, 10)),
    ("round 3: im2col on config 63 (324 rows)", "conv", (1, 18, 18, 128, 128, 1, 3, 1), (63, 2)),
    ("round 3: im2col with M <= 128 (81 rows)", "conv", (1, 9, 9, 512, 128, 1, 3, 1), (3, 10)),
    ("round 3: two-slice dense (1296 rows)", "dense", (1296, 2048, 640), (3, 2)),
    ("level 3: im2col nk >= 128 on config 59", "conv", (1, 30, 40, 960, 1024, 1, 3, 1), (59, 4)),
    ("level 3: temporal conv nk >= 48 on config 63", "conv", (25, 6, 8, 1024, 1024, 3, 1, 1), (63, 3)),
    ("level 3: dense nk >= 64 on config 59", "dense", (1200, 4096, 1280), (59, 3)),
    ("under-filled im2col on config 63", "conv", (1, 48, 48, 256, 128, 1, 3, 1), (63, 4)),
    ("under-filled im2col on the 128x128 tile", "conv", (1, 72, 72, 256, 640, 1, 3, 1), (0, 2)),
    ("under-filled dense", "dense", (2304, 1280, 320), (3, 2)),
]


@pytest.mark.parametrize("what,kind,dims,want", PLANNER_BRANCHES, ids=[b[0] for b in PLANNER_BRANCHES])
def test_planner_split_branches(engine, what, kind, dims, want):
    rng = np.random.default_rng(sum(dims))
    if kind == "dense":
        M, K, N = dims
        A, W, b, R = rnd(rng, M, K), rnd(rng, N, K, scale=K ** -0.5), rnd(rng, N), rnd(rng, M, N)
        got = engine.op_linear(A, W, b, R1=R)
        ref = A.astype(np.float64) @ W.astype(np.float64).T + b + R
        plan = engine.bench_gemm(M, N, K, cfg=-1, split=0, iters=1)[2:]
    else:
        T, H, Wd, C, O, kt, k, ups = dims
        x, w, b = rnd(rng, T, H, Wd, C), rnd(rng, O, C, kt, k, k, scale=(kt * k * k * C) ** -0.5), rnd(rng, O)
        got = engine.op_conv(x, w, b, kt=kt, k=k, pad_t=k // 2, pad_l=k // 2, ups=ups)
        ref = conv_f64(x, w, b, kt=kt, k=k, pad_t=k // 2, pad_l=k // 2, ups=ups)
        plan = engine.bench_gemm(N=O, conv=dict(T=T, H=H, W=Wd, C0=C, C1=0, kt=kt, k=k, stride=1, ups=ups), cfg=-1, split=0, iters=1)[2:]
    assert plan == want and plan[1] > 1, f"{what}: the planner chose (cfg, split) = {plan}, this test is written for {want}"
    assert_close(got, ref, TOL, f"planner split branch: {what}")
