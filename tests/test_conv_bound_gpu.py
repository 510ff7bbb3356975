"""Convolutions as the product runs them: bound on the device by bind_conv and launched by conv() (engine.hip), op by op.

Engine.op_conv packs its weights on the host and fills a GemmP by hand; no model does either.  Engine.op_bind_conv / op_conv_bound drive the
product's own code: k_permute_conv_w, k_rechunk_conv_w and k_upsample_phase_w for the weights, conv() for the launch - for an upsampler
(ups == 2 with bound phase weights) four 2x2 convolutions on the source grid, one per output parity, whose epilogue scatters to (2y + a, 2x + b)
(GemmP::up_phase).  The numpy restatements and their own checks are in tests/test_conv_bound_cpu.py.

1. the bound weight and the phase weights, bit for bit against bound_layout / phase_weights;
2. the sub-pixel path on integer data, where everything is exact: equal to the definition conv_f64(..., ups=2) everywhere, every output pixel
   written, nothing else written - on the planner's tile and on every tile family, at frame shapes where half of a phase's taps are outside;
3. the same path on fp16-rounded Gaussian data against the definition at TOL.  The reference side of that comparison - the four-phase form in fp64
   with phase weights rounded once to fp16, against the definition - measures (test_conv_bound_cpu.REF_ONLY_ERR, asserted there)
       (2, 6, 8, 128, 128): 2.08e-4   (3, 5, 7, 64, 64): 1.91e-4   (2, 3, 5, 40, 72): 2.22e-4   (1, 4, 4, 320, 320): 2.16e-4
   of max|ref|; with the fp16 store (2^-11 = 4.9e-4) under half of TOL = 2e-3;
4. the other bound forms against Engine.op_conv bit for bit (same kernels; only who laid out the weights differs) and against conv_f64."""
import functools

import numpy as np
import pytest

import test_conv_bound_cpu as ref_cpu
import test_ops_gpu
from test_conv_bound_cpu import EXACT_SHAPES, RANDOM_SHAPES, bound_layout, bound_phase_layout, exact_problem, pad8, random_problem
from util import assert_close, conv_f64, h16, where_differ

pytestmark = pytest.mark.gpu
TOL = test_ops_gpu.TOL
assert TOL == ref_cpu.TOL

GUARD = 64


def bits(a):
    """fp16 bit patterns of float32 values that are fp16 numbers."""
    h = np.asarray(a, np.float32).astype(np.float16)
    assert np.array_equal(h.astype(np.float32), a)
    return h.view(np.uint16)


# ---------------------------------------------------------------------------------------------------
# 1. Weight layouts.  Weights are multiples of 2^-10 in (-1, 1): fp16 numbers, and every phase sum (at most four of them) is a multiple of 2^-10 below 4,
# exact in fp32 in any order - the single fp32 -> fp16 rounding is numpy's.
# ---------------------------------------------------------------------------------------------------
LAYOUTS = [(O, I, kt, k, 0) for (O, I, kt, k) in ref_cpu.LAYOUT_CASES] + [(O, I, kt, k, 1) for (O, I, kt, k) in ref_cpu.LAYOUT_CASES[:4]]


@pytest.mark.parametrize("O,I,kt,k,upsampler", LAYOUTS)
def test_bound_weight_layouts_bitwise(engine, O, I, kt, k, upsampler):
    rng = np.random.default_rng(O + I + kt + k)
    w = (rng.integers(-1023, 1024, (O, I, kt, k, k)) / 1024.0).astype(np.float32)
    b = (rng.integers(-1023, 1024, O) / 1024.0).astype(np.float32)
    taps, cinp = kt * k * k, pad8(I)
    got = engine.op_bind_conv(w, b, upsampler=bool(upsampler))
    assert got["cinp"] == cinp
    chunked = taps > 1 and cinp % 64 == 0
    assert got["kchunk"] == int(chunked), f"kchunk flag {got['kchunk']} for taps {taps}, cinp {cinp}"
    want = bound_layout(w, kt, k, cinp)
    assert np.array_equal(bits(got["w"]), bits(want)), f"Conv::w: {where_differ(got['w'], want)}"
    if cinp != I:       # tap-major with pad columns: each tap's columns I .. cinp - 1 are +0
        assert not chunked
        assert not bits(got["w"]).reshape(O, taps, cinp)[:, :, I:].any()
    if not upsampler:
        assert got["wphase"] is None
        return
    assert got["wphase"] is not None, "an upsampler was bound without phase weights"
    wantp = bound_phase_layout(w, cinp)
    assert not np.isnan(got["wphase"]).any(), "phase weights not written"
    assert np.array_equal(bits(got["wphase"]), bits(wantp)), f"Conv::wphase [4, O, 4 cinp]: {where_differ(got['wphase'], wantp)}"
    if cinp != I:
        assert not bits(got["wphase"]).reshape(4, O, 4, cinp)[..., I:].any()


# ---------------------------------------------------------------------------------------------------
# 2. Exact-integer screen of the sub-pixel path.  x, w in {-1, 0, 1}, bias in [-2, 2]: phase weights are integers in [-4, 4], every product and partial sum
# an integer below 2^24, |ref| <= 9 C + 2 < 2048 an exact fp16 integer.  The output goes up full of NaN with GUARD rows behind it.
#   (5, 20, 28, 128, 192): 2800 rows per phase - ragged against 128-, 192- and 256-row tiles - two channel chunks, 1.5 column tiles of 128
#   (3, 7, 9, 192, 64):    odd frame, less than one tile, three frames: a y + 1 tap that escapes its mask reads the next frame
#   (2, 1, 1, 64, 64), (2, 1, 6, 64, 64), (2, 6, 1, 64, 64): half of each phase's taps are outside the frame
#   (3, 5, 7, 40, 72):     tap-major weights on the general loader path, K = 160 with a K tail
# ---------------------------------------------------------------------------------------------------
def run_subpixel(engine, shape, data, ldo=0, upsampler=True):
    """-> (image [T, 2H, 2W, O], surplus columns [rows, ldo - O], guard rows [GUARD, ldo], plan)"""
    T, H, W, C, O = shape
    x, w, b, _ = data
    out, plan = engine.op_conv_bound(x, w, b, ups=2, upsampler=upsampler, ldo=ldo, guard=GUARD, fill=np.nan)
    rows = T * 2 * H * 2 * W
    assert out.shape == (rows + GUARD, ldo or O)
    return out[:rows, :O].reshape(T, 2 * H, 2 * W, O), out[:rows, O:], out[rows:], plan


def check_exact(what, img, surplus, guard, ref):
    assert np.isnan(guard).all(), f"{what}: {np.count_nonzero(~np.isnan(guard))} guard elements were written"
    assert np.isnan(surplus).all(), f"{what}: {np.count_nonzero(~np.isnan(surplus))} elements of the surplus columns were written"
    unwritten = np.argwhere(np.isnan(img).any(-1))
    assert len(unwritten) == 0, f"{what}: {len(unwritten)} output pixels no phase wrote, first (t, y, x) = {tuple(unwritten[0])}, parities (y, x) " \
                                f"{sorted(set((int(p[1]) & 1, int(p[2]) & 1) for p in unwritten))}"
    assert np.array_equal(img, ref), f"{what} vs integer reference: {where_differ(img, ref)}"


# symmetric kernel: 0, 3, 12, 14, 19, 61; loader kernel: 35, 39; producer / consumer kernel: 54, 59, 63, 64; -1: the planner's tile
@pytest.mark.parametrize("cfg", [-1, 0, 3, 12, 14, 19, 61, 35, 39, 54, 59, 63, 64])
def test_subpixel_exact_integer_screen(engine, cfg):
    try:
        engine.tune_force(cfg, -1)
        for shape in EXACT_SHAPES:
            data = exact_problem(shape)
            ref = data[3]
            assert np.abs(ref).max() < 2048, f"{shape}: the reference leaves the exact fp16 integers"
            img, surplus, guard, plan = run_subpixel(engine, shape, data)
            print(f"PLAN sub-pixel {shape} forced cfg {cfg}: (tile config, split) per phase {plan}")
            assert len(plan) == 4, f"{shape}: {len(plan)} launches, not the four phases"
            assert all(sp == 1 for _, sp in plan), f"{shape}: a phase launch was planned with a split: {plan}"
            if cfg >= 0:
                assert all(cf == cfg for cf, _ in plan), f"{shape}: forced tile {cfg}, planned {plan}"
            check_exact(f"cfg {cfg} {shape}", img, surplus, guard, ref)
    finally:
        engine.tune_force(-1, -1)


def test_subpixel_forced_split_is_declined(engine):
    """gemm_plan's plain_epi turns a forced factor off for GemmP::up_phase: the scatter epilogue has no split-K form."""
    try:
        for shape in EXACT_SHAPES:
            data = exact_problem(shape)
            engine.tune_force(0, 1)
            base = run_subpixel(engine, shape, data)
            engine.tune_force(0, 5)
            img, surplus, guard, plan = run_subpixel(engine, shape, data)
            assert plan == ((0, 1),) * 4, f"{shape}: forced (0, 5), planned {plan}"
            check_exact(f"forced split 5 {shape}", img, surplus, guard, data[3])
            assert np.array_equal(img, base[0]), f"{shape}: forced split 5 vs split 1: {where_differ(img, base[0])}"
    finally:
        engine.tune_force(-1, -1)


def test_subpixel_surplus_columns_come_back_as_given(engine):
    shape = EXACT_SHAPES[0]
    data = exact_problem(shape)
    img, surplus, guard, plan = run_subpixel(engine, shape, data, ldo=shape[4] + 8)
    assert surplus.shape[1] == 8 and guard.shape[1] == shape[4] + 8
    check_exact(f"ldo = O + 8 {shape}", img, surplus, guard, data[3])


# ---------------------------------------------------------------------------------------------------
# 3. fp16-rounded Gaussian data against the definition (raw weights, nearest-2x source, 3x3) at TOL, through both bound upsample forms: the sub-pixel
# phases (upsampler) and the general loader's nearest-2x addressing (a convolution not bound as an upsampler, launched with ups = 2).
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upsampler", [1, 0], ids=["subpixel", "nearest2x"])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=str)
def test_upsample_conv_against_the_definition(engine, shape, upsampler):
    data = random_problem(shape)
    img, surplus, guard, plan = run_subpixel(engine, shape, data, upsampler=bool(upsampler))
    assert len(plan) == (4 if upsampler else 1), plan
    assert np.isnan(guard).all() and not np.isnan(img).any()
    assert_close(img, data[3], TOL, f"bound upsample conv {'sub-pixel' if upsampler else 'nearest-2x'} {shape}")


# ---------------------------------------------------------------------------------------------------
# 4. The other bound forms: device binding against host packing.  Integer data (|ref| <= 9 * 192 + 2 + 8 < 2048): bound == op_conv == conv_f64 exactly;
# Gaussian data: bound == op_conv bit for bit and both at TOL.  op_conv has no residual argument: that form is compared with conv_f64 + R alone.
# name: (frame (T, H, W), C0, C1, O, kt, k, stride, pad_t, pad_l)
# ---------------------------------------------------------------------------------------------------
FORMS = {
    "two-source 3x3": ((5, 20, 28), 128, 64, 192, 1, 3, 1, 1, 1),
    "temporal (3,1,1)": ((5, 20, 28), 128, 0, 192, 3, 1, 1, 0, 0),
    "stride 2 pad 1": ((5, 20, 28), 128, 0, 192, 1, 3, 2, 1, 1),
    "stride 2 pad (0,1,0,1)": ((5, 20, 28), 128, 0, 192, 1, 3, 2, 0, 0),
    "1x1 two-source": ((5, 20, 28), 128, 64, 192, 1, 1, 1, 0, 0),
    "cin 4 padded to 8": ((3, 12, 20), 4, 0, 128, 1, 3, 1, 1, 1),
    "cout 4": ((3, 12, 20), 128, 0, 4, 1, 3, 1, 1, 1),
}


@functools.lru_cache(maxsize=None)
def form_problem(name, integer):
    (T, H, W), C0, C1, O, kt, k, stride, pad_t, pad_l = FORMS[name]
    rng = np.random.default_rng(len(name) + 100 * integer + C0 + O)
    C = C0 + C1
    if integer:
        x, w = rng.integers(-1, 2, (T, H, W, C)).astype(np.float32), rng.integers(-1, 2, (O, C, kt, k, k)).astype(np.float32)
        b = rng.integers(-2, 3, O).astype(np.float32)
    else:
        x, w, b = h16(rng.standard_normal((T, H, W, C))), h16(rng.standard_normal((O, C, kt, k, k)) * (kt * k * k * C) ** -0.5), h16(rng.standard_normal(O))
    kw = dict(stride=stride, pad_t=pad_t, pad_l=pad_l)
    ref = conv_f64(x, w, b, kt=kt, k=k, **kw)
    x0, x1 = np.ascontiguousarray(x[..., :C0]), (np.ascontiguousarray(x[..., C0:]) if C1 else None)
    return x0, x1, w, b, kw, ref


@pytest.mark.parametrize("integer", [1, 0], ids=["integer", "gaussian"])
@pytest.mark.parametrize("name", list(FORMS))
def test_bound_forms_equal_host_packed(engine, name, integer):
    x0, x1, w, b, kw, ref = form_problem(name, integer)
    O, C, kt, k = w.shape[:4]
    out, plan = engine.op_conv_bound(x0, w, b, x1=x1, guard=GUARD, fill=np.nan, **kw)
    assert len(plan) == 1
    got, guard = out[:-GUARD].reshape(ref.shape), out[-GUARD:]
    assert np.isnan(guard).all(), f"{name}: guard rows were written"
    if C % 8:       # op_conv takes whole 8-channel groups: the same problem with the zero channels spelled out
        xp, wp = np.zeros(x0.shape[:3] + (pad8(C),), np.float32), np.zeros((O, pad8(C), kt, k, k), np.float32)
        xp[..., :C], wp[:, :C] = x0, w
        host = engine.op_conv(xp, wp, b, kt=kt, k=k, **kw)
    else:
        host = engine.op_conv(x0, w, b, x1=x1, kt=kt, k=k, **kw)
    assert not np.isnan(got).any(), f"{name}: output elements not written"
    assert np.array_equal(got, host), f"{name}: device-bound vs host-packed weights: {where_differ(got, host)}"
    if integer:
        assert np.abs(ref).max() < 2048
        assert np.array_equal(got, ref), f"{name} vs integer reference: {where_differ(got, ref)}"
    else:
        assert_close(got, ref, TOL, f"bound conv {name}")


@pytest.mark.parametrize("integer", [1, 0], ids=["integer", "gaussian"])
def test_bound_conv_with_residual(engine, integer):
    x0, x1, w, b, kw, ref = form_problem("two-source 3x3", integer)
    rng = np.random.default_rng(77 + integer)
    R = rng.integers(-8, 9, ref.shape).astype(np.float32) if integer else h16(rng.standard_normal(ref.shape))
    out, plan = engine.op_conv_bound(x0, w, b, x1=x1, R1=R, c0=1.0, c1=1.0, guard=GUARD, fill=np.nan, **kw)
    got, guard = out[:-GUARD].reshape(ref.shape), out[-GUARD:]
    assert np.isnan(guard).all() and not np.isnan(got).any()
    want = ref + R
    if integer:
        assert np.abs(want).max() < 2048
        assert np.array_equal(got, want), f"3x3 + residual vs integer reference: {where_differ(got, want)}"
    else:
        assert_close(got, want, TOL, "bound conv 3x3 + residual")
