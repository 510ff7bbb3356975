"""The float32-grade VAE encoder's kernels op by op (kernels/wide.hip; conv_w, dup_conv and the attention core of vattn_wide in engine.hip), driven
through float32-in / float32-out entry points: nothing is rounded to fp16 on the way in, float32 inputs are the point.

Two references, named in every check:

* PAIR MODEL - the same operation in fp64 on the rounded operands the kernel actually multiplies.  hi = fp16(x), lo = fp16(x - hi) come from numpy's
  float16 conversion (round to nearest even, subnormals kept; the MFMA does not flush them).  W (hi + lo) for a convolution, the three terms
  al bh + ah bl + ah bh for QK^T and PV (with the power-of-two scale of the probabilities).  All that separates the device from it is fp32
  accumulation (and, in the attention, fp32 softmax arithmetic).  A lost lo half shows at 2^-12 ~ 2.4e-4 relative, a layout slip at O(1).
* TRUTH - fp64 of the float32 operation itself.

No tolerance is a fixed number.  The FLOOR of a check is the distance of a plain float32 evaluation from the same reference on the same inputs:
numpy float32 of the K-doubled product for the pair model, torch-CPU float32 of the operation for truth.  Against the pair model the device may be
8 x its floor away (three bits for a different summation order), against truth at unit input scale 4 x.  With floors of 1e-7 .. 1e-6 (split, GroupNorm,
convolutions, flat attention rows) 8 x is still 30 - 60 x below the smallest bug signature; on the peaked attention rows, whose float32 floor is 5e-6 ..
1.2e-5 (fp32 rounding of scores of size 30 - 50), it is ~1e-4, only 2.5 x below a lost lo half - there the 4 x truth check (1e-5) is the tighter one.
Errors are max |err| / max |ref|.  Every measured value goes through util.report next to its floor; DESIGN.md section 3 tabulates them."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_ops_gpu
from util import conv_f64, h16, rel_err, report

pytestmark = pytest.mark.gpu

PAIR_FACTOR = 8.0       # device vs pair model: <= 8 x the float32 floor
TRUTH_FACTOR = 4.0      # device vs truth at unit input scale: <= 4 x the float32 floor
P_SCALE = 4096.0        # k_softmax_pair splits 2^12 p (engine.hip: kPScale)


def split_np(x):
    """The pair as numpy rounds it: (hi, lo) as float32 arrays holding fp16 values."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)       # x - hi is exact in float32
    return hi.astype(np.float32), lo.astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(got, ref, plain32, factor, what, ref_name):
    """got within factor x the float32 floor of ref; both distances reported."""
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    floor = rel_err(plain32, ref)
    err = rel_err(got, ref)
    report(f"wide {what} vs {ref_name}", err, floor=floor, factor=factor, ratio=err / floor if floor > 0 else float("inf"), kind="max|err|/max|ref|")
    assert floor > 0, f"{what}: the float32 evaluation equals {ref_name} exactly - no floor to measure against"
    assert err <= factor * floor, f"{what} vs {ref_name}: {err:.3e} > {factor:g} x float32 floor {floor:.3e} (ratio {err / floor:.1f})"
    return err, floor


# --------------------------------------------------------------------------------------------------- 1. split_pair
def _hand_picked():
    e = np.float32(2.0) ** -14
    vals = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(1)),
            -np.nextafter(e, np.float32(0)), -np.nextafter(e, np.float32(1)), 65504.0, -65504.0, 1.0 + 2.0 ** -11, -(1.0 + 2.0 ** -11),
            1.0 + 3 * 2.0 ** -11, 1e-8, -1e-8, 2.0 ** -24 + 2.0 ** -25, 3 * 2.0 ** -25 + 2.0 ** -40, 2.0 ** -14 + 2.0 ** -25, 0.1, -0.3, 1.0, 1000.7,
            65503.9, 2.0 ** -3, np.nextafter(np.float32(2.0 ** -3), np.float32(0)), 0.99999994, 3.14159274, 2.0 ** -20, 6.1e-5, 5.9e-8, 6.0e-8, 2047.5,
            2048.5, -2049.5, 0.33333334, 1e-3, 7e-6]
    assert len(vals) == 40
    return np.asarray(vals, np.float32).reshape(5, 8)


@pytest.mark.parametrize("case", ["hand-picked", "gaussian", "gaussian 2^-10"])
def test_split_pair_is_bit_identical_to_the_numpy_rounding(engine, case):
    """hi = fp16(x), lo = fp16(x - hi), bit for bit (the sign of zero included): +-0, the smallest subnormal 2^-24 and the tie below it 2^-25 (-> 0), one
    float32 ulp either side of the smallest normal 2^-14, the largest fp16 65504, the tie 1 + 2^-11 (-> even), 1e-8 (lost altogether); Gaussian data at
    unit scale and at 2^-10, where nearly every lo half is subnormal."""
    if case == "hand-picked":
        x = _hand_picked()
    else:
        x = (np.random.default_rng(11).standard_normal((300, 32)) * (1.0 if case == "gaussian" else 2.0 ** -10)).astype(np.float32)
    hi, lo = engine.op_split_pair(x)
    rh, rl = split_np(x)
    bad = np.argwhere((bits(hi) != bits(rh)) | (bits(lo) != bits(rl)))
    report(f"wide split_pair {case}: elements that differ from the numpy rounding", len(bad), of=int(x.size))
    assert len(bad) == 0, (f"{len(bad)} of {x.size} differ; first x = {x[tuple(bad[0])]!r}: got ({hi[tuple(bad[0])]!r}, {lo[tuple(bad[0])]!r}), "
                           f"numpy ({rh[tuple(bad[0])]!r}, {rl[tuple(bad[0])]!r})")
    if case != "hand-picked":
        report(f"wide split_pair {case}: subnormal or zero lo halves", float((np.abs(rl) < 2.0 ** -14).mean()))


# --------------------------------------------------------------------------------------------------- 2. gn32_pair
def _gn_truth(x, G, eps, gamma, beta, silu):
    T, HW, C = x.shape
    xg = x.astype(np.float64).reshape(T, HW, G, C // G)
    mean = xg.mean((1, 3), keepdims=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdims=True)
    y = ((xg - mean) / np.sqrt(var + eps)).reshape(T, HW, C) * gamma.astype(np.float64) + beta.astype(np.float64)
    return y / (1.0 + np.exp(-y)) if silu else y


def _gn_torch32(x, G, eps, gamma, beta, silu):
    y = F.group_norm(torch.from_numpy(x).permute(0, 2, 1).contiguous(), G, torch.from_numpy(gamma), torch.from_numpy(beta), eps)
    if silu:
        y = F.silu(y)
    return y.permute(0, 2, 1).numpy()


def _check_gn(engine, C, G, HW, T, silu, shift, what):
    rng = np.random.default_rng(C * 131 + HW + 7 * T + int(silu))
    x = (rng.standard_normal((T, HW, C)) * (1.0 + 0.5 * rng.random((1, 1, C))) + 0.3 * rng.standard_normal((T, 1, C)) + shift).astype(np.float32)
    gamma, beta = h16(1.0 + 0.2 * rng.standard_normal(C)), h16(0.2 * rng.standard_normal(C))
    eps = 1e-6
    hi, lo = engine.op_gn32_pair(x, G, eps, gamma, beta, silu=silu)
    assert np.isfinite(hi).all() and np.isfinite(lo).all(), f"{what}: non-finite output"
    # hi is the fp16 rounding of the value the pair stands for.  lo = fp16(v - hi) is itself rounded, and where that rounding lands exactly on half an ulp
    # of hi (the 13 float32 bits below hi's are 1000...0 or 0111...1, either side: 4 patterns in 2^13 = 5e-4 of the elements of ANY correct split,
    # numpy's included) hi + lo is a tie, which fp16() resolves to even whatever hi was: the identity is asserted wherever |lo| is below half an ulp of
    # hi, |lo| <= half an ulp everywhere, and the exact-half-ulp elements have to stay an exception (< 0.5 %: 10 x the pattern count, for values whose
    # low bits are not uniform; a split that put them there wholesale would also miss the truth check below by 2^-12).
    half = np.spacing(np.abs(hi).astype(np.float16)).astype(np.float64) / 2
    again = (hi.astype(np.float64) + lo.astype(np.float64)).astype(np.float16).astype(np.float32)
    assert (np.abs(lo) <= half).all(), f"{what}: |lo| above half an ulp of hi in {(np.abs(lo) > half).sum()} elements"
    inside = np.abs(lo) < half
    assert np.array_equal(again[inside], hi[inside]), f"{what}: hi != fp16(hi + lo) in {(again[inside] != hi[inside]).sum()} elements"
    ties = 1.0 - inside.mean()
    report(f"wide gn32_pair {what}: elements with |lo| = half an ulp of hi", ties)
    assert ties < 5e-3, f"{what}: {ties:.2e} of the lo halves sit exactly on half an ulp of hi (a correct split: ~5e-4)"
    check(hi.astype(np.float64) + lo, _gn_truth(x, G, eps, gamma, beta, silu), _gn_torch32(x, G, eps, gamma, beta, silu), TRUTH_FACTOR, f"gn32_pair {what}", "truth")


GN_SHAPES = [(32, 8, 64, 2),          # cpg 4 (k_gn32_stats4), one chunk, every thread row in use
             (64, 8, 100, 1),         # cpg 8, ragged rows
             (128, 32, 4096, 1),      # cpg 4, many chunks: the real encoder's 128-channel level
             (256, 32, 2500, 2),      # ragged last chunk of k_gn32_stats / k_gn32_apply
             (512, 32, 48, 3)]        # 4 rows per iteration


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("C,G,HW,T", GN_SHAPES)
def test_gn32_pair(engine, C, G, HW, T, silu):
    _check_gn(engine, C, G, HW, T, silu, 0.0, f"C{C} G{G} HW{HW} T{T}{' silu' if silu else ''}")


def test_gn32_pair_shifted_input(engine):
    """Input mean 4 standard deviations off zero: the statistics are E[x^2] - mean^2 with fp32 per-thread partial sums (fp64 above them), under the same
    truth rule as the centred cases."""
    _check_gn(engine, 128, 32, 4096, 1, True, 4.0, "C128 G32 HW4096 T1 silu, input + 4 sigma")


# --------------------------------------------------------------------------------------------------- 3. conv_wide
CONV_SHAPES = [(1, 8, 8, 32, 32, 3, 1, 1),        # tap-major base, 2C = 64: one chunk, both K orders coincide
               (1, 8, 8, 96, 64, 3, 1, 1),        # tap-major base, 2C = 192: a multiple of 64 that stays tap-major
               (2, 6, 10, 64, 64, 3, 1, 1),       # chunk-major base: the whole row twice
               (1, 12, 16, 128, 256, 1, 1, 0),    # 1x1 shortcut
               (1, 8, 8, 64, 64, 3, 2, 0),        # the encoder's bottom / right padding, stride 2
               (1, 8, 8, 64, 8, 3, 1, 1),         # N = 8: scalar epilogue
               (1, 8, 8, 8, 8, 1, 1, 0),          # the quant conv, K = 16
               (2, 6, 8, 512, 512, 3, 1, 1)]      # long K, few tiles: where the planner splits fp16 launches


def _im2col(x, k, stride, pad):
    """[T,H,W,C] -> [T*Ho*Wo, k*k*C] (tap-major), zero outside; pad = top / left, the bottom / right padding is whatever the taps reach."""
    T, H, W, C = x.shape
    Ho, Wo = H // stride, W // stride
    xp = np.zeros((T, H + k, W + k, C), x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = [xp[:, iy:iy + stride * Ho:stride, ix:ix + stride * Wo:stride].reshape(T * Ho * Wo, C) for iy in range(k) for ix in range(k)]
    return np.concatenate(cols, 1)


@functools.lru_cache(maxsize=None)
def _conv_problem(shape, scale):
    """Inputs and every reference of one convolution, computed once: x float32 at `scale`, fp16-valued weight / bias (as the checkpoint stores them),
    float32 residual; pair model and truth in fp64 (conv_f64), the float32 floors of both."""
    T, H, W, C, O, k, stride, pad = shape
    rng = np.random.default_rng(sum(v * 31 ** i for i, v in enumerate(shape)))
    x = (rng.standard_normal((T, H, W, C)) * scale).astype(np.float32)
    w = h16(rng.standard_normal((O, C, k, k)) * (C * k * k) ** -0.5)
    b = h16(rng.standard_normal(O) * 0.3 * scale)
    res = (rng.standard_normal((T, H // stride, W // stride, O)) * scale).astype(np.float32)
    hi, lo = split_np(x)
    w5 = w.reshape(O, C, 1, k, k)
    kw = dict(kt=1, k=k, stride=stride, pad_t=pad, pad_l=pad)
    pair = conv_f64(hi.astype(np.float64) + lo, w5, b, **kw)
    truth = conv_f64(x, w5, b, **kw)
    # float32 floor of the pair model: the K-doubled product [hi | lo] [W | W]^T as one float32 matrix product
    a32 = np.concatenate([_im2col(hi, k, stride, pad), _im2col(lo, k, stride, pad)], 1)
    wt = np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(O, k * k * C)
    pair32 = (a32 @ np.concatenate([wt, wt], 1).T + b).reshape(pair.shape)
    # float32 floor of truth: torch-CPU conv2d (bottom / right padding: one more row / column than the stride-2 taps reach, never read)
    xt = F.pad(torch.from_numpy(x).permute(0, 3, 1, 2), (pad, k - 1 - pad if stride == 1 else 1, pad, k - 1 - pad if stride == 1 else 1))
    truth32 = F.conv2d(xt, torch.from_numpy(w), torch.from_numpy(b), stride=stride).permute(0, 2, 3, 1).numpy()
    assert truth32.shape == truth.shape and rel_err(pair32, pair) < 1e-5 and rel_err(truth32, truth) < 1e-5     # the test's own three evaluations agree
    out = dict(x=x, w=w, b=b, res=res, pair=pair, truth=truth, pair32=pair32, truth32=truth32, wabs=np.abs(w.astype(np.float64)).sum((1, 2, 3)))
    for v in out.values():
        v.setflags(write=False)
    return out


def _conv_args(shape):
    T, H, W, C, O, k, stride, pad = shape
    return dict(k=k, stride=stride, pad_t=pad, pad_l=pad)


def _name(shape):
    T, H, W, C, O, k, stride, pad = shape
    return f"conv {T}x{H}x{W} {C}->{O} k{k} s{stride} p{pad}"


@pytest.mark.parametrize("residual", ["none", "float32", "in place"])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=_name)
def test_conv_wide(engine, shape, residual):
    """bind_conv -> dup_conv -> split_pair -> conv_w on the planner's tile, float32 output: without a residual, with a float32 residual (UG_F_R1_F32), and
    with the residual in the output buffer (res == out: res2d_wide with a shortcut)."""
    p = _conv_problem(shape, 1.0)
    res = None if residual == "none" else p["res"]
    got = engine.op_conv_wide(p["x"], p["w"], p["b"], res=res, res_in_place=residual == "in place", **_conv_args(shape))
    add = 0.0 if res is None else res.astype(np.float64)
    add32 = np.float32(0) if res is None else res
    what = f"{_name(shape)} residual {residual}"
    check(got, p["pair"] + add, p["pair32"] + add32, PAIR_FACTOR, what, "pair model")
    check(got, p["truth"] + add, p["truth32"] + add32, TRUTH_FACTOR, what, "truth")


@pytest.mark.parametrize("log2_scale", [-8, -12])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=_name)
def test_conv_wide_small_inputs_keep_the_analytic_floor(engine, shape, log2_scale):
    """Below 2^-3 the lo half is an fp16 subnormal: the pair is x to within 2^-25 ABSOLUTE per element, so an output is within 2^-25 sum_k |w_k| of
    truth (all taps: a bound for border pixels too) plus the pair-model tolerance.  A per-tensor scale would remove the term; it is not applied
    (kernels/wide.hip), this pins what the floor costs: the reported ratio to a float32 evaluation grows as the scale shrinks."""
    p = _conv_problem(shape, 2.0 ** log2_scale)
    got = engine.op_conv_wide(p["x"], p["w"], p["b"], **_conv_args(shape))
    assert np.isfinite(got).all()
    what = f"{_name(shape)} input scale 2^{log2_scale}"
    _, floor = check(got, p["pair"], p["pair32"], PAIR_FACTOR, what, "pair model")
    err = np.abs(got - p["truth"])
    bound = 2.0 ** -25 * p["wabs"] + PAIR_FACTOR * floor * np.abs(p["pair"]).max()
    report(f"wide {what} vs truth", rel_err(got, p["truth"]), float32_floor=rel_err(p["truth32"], p["truth"]), worst_over_analytic_bound=float((err / bound).max()),
           kind="max|err|/max|ref|")
    assert (err <= bound).all(), f"{what}: |err| up to {float((err / bound).max()):.2f} x (2^-25 sum|w| + pair tolerance)"


# --------------------------------------------------------------------------------------------------- 4. forced tiles
# every tile family that test_lean_epilogue_forms_equal_the_general_epilogue_bit_for_bit forces (-1: the planner's), and 60: the 80-column wave tile (CH = 4)
FORCED_CFGS = list(test_ops_gpu.LEAN_EPILOGUE_CFGS) + [60]


@pytest.mark.parametrize("cfg", FORCED_CFGS)
def test_conv_wide_on_forced_tiles_and_split_k_steps_aside(engine, cfg):
    """UG_F_OUT_F32 / UG_F_R1_F32 of tile_epilogue on every tile, not only the planner's own, residual apart and in place; and a forced split-K factor
    changes nothing: splitk_epilogue writes fp16 and reads R1 as fp16, so gemm_plan keeps float32-output launches away from it (plain_epi)."""
    try:
        for shape in (CONV_SHAPES[2], CONV_SHAPES[7]):
            p = _conv_problem(shape, 1.0)
            for in_place in (False, True):
                engine.tune_force(cfg, -1)
                got = engine.op_conv_wide(p["x"], p["w"], p["b"], res=p["res"], res_in_place=in_place, **_conv_args(shape))
                what = f"{_name(shape)} forced tile {cfg} residual {'in place' if in_place else 'float32'}"
                check(got, p["pair"] + p["res"].astype(np.float64), p["pair32"] + p["res"], PAIR_FACTOR, what, "pair model")
                engine.tune_force(cfg, 5)
                split = engine.op_conv_wide(p["x"], p["w"], p["b"], res=p["res"], res_in_place=in_place, **_conv_args(shape))
                assert np.array_equal(bits(split), bits(got)), f"{what}: a forced split-K factor changed the float32 output, max diff {np.abs(split - got).max()}"
    finally:
        engine.tune_force(-1, -1)


# --------------------------------------------------------------------------------------------------- 5. attn_wide
ATTN_SHAPES = [(1, 64, 64), (2, 256, 64), (1, 1024, 64),
               (1, 200, 128),      # S not a multiple of 32: k_vt_terms' ragged tile
               (1, 9, 64)]         # Spad = 16: zero tails of k_vt_terms and k_softmax_pair, scalar epilogue of the scores GEMM


def _softmax(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def attn_references(qkv, T, S, p_scale=P_SCALE):
    """(pair model, its float32 floor evaluation, truth, torch float32) of softmax(q k^T / sqrt(C)) v per frame, qkv [T*S, 3C] float32."""
    C = qkv.shape[1] // 3
    c0 = 1.0 / np.sqrt(np.float32(C))
    pair, pair32, truth, truth32 = (np.empty((T * S, C), dt) for dt in (np.float64, np.float32, np.float64, np.float32))
    for t in range(T):
        q, k, v = (qkv[t * S:(t + 1) * S, i * C:(i + 1) * C] for i in range(3))
        (qh, ql), (kh, kl), (vh, vl) = split_np(q), split_np(k), split_np(v)
        d = np.float64
        # pair model: three-term scores in fp64, the probabilities as float32 numbers scaled by the power of two and split, three-term PV in fp64
        s = (ql.astype(d) @ kh.astype(d).T + qh.astype(d) @ kl.astype(d).T + qh.astype(d) @ kh.astype(d).T) * d(c0)
        ph, pl = split_np(_softmax(s).astype(np.float32) * np.float32(p_scale))
        pair[t * S:(t + 1) * S] = (pl.astype(d) @ vh.astype(d) + ph.astype(d) @ vl.astype(d) + ph.astype(d) @ vh.astype(d)) / p_scale
        # its float32 floor: the K-tripled products as float32 matrix products (the kernels' term order: small terms first), float32 softmax
        s32 = (np.concatenate([ql, qh, qh], 1) @ np.concatenate([kh, kl, kh], 1).T) * c0
        ph, pl = split_np(_softmax(s32) * np.float32(p_scale))
        pair32[t * S:(t + 1) * S] = (np.concatenate([pl, ph, ph], 1) @ np.concatenate([vh, vl, vh], 0)) / np.float32(p_scale)
        truth[t * S:(t + 1) * S] = _softmax(q.astype(d) @ k.astype(d).T * d(c0)) @ v.astype(d)
        tq, tk, tv = (torch.from_numpy(np.ascontiguousarray(a)) for a in (q, k, v))
        truth32[t * S:(t + 1) * S] = (torch.softmax(tq @ tk.T * float(c0), -1) @ tv).numpy()
    return pair, pair32, truth, truth32


def attn_inputs(T, S, C, qk_scale, v_mean):
    rng = np.random.default_rng(S * 1009 + C + int(qk_scale * 100) + int(v_mean))
    qkv = rng.standard_normal((T * S, 3 * C))
    qkv[:, :2 * C] *= qk_scale
    qkv[:, 2 * C:] += v_mean
    return qkv.astype(np.float32)


@pytest.mark.parametrize("qk_scale,v_mean", [(0.25, 0.0), (3.0, 0.0), (0.25, 1.0)], ids=["flat", "peaked", "flat, v mean 1"])
@pytest.mark.parametrize("T,S,C", ATTN_SHAPES)
def test_attn_wide(engine, T, S, C, qk_scale, v_mean):
    """qk_terms, vt_terms, scores GEMM, softmax_pair, PV GEMM.  Flat rows (q, k ~ N(0, 0.25^2): every p ~ 1 / S) are where a split of the unscaled
    probabilities would leave 2^-25 absolute per p; peaked rows (scale 3) have few, large p.  v of mean 1: every term of a row's sum has one sign, the
    case where the order of the three terms along K shows (DESIGN.md section 3 has the measurements)."""
    qkv = attn_inputs(T, S, C, qk_scale, v_mean)
    got = engine.op_attn_wide(qkv, T, S)
    pair, pair32, truth, truth32 = attn_references(qkv, T, S)
    what = f"attention T{T} S{S} C{C} qk scale {qk_scale:g} v mean {v_mean:g}"
    check(got, pair, pair32, PAIR_FACTOR, what, "pair model")
    check(got, truth, truth32, TRUTH_FACTOR, what, "truth")
