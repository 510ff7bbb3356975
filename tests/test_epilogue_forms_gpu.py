"""The res-block and blend operands of the GEMM epilogue on every kernel family.

Every 3x3, temporal and dense launch of the UNet ends in one of the copies of

    Out = act(c0 * f(acc + bias + bias2) + c1 * R1 + c2 * R2)

(kernels/gemm_common.h: tile_epilogue vector / scalar, tile_epilogue_lean, tile_epilogue_geglu_lean, tile_epilogue_stats modes 0 / 1 / 2, the EpiPre
prefetch; kernels/gemm.hip: splitk_epilogue; kernels/conv_halo.hip: the same through the 2-D pixel mapping).  bias2 is the time-embedding row of every
res-block's conv1, R2 / c2 the AlphaBlender of the temporal feed-forward, the statistics epilogue with c0 != 1 the temporal blend convolution.  The launches
go through the engine's linear() / conv() (ug_op_linear_ex, ug_op_conv_epi) under ug_tune_force; plan = (tile config launched, split factor).

a. exact operand screen on integer data (tests/epilogue_oracle.py: EXACT_COEF, SUBSETS): equality with the integer reference;
b. fp16-representable Gaussian data, all operands, c0 = c1 = 0.3, c2 = 0.7: the derived bound of epilogue_oracle.gauss_bound, no measured constant;
c. the raw statistics partial sums against the fp16 output the same launch stored, and the launches that must decline."""
import functools

import numpy as np
import pytest

import epilogue_oracle as eo
import test_ops_gpu
from util import assert_close, report, where_differ as _where

pytestmark = pytest.mark.gpu
TOL = test_ops_gpu.TOL
SENT = 0x7FC5A5A5
FILL = -777.0               # an exact fp16 number no case computes: guard rows and surplus columns must come back with it
GUARD = 3

CFGS = [-1, 0, 1, 3, 4, 8, 12, 14, 15, 19, 34, 35, 39, 54, 59, 60, 61, 62, 63, 64]
GEGLU_CFGS = [-1, 0, 4, 8, 15, 35, 54, 62, 64]
SPLIT_CFGS = [0, 3, 59, 63]
GCOEF = dict(c0=0.3, c1=0.3, c2=0.7)


def _force(engine, cfg, split=None):
    engine.tune_force(cfg, (1 if cfg >= 0 else -1) if split is None else split)


def _f64(a):
    return np.asarray(a, np.float64)


class Problem:
    """One matrix product / convolution with everything the references need: acc (float64, no bias), optionally the product of absolute values."""

    def __init__(self, name, kind, args, acc, K, n_bias, nout, absacc=None, ldo=0, ldr1=0, ldr2=0, geglu=False, geom=None):
        self.name, self.kind, self.args, self.acc, self.K, self.n_bias, self.nout = name, kind, args, acc, K, n_bias, nout
        self.absacc, self.ldo, self.ldr1, self.ldr2, self.geglu, self.geom = absacc, ldo, ldr1, ldr2, geglu, geom
        self.rows = acc.shape[0]

    def run(self, engine, stats=False, ldo=None, **kw):
        ldo = self.ldo if ldo is None else ldo
        if self.kind == "dense":
            A, W = self.args
            return engine.op_linear_ex(A, W, geglu=self.geglu, ldo=ldo, guard=GUARD, fill=FILL, **kw)
        x, x1, w, ckw = self.args
        return engine.op_conv_epi(x, w, x1=x1, ldo=ldo, guard=GUARD, fill=FILL, stats=stats, **ckw, **kw)

    def ref(self, **kw):
        return eo.epilogue64(self.acc, geglu=self.geglu, **kw)


def _dense(name, A, W, gauss=False, **kw):
    A64, W64 = _f64(A), _f64(W)
    return Problem(name, "dense", (A, W), A64 @ W64.T, A.shape[1], W.shape[0], W.shape[0], absacc=np.abs(A64) @ np.abs(W64).T if gauss else None, **kw)


def _conv(name, x, w, x1=None, gauss=False, geom=None, ldo=0, **ckw):
    ref_kw = dict(kt=w.shape[2], k=w.shape[3], **ckw)
    acc = eo.conv_acc64(x, w, x1=x1, **ref_kw)
    absacc = eo.conv_acc64(np.abs(x), np.abs(w), x1=None if x1 is None else np.abs(x1), **ref_kw) if gauss else None
    O = w.shape[0]
    return Problem(name, "conv", (x, x1, w, ckw), acc, int(np.prod(w.shape[1:])), O, O, absacc=absacc, geom=geom, ldo=ldo)


def _check_whole(out, ref, prob, what, ldo=None):
    """The computed part equals ref; guard rows and surplus columns came back as given."""
    M, n = prob.rows, prob.nout
    assert out.shape == (M + GUARD, (prob.ldo if ldo is None else ldo) or n), out.shape
    assert np.array_equal(out[:M, :n], ref), f"{what}: {_where(out[:M, :n], ref)}"
    assert (out[M:] == FILL).all(), f"{what}: guard rows written"
    assert (out[:, n:] == FILL).all(), f"{what}: surplus columns written"


# ===================================================================================================
# a. Exact operand screen
# ===================================================================================================
@functools.lru_cache(maxsize=None)
def _exact_dense():
    """Dense shapes (M x N x K): 2049 x 640 x 1344 buffer-addressed, x 1352 the flat-address fall-back, 77 x 128 one tile, 260 x 328 lanes on the scalar
    path with every operand (N % 16 != 0), 260 x 324 the same for the 8-column lanes, ldo = ldr1 = ldr2 = 648 the strided vector path, ldo = 644 the
    scalar path of ldo % 8 != 0."""
    rng = np.random.default_rng(2801)
    out = []
    A, W = eo.tri(rng, 2049, 1344), eo.tri(rng, 640, 1344)
    out.append((_dense("dense 2049x640x1344", A, W), eo.exact_operands(rng, 2049, 640, 640)))
    out.append((_dense("dense 2049x640x1344 ld 648", A, W, ldo=648), eo.exact_operands(rng, 2049, 640, 640, 648, 648)))
    out.append((_dense("dense 2049x640x1344 ldo 644", A, W, ldo=644), eo.exact_operands(rng, 2049, 640, 640)))
    # (260 x 324: N % 8 != 0.  The tiles whose lanes hold 8 columns - 1, 3, 12, 14, 19, 34, 39, 59, 61, 63 - have no lane astride N at N = 328, so the
    # per-column bias / bias2 loop of the scalar path is theirs only here; a scratch build without bias2 in that loop passed on exactly those ten.)
    for (M, K, N) in [(2049, 1352, 640), (77, 1344, 128), (260, 1344, 328), (260, 1344, 324)]:
        out.append((_dense(f"dense {M}x{N}x{K}", eo.tri(rng, M, K), eo.tri(rng, N, K)), eo.exact_operands(rng, M, N, N)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _exact_convs():
    """The two-source 3x3 and the temporal convolution of test_tile_configs_bitwise_identical_small_ragged (2800 ragged rows), and a stride-2 one."""
    rng = np.random.default_rng(2802)
    x, x1 = eo.tri(rng, 5, 20, 28, 128), eo.tri(rng, 5, 20, 28, 64)
    w, wt = eo.tri(rng, 192, 192, 1, 3, 3), eo.tri(rng, 192, 128, 3, 1, 1)
    w128 = np.ascontiguousarray(w[:, :128])
    probs = [_conv("two-source conv3x3", x, w, x1=x1), _conv("temporal conv", x, wt, pad_t=0, pad_l=0), _conv("stride-2 conv3x3 ldo 200", x, w128, stride=2, ldo=200)]
    return tuple((p, eo.exact_operands(rng, p.rows, 192, 192)) for p in probs)


# halo-stageable 3x3 convolutions: (tile config, T, H, W, O, the geometry halo_pick_lg is left with).  256-pixel tiles: 16 x 16 (LG 4) needs H % 16 == 0 and
# W % 16 == 0; 8 x 32 (LG 5) H % 8 == 0 and W % 32 == 0; 4 x 64 (LG 6) H % 4 == 0 and W % 64 == 0; it takes the first that fits.  24 x 64 leaves LG 5,
# 20 x 64 leaves LG 6.  256 x 160 tiles are 8 x 32 only, 192-pixel tiles 12 x 16 only.
# More than 2048 rows each: below that the planner slices K (gemm_plan) and the halo kernel, which takes unsplit launches only, is not offered the launch.
HALO = {"71 LG4": (71, 2, 32, 48, 192, 4), "71 LG5": (71, 2, 24, 64, 192, 5), "71 LG6": (71, 2, 20, 64, 192, 6), "70": (70, 2, 24, 64, 320, 5),
        "72": (72, 3, 24, 32, 192, 4), "73": (73, 3, 24, 32, 160, 4)}


@functools.lru_cache(maxsize=None)
def _exact_halo(key):
    cfg, T, H, W, O, lg = HALO[key]
    rng = np.random.default_rng(2803 + H * W + O)
    p = _conv(f"halo conv3x3 {key} {T}x{H}x{W} 128->{O}", eo.tri(rng, T, H, W, 128), eo.tri(rng, O, 128, 1, 3, 3))
    return p, eo.exact_operands(rng, p.rows, O, O)


def _exact_subsets(engine, prob, ops, what, subsets=None, twice=("all five",)):
    plans = set()
    for name in subsets or eo.SUBSETS:
        kw = eo.subset_kwargs(ops, name)
        ref = eo.exact_ref(prob.acc, geglu=prob.geglu, **kw)           # asserts |ref| < 2048 and integrality
        for rep in range(2 if name in twice else 1):
            out, plan = prob.run(engine, **kw)
            _check_whole(out, ref, prob, f"{what} {prob.name} [{name}] run {rep} plan {plan}")
            plans.add(plan)
    return plans


@pytest.mark.parametrize("cfg", CFGS)
def test_exact_operand_screen_dense(engine, cfg):
    try:
        _force(engine, cfg)
        for prob, ops in _exact_dense():
            plans = _exact_subsets(engine, prob, ops, f"cfg {cfg}")
            assert cfg < 0 or all(p[0] == cfg for p in plans), plans
            report(f"epilogue exact cfg {cfg} {prob.name}", 0.0, kind="mismatches", plans=sorted(plans))
    finally:
        _force(engine, -1)


@pytest.mark.parametrize("cfg", CFGS)
def test_exact_operand_screen_conv(engine, cfg):
    try:
        _force(engine, cfg)
        for prob, ops in _exact_convs():
            plans = _exact_subsets(engine, prob, ops, f"cfg {cfg}")
            assert cfg < 0 or all(p[0] == cfg for p in plans), plans
            report(f"epilogue exact cfg {cfg} {prob.name}", 0.0, kind="mismatches", plans=sorted(plans))
    finally:
        _force(engine, -1)


@pytest.mark.parametrize("key", list(HALO))
@pytest.mark.parametrize("forced", [True, False])
def test_exact_operand_screen_halo(engine, key, forced):
    """Every instantiated halo geometry, forced and as launch_gemm picks it for the planner's launch (some halo tile then: 70 .. 73)."""
    cfg = HALO[key][0]
    prob, ops = _exact_halo(key)
    try:
        _force(engine, cfg if forced else -1)
        plans = _exact_subsets(engine, prob, ops, f"halo {key} forced {forced}")
        assert all((p[0] == cfg) if forced else (70 <= p[0] <= 73) for p in plans) and all(p[1] == 1 for p in plans), plans
        report(f"epilogue exact halo {key} {'forced' if forced else 'planner'} {prob.name}", 0.0, kind="mismatches", plans=sorted(plans))
    finally:
        _force(engine, -1)


@pytest.mark.parametrize("cfg", SPLIT_CFGS)
@pytest.mark.parametrize("split", [2, 5])
def test_exact_operand_screen_splitk(engine, cfg, split):
    """splitk_epilogue carries its own bias2 / R2."""
    probs = [_exact_dense()[i] for i in (0, 3, 4)] + list(_exact_convs()[:2])
    try:
        _force(engine, cfg, split)
        for prob, ops in probs:
            plans = _exact_subsets(engine, prob, ops, f"cfg {cfg} split {split}", subsets=("all five", "bias2 alone", "R2 alone", "bias2 without bias"))
            assert plans == {(cfg, split)}, plans
            report(f"epilogue exact cfg {cfg} split {split} {prob.name}", 0.0, kind="mismatches", plans=sorted(plans))
    finally:
        _force(engine, -1)


def test_planner_reaches_splitk_epilogue_with_bias2_and_r2(engine):
    """The planner's own split of a small dense launch (77 x 128 x 1344) carries every operand through splitk_epilogue."""
    prob, ops = _exact_dense()[4]
    plans = _exact_subsets(engine, prob, ops, "planner")
    assert all(p[1] > 1 for p in plans), plans


# ---- GEGLU with bias2.  W, bias, bias2 in checkpoint order [values | gates].  Zero gate weights make the gate column a constant g = bias + bias2:
#   g = 0:  geglu(h, 0) = 0, the output is c1 R1 + c2 R2 exactly - the residual columns are those of the N / 2 outputs (residuals given with ld = N, surplus
#           columns filled: a kernel that takes them at the GEMM's column comes out with another integer);
#   g = 16: exp(-g^2 / 2) underflows to 0 in fp32, Phi(g) = 1 exactly in the kernels' erfc form and in float64 alike: geglu(h, 16) = 16 h, exact.  This is the
#           case that sees bias2 on the value columns - with residuals through tile_epilogue, without (c0 = 1) through tile_epilogue_geglu_lean.
@functools.lru_cache(maxsize=None)
def _geglu_problem(gate, gauss=False):
    rng = np.random.default_rng(2810 + int(gate))
    M, K, N = 260, 320, 512
    if gauss:
        A, W = eo.gauss(rng, M, K), eo.gauss(rng, N, K, scale=K ** -0.5)
        ops = dict(bias=eo.gauss(rng, N), bias2=eo.gauss(rng, N), R1=eo.gauss(rng, M, N), R2=eo.gauss(rng, M, N))
    else:
        A, W = eo.tri(rng, M, K), eo.tri(rng, N, K)
        W[N // 2:] = 0
        ops = eo.exact_operands(rng, M, N, N // 2, N, N)
        ops["bias"][N // 2:] = gate; ops["bias2"][N // 2:] = 0
    p = _dense(f"GEGLU {M}x{N}x{K} gate {gate}", A, W, gauss=gauss, geglu=True)
    p.nout = N // 2
    return p, ops


@pytest.mark.parametrize("cfg", GEGLU_CFGS)
def test_geglu_with_bias2_and_residuals(engine, cfg):
    try:
        _force(engine, cfg)
        for gate in (0.0, 16.0):
            prob, ops = _geglu_problem(gate)
            plans = _exact_subsets(engine, prob, ops, f"cfg {cfg}", subsets=("all five", "R1 with R2", "bias2 without bias", "lean bias + bias2"))
            assert cfg < 0 or all(p[0] == cfg for p in plans), plans
            if gate == 0.0:
                kw = eo.subset_kwargs(ops, "all five")
                assert np.array_equal(prob.ref(**kw), -1.0 * ops["R1"][:, :prob.nout] + 0.5 * ops["R2"][:, :prob.nout])
            report(f"epilogue exact GEGLU cfg {cfg} {prob.name}", 0.0, kind="mismatches", plans=sorted(plans))
        prob, ops = _geglu_problem(1.0, gauss=True)
        for name, kw in (("bias2, lean", dict(bias=ops["bias"], bias2=ops["bias2"])), ("all operands", dict(**ops, **GCOEF))):
            out, plan = prob.run(engine, **kw)
            assert_close(out[:prob.rows, :prob.nout], prob.ref(**kw), TOL, f"epilogue GEGLU Gaussian cfg {cfg} [{name}] plan {plan}")
            assert (out[prob.rows:] == FILL).all()
    finally:
        _force(engine, -1)


def test_streaming_gemm_steps_aside_for_bias2_and_r2(engine):
    """16384 x 320 x 320 is the streaming kernel's (config 80): with bias + R1 it takes the launch, with bias2 or R2 - which it does not implement - it must not."""
    rng = np.random.default_rng(2820)
    M, K, N = 16384, 320, 320
    prob = _dense("dense 16384x320x320", eo.tri(rng, M, K), eo.tri(rng, N, K))
    ops = eo.exact_operands(rng, M, N, N)
    for name, aside in (("lean bias + bias2 + R1", True), ("bias2 alone", True), ("R2 alone", True), ("all five", True)):
        (plan,) = _exact_subsets(engine, prob, ops, "planner", subsets=(name,), twice=())
        assert (plan[0] != 80) == aside, f"[{name}] launched {plan}"
        report(f"epilogue exact streaming shape [{name}]", 0.0, kind="mismatches", plans=[plan])
    kw = dict(bias=ops["bias"], R1=ops["R1"])
    out, plan = prob.run(engine, **kw)
    _check_whole(out, eo.exact_ref(prob.acc, **kw), prob, f"streaming control plan {plan}")
    assert plan == (80, 1), f"the control launch (bias + R1) did not reach the streaming kernel: {plan}"


# ===================================================================================================
# b. Gaussian data, all operands, the derived bound
# ===================================================================================================
@functools.lru_cache(maxsize=None)
def _gauss_problems():
    rng = np.random.default_rng(2830)
    g = eo.gauss

    def ops(rows, N, ld1=0, ld2=0):
        return dict(bias=g(rng, N), bias2=g(rng, N), R1=g(rng, rows, ld1 or N), R2=g(rng, rows, ld2 or N))
    out = []
    for (M, K, N, ld) in [(260, 1352, 328, 0), (2049, 1344, 640, 648)]:
        p = _dense(f"dense {M}x{N}x{K}" + (f" ld {ld}" if ld else ""), g(rng, M, K), g(rng, N, K, scale=K ** -0.5), gauss=True, ldo=ld)
        out.append((p, ops(M, N, ld, ld)))
    x, x1 = g(rng, 5, 20, 28, 128), g(rng, 5, 20, 28, 64)
    for p in (_conv("two-source conv3x3", x, g(rng, 192, 192, 1, 3, 3, scale=(9 * 192) ** -0.5), x1=x1, gauss=True),
              _conv("temporal conv", x, g(rng, 192, 128, 3, 1, 1, scale=(3 * 128) ** -0.5), gauss=True, pad_t=0, pad_l=0)):
        out.append((p, ops(p.rows, 192)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _gauss_halo(key):
    cfg, T, H, W, O, lg = HALO[key]
    rng = np.random.default_rng(2840 + H * W + O)
    p = _conv(f"halo conv3x3 {key}", eo.gauss(rng, T, H, W, 128), eo.gauss(rng, O, 128, 1, 3, 3, scale=(9 * 128) ** -0.5), gauss=True)
    return p, dict(bias=eo.gauss(rng, O), bias2=eo.gauss(rng, O), R1=eo.gauss(rng, p.rows, O), R2=eo.gauss(rng, p.rows, O))


def _gauss_check(engine, prob, ops, what):
    kw = dict(**ops, **GCOEF)
    out, plan = prob.run(engine, **kw)
    M, n = prob.rows, prob.nout
    ex = eo.gauss_excess(out[:M, :n], prob.ref(**kw), eo.epilogue_mag(prob.absacc, **kw), prob.K)
    report(f"epilogue gauss {what} {prob.name}", ex, tol=1.0, kind="max|err|/bound", plan=plan)
    assert ex <= 1.0, f"{what} {prob.name} plan {plan}: {ex:.3g} x the bound"
    assert (out[M:] == FILL).all() and (out[:, n:] == FILL).all(), f"{what} {prob.name}: guard rows / surplus columns written"
    return plan


@pytest.mark.parametrize("cfg", CFGS)
def test_gaussian_all_operands_tight_bound(engine, cfg):
    try:
        _force(engine, cfg)
        for prob, ops in _gauss_problems():
            plan = _gauss_check(engine, prob, ops, f"cfg {cfg}")
            assert cfg < 0 or plan[0] == cfg, plan
        prob, ops = _gauss_problems()[0]
        for act in (1, 2):           # SiLU / GELU: the hardware reciprocal and exponent have no bound one can derive - the project's TOL
            kw = dict(**ops, **GCOEF, act=act)
            out, plan = prob.run(engine, **kw)
            assert_close(out[:prob.rows, :prob.nout], prob.ref(**kw), TOL, f"epilogue gauss cfg {cfg} act {act} {prob.name}")
    finally:
        _force(engine, -1)


@pytest.mark.parametrize("key", list(HALO))
def test_gaussian_all_operands_tight_bound_halo(engine, key):
    prob, ops = _gauss_halo(key)
    try:
        _force(engine, HALO[key][0])
        assert _gauss_check(engine, prob, ops, f"halo {key}") == (HALO[key][0], 1)
    finally:
        _force(engine, -1)


@pytest.mark.parametrize("cfg", SPLIT_CFGS)
def test_gaussian_all_operands_tight_bound_splitk(engine, cfg):
    """Each slice adds at most ceil(K / split) products and splitk_epilogue adds the `split` partial sums: no more than K additions for split <= 5, K >= 384."""
    try:
        for split in (2, 5):
            _force(engine, cfg, split)
            for prob, ops in _gauss_problems()[1:]:
                assert _gauss_check(engine, prob, ops, f"cfg {cfg} split {split}") == (cfg, split)
    finally:
        _force(engine, -1)


# ===================================================================================================
# c. The statistics epilogue, raw
# ===================================================================================================
RB = {14: 64, 19: 128, 35: 128, 54: 64, 59: 128, 63: 96, 64: 48, 71: 64, 72: 48}       # rows of the wave tile = rows per statistics block
BM = {14: 256, 19: 256, 35: 256, 54: 256, 59: 256, 63: 192, 64: 192, 71: 256, 72: 192}
# (family id, tile config, convolutions): every general tile on a 3x3 and on temporal convolutions of T = 3 and 5 frames with HW % bm == 0 (768 = 3 x 256 = 4 x 192:
# the frame-fastest walk engages, and again with knob 256, which turns it off); the halo tiles on their geometries (3x3 only)
STAT_FAMILIES = [(str(c), c, ("3x3", "T3", "T5", "T3 knob256", "T5 knob256")) for c in (14, 19, 35, 54, 59, 63, 64)] + \
                [("71 LG4", 71, ("halo",)), ("71 LG5", 71, ("halo",)), ("71 LG6", 71, ("halo",)), ("72", 72, ("halo",))]


@functools.lru_cache(maxsize=None)
def _stat_problem(which, gauss, fam=None):
    """64 -> 128 channels: 3x3 (K = 576) on 2 x 32 x 96, temporal (K = 192) on T x 24 x 32, halo 3x3 on the geometry's shape."""
    rng = np.random.default_rng(2850 + sum(map(ord, which + str(fam))) + gauss)
    gen = (lambda *s: eo.gauss(rng, *s)) if gauss else (lambda *s: eo.tri(rng, *s))
    C, O = 64, 128
    if which.startswith("T"):
        T = int(which[1])
        x, w, ckw, geom = gen(T, 24, 32, C), gen(O, C, 3, 1, 1), dict(pad_t=0, pad_l=0), (T, 24, 32)
        scale = (3 * C) ** -0.5
    else:
        T, H, W = (2, 32, 96) if which == "3x3" else HALO[fam][1:4]
        x, w, ckw, geom = gen(T, H, W, C), gen(O, C, 1, 3, 3), {}, (T, H, W)
        scale = (9 * C) ** -0.5
    if gauss:
        w = eo.h16(w * scale)
    p = _conv(f"{which} {geom[0]}x{geom[1]}x{geom[2]} {C}->{O}", x, w, gauss=False, geom=geom, **ckw)
    rows = p.rows
    if gauss:
        ops = dict(bias=eo.gauss(rng, O), bias2=eo.gauss(rng, O), R1=eo.gauss(rng, rows, O), R2=eo.gauss(rng, rows, O))
    else:
        ops = eo.exact_operands(rng, rows, O, O)
    return p, ops


def _stat_forms(ops, gauss):
    """(name, operands + coefficients).  Modes 2 / 1: c0 = c1 = 1 without / with R1; mode 0: c0 != 1 with R1 and c1 = 1 (the temporal blend convolution's
    form - c0 = 0.6 on Gaussian data, 2 on integer data), with R2, with SiLU (Gaussian data only); each without and with bias2."""
    b, b2, r1, r2 = ops["bias"], ops["bias2"], ops["R1"], ops["R2"]
    forms = [("mode 2", dict(bias=b)), ("mode 1", dict(bias=b, R1=r1)),
             ("mode 0 blend", dict(bias=b, R1=r1, c0=0.6 if gauss else 2.0, c1=1.0)),
             ("mode 0 R2", dict(bias=b, R1=r1, R2=r2, c2=0.7 if gauss else 0.5))]
    if gauss:
        forms.append(("mode 0 SiLU", dict(bias=b, R1=r1, act=1)))
    return [(n + s, dict(kw, **({"bias2": b2} if s else {}))) for n, kw in forms for s in ("", " + bias2")]


def _block_of_row(fam, cfg, prob):
    T, H, W = prob.geom
    if cfg in (71, 72):
        return eo.halo_block_of_row(T, H, W, BM[cfg], HALO[fam][5], RB[cfg])
    return eo.consecutive_block_of_row(prob.rows, RB[cfg])


def _stat_run(engine, fam, cfg, which, gauss):
    prob, ops = _stat_problem(which.split()[0], gauss, fam if which == "halo" else None)
    T, H, W = prob.geom
    knob = "knob256" in which
    worst = (0.0, 0.0)
    try:
        _force(engine, cfg)
        if knob:
            engine.tune_force(-100 - 256, 0)
        forms = _stat_forms(ops, gauss)
        if gauss:       # a column that is constant over a frame (zero weights): the rounding errors of its rows add up coherently - statistics taken before the rounding to fp16 miss this bound 15 - 40 x
            zero = Problem(prob.name + " zero weights", "conv", (prob.args[0], None, 0 * prob.args[2], prob.args[3]), 0 * prob.acc, prob.K, 128, 128, geom=prob.geom)
            forms.append(("mode 0 column-constant", dict(bias=ops["bias"], bias2=ops["bias2"], c0=0.6)))
        for name, kw in forms:
            pr = zero if name.endswith("column-constant") else prob
            what = f"stats {fam} {which} [{name}]"
            out, plan, rb, part = pr.run(engine, stats=True, **kw)
            assert plan == (cfg, 1), f"{what}: launched {plan}"
            assert rb == RB[cfg], f"{what}: rows per statistics block {rb}, expected {RB[cfg]}"
            plain, plan2 = pr.run(engine, **kw)
            assert plan2 == plan and np.array_equal(out, plain), f"{what}: the statistics epilogue changed the output: {_where(out, plain)}"
            o16 = out[:pr.rows]
            if gauss:
                assert_close(o16, pr.ref(**kw), TOL, "")
            else:
                _check_whole(out, eo.exact_ref(pr.acc, **kw), pr, what)
            ex = eo.check_stats(part, rb, o16, T, H * W, SENT, not gauss, _block_of_row(fam, cfg, pr), what=what)
            worst = (max(worst[0], ex[0]), max(worst[1], ex[1]))
    finally:
        if knob:
            engine.tune_force(-100, 0)
        _force(engine, -1)
    return worst


@pytest.mark.parametrize("fam,cfg,convs", STAT_FAMILIES, ids=[f[0] for f in STAT_FAMILIES])
def test_statistics_raw_exact_on_integer_data(engine, fam, cfg, convs):
    for which in convs:
        _stat_run(engine, fam, cfg, which, False)
        report(f"epilogue stats exact {fam} {which}", 0.0, kind="mismatches", plan=(cfg, 1), rb=RB[cfg])


@pytest.mark.parametrize("fam,cfg,convs", STAT_FAMILIES, ids=[f[0] for f in STAT_FAMILIES])
def test_statistics_raw_gaussian_bound(engine, fam, cfg, convs):
    for which in convs:
        ex_f, ex_b = _stat_run(engine, fam, cfg, which, True)
        report(f"epilogue stats gauss per-frame {fam} {which}", ex_f, tol=1.0, kind="max|err|/bound", plan=(cfg, 1), rb=RB[cfg])
        report(f"epilogue stats gauss per-block {fam} {which}", ex_b, tol=1.0, kind="max|err|/bound", plan=(cfg, 1), rb=RB[cfg])


@pytest.mark.parametrize("case", ["M % bm != 0", "forced split", "ldo % 8 != 0", "stat_hw % rb != 0"])
def test_statistics_launches_that_must_decline(engine, case):
    """rb = 0, the statistics area untouched, the output right (tile 59: 256 x 128, blocks of 128 rows)."""
    rng = np.random.default_rng(2860)
    T, H, W = {"M % bm != 0": (1, 20, 28), "stat_hw % rb != 0": (4, 12, 16)}.get(case, (2, 32, 48))
    prob = _conv(f"3x3 {T}x{H}x{W} 64->128", eo.tri(rng, T, H, W, 64), eo.tri(rng, 128, 64, 1, 3, 3), ldo=132 if case.startswith("ldo") else 0)
    ops = eo.exact_operands(rng, prob.rows, 128, 128)
    kw = dict(bias=ops["bias"], bias2=ops["bias2"], R1=ops["R1"], c0=2.0, c1=1.0)
    split = 2 if case == "forced split" else 1
    try:
        _force(engine, 59, split)
        if case not in ("M % bm != 0",):
            assert prob.rows % 256 == 0
        out, plan, rb, part = prob.run(engine, stats=True, **kw)
    finally:
        _force(engine, -1)
    assert plan == (59, 1 if case.startswith("ldo") else split), plan       # (a forced factor applies to 8-aligned leading dimensions only: gemm_plan)
    assert rb == 0, f"{case}: the launch reported blocks of {rb} rows"
    assert (part.view(np.uint32) == SENT).all(), f"{case}: {(part.view(np.uint32) != SENT).sum()} statistics words written by a launch that declined"
    _check_whole(out, eo.exact_ref(prob.acc, **kw), prob, case)


def test_bad_calls_leave_the_context_usable(engine):
    rng = np.random.default_rng(2870)
    A, W = eo.tri(rng, 16, 64), eo.tri(rng, 32, 64)
    with pytest.raises(RuntimeError):
        engine.op_linear_ex(A[:, :60], W[:, :60])                      # K % 8 != 0
    with pytest.raises(RuntimeError):
        engine.op_linear_ex(A, W, R1=eo.tri(rng, 16, 24))             # residual rows narrower than the output
    with pytest.raises(RuntimeError):
        engine.op_conv_epi(eo.tri(rng, 1, 8, 8, 64), eo.tri(rng, 32, 64, 1, 3, 3), ldo=24)
    try:
        engine.set_fp8_linears(True)
        with pytest.raises(RuntimeError):
            engine.op_linear_ex(A, W)                                  # the fp16 path only
    finally:
        engine.set_fp8_linears(False)
    out, _ = engine.op_linear_ex(A, W)
    assert np.array_equal(out, A @ W.T)
