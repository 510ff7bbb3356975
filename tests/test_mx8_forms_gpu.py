"""The MX-fp8 quantiser, the scaled GEMM and the engine's fp8 linear() op by op.

References and generators live in tests/mx8_oracle.py and are pinned on the CPU by tests/test_mx8_oracle_cpu.py: util.mx8_quantise (checked against
torch's float8_e4m3fn on every fp16 value in range) and a float64 product of the dequantised operands.

  * quantiser: bytes and exponents bit for bit on the edge matrix (every e4m3 tie, the saturation band, subnormals, signed zeros, fp16-subnormal and
    65504 block maxima), with row strides, scale strides, guards, small M and a second grid-stride lap;
  * GEMM: on the exact screen - integers times a per-(row, block) power of two, five exponents - fp16(float64 reference) is the only admissible output, so a
    scale taken from the wrong row, block, K step, tile or ring slot changes thousands of outputs.  Every case runs over a workspace filled with 0xFF
    (e8m0 NaN in every scale dword the quantiser does not write), on each of the four tile shapes and the planner's pick;
  * epilogue forms the engine sends through launch_gemm_mx8, exact where the coefficients allow it, Gaussian with a derived bound where they do not;
  * the engine's own quant_lin() / linear() / ln_linear() rules.
"""
import numpy as np
import pytest
import torch

import mx8_oracle as mo
from util import assert_close, h16, mx8_quantise, rel_err, report, where_differ

pytestmark = pytest.mark.gpu

PICKS = (None, 0, 1, 2, 3)                      # planner, then 256x256, 256x128, 128x128, 192x128
TILE = {0: (256, 256, 256), 1: (256, 128, 256), 2: (128, 128, 512), 3: (192, 128, 256)}      # pick -> (BM, BN, persistent workgroups)
SENT = 777.0                                    # what the output buffer holds where no kernel may write


def pad256(n):
    return (n + 255) // 256 * 256


class forced:
    """ug_tune_force(100 + pick) for the block; None = the planner."""

    def __init__(self, engine, pick):
        self.engine, self.pick = engine, pick

    def __enter__(self):
        if self.pick is not None:
            self.engine.tune_force(100 + self.pick, -1)

    def __exit__(self, *exc):
        self.engine.tune_force(-1, -1)


def same_bits(got, ref, what):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{what}: {where_differ(got, ref)}"


# ---------------------------------------------------------------------------------------------------------------- quantiser
def quant_check(engine, x, M, K, ldx, ld_s, guard=3):
    """x [M, K] through the quantiser with row stride ldx and scale stride ld_s; everything around what it may touch is planted and checked."""
    xin = np.full((M + guard, ldx), 60000.0, np.float32)          # surplus columns and guard rows: a read of them would move a block maximum
    xin[:M, :K] = x
    q0 = np.full((M + guard, K), 0xA5, np.uint8)
    s0 = np.full((K // 128, ld_s), 0xDEADBEEF, np.uint32)
    q, s = engine.op_quant_mx8_ex(xin, M, K, q0, s0)
    _, bytes_ref, e_ref = mx8_quantise(x)
    bad = np.argwhere(q[:M] != bytes_ref)
    assert len(bad) == 0, (f"{len(bad)} bytes differ, first at {tuple(bad[0])}: x = {x[tuple(bad[0])]!r}, got {q[tuple(bad[0])]:#x}, "
                           f"expected {bytes_ref[tuple(bad[0])]:#x}")
    assert (q[M:] == 0xA5).all(), "guard rows of the byte buffer were written"
    want = mo.scale_dwords(e_ref, ld_s, s0)
    bad = np.argwhere(s != want)
    assert len(bad) == 0, f"{len(bad)} scale dwords differ, first at (K step, row) {tuple(bad[0])}: got {s[tuple(bad[0])]:#x}, expected {want[tuple(bad[0])]:#x}"


@pytest.mark.parametrize("K", [128, 256, 640])
@pytest.mark.parametrize("stride", ["tight", "ldx+8", "ldx+136"])
def test_quantiser_edge_matrix(engine, K, stride):
    x = mo.edge_matrix(K)
    M = x.shape[0]
    ldx, ld_s = {"tight": (K, M), "ldx+8": (K + 8, M + 4), "ldx+136": (K + 136, pad256(M))}[stride]
    quant_check(engine, x, M, K, ldx, ld_s)


@pytest.mark.parametrize("M", [1, 7, 8, 9, 63, 65, 255, 257])
def test_quantiser_small_row_counts(engine, M):
    """Row counts around the 8 rows a wave's 64 lanes cover at K = 128 and around the 256-row scale padding; the tail lanes of the last wave clamp to the
    last item and must not store."""
    for K in (128, 256, 640):
        full = mo.edge_matrix(K)
        rows = np.random.default_rng([M, K]).choice(full.shape[0], M, replace=M > full.shape[0])
        for ld_s in sorted({M, M + 4, pad256(M)}):
            quant_check(engine, full[rows], M, K, K + 8, ld_s)


def test_quantiser_second_grid_stride_lap(engine):
    """The launch caps its grid at 16384 blocks of 256 items (16 elements each): more than 16384 * 256 = 4194304 items make the loop run a second lap.
    That takes M * K > 67.1 M elements - M = 135000 at K = 512 is 4320000 items.  (M = 8200 at K = 512 is 262400 items and stays inside one lap.)
    The rows repeat a 101-row pattern of edge blocks, so the reference is computed once on the pattern; 101 is prime and the lap boundary falls at
    row 131072, so no period of the data coincides with the stride of the loop."""
    M, K, P = 135000, 512, 101
    assert M * (K // 128) * 8 > 16384 * 256
    full = mo.edge_matrix(K)
    base = full[np.random.default_rng(3).choice(full.shape[0], P, replace=False)]
    x = np.tile(base, ((M + P - 1) // P, 1))[:M]
    guard = 2
    xin = np.concatenate([x, np.full((guard, K), 60000.0, np.float32)])
    q, s = engine.op_quant_mx8_ex(xin, M, K, np.full((M + guard, K), 0xA5, np.uint8), np.full((K // 128, M), 0xDEADBEEF, np.uint32))
    _, b_ref, e_ref = mx8_quantise(base)
    rep = (M + P - 1) // P
    assert np.array_equal(q[:M], np.tile(b_ref, (rep, 1))[:M]) and (q[M:] == 0xA5).all()
    assert np.array_equal(s, mo.scale_dwords(np.tile(e_ref, (rep, 1))[:M], M))


def test_bad_calls_return_errors_and_leave_the_context_usable(engine):
    M, K = 16, 128
    x = np.ones((M, K), np.float32)
    q, s = np.zeros((M, K), np.uint8), np.zeros((K // 128, M), np.uint32)
    with pytest.raises(RuntimeError):      # K % 128 != 0
        engine.op_quant_mx8_ex(np.ones((M, 192), np.float32), M, 192, np.zeros((M, 192), np.uint8), np.zeros((1, M), np.uint32))
    with pytest.raises(RuntimeError):      # ldx % 8 != 0
        engine.op_quant_mx8_ex(np.ones((M, K + 4), np.float32), M, K, q, s)
    with pytest.raises(RuntimeError):      # ld_s < M
        engine.op_quant_mx8_ex(x, M, K, q, np.zeros((1, M - 1), np.uint32))
    with pytest.raises(RuntimeError):      # GEGLU with N % 128 != 0
        engine.op_linear_mx8_ex(np.ones((256, K), np.float32), np.ones((192, K), np.float32), geglu=True)
    with pytest.raises(RuntimeError):      # the GEMM's own K rule
        engine.op_linear_mx8_ex(np.ones((256, 192), np.float32), np.ones((128, 192), np.float32))
    quant_check(engine, mo.edge_matrix(K)[:M], M, K, K, M)
    c = mo.exact_case(129, 8, 128)
    out, _ = engine.op_linear_mx8_ex(c["A"], c["W"])
    same_bits(out, h16(c["prod"]), "after the bad calls")


# ---------------------------------------------------------------------------------------------------------------- GEMM, exact screen
def gemm_exact_check(engine, c, what, picks=PICKS, want_plan=None, **form):
    """One exact case on every pick over the poisoned workspace: the output equals fp16(ref64) bit for bit, the guard rows and the columns [N, ldo) keep
    their sentinel, and (therefore, and checked on its own) the picks agree with each other."""
    M, N = c["A"].shape[0], c["W"].shape[0]
    flags = {k: form.get(k, False) for k in ("bias", "R1", "R2")}
    coef = {k: form.get(k, 1.0) for k in ("c0", "c1", "c2")}
    ref = h16(mo.exact_ref(c, **flags, **coef))
    wide = form.get("wide", 8)
    first = None
    for pick in picks:
        buf = np.full((M + 2, N + wide), SENT, np.float32)
        with forced(engine, pick):
            out, plan = engine.op_linear_mx8_ex(c["A"], c["W"], bias=c["bias"] if flags["bias"] else None, R1=c["R1"] if flags["R1"] else None,
                                                R2=c["R2"] if flags["R2"] else None, **coef, out=buf, guard=2, poison=True)
        tag = f"{what}, pick {pick} (launched {plan})"
        if pick is not None:
            assert plan[0] == pick, tag
        if want_plan is not None:
            want_plan(plan, tag)
        same_bits(out[:M, :N], ref, tag)
        assert (out[M:] == SENT).all() and (out[:, N:] == SENT).all(), f"{tag}: guard rows or columns [N, ldo) were written"
        if first is None:
            first = out
        assert np.array_equal(out, first), f"{tag}: differs from pick {picks[0]}"


@pytest.mark.parametrize("M", mo.EXACT_MS)
def test_gemm_exact_screen(engine, M):
    """M around every tile height (128, 192, 256) and, at 385 and 449 on the 192-row tile, a last tile that reaches past round_up(M, 256) = 512 rows of
    scales; N below one MFMA column group, ragged against 128 and 256; K of one step, a wrap of the two-slot ring and of the three-slot ring."""
    for N in mo.EXACT_NS:
        for K in mo.EXACT_KS:
            gemm_exact_check(engine, mo.exact_case(M, N, K), f"exact {M}x{N}x{K}", wide=8 if K in (128, 384) else 0)


def test_gemm_exact_more_than_one_tile_per_workgroup(engine):
    M, N, K = mo.EXACT_WALK
    c = mo.exact_case(M, N, K)

    def walks(plan, tag):
        bm, bn, wgs = TILE[plan[0]]
        assert -(-M // bm) * -(-N // bn) > wgs, f"{tag}: every workgroup has one tile only"
    gemm_exact_check(engine, c, f"exact {M}x{N}x{K}", want_plan=walks, wide=0)


def test_gemm_exact_grouped_walk_with_ragged_tile_rows(engine):
    M, N, K = mo.EXACT_GROUPED
    c = mo.exact_case(M, N, K)

    def grouped(plan, tag):
        assert plan[1] > 1 and -(-M // TILE[plan[0]][0]) % plan[1] != 0, f"{tag}: not a grouped walk over a ragged tile-row count"
    gemm_exact_check(engine, c, f"exact {M}x{N}x{K}", want_plan=grouped, wide=0)


def test_gemm_2500_rows_on_the_192_row_tile(engine):
    """M = 2500: the 192-row tile's last tile ends at row 2687 against 2560 rows of scales."""
    gemm_exact_check(engine, mo.exact_case(2500, 136, 256), "exact 2500x136x256", picks=(3, 2))


# ---------------------------------------------------------------------------------------------------------------- epilogue forms
@pytest.mark.parametrize("form", list(mo.EPI_FORMS))
@pytest.mark.parametrize("shape", [(257, 136, 384), (449, 264, 256)])
def test_epilogue_forms_exact(engine, form, shape):
    """bias, none, R1, R1 with c1 != 1, R1 + R2 with c0, c1, c2 - integers and powers of two, so the fp32 epilogue is exact too; tight rows and
    ldr1 = N + 8, ldr2 = N + 8, ldo = N + 24 (what the vector path takes) and ldo = N + 4 (what sends it to the scalar path)."""
    bias, R1, R2, c0, c1, c2 = mo.EPI_FORMS[form]
    for wide_r, wide_o in ((0, 0), (8, 24), (0, 4)):
        c = mo.exact_case(*shape, epilogue=True, wide=wide_r)
        gemm_exact_check(engine, c, f"{form} {shape} ldr +{wide_r} ldo +{wide_o}", bias=bias, R1=R1, R2=R2, c0=c0, c1=c1, c2=c2, wide=wide_o)


def gauss_ref(g, geglu=False):
    y = mx8_quantise(g["A"])[0].astype(np.float64) @ mx8_quantise(g["W"])[0].astype(np.float64).T + g["bias"]
    if not geglu:
        return y
    n = y.shape[1] // 2
    return y[:, :n] * torch.nn.functional.gelu(torch.from_numpy(y[:, n:])).numpy()


def test_blend_epilogue_gaussian(engine):
    """c0 * (A W^T + b) + c1 * R1 + c2 * R2 with c0 = c1 = 1 - alpha, c2 = alpha (the temporal blocks' mix), alpha = 0.3: not exact.  Bound: twice the
    error of fp16(ref64) against ref64 on the same data - the reference's own output rounding, doubled for the fp32 summation order."""
    M, N, K, alpha = 300, 256, 640, 0.3
    g = mo.gauss_case(M, N, K)
    ref = (1 - alpha) * gauss_ref(g) + (1 - alpha) * g["R1"] + alpha * g["R2"]
    own = report(f"MX-fp8 blend epilogue {M}x{N}x{K}: fp16(ref64) vs ref64 (reference only)", rel_err(h16(ref), ref))
    first = None
    for pick in PICKS:
        with forced(engine, pick):
            out, _ = engine.op_linear_mx8_ex(g["A"], g["W"], bias=g["bias"], R1=g["R1"], R2=g["R2"], c0=1 - alpha, c1=1 - alpha, c2=alpha)
        assert_close(out, ref, 2 * own, f"MX-fp8 blend epilogue {M}x{N}x{K}, pick {pick}")
        first = out if first is None else first
        assert np.array_equal(out, first), f"pick {pick} differs from the planner's"


@pytest.mark.parametrize("N", [128, 384])
def test_geglu_epilogue_gaussian(engine, N):
    """Measured against the 7e-4 of tests/test_fp8_gpu.py: 1.38e-4 at N = 128 and 3.06e-4 at N = 384, on every pick, each equal to the error of
    fp16(ref64) itself on the same data.  At N = 128 that is more than 4x below 7e-4, so the bound here is the derived one - twice the reference's own
    output rounding, as for the blend - and never above 7e-4."""
    M, K = 300, 640
    g = mo.gauss_case(M, N, K)
    ref = gauss_ref(g, geglu=True)
    own = report(f"MX-fp8 GEGLU epilogue {M}x{N}x{K}: fp16(ref64) vs ref64 (reference only)", rel_err(h16(ref), ref))
    tol = min(7e-4, 2 * own)
    first = None
    for pick in PICKS:
        buf = np.full((M + 2, N // 2 + 8), SENT, np.float32)
        with forced(engine, pick):
            out, _ = engine.op_linear_mx8_ex(g["A"], g["W"], bias=g["bias"], geglu=True, out=buf, guard=2)
        assert_close(out[:M, :N // 2], ref, tol, f"MX-fp8 GEGLU epilogue {M}x{N}x{K}, pick {pick}")
        assert (out[M:] == SENT).all() and (out[:, N // 2:] == SENT).all()
        first = out if first is None else first
        assert np.array_equal(out, first), f"pick {pick} differs from the planner's"


# ---------------------------------------------------------------------------------------------------------------- the engine's linear()
@pytest.fixture
def fp8(engine):
    engine.set_fp8_linears(True)
    yield engine
    engine.set_fp8_linears(False)
    engine.tune_force(-1, -1)


def test_linear_row_threshold(fp8):
    """M = 255 stays on the fp16 GEMM although the weight has its MX-fp8 copy; M = 256 takes the MX path."""
    g = mo.gauss_case(256, 192, 256)
    A, W, b, R1 = g["A"], g["W"], g["bias"], g["R1"]
    out, info = fp8.op_linear_engine(A[:255], W, bias=b, R1=R1[:255])
    assert info == (1, 0, 0), info
    same_bits(out, fp8.op_linear(A[:255], W, bias=b, R1=R1[:255]), "M = 255 with fp8 on vs ug_op_linear")
    out, info = fp8.op_linear_engine(A, W, bias=b, R1=R1)
    assert info == (1, 1, 0), info
    same_bits(out, fp8.op_linear_mx8_ex(A, W, bias=b, R1=R1)[0], "M = 256 with fp8 on vs ug_op_linear_mx8_ex")
    fp8.set_fp8_linears(False)
    out, info = fp8.op_linear_engine(A, W, bias=b, R1=R1)
    assert info == (1, 0, 0), info
    same_bits(out, fp8.op_linear(A, W, bias=b, R1=R1), "fp8 off vs ug_op_linear")


@pytest.mark.parametrize("K,N", [(192, 128), (256, 56)])
def test_quant_lin_rule_keeps_fp16(fp8, K, N):
    """in % 128 != 0 or out < 64: quant_lin binds no MX-fp8 weight and linear() stays on the fp16 GEMM."""
    g = mo.gauss_case(300, N, K)
    out, info = fp8.op_linear_engine(g["A"], g["W"], bias=g["bias"])
    assert info == (0, 0, 0), info
    same_bits(out, fp8.op_linear(g["A"], g["W"], bias=g["bias"]), f"in = {K}, out = {N}")


def test_linear_row_stride(fp8):
    M, N, K = 385, 136, 256
    c = mo.exact_case(M, N, K, epilogue=True)
    A = np.full((M, K + 64), 60000.0, np.float32)
    A[:, :K] = c["A"]
    buf = np.full((M + 2, N + 8), SENT, np.float32)
    out, info = fp8.op_linear_engine(A, c["W"], bias=c["bias"], out=buf, guard=2)
    assert info == (1, 1, 0), info
    same_bits(out[:M, :N], h16(mo.exact_ref(c, bias=True)), "lda = K + 64")
    assert (out[M:] == SENT).all() and (out[:, N:] == SENT).all()


@pytest.mark.parametrize("form", list(mo.EPI_FORMS))
def test_linear_epilogue_forms_exact(fp8, form):
    bias, R1, R2, c0, c1, c2 = mo.EPI_FORMS[form]
    M, N, K = 385, 136, 384
    for pick in (None, 3):
        for wide in (0, 8):
            c = mo.exact_case(M, N, K, epilogue=True, wide=wide)
            buf = np.full((M + 2, N + wide), SENT, np.float32)
            with forced(fp8, pick):
                out, info = fp8.op_linear_engine(c["A"], c["W"], bias=c["bias"] if bias else None, R1=c["R1"] if R1 else None, R2=c["R2"] if R2 else None,
                                                 c0=c0, c1=c1, c2=c2, out=buf, guard=2)
            assert info == (1, 1, 0), info
            same_bits(out[:M, :N], h16(mo.exact_ref(c, bias, R1, R2, c0, c1, c2)), f"linear() {form}, pick {pick}, rows + {wide}")
            assert (out[M:] == SENT).all() and (out[:, N:] == SENT).all()


def test_linear_blend_and_geglu_match_the_op_entry(fp8):
    """The non-power-of-two blend and GEGLU through linear() are the launches ug_op_linear_mx8_ex makes: bit-identical."""
    M, N, K, alpha = 300, 256, 640, 0.3
    g = mo.gauss_case(M, N, K)
    kw = dict(bias=g["bias"], R1=g["R1"], R2=g["R2"], c0=1 - alpha, c1=1 - alpha, c2=alpha)
    out, info = fp8.op_linear_engine(g["A"], g["W"], **kw)
    assert info == (1, 1, 0), info
    same_bits(out, fp8.op_linear_mx8_ex(g["A"], g["W"], **kw)[0], "blend")
    out, info = fp8.op_linear_engine(g["A"], g["W"], bias=g["bias"], geglu=True)
    assert info == (1, 1, 0), info
    same_bits(out, fp8.op_linear_mx8_ex(g["A"], g["W"], bias=g["bias"], geglu=True)[0], "GEGLU")


@pytest.mark.parametrize("C", [640, 1280])
@pytest.mark.parametrize("M", [256, 385])
def test_ln_linear_prequantised_handoff(fp8, C, M):
    """ln_linear() with the QAct the LayerNorm fills - over the 0xFF-filled workspace, the scale rows [M, round_up(M, 256)) never written - against
    LayerNorm -> fp16 -> quantiser launch -> GEMM; and the same hand-off with the GEGLU epilogue (the feed-forward's first projection)."""
    rng = np.random.default_rng([C, M])
    x = h16(rng.standard_normal((M, C)) * np.exp(rng.normal(0, 1.0, (M, 1))) + rng.normal(0, 0.5, (M, 1)))
    gamma, beta = h16(1 + 0.2 * rng.standard_normal(C)), h16(0.1 * rng.standard_normal(C))
    W, b = h16(rng.standard_normal((256, C)) / np.sqrt(C)), h16(rng.standard_normal(256) * 0.1)
    y = fp8.op_layernorm_ex(x, 1e-5, gamma, beta)["out"]
    for pick in (None, 3):
        for geglu in (False, True):
            with forced(fp8, pick):
                out, info = fp8.op_linear_engine(x, W, bias=b, gamma=gamma, beta=beta, geglu=geglu)
                ref, _ = fp8.op_linear_mx8_ex(y, W, bias=b, geglu=geglu)
            assert info == (1, 1, 1), info
            same_bits(out, ref, f"ln_linear C = {C}, M = {M}, pick {pick}, geglu {geglu}")
    fp8.set_fp8_linears(False)
    out, info = fp8.op_linear_engine(x, W, bias=b, gamma=gamma, beta=beta)
    assert info == (1, 0, 0), info
    same_bits(out, fp8.op_linear(y, W, bias=b), "ln_linear with fp8 off")
