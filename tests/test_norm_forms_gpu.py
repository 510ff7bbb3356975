"""Every launch form of kernels/norm.hip, reached on purpose: the four GroupNorm schemes (forced through GroupNormP::mode where the measured heuristics
would not pick them), the seven gn_slab instantiations in each of their MODEs, ln_kernel<1..4> and ln40_kernel<8|16|32> with their MX-fp8 output.
Every GroupNorm case asserts the plan the launcher reports, an elementwise bound against the float64 reference of tests/norm_oracle.py
(|err| <= 2 (2^-10 |ref| + 2^-20 (mag + 1)); tests/test_norm_oracle_cpu.py holds an fp32 emulation of the kernels to the same bound without the 2),
bit-identical repeats, and guard rows behind the output that must come back untouched."""
import numpy as np
import pytest

import norm_oracle as no
from util import assert_close, h16, mx8_quantise, report

pytestmark = pytest.mark.gpu

TOL = 2e-3            # the coarse whole-tensor line of tests/test_ops_gpu.py, kept next to the elementwise bound
EPS = 1e-6
GUARD, FILL = 3, -1234.0          # rows behind the output, and what the whole output buffer holds before the launch (exact in fp16)


def check(got, ref, mag, what, factor=no.BOUND_FACTOR_GPU):
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    r, i = no.worst_ratio(got, ref, mag, factor)
    report(f"norm forms: {what}", r, tol=1.0, kind=f"max |err| / ({factor:g} (2^-10 |ref| + 2^-20 (mag + 1)))")
    idx = np.unravel_index(i, ref.shape)
    assert r <= 1.0, f"{what}: |err| / bound = {r:.3f} at {idx}: got {got[idx]!r}, reference {ref[idx]!r}"
    assert_close(got, ref, TOL, f"norm forms (coarse): {what}")
    return r


def run_gn(engine, x0, x1, G, gm, bt, temporal, silu, mode, what):
    """two launches with guard rows: bit-identical, guard rows untouched -> (output [T,HW,C], plan)"""
    T, HW, C = x0.shape[0], x0.shape[1], x0.shape[2] + (0 if x1 is None else x1.shape[2])
    outs = [engine.op_groupnorm_ex(x0, G, EPS, gm, bt, x1=x1, temporal=temporal, silu=silu, mode=mode, guard=GUARD, guard_fill=FILL) for _ in range(2)]
    (a, plan), (b, plan_b) = outs
    assert plan == plan_b
    assert np.array_equal(a, b), f"{what}: two launches differ in {np.count_nonzero(a != b)} elements"
    assert np.array_equal(a[T * HW:], np.full((GUARD, C), FILL, np.float32)), f"{what}: the rows behind the output were written"
    return a[: T * HW].reshape(T, HW, C), plan


def assert_plan(plan, want, what):
    got = plan[: len(want)]
    assert got == tuple(want), f"{what}: the launcher chose {got}, this test is written for {tuple(want)}"


@pytest.mark.parametrize("case", no.GN_CASES, ids=[c["id"] for c in no.GN_CASES])
def test_groupnorm_forms(engine, case):
    x0, x1, gm, bt = no.gn_inputs(case)
    what = f"groupnorm {case['id']} (C {case['C0']}+{case['C1']} G {case['G']} T {case['T']} HW {case['HW']} temporal={case['temporal']} mode={case['mode']})"
    got, plan = run_gn(engine, x0, x1, case["G"], gm, bt, case["temporal"], case["silu"], case["mode"], what)
    assert_plan(plan, case["want"], what)
    if plan[0] != 1:
        assert plan[3] == 0
    if case["fin"]:
        fin = 1024 if (case["T"] if case["temporal"] else 1) * plan[3] > 64 else 256
        assert fin == case["fin"], f"{what}: gn_finalize runs on {fin} threads, this test is written for {case['fin']}"
    ref, mag = no.groupnorm_f64(x0, x1, case["G"], EPS, gm, bt, case["temporal"], case["silu"])
    check(got, ref, mag, what)


def test_groupnorm_scheme6_on_both_sides_of_64_frames(engine):
    """the same input with 64 frames (lane t of a wave holds frame t's partial) and extended by one frame (the serial combine); the pooled statistics of
    the first 64 frames differ between the two, so each is held to its own reference"""
    case = no.GN_T64_65
    x, _, gm, bt = no.gn_inputs(case)
    for T in (64, 65):
        what = f"groupnorm scheme 6, T = {T} of the 65-frame input"
        got, plan = run_gn(engine, x[:T], None, case["G"], gm, bt, True, case["silu"], 0, what)
        assert_plan(plan, (6, 256, 4), what)
        ref, mag = no.groupnorm_f64(x[:T], None, case["G"], EPS, gm, bt, True, case["silu"])
        check(got, ref, mag, what)


@pytest.mark.parametrize("case", no.GN_TWO_SOURCE, ids=[c["id"] for c in no.GN_TWO_SOURCE])
def test_groupnorm_two_sources_equal_the_concatenated_tensor(engine, case):
    """every group inside one source: the slab reads it from X0 or X1 with that source's row stride - the same bytes as from the concatenated tensor"""
    x0, x1, gm, bt = no.gn_inputs(case)
    xc = np.concatenate([x0, x1], -1)
    what = f"groupnorm two sources {case['id']}"
    two, plan2 = run_gn(engine, x0, x1, case["G"], gm, bt, case["temporal"], case["silu"], 0, what + " (two)")
    one, plan1 = run_gn(engine, xc, None, case["G"], gm, bt, case["temporal"], case["silu"], 0, what + " (one)")
    want = (6, 256, 4) if case["temporal"] else (4, 256, 4)
    assert_plan(plan2, want, what + " (two)")
    assert_plan(plan1, want, what + " (one)")
    assert np.array_equal(two, one), f"{what}: {np.count_nonzero(two != one)} elements differ between the two-source and the concatenated call"
    ref, mag = no.groupnorm_f64(xc, None, case["G"], EPS, gm, bt, case["temporal"], case["silu"])
    check(two, ref, mag, what)


@pytest.mark.parametrize("case", no.GN_VERSUS, ids=[c["id"] for c in no.GN_VERSUS])
def test_groupnorm_schemes_against_each_other(engine, case):
    """one input under every scheme that accepts it: each within the bound of the reference, any two within twice the bound of each other (not
    bit-equal: the statistics are summed differently)"""
    x0, x1, gm, bt = no.gn_inputs(case)
    ref, mag = no.groupnorm_f64(x0, x1, case["G"], EPS, gm, bt, case["temporal"], case["silu"])
    outs = []
    for mode, scheme in zip(case["modes"], case["schemes"]):
        what = f"groupnorm {case['id']} under mode {mode}"
        got, plan = run_gn(engine, x0, x1, case["G"], gm, bt, case["temporal"], case["silu"], mode, what)
        assert_plan(plan, (scheme,), what)
        check(got, ref, mag, what)
        outs.append((mode, got))
    lim = 2 * no.bound(ref, mag, no.BOUND_FACTOR_GPU)
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            r = float((np.abs(outs[i][1].astype(np.float64) - outs[j][1]) / lim).max())
            report(f"norm forms: groupnorm {case['id']} mode {outs[i][0]} vs mode {outs[j][0]}", r, tol=1.0, kind="max |a - b| / (2 x bound)")
            assert r <= 1.0, f"groupnorm {case['id']}: modes {outs[i][0]} and {outs[j][0]} differ by {r:.3f} x twice the bound"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------------------
LN_EPS = 1e-5
# (C, form asked for, kernel expected: L of ln40_kernel<L>, -VPL of ln_kernel<VPL>)
LN_FORMS = [(64, 0, -1), (768, 0, -2), (1024, 0, -2), (1536, 0, -3), (2048, 0, -4), (320, 1, -1), (640, 1, -2), (1280, 1, -3),
            (320, 0, 8), (640, 0, 16), (1280, 0, 32)]
# 1; 3 (less than the 8 / 4 rows one wave of ln40_kernel<8> / <16> holds, less than one workgroup's in every kernel); 41 = 8 * 5 + 1, 21 = 4 * 5 + 1 and every odd M: the last wave of ln40_kernel<8> / <16> / <32> holds one valid
# row; 203 (the row count of tests/test_ops_gpu.py)
LN_ROWS = [1, 3, 21, 41, 203]


def ln_inputs(seed, M, C):
    """rows of distinct scale and mean (a wrong row fails by many ulps), gamma and beta distinct per channel; all exact in fp16"""
    rng = np.random.default_rng(seed)
    x = h16(rng.standard_normal((M, C)) * 2.0 ** rng.uniform(-2, 1, (M, 1)) + rng.uniform(-2, 2, (M, 1)))
    return rng, x, h16(1 + 0.3 * rng.standard_normal(C)), h16(0.5 * rng.standard_normal(C))


def run_ln(engine, x, gm, bt, form, want_form, what, **kw):
    M, C = x.shape
    r = engine.op_layernorm_ex(x, LN_EPS, gm, bt, form=form, guard=GUARD, guard_fill=FILL, **kw)
    assert r["form"] == want_form, f"{what}: the launcher chose {r['form']}, this test is written for {want_form}"
    assert np.array_equal(r["out"][M:], np.full((GUARD, C), FILL, np.float32)), f"{what}: the rows behind the output were written"
    r["y"] = r["out"][:M]
    return r


@pytest.mark.parametrize("C,form,want", LN_FORMS)
def test_layernorm_forms(engine, C, form, want):
    for M in LN_ROWS:
        _, x, gm, bt = ln_inputs(C + M, M, C)
        what = f"layernorm C {C} form {form} (kernel {want}) M {M}"
        r = run_ln(engine, x, gm, bt, form, want, what)
        ref, mag, _ = no.layernorm_f64(x, LN_EPS, gm, bt)
        check(r["y"], ref, mag, what)


@pytest.mark.parametrize("C,form,want", [(320, 0, 8), (640, 0, 16), (1280, 0, 32), (320, 1, -1), (640, 1, -2), (1280, 1, -3), (768, 0, -2)])
@pytest.mark.parametrize("row0", [0, 1, 4])
def test_layernorm_pre_add_row_numbering(engine, C, form, want, row0):
    """rows_per_vec = 5: vector boundaries fall inside the 8 / 4 / 2 rows one wave of ln40_kernel<8> / <16> / <32> holds (at row0 = 1 between rows 3 | 4
    and 8 | 9 ...); row0 = 0, one row, rows_per_vec - 1.  The written-back sum is fp16(x + vec) bit for bit."""
    M, rpv = 43, 5
    rng, x, gm, bt = ln_inputs(C + row0, M, C)
    av = h16(rng.standard_normal(((M + row0 + rpv - 1) // rpv, C)) * 2)
    what = f"layernorm pre-add C {C} form {form} (kernel {want}) row0 {row0}"
    r = run_ln(engine, x, gm, bt, form, want, what, addvec=av, rows_per_vec=rpv, row0=row0)
    ref, mag, xout = no.layernorm_f64(x, LN_EPS, gm, bt, av, rpv, row0)
    assert np.array_equal(r["xout"], xout), f"{what}: {np.count_nonzero(r['xout'] != xout)} elements of the written-back sum differ from fp16(x + vec)"
    check(r["y"], ref, mag, what)


@pytest.mark.parametrize("C,L", [(320, 8), (640, 16), (1280, 32)])
def test_layernorm_both_kernels_agree(engine, C, L):
    M, rpv, row0 = 203, 70, 3
    rng, x, gm, bt = ln_inputs(C, M, C)
    av = h16(rng.standard_normal(((M + row0 + rpv - 1) // rpv, C)))
    ref, mag, xout = no.layernorm_f64(x, LN_EPS, gm, bt, av, rpv, row0)
    a = run_ln(engine, x, gm, bt, 0, L, f"layernorm C {C} ln40", addvec=av, rows_per_vec=rpv, row0=row0)
    b = run_ln(engine, x, gm, bt, 1, -((C // 8 + 63) // 64), f"layernorm C {C} ln_kernel", addvec=av, rows_per_vec=rpv, row0=row0)
    assert np.array_equal(a["xout"], xout) and np.array_equal(b["xout"], xout)
    check(a["y"], ref, mag, f"layernorm C {C} ln40_kernel<{L}> with pre-add")
    check(b["y"], ref, mag, f"layernorm C {C} ln_kernel with pre-add")
    r = float((np.abs(a["y"].astype(np.float64) - b["y"]) / (2 * no.bound(ref, mag, no.BOUND_FACTOR_GPU))).max())
    report(f"norm forms: layernorm C {C} ln40_kernel<{L}> vs ln_kernel", r, tol=1.0, kind="max |a - b| / (2 x bound)")
    assert r <= 1.0, f"layernorm C {C}: the two kernels differ by {r:.3f} x twice the bound"


@pytest.mark.parametrize("C,form,want", [(640, 0, 16), (640, 1, -2), (1280, 0, 32), (1280, 1, -3), (1024, 0, -2), (2048, 0, -4)])
@pytest.mark.parametrize("M", [203, 260])
def test_layernorm_mx8_output_is_the_quantiser_of_its_fp16_output(engine, C, form, want, M):
    """The quantiser fused into both LayerNorm kernels against mx8_quantise of the SAME kernel's fp16 output (device output, not the reference: exact).
    Block 1 (channels 32..63) has gamma = beta = 0: an all-zero block in every row; beta[200] = 300 and one input outlier set their blocks' scales;
    M = 203 / 260: the scale rows are padded to 256 / 512 dwords and the dwords of the rows past M stay as the entry zeroed them."""
    _, x, gm, bt = ln_inputs(C + M, M, C)
    gm[32:64] = 0.0; bt[32:64] = 0.0
    bt[200] = 300.0
    x[1, 5] = 100.0
    what = f"layernorm MX-fp8 output C {C} form {form} (kernel {want}) M {M}"
    r = run_ln(engine, x, gm, bt, form, want, what, fp8=True)
    ref, mag, _ = no.layernorm_f64(x, LN_EPS, gm, bt)
    check(r["y"], ref, mag, what)
    assert (r["y"][:, 32:64] == 0).all()
    _, bytes_ref, e_ref = mx8_quantise(r["y"])
    np.testing.assert_array_equal(r["y8"], bytes_ref)
    s8 = r["s8"]
    assert s8.shape == (C // 128, (M + 255) // 256 * 256)
    e_dev = np.stack([(s8[:, :M] >> (8 * j)) & 0xff for j in range(4)], -1).transpose(1, 0, 2).reshape(M, C // 32)
    np.testing.assert_array_equal(e_dev.astype(np.uint8), e_ref)
    assert (e_ref[:, 1] == 127).all() and (e_ref[:, 200 // 32] == 127).all()      # zero block: scale 2^0; 300 +- a few in [256, 512): 2^(8 - 8)
    assert not s8[:, M:].any(), f"{what}: scale dwords of rows past M were written"
