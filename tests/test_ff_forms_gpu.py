"""Every launch form of the fused GEGLU feed-forward (kernels/ff_fused.hip), reached on purpose through ug_op_ff_ex: workgroups that walk several tiles
(FFusedP::max_wg at small M, the real grid at M > 32768) in both kernel variants, the in-kernel LayerNorm with the pre-add, the engine's whole-rounds
row split, the edges of M with guard rows behind inputs and output, the optional operands and the launcher's refusals.  Every case asserts the launch
the entry reports (grid, tiles per workgroup, rows of the fused kernel), so a case written for "two tiles, then none" cannot turn into a one-tile case;
outputs are held to the staged float64 reference of tests/ff_oracle.py by its elementwise bound (|err| <= 2 (2^-10 |ref| + 2^-13 (mag + 1));
tests/test_ff_oracle_cpu.py holds an fp32 emulation of the kernel to the same bound without the 2) and to each other bit for bit."""
import numpy as np
import pytest

import ff_oracle as fo
from util import report, where_differ

pytestmark = pytest.mark.gpu

GUARD, FILL = 3, -1234.0          # rows behind the output and what they hold before the launch (exact in fp16)
IN_GUARD = 2                      # rows behind X / R1 / R2 (and one vector behind addvec)


def launch(engine, inp, mode=2, max_wg=0, variant=0, in_guard=0, out_guard=0):
    """one ug_op_ff_ex call on the operands of ff_oracle.ff_inputs -> (output [M, C], guard rows [out_guard, C], info)"""
    M, C = inp["M"], inp["C"]
    engine.tune_ff(variant)
    try:
        buf, info = engine.op_ff_ex(inp["X"], inp["W1"], inp["b1"], inp["W2"], inp["b2"], R1=inp["R1"], R2=inp["R2"], c0=inp["c0"], c1=inp["c1"], c2=inp["c2"],
                                    gamma=inp["gamma"], beta=inp["beta"], eps=inp["eps"], addvec=inp["addvec"], rows_per_vec=inp["rows_per_vec"],
                                    mode=mode, max_wg=max_wg, in_guard=in_guard, out=np.full((M + out_guard, C), FILL, np.float32), out_guard=out_guard)
    finally:
        engine.tune_ff(0)
    return buf[:M], buf[M:], info


def check(got, ref, mag, what):
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    f = fo.BOUND_FACTOR_GPU
    r, i = fo.worst_ratio(got, ref, mag, f)
    report(f"ff forms: {what}", r, tol=1.0, kind=f"max |err| / ({f:g} (2^-10 |ref| + 2^-13 (mag + 1)))")
    idx = np.unravel_index(i, ref.shape)
    assert r <= 1.0, f"{what}: |err| / bound = {r:.3f} at {idx}: got {got[idx]!r}, reference {ref[idx]!r}"
    return r


def assert_info(info, want, what):
    assert info == tuple(want), f"{what}: the entry reports (grid, tiles per workgroup, fused rows) = {info}, this test is written for {tuple(want)}"


def assert_same(got, want, what):
    assert np.array_equal(got, want), f"{what}: {where_differ(got, want)}"


def tiles(M):
    return (M + 127) // 128


# ---------------------------------------------------------------------------------------------------------------------------------------------
# a. tile walks at small M
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fo.WALK_CASES, ids=[c["id"] for c in fo.WALK_CASES])
def test_tile_walks_are_bit_identical_to_one_tile_per_workgroup(engine, case):
    """M = 421 = three full tiles and 37 rows.  One workgroup walks all four tiles; two walk two each (one ends on the ragged tile); of three, one walks
    two tiles and two walk one - `more` true and false in one launch.  Variant 0 (cross-tile prefetch where C has it: 192, 256, 320) and variant 1, every
    cap, give the bytes of the uncapped variant-1 launch, which is held to the reference.  With rows_per_vec = 100 the pre-add vector changes inside
    every tile and between the tiles of one workgroup."""
    inp = fo.ff_inputs(case)
    M = case["M"]
    assert tiles(M) == 4 and M % 128 == 37
    what = f"{case['id']} M {M}"
    base, _, info = launch(engine, inp, variant=1)
    assert_info(info, (4, 1, M), what + " uncapped variant 1")
    ref, mag = fo.ff_f64(inp)
    check(base, ref, mag, what + " uncapped variant 1")
    got, _, info = launch(engine, inp, variant=0)
    assert_info(info, (4, 1, M), what + " uncapped variant 0")
    assert_same(got, base, what + " uncapped variant 0 vs variant 1")
    for max_wg, walked in ((1, 4), (2, 2), (3, 2)):
        for variant in (0, 1):
            w = f"{what} max_wg {max_wg} variant {variant}"
            got, _, info = launch(engine, inp, max_wg=max_wg, variant=variant)
            assert_info(info, (max_wg, walked, M), w)
            assert_same(got, base, w + " vs uncapped variant 1")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# b. the real launch geometry
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fo.REAL_CASES, ids=[c["id"] for c in fo.REAL_CASES])
def test_real_grid_with_two_tile_workgroups(engine, case):
    """More tiles than the 256 workgroups of the grid, uncapped, in-kernel LayerNorm with the pre-add (rows_per_vec = 1339): the first workgroups walk
    two tiles, the others one.  Both variants give the same bytes; the rows of the two-tile workgroups and 256 sampled rows are held to the reference."""
    inp = fo.ff_inputs(case)
    M, rows = case["M"], case["rows"]
    assert tiles(M) > 256 and M % 128
    what = f"{case['id']} mode 2"
    v0, _, info = launch(engine, inp, variant=0)
    assert_info(info, (256, 2, M), what + " variant 0")
    v1, _, info = launch(engine, inp, variant=1)
    assert_info(info, (256, 2, M), what + " variant 1")
    assert_same(v0, v1, what + " variant 0 vs variant 1")
    ref, mag = fo.ff_f64(inp, rows=rows)
    check(v0[rows], ref, mag, what + f" ({len(rows)} rows)")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# c. the engine's row split
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_engine_row_split_numbers_the_tail_rows_from_m1(engine):
    """M = 33485 through the engine's ln_ff: the fused kernel takes the whole round (M1 = 32768 rows, bit-identical to the same rows of the one-launch
    mode 2), the 717 rows of the thin last round go through layernorm(..., row0 = M1) and two GEMMs.  rows_per_vec = 1339: the tail's first vector is
    number 24 and changes at row 33475 - a tail numbered from 0 reads vector 0."""
    case = fo.SPLIT_CASES[0]
    inp = fo.ff_inputs(case)
    M, m1, rows = case["M"], case["m1"], case["rows"]
    assert m1 // case["rpv"] == 24 and rows[0] == m1 and rows[-1] == M - 1
    got, _, info = launch(engine, inp, mode=3)
    assert_info(info, (256, 1, m1), "ln_ff M 33485")
    one, _, info = launch(engine, inp, mode=2)
    assert_info(info, (256, 2, M), "mode 2 M 33485")
    assert_same(got[:m1], one[:m1], "ln_ff rows below M1 vs the one-launch mode 2")
    ref, mag = fo.ff_f64(inp, rows=rows)
    check(got[rows], ref, mag, "ln_ff M 33485, the two-GEMM tail rows")


@pytest.mark.parametrize("case", fo.SPLIT_CASES[1:], ids=[c["id"] for c in fo.SPLIT_CASES[1:]])
def test_engine_row_split_boundary(engine, case):
    """a last round of 160 tiles still goes to the two-GEMM tail, one of 161 tiles stays in the fused launch"""
    inp = fo.ff_inputs(case)
    M, m1, rows = case["M"], case["m1"], case["rows"]
    got, _, info = launch(engine, inp, mode=3)
    assert_info(info, (256, (tiles(m1) + 255) // 256, m1), case["id"])
    ref, mag = fo.ff_f64(inp, rows=rows)
    check(got[rows], ref, mag, f"ln_ff {case['id']} ({len(rows)} rows)")


def test_engine_row_split_with_the_layernorm_launch_equals_two_gemms(engine):
    """ug_set_ff_fused bit 1 off: LayerNorm launch, fused kernel on the whole round, two GEMMs on the tail.  With every GEMM unsplit
    (ug_tune_force(-1, 1)) that is the MFMA chain of mode 0 (LayerNorm launch + two GEMMs on all rows) for every output: bit-identical.  Under the
    planner's own choice the rows of the fused kernel are still those bytes; the 717 tail rows are not - their down-projection (717 x 320 x 1280, 30
    tiles of 128 x 64) is planned as tile config 3 with split-K 4, another summation order - and are held to the reference instead."""
    case = fo.SPLIT_CASES[0]
    inp = fo.ff_inputs(case)
    M, m1, rows = case["M"], case["m1"], case["rows"]
    try:
        engine.set_ff_fused(True, prenorm=False)
        planned, _, info = launch(engine, inp, mode=3)
        assert_info(info, (256, 1, m1), "ln_ff, LayerNorm launch")
        engine.tune_force(-1, 1)
        unsplit, _, info = launch(engine, inp, mode=3)
        assert_info(info, (256, 1, m1), "ln_ff, LayerNorm launch, unsplit GEMMs")
        two, _, info = launch(engine, inp, mode=0)
        assert_info(info, (0, 0, 0), "mode 0")
    finally:
        engine.tune_force(-1, -1)
        engine.set_ff_fused(True, prenorm=True)
    assert_same(unsplit, two, "ln_ff with the LayerNorm launch vs LayerNorm + two GEMMs, all unsplit")
    assert_same(planned[:m1], two[:m1], "ln_ff with the LayerNorm launch, planner's GEMMs, rows below M1 vs LayerNorm + two GEMMs")
    report("ff forms: ln_ff tail rows, planner's GEMMs vs unsplit", np.count_nonzero(planned[m1:] != two[m1:]), kind=f"elements that differ, of {(M - m1) * case['C']}")
    ref, mag = fo.ff_f64(inp, rows=rows)
    check(planned[rows], ref, mag, "ln_ff with the LayerNorm launch, the planner's tail rows")
    check(two[rows], ref, mag, "mode 0, the same rows")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# d. edges of M, guards and leakage
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fo.EDGE_CASES, ids=[c["id"] for c in fo.EDGE_CASES])
def test_edges_of_m_with_guards(engine, case):
    """One row, part of a tile, a whole tile, one row and all but one row of a second tile.  Three rows behind the output keep their fill; two rows of NaN
    behind X and R1 and one NaN vector behind addvec change no byte of the output against zeros there; a second launch repeats the first."""
    M, C = case["M"], case["C"]
    what = case["id"]
    zeros = fo.ff_inputs(case, in_guard=IN_GUARD, guard_value=0.0)
    nans = fo.ff_inputs(case, in_guard=IN_GUARD, guard_value=np.nan)
    a, ga, info = launch(engine, zeros, in_guard=IN_GUARD, out_guard=GUARD)
    assert_info(info, (tiles(M), 1, M), what)
    b, gb, _ = launch(engine, nans, in_guard=IN_GUARD, out_guard=GUARD)
    c, gc, _ = launch(engine, nans, in_guard=IN_GUARD, out_guard=GUARD)
    for g in (ga, gb, gc):
        assert_same(g, np.full((GUARD, C), FILL, np.float32), what + ": the rows behind the output")
    assert np.isfinite(b).all(), f"{what}: NaN behind the inputs reached the output"
    assert_same(b, a, what + ": NaN behind the inputs vs zeros")
    assert_same(c, b, what + ": second launch vs first")
    ref, mag = fo.ff_f64(zeros)
    check(a, ref, mag, what)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# e. optional operands and refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fo.OPT_CASES, ids=[c["id"] for c in fo.OPT_CASES])
def test_optional_operands(engine, case):
    """no b2; no residual; R2 with c2 = -0.5 next to R1; pre-norm without pre-add and a residual tensor that is not the stream"""
    inp = fo.ff_inputs(case)
    got, _, info = launch(engine, inp)
    assert_info(info, (tiles(case["M"]), 1, case["M"]), case["id"])
    ref, mag = fo.ff_f64(inp)
    check(got, ref, mag, case["id"])
    if case["form"] == "r2":          # the second residual is really read: without it the output moves by c2 * R2
        assert np.abs(got - fo.ff_f64(dict(inp, R2=None))[0]).max() > 0.5


def test_refusals_leave_the_context_usable(engine):
    """the launcher refuses a pre-add next to a residual that is not the stream, and a channel count that is no multiple of 64; after each error the
    next launch is correct"""
    good = fo.ff_inputs(fo.WALK_CASES[-1])
    ref, mag = fo.ff_f64(good)
    bad = dict(good, R1=fo.h16(np.random.default_rng(1).standard_normal(good["X"].shape)))
    with pytest.raises(RuntimeError, match="residual is not the normalised stream"):
        launch(engine, bad)
    got, _, _ = launch(engine, good)
    check(got, ref, mag, "after the refused pre-add with its own residual")
    rng = np.random.default_rng(2)
    M, C = 50, 100
    odd = dict(M=M, C=C, X=fo.h16(rng.standard_normal((M, C))), W1=fo.h16(rng.standard_normal((8 * C, C)) * 0.1), b1=fo.h16(rng.standard_normal(8 * C) * 0.1),
               W2=fo.h16(rng.standard_normal((C, 4 * C)) * 0.05), b2=fo.h16(rng.standard_normal(C) * 0.1), R1=None, R2=None, c0=1.0, c1=1.0, c2=1.0,
               gamma=None, beta=None, eps=fo.EPS, addvec=None, rows_per_vec=1)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        launch(engine, odd)
    got, _, _ = launch(engine, good)
    check(got, ref, mag, "after the refused C = 100")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f. rows a LayerNorm can get wrong, and the GELU tails
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fo.ROW_CASES, ids=[c["id"] for c in fo.ROW_CASES])
def test_hard_rows_and_gelu_tails(engine, case):
    """One tile with a constant row, an all-zero row, a row of 1000 +- noise, a row with one 3e4 outlier and a row of values near 2^-14, and 64 gate
    biases that put the gate pre-activation near +-3, +-6, +-12 and +-40 (the stored intermediate stays inside fp16)."""
    inp = fo.ff_inputs(case)
    got, _, info = launch(engine, inp)
    assert_info(info, (1, 1, case["M"]), case["id"])
    ref, mag = fo.ff_f64(inp)
    check(got, ref, mag, case["id"])
    check(got[:5], ref[:5], mag[:5], case["id"] + ", the five hard rows")
    v1, _, _ = launch(engine, inp, variant=1)
    assert_same(v1, got, case["id"] + " variant 1 vs variant 0")
