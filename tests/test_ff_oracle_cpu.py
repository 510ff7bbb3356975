"""CPU: the staged float64 feed-forward reference of tests/ff_oracle.py equals the oracle's FeedForward in float64 up to its own fp16 roundings, and an
fp32 emulation of kernels/ff_fused.hip stays inside the bound the GPU tests assert (without their factor 2) on every case of tests/test_ff_forms_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ff_oracle as fo
from oracle.svd_unet import FeedForward


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def oracle_ff(inp, x):
    C = inp["C"]
    ff = FeedForward(C).double()
    with torch.no_grad():
        ff.net[0].proj.weight.copy_(t64(inp["W1"])); ff.net[0].proj.bias.copy_(t64(inp["b1"]))
        ff.net[2].weight.copy_(t64(inp["W2"])); ff.net[2].bias.copy_(t64(inp["b2"]))
        return ff(t64(x)).numpy()


@pytest.mark.parametrize("C,form,rpv", [(64, "plain", 0), (192, "ln", 0), (320, "lnvec", 7)])
def test_reference_equals_the_oracle_feed_forward_up_to_its_fp16_roundings(C, form, rpv):
    """Stage by stage: the pre-add is fp16(X + vec); the LayerNorm before its rounding is torch's float64 layer_norm; FeedForward in float64 on the
    reference's own (rounded) normalised rows differs from the reference only by the fp16 rounding of mid: at most half an ulp, 2^-11 |mid_j|, per
    term of the second product - and it does differ, the rounding is there."""
    inp = fo.ff_inputs(fo._case("t", 45, C, form, 7 + C, rpv=rpv))
    inp.update(c0=1.0, c1=0.0, c2=0.0)
    ref, mag, st = fo.ff_f64(inp, stages=True)
    xs = inp["X"] if rpv == 0 else (inp["X"] + np.repeat(inp["addvec"], rpv, 0)[:45]).astype(np.float16).astype(np.float32)
    assert np.array_equal(st["xs"], xs.astype(np.float64))
    if form != "plain":
        ln = F.layer_norm(t64(xs), (C,), t64(inp["gamma"]), t64(inp["beta"]), fo.EPS).numpy()
        assert np.abs(st["xn_exact"] - ln).max() <= 1e-12 * max(1.0, np.abs(ln).max())
        assert (np.abs(st["xn"] - ln) <= 2.0 ** -11 * np.abs(ln) + 2.0 ** -25).all()          # half an ulp; subnormal spacing 2^-24
    assert (np.abs(st["mid"] - st["mid_exact"]) <= 2.0 ** -11 * np.abs(st["mid_exact"]) + 2.0 ** -25).all()
    want = oracle_ff(inp, st["xn"])
    d = np.abs(ref - want)          # ref has no residual here: mag = |mid| |W2|^T + |b2|
    assert (d <= 2.0 ** -11 * mag + 1e-7).all(), float((d / mag).max())
    assert d.max() > 2.0 ** -20 * np.abs(want).max()
    assert (mag >= np.abs(ref) - 1e-12).all()


def test_reference_residuals_and_optional_operands():
    base = fo.ff_inputs(fo._case("t", 20, 64, "r2", 11))
    ref, mag = fo.ff_f64(base)
    core, cmag = fo.ff_f64(dict(base, R1=None, R2=None, b2=None, c0=1.0))
    b2, r1, r2 = (base[k].astype(np.float64) for k in ("b2", "R1", "R2"))
    want = fo.C0 * (core + b2) + fo.C1 * r1 + fo.C2 * r2
    assert np.abs(ref - want).max() <= 1e-12
    wmag = fo.C0 * (cmag + np.abs(b2)) + np.abs(fo.C1 * r1) + np.abs(fo.C2 * r2)
    assert np.abs(mag - wmag).max() <= 1e-12
    rows = np.array([3, 17, 5])
    sub, smag = fo.ff_f64(base, rows=rows)
    assert np.array_equal(sub, ref[rows]) and np.array_equal(smag, mag[rows])


def test_polynomial_gelu_against_the_exact_one():
    """Abramowitz-Stegun 7.1.26: |erfc error| <= 1.5e-7, so |Phi error| <= 7.5e-8 plus the fp32 arithmetic; both tails end in exactly 0 and 1"""
    g = np.linspace(-45, 45, 20001).astype(np.float32)
    got = fo.geglu32(np.ones_like(g), g).astype(np.float64)
    want = g.astype(np.float64) * fo._phi64(g.astype(np.float64))
    assert (np.abs(got - want) <= 3e-7 * np.maximum(np.abs(g), 1.0)).all()
    assert got[0] == 0.0 and got[-1] == 45.0


def test_case_table_is_well_formed():
    cases = fo.ALL_CASES + fo.SPLIT_CASES[:1]          # the first split case is the first real case again, under another id
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids)
    for c in cases:
        inp = fo.ff_inputs(c) if c["M"] <= 1000 else None
        if inp is not None:
            for k in ("X", "W1", "b1", "W2", "b2", "R1", "R2", "gamma", "beta", "addvec"):
                if isinstance(inp[k], np.ndarray):
                    assert np.array_equal(inp[k], fo.h16(inp[k])), (c["id"], k)
        if c["rows"] is not None:
            assert c["rows"].min() >= 0 and c["rows"].max() < c["M"] and len(c["rows"]) <= 2000, c["id"]
    g = fo.ff_inputs(fo.EDGE_CASES[-1], in_guard=2, guard_value=np.nan)
    p = fo.ff_inputs(fo.EDGE_CASES[-1])
    assert g["X"].shape[0] == p["X"].shape[0] + 2 and g["addvec"].shape[0] == p["addvec"].shape[0] + 1
    assert np.array_equal(g["X"][:-2], p["X"]) and np.isnan(g["X"][-2:]).all() and np.isnan(g["addvec"][-1]).all()
    a, b = fo.ff_f64(g), fo.ff_f64(p)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])          # the reference never reads a guard row
    rc = fo.ff_inputs(fo.ROW_CASES[0])
    _, _, st = fo.ff_f64(rc, stages=True)
    I = 4 * rc["C"]
    hg = st["xn"] @ rc["W1"].astype(np.float64).T[:, I:] + rc["b1"][I:]
    assert hg.max() > 38 and hg.min() < -38 and np.abs(st["mid"]).max() < 6e4          # both GELU tails, and the stored intermediate inside fp16


@pytest.mark.parametrize("case", fo.ALL_CASES, ids=[c["id"] for c in fo.ALL_CASES])
def test_fp32_emulation_of_the_kernel_meets_the_unscaled_bound(case):
    """What keeps the GPU bound honest: the kernel's arithmetic in fp32 with its polynomial GELU and its fp16 roundings stays within
    2^-10 |ref| + 2^-13 (mag + 1) of the staged float64 reference, the GPU bound without its factor 2, on every case the GPU file runs (on the rows it
    checks, for the cases too large to evaluate whole)."""
    inp = fo.ff_inputs(case)
    ref, mag = fo.ff_f64(inp, rows=case["rows"])
    got = fo.ff_emulated(inp, rows=case["rows"])
    assert np.isfinite(got).all()
    r, i = fo.worst_ratio(got, ref, mag)
    idx = np.unravel_index(i, ref.shape)
    print(f"fp32 emulation, {case['id']}: worst |err| / bound = {r:.3f} at {idx}; max |err| / max |ref| = {np.abs(got - ref).max() / np.abs(ref).max():.2e}")
    assert r <= 1.0, f"{case['id']}: |err| / bound = {r:.3f} at {idx}"
