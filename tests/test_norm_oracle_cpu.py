"""CPU: the float64 norm references of tests/norm_oracle.py equal torch's float64 group_norm / layer_norm, and an fp32 emulation of the kernels' two
statistics schemes stays inside the bound the GPU tests assert (without their factor 2) on every GroupNorm input of tests/test_norm_forms_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_oracle as no


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def torch_groupnorm(x, G, eps, gm, bt, temporal, silu):
    xt = t64(x)
    if temporal:
        y = F.group_norm(xt.permute(2, 0, 1)[None], G, t64(gm), t64(bt), eps)[0].permute(1, 2, 0)
    else:
        y = F.group_norm(xt.permute(0, 2, 1), G, t64(gm), t64(bt), eps).permute(0, 2, 1)
    return (F.silu(y) if silu else y).numpy()


@pytest.mark.parametrize("temporal", [False, True])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("C0,C1,G,T,HW", [(64, 0, 16, 3, 10), (96, 48, 4, 2, 7), (40, 0, 2, 5, 1)])
def test_groupnorm_reference_equals_torch_float64(C0, C1, G, T, HW, temporal, silu):
    rng = np.random.default_rng(C0 + T)
    x, gm, bt = no.make_groups(rng, T, HW, G, (C0 + C1) // G, temporal)
    x0, x1 = (x[..., :C0], x[..., C0:]) if C1 else (x, None)
    ref, mag = no.groupnorm_f64(x0, x1, G, 1e-6, gm, bt, temporal, silu)
    want = torch_groupnorm(x, G, 1e-6, gm, bt, temporal, silu)
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    if not silu:
        assert (mag >= np.abs(ref) - 1e-12).all()            # |x a| + |b| >= |x a + b|


def test_make_groups_gives_every_group_its_own_statistics():
    rng = np.random.default_rng(5)
    x, gm, bt = no.make_groups(rng, 4, 300, 8, 16, False)
    sd = x.reshape(4, 300, 8, 16).std((1, 3))
    mu = x.reshape(4, 300, 8, 16).mean((1, 3))
    assert sd.min() > 0.2 and sd.max() < 2.4 and len(np.unique(np.round(sd, 3))) >= 28
    assert (np.abs(mu) <= 2.2 * sd).all()
    assert np.array_equal(x, no.h16(x)) and np.array_equal(gm, no.h16(gm)) and np.array_equal(bt, no.h16(bt))
    assert len(np.unique(gm)) > 100 and len(np.unique(bt)) > 100
    xt, _, _ = no.make_groups(rng, 4, 300, 8, 16, True)         # pooled: one parameter pair per group across the frames
    sdt = xt.reshape(4, 300, 8, 16).std((1, 3))
    assert (np.abs(sdt / sdt.mean(0) - 1) < 0.1).all()


@pytest.mark.parametrize("M,C,rpv,row0", [(7, 64, 0, 0), (203, 320, 70, 0), (50, 768, 8, 5), (9, 1024, 4, 3)])
def test_layernorm_reference_equals_torch_float64(M, C, rpv, row0):
    rng = np.random.default_rng(M + C)
    x = no.h16(rng.standard_normal((M, C)) * 2 + 0.3)
    gm, bt = no.h16(1 + 0.3 * rng.standard_normal(C)), no.h16(0.5 * rng.standard_normal(C))
    av = no.h16(rng.standard_normal(((M + row0 + rpv - 1) // rpv, C))) if rpv else None
    ref, mag, xout = no.layernorm_f64(x, 1e-5, gm, bt, av, max(rpv, 1), row0)
    xs = x
    if rpv:
        xs = (x + np.repeat(av, rpv, 0)[row0: row0 + M]).astype(np.float16).astype(np.float32)
        assert np.array_equal(xout, xs)
    else:
        assert xout is None
    want = F.layer_norm(t64(xs), (C,), t64(gm), t64(bt), 1e-5).numpy()
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (mag >= np.abs(ref) - 1e-12).all()


def test_case_table_is_well_formed():
    ids = [c["id"] for c in no.GN_CASES]
    assert len(set(ids)) == len(ids)
    for c in no.GN_CASES + no.GN_VERSUS + no.GN_TWO_SOURCE + [no.GN_T64_65]:
        C = c["C0"] + c["C1"]
        assert c["C0"] % 8 == 0 and c["C1"] % 8 == 0 and C % c["G"] == 0 and 256 % c["G"] == 0, c["id"]
        assert c["T"] * c["HW"] * C <= 4.4e6, c["id"]
    assert {c["silu"] for c in no.GN_CASES} == {False, True}


@pytest.mark.parametrize("scheme", ["chunked", "small", "twopass"])
def test_fp32_emulation_of_both_statistics_schemes_meets_the_unscaled_bound(scheme):
    """What keeps the GPU bound honest: fp32 statistics as schemes 1 (chunked sum / sum of squares), 2 (gn_small: one workgroup's sum / sum of squares,
    per-frame inputs only - the kernel has no pooled form) and 4 / 6 (two-pass) take them, fp32 scale / shift / output, fp16 rounding - on every
    GroupNorm input of the GPU file the error stays within 2^-10 |ref| + 2^-20 (mag + 1), the GPU bound without its factor 2."""
    worst, where = 0.0, ""
    for id_, x0, x1, G, temporal, silu, gm, bt in no.all_gn_inputs():
        if scheme == "small" and temporal:
            continue
        ref, mag = no.groupnorm_f64(x0, x1, G, 1e-6, gm, bt, temporal, silu)
        got = no.groupnorm_emulated(x0, x1, G, 1e-6, gm, bt, temporal, silu, scheme)
        r, _ = no.worst_ratio(got, ref, mag)
        if r > worst:
            worst, where = r, id_
    print(f"fp32 emulation, {scheme}: worst |err| / bound = {worst:.3f} at '{where}'")
    assert worst <= 1.0, f"{scheme}: |err| / bound = {worst:.3f} at '{where}'"
