"""GPU: the pipeline glue kernels of kernels/misc.hip one launch at a time against the references of tests/glue_oracle.py (pinned to the oracle by
tests/test_glue_oracle_cpu.py).  Every output buffer carries guard rows that must come back as sent.  Bounds: bit equality
where a kernel selects, copies or reproduces an fp16 rounding sequence; otherwise |got - ref64| <= 0.5 * ulp16(ref64) + slack with the slack the
float32 evaluation error of the kernel's expression."""
import numpy as np
import pytest
import torch

import glue_oracle as G
from glue_oracle import CLIP_CASES, F32, h16
from util import report, where_differ

pytestmark = pytest.mark.gpu
FILL = -777.0
BIG = 1048837            # 7 * 269 * 557: past the 4096 x 256 threads of the grid-stride launches, and odd


def _equal(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), f"{what}: {where_differ(got, ref)}"


def _guard(buf, rows, what):
    assert (buf[rows:] == FILL).all(), f"{what}: guard rows written"


def _half_ulp(got, ref64, slack, what):
    ex = G.f16_excess(got, ref64, slack)
    report(what, ex, tol=0.5, kind="max (|got - ref64| - slack) / ulp16(ref64)")
    assert ex <= 0.5, f"{what}: {ex:.4f} fp16 ulps from the float64 reference after the slack, bound 0.5"


# ---------------------------------------------------------------------------------------------------- CLIP / DINO pre-processing
def _clip_check(engine, case, seed):
    from oracle.clip import resize_with_antialiasing
    cid, T, H, W, S, P, Kpad, inet, _ = case
    v = G.clip_case_input(np.random.default_rng(seed), T, H, W)
    rows = T * (S // P) ** 2
    got = engine.op_clip_patchify(v, S, P, Kpad, inet, guard=3, fill=FILL)
    _guard(got, rows, f"clip patchify {cid}")
    assert (got[:rows, 3 * P * P:] == FILL).all(), f"clip patchify {cid}: columns past 3*P*P written"
    r64 = G.resize_antialias(v, S)
    r32 = resize_with_antialiasing(torch.from_numpy(v).permute(0, 3, 1, 2).contiguous(), (S, S)).permute(0, 2, 3, 1).numpy()
    floor = report(f"clip patchify {cid}: float32 floor of the resize", float(np.abs(r32.astype(np.float64) - r64).max()), kind="max|err|")
    ref = G.clip_patchify(v, S, P, Kpad, inet, fill=FILL)
    _half_ulp(got[:rows], ref, G.clip_slack(floor, S, P, Kpad, inet), f"clip patchify {cid} {H}x{W}->{S} T={T}")


@pytest.mark.parametrize("case", CLIP_CASES, ids=[c[0] for c in CLIP_CASES])
def test_clip_patchify(engine, case):
    _clip_check(engine, case, 100 + CLIP_CASES.index(case))


def test_clip_patchify_refusals_leave_the_context_usable(engine):
    for H, W in ((168, 28), (28, 200), (1, 28)):          # factor 6, factor 7.1: more than 9 taps; one row: no reflect border
        with pytest.raises(RuntimeError, match="antialias kernel"):
            engine.op_clip_patchify(np.zeros((1, H, W, 3), F32), 28, 14, 592)
        _clip_check(engine, CLIP_CASES[2], 7)


# ---------------------------------------------------------------------------------------------------- input preparation
@pytest.mark.parametrize("T,H,W,aug", [(3, 5, 7, 0.0), (3, 5, 7, 0.02), (7, 269, 557, 0.02)])
def test_prep_video(engine, T, H, W, aug):
    rng = np.random.default_rng(20)
    frames = rng.uniform(0, 1, (T, H, W, 3)).astype(F32); noise = rng.standard_normal((T, 3, H, W)).astype(F32)
    src, vin = engine.op_prep_video(frames, noise, aug, guard=2, fill=FILL)
    n = T * H * W
    _guard(src, n, "prep video clip_src"); _guard(vin, n, "prep video vae_in")
    ref_src, ref_vin = G.prep_video(frames, noise, aug)
    _equal(src[:n], ref_src, f"prep video clip_src T={T} {H}x{W} aug={aug}")
    _equal(vin[:n], ref_vin, f"prep video vae_in T={T} {H}x{W} aug={aug}")
    assert (vin[:n, 3:] == 0).all()


# ---------------------------------------------------------------------------------------------------- sampler
@pytest.fixture(scope="module")
def sched():
    from oracle.scheduler import EulerKarrasVPred
    sch = EulerKarrasVPred(); sch.set_timesteps(5)
    assert float(sch.sigmas[0]) == 700.0 and float(sch.sigmas[5]) == 0.0
    return sch


@pytest.mark.parametrize("T,h,w", [(3, 5, 7), (7, 269, 557)])
def test_init_latents(engine, sched, T, h, w):
    noise = np.random.default_rng(21).standard_normal((T, 4, h, w)).astype(F32)
    sigma0 = np.sqrt(F32(700.0) * F32(700.0) + F32(1))
    got = engine.op_init_latents(noise, sigma0, guard=2, fill=FILL)
    _guard(got, T * h * w, "init latents")
    _equal(got[:T * h * w], G.init_latents(noise, sigma0), f"init latents T={T} {h}x{w}")


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("pixels,steps", [(105, (0, 1, 2, 3, 4)), (BIG, (0,))])
def test_unet_input(engine, sched, pixels, steps, guided):
    rng = np.random.default_rng(22)
    for i in steps:
        s = F32(float(sched.sigmas[i]))
        den = np.sqrt(s * s + F32(1))
        lat = h16(rng.standard_normal((pixels, 4)) * s); cond = h16(rng.standard_normal((pixels, 4)))
        got = engine.op_unet_input(lat, cond, den, guided=guided, guard=2, fill=FILL)
        rows = (2 if guided else 1) * pixels
        _guard(got, rows, "unet input")
        ref = G.unet_input64(lat, cond, den, guided)
        _half_ulp(got[:rows, :4], ref[:, :4], 2.0 ** -23 * np.abs(ref[:, :4]), f"unet input sigma={s:.4g} pixels={pixels} guided={guided}")
        _equal(got[:rows, 4:], ref[:, 4:].astype(F32), "unet input: conditioning / zero channels")
        if guided:
            _equal(got[pixels:rows, :4], got[:pixels, :4], "unet input: the scaled latents of the two videos")


def _share(got, ref, what):
    return report(what + ": bit-equal share", float((got == ref).mean()), kind="share")


@pytest.mark.parametrize("n,steps", [(420, (0, 1, 2, 3, 4)), (BIG, (0, 4))])
def test_euler_step_within_one_ulp(engine, sched, n, steps):
    rng = np.random.default_rng(23)
    for i in steps:
        s, sn = float(sched.sigmas[i]), float(sched.sigmas[i + 1])
        x = h16(rng.standard_normal(n) * s); v = h16(rng.standard_normal(n))
        ref = sched.step(torch.from_numpy(v).half(), i, torch.from_numpy(x).half()).float().numpy()
        got = engine.op_euler_step(v, x, s, sn)
        what = f"euler step {i} sigma={s:.4g} n={n}"
        _share(got, ref, what)
        d = report(what, G.ulps16_apart(got, ref), tol=1.0, kind="max fp16 ulps from the oracle")
        assert d <= 1.0, what


@pytest.mark.parametrize("g", [1.0, 1.5, 7.0])
@pytest.mark.parametrize("n,steps", [(420, (0, 1, 2, 3, 4)), (BIG, (0, 4))])
def test_euler_step_cfg_within_one_ulp(engine, sched, n, steps, g):
    rng = np.random.default_rng(24)
    for i in steps:
        s, sn = float(sched.sigmas[i]), float(sched.sigmas[i + 1])
        x = h16(rng.standard_normal(n) * s); vc = h16(rng.standard_normal(n)); vu = h16(rng.standard_normal(n))
        v = G.guided_v(vc, vu, g)                  # tests/cfg_oracle.py's combination on fp16 tensors (pinned on the CPU)
        ref = sched.step(torch.from_numpy(v).half(), i, torch.from_numpy(x).half()).float().numpy()
        got = engine.op_euler_step_cfg(vc, vu, g, x, s, sn, guard=5, fill=FILL)
        _guard(got, n, "guided euler step")
        what = f"guided euler step {i} g={g} sigma={s:.4g} n={n}"
        _share(got[:n], ref, what)
        d = report(what, G.ulps16_apart(got[:n], ref), tol=1.0, kind="max fp16 ulps from the oracle")
        assert d <= 1.0, what


# ---------------------------------------------------------------------------------------------------- latent sliding windows
@pytest.mark.parametrize("fe", [140, 4099])
@pytest.mark.parametrize("overlap", [1, 2, 3, 5])
def test_window_blend(engine, sched, overlap, fe):
    rng = np.random.default_rng(25)
    sig0 = F32(float(sched.sigmas[0]))
    coef = sig0 / np.sqrt(sig0 * sig0 + F32(1))
    prev = h16(rng.standard_normal((overlap, fe))); noise = h16(rng.standard_normal((overlap, fe)) * 700.0); cur = h16(rng.standard_normal((overlap, fe)))
    rn, _ = engine.op_window_blend(prev, noise, overlap, coef, guard=3, fill=FILL)
    _, fd = engine.op_window_blend(prev, cur, overlap, coef, guard=3, fill=FILL)
    n = overlap * fe
    _guard(rn, n, "re-noising"); _guard(fd, n, "cross-fade")
    _half_ulp(rn[:n].reshape(overlap, fe), G.renoise64(prev, noise, coef), 2.0 ** -22 * (np.abs(prev) + np.abs(noise)), f"window re-noising overlap={overlap} fe={fe}")
    _half_ulp(fd[:n].reshape(overlap, fe), G.crossfade64(cur, prev), 2.0 ** -22 * (np.abs(cur) + np.abs(prev)), f"window cross-fade overlap={overlap} fe={fe}")
    if overlap == 1:
        _equal(fd[:n], prev.ravel(), "cross-fade of one frame: weight 0")


# ---------------------------------------------------------------------------------------------------- decoder tail, post-processing
@pytest.mark.parametrize("T", [1, 2, 5])
def test_time_conv_out(engine, T):
    x, w, b = G.time_conv_case(np.random.default_rng(9), T)
    got = engine.op_time_conv_out(x, w, b, guard=3, fill=FILL)
    n = T * x.shape[1]
    _guard(got, n, "time conv out")
    acc = G.time_conv_acc64(x, w, b)
    assert np.isfinite(got).all()
    ex = float(((np.abs(got[:n].astype(np.float64) - G.time_conv_frames64(acc)) - 1e-6) / G.ulp16(acc)).max())
    report(f"time conv out T={T}", ex, tol=0.25, kind="max (|got - ref64| - 1e-6) / ulp16(acc64)")
    assert ex <= 0.25
    assert (got[:n] == 0.0).any() and (got[:n] == 1.0).any(), "the case must reach both clamps"


@pytest.mark.parametrize("offset", [0.0, -0.7])
@pytest.mark.parametrize("n", [1, 63, 300, BIG])
def test_depth_post(engine, n, offset):
    rng = np.random.default_rng(26)
    fr = (rng.uniform(0, 1, (n, 3)) + offset).astype(F32)
    if n > 1:
        fr[0] = 1.5; fr[-1] = -1.25 if offset else 0.0      # the maximum first, the minimum last
    depth, disp, mm = engine.op_depth_post(fr, guard=4, fill=FILL)
    _guard(depth, n, "depth"); _guard(disp, n, "disparity")
    with np.errstate(invalid="ignore", divide="ignore"):
        rd, rx, rmm = G.depth_post32(fr)
        recip = F32(1.0) / (disp[:n] + F32(0.1))
    _equal(mm, rmm, f"depth post n={n}: min-max words")
    if n > 1:
        assert mm[1] == 1.5 and mm[0] == (-1.25 if offset else 0.0)
    for name, got, ref in (("disparity", disp[:n], rx), ("depth", depth[:n], rd), ("1 / (disparity + 0.1)", depth[:n], recip)):
        ulps = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        ulps = ulps[~(np.isnan(got) & np.isnan(ref))]
        report(f"depth post n={n} offset={offset}: {name}", float(ulps.max()) if ulps.size else 0.0, tol=0, kind="max float32 ulps")
        assert np.array_equal(got, ref, equal_nan=True), f"{name}: {where_differ(got, ref)}"


# ---------------------------------------------------------------------------------------------------- StableNormal glue
@pytest.mark.parametrize("h,w,g", [(12, 20, 16), (7, 9, 3), (16, 16, 16)])
def test_add_grid_nearest(engine, h, w, g):
    rng = np.random.default_rng(27)
    x, grid = h16(rng.standard_normal((2, h, w, 16))), h16(rng.standard_normal((2, g, g, 16)))
    got = engine.op_add_grid_nearest(x, grid, guard=3, fill=FILL)
    _guard(got, 2 * h * w, "add grid")
    _equal(got[:2 * h * w], G.add_grid_nearest(x, grid), f"add grid {h}x{w} g={g}")


def test_sn_normals_out(engine):
    rng = np.random.default_rng(28)
    dec = np.full((1000, 8), 1e4, F32)
    dec[:, :3] = h16(rng.standard_normal((1000, 3)) * 1.5)
    dec[5, :3] = 0.0
    assert (np.abs(dec[:, :3]) > 1).any()
    got = engine.op_sn_normals_out(dec, guard=3, fill=FILL)
    _guard(got, 1000, "normals out")
    ref = G.sn_normals64(dec)
    assert np.isfinite(got).all() and (got[5] == 0).all()
    rel = report("sn normals out", float((np.abs(got[:1000] - ref) / np.maximum(np.abs(ref), 1e-30)).max()), tol=4 * 2.0 ** -24, kind="max relative error")
    assert rel <= 4 * 2.0 ** -24


def test_clip_assemble(engine):
    rng = np.random.default_rng(29)
    T, npp, d = 3, 4, 24
    patches, cls, pos = h16(rng.standard_normal((T * npp, d))), h16(rng.standard_normal(d)), h16(rng.standard_normal((npp + 1, d)))
    got = engine.op_clip_assemble(patches, cls, pos, T, guard=2, fill=FILL)
    _guard(got, T * (npp + 1), "clip assemble")
    _equal(got[:T * (npp + 1)], G.clip_assemble(patches, cls, pos, T), "clip assemble")
