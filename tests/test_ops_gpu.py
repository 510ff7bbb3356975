"""Kernel-level parity: every hand-written HIP kernel, driven through the C ABI, against a plain
torch-CPU fp32 evaluation of the same op on the same (fp16-rounded) inputs.

Tolerance: outputs are stored in fp16 (rel. spacing 2^-11 ~ 4.9e-4) after fp32 accumulation, so the
bound is a few fp16 ulps of the output scale: max|err| / max|ref| < 2e-3 unless stated."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import assert_close, h16, t

pytestmark = pytest.mark.gpu
TOL = 2e-3


def rnd(rng, *shape, scale=1.0):
    return h16(rng.standard_normal(shape) * scale)


@pytest.mark.parametrize("M,K,N", [(128, 64, 128), (200, 320, 320), (77, 1280, 640), (1200, 2560, 1280),
                                   (25, 1024, 320), (1, 320, 1280), (300, 72, 8), (513, 136, 200)])
def test_linear_shapes(engine, M, K, N):
    rng = np.random.default_rng(M * 7 + K + N)
    A, W, b = rnd(rng, M, K), rnd(rng, N, K, scale=K ** -0.5), rnd(rng, N)
    got = engine.op_linear(A, W, b)
    assert_close(got, A @ W.T + b, TOL, f"linear {M}x{K}x{N}")


def test_linear_transpose_detecting(engine):
    # A = I with an asymmetric W catches any row/col swap in the MFMA output mapping
    K = 128
    A = np.eye(K, dtype=np.float32)
    W = h16(np.arange(K * K).reshape(K, K) % 251 / 251.0)
    assert_close(engine.op_linear(A, W), W.T, 1e-3, "identity x asymmetric")


@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_epilogue(engine, act):
    rng = np.random.default_rng(act)
    M, K, N = 260, 192, 320
    A, W, b, R = rnd(rng, M, K), rnd(rng, N, K, scale=K ** -0.5), rnd(rng, N), rnd(rng, M, N)
    got = engine.op_linear(A, W, b, R1=R, c0=0.3, c1=0.7, act=act)
    ref = 0.3 * (A @ W.T + b) + 0.7 * R
    if act == 1:
        ref = F.silu(t(ref)).numpy()
    elif act == 2:
        ref = F.gelu(t(ref)).numpy()
    assert_close(got, ref, TOL, f"epilogue act={act}")


def test_linear_geglu(engine):
    rng = np.random.default_rng(5)
    M, K, inner = 150, 320, 1280
    A, W, b = rnd(rng, M, K), rnd(rng, 2 * inner, K, scale=K ** -0.5), rnd(rng, 2 * inner)
    got = engine.op_linear(A, W, b, geglu=True)
    y = t(A @ W.T + b)
    h, g = y.chunk(2, dim=-1)
    assert_close(got, (h * F.gelu(g)).numpy(), TOL, "geglu")


def conv_ref(x_thwc, w, b, stride=1, pad=(1, 1, 1, 1), ups=1):
    x = t(x_thwc).permute(0, 3, 1, 2)
    if ups == 2:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    x = F.pad(x, pad)
    y = F.conv2d(x, t(w), None if b is None else t(b), stride=stride)
    return y.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("C,O,H,W", [(64, 64, 8, 8), (320, 320, 12, 16), (128, 64, 6, 10), (8, 320, 8, 8), (320, 4, 8, 8)])
def test_conv3x3(engine, C, O, H, W):
    rng = np.random.default_rng(C + O)
    x, w, b = rnd(rng, 2, H, W, C), rnd(rng, O, C, 3, 3, scale=(9 * C) ** -0.5), rnd(rng, O)
    got = engine.op_conv(x, w.reshape(O, C, 1, 3, 3), b)
    assert_close(got, conv_ref(x, w, b), TOL, f"conv3x3 {C}->{O}")


def test_conv_stride2_and_vae_asym_pad(engine):
    rng = np.random.default_rng(11)
    C, O = 64, 128
    x, w, b = rnd(rng, 2, 8, 12, C), rnd(rng, O, C, 3, 3, scale=(9 * C) ** -0.5), rnd(rng, O)
    assert_close(engine.op_conv(x, w.reshape(O, C, 1, 3, 3), b, stride=2), conv_ref(x, w, b, stride=2), TOL, "stride 2 pad 1")
    got = engine.op_conv(x, w.reshape(O, C, 1, 3, 3), b, stride=2, pad_t=0, pad_l=0)
    assert_close(got, conv_ref(x, w, b, stride=2, pad=(0, 1, 0, 1)), TOL, "stride 2 pad (0,1,0,1)")


def test_conv_upsample_and_concat(engine):
    rng = np.random.default_rng(12)
    C0, C1, O = 128, 64, 64
    x0, x1 = rnd(rng, 2, 6, 8, C0), rnd(rng, 2, 6, 8, C1)
    w, b = rnd(rng, O, C0 + C1, 3, 3, scale=(9 * (C0 + C1)) ** -0.5), rnd(rng, O)
    x = np.concatenate([x0, x1], -1)
    assert_close(engine.op_conv(x0, w.reshape(O, C0 + C1, 1, 3, 3), b, x1=x1), conv_ref(x, w, b), TOL, "concat")
    w2 = w[:, :C0]
    assert_close(engine.op_conv(x0, w2.reshape(O, C0, 1, 3, 3), b, ups=2), conv_ref(x0, w2, b, ups=2), TOL, "nearest-2x + conv")
    w1 = rnd(rng, O, C0 + C1, 1, 1, scale=(C0 + C1) ** -0.5)
    got = engine.op_conv(x0, w1.reshape(O, C0 + C1, 1, 1, 1), b, x1=x1, k=1, pad_t=0, pad_l=0)
    assert_close(got, conv_ref(x, w1, b, pad=(0, 0, 0, 0)), TOL, "1x1 shortcut over concat")


@pytest.mark.parametrize("T", [1, 3, 8])
def test_temporal_conv(engine, T):
    rng = np.random.default_rng(T)
    C, H, W = 64, 4, 6
    x, w, b = rnd(rng, T, H, W, C), rnd(rng, C, C, 3, 1, 1, scale=(3 * C) ** -0.5), rnd(rng, C)
    got = engine.op_conv(x, w, b, kt=3, k=1, pad_t=0, pad_l=0)
    x5 = t(x).permute(3, 0, 1, 2)[None]
    ref = F.conv3d(x5, t(w), t(b), padding=(1, 0, 0))[0].permute(1, 2, 3, 0).numpy()
    assert_close(got, ref, TOL, f"temporal conv T={T}")


@pytest.mark.parametrize("C,G,HW,T", [(320, 32, 192, 3), (64, 16, 100, 2), (1280, 32, 48, 2), (32, 8, 4096, 1), (2560, 32, 12, 2)])
@pytest.mark.parametrize("temporal", [False, True])
def test_groupnorm(engine, C, G, HW, T, temporal):
    rng = np.random.default_rng(C + HW)
    x = rnd(rng, T, HW, C) * 2 + 0.5
    gm, bt = rnd(rng, C) + 1, rnd(rng, C)
    got = engine.op_groupnorm(x, G, 1e-6, gm, bt, temporal=temporal, silu=True)
    xt = t(x)
    if temporal:
        y = F.group_norm(xt.permute(2, 0, 1)[None], G, t(gm), t(bt), 1e-6)[0].permute(1, 2, 0)
    else:
        y = F.group_norm(xt.permute(0, 2, 1), G, t(gm), t(bt), 1e-6).permute(0, 2, 1)
    assert_close(got, F.silu(y).numpy(), TOL, f"groupnorm C={C} temporal={temporal}")


def test_groupnorm_concat_groups_straddle_sources(engine):
    rng = np.random.default_rng(3)
    C0, C1, G, HW, T = 1280, 640, 32, 48, 2        # 60 channels per group: group 21 straddles x0|x1
    x0, x1 = rnd(rng, T, HW, C0), rnd(rng, T, HW, C1) * 3
    gm, bt = rnd(rng, C0 + C1) + 1, rnd(rng, C0 + C1)
    got = engine.op_groupnorm(x0, G, 1e-6, gm, bt, x1=x1)
    x = t(np.concatenate([x0, x1], -1))
    ref = F.group_norm(x.permute(0, 2, 1), G, t(gm), t(bt), 1e-6).permute(0, 2, 1).numpy()
    assert_close(got, ref, TOL, "groupnorm over virtual concat")


@pytest.mark.parametrize("C", [64, 320, 640, 1280])
def test_layernorm(engine, C):
    rng = np.random.default_rng(C)
    M = 203
    x, gm, bt = rnd(rng, M, C) * 2 + 0.3, rnd(rng, C) + 1, rnd(rng, C)
    got = engine.op_layernorm(x, 1e-5, gm, bt)
    assert_close(got, F.layer_norm(t(x), (C,), t(gm), t(bt), 1e-5).numpy(), TOL, f"layernorm {C}")
    av = rnd(rng, 3, C)
    y, xo = engine.op_layernorm(x, 1e-5, gm, bt, addvec=av, rows_per_vec=70)
    xs = h16(x + np.repeat(av, 70, 0)[:M])
    assert_close(xo, xs, 1e-3, "layernorm pre-add write-back")
    assert_close(y, F.layer_norm(t(xs), (C,), t(gm), t(bt), 1e-5).numpy(), TOL, "layernorm with pre-add")


def attn_ref(qkv, B, S, H, d):
    q, k, v = t(qkv).reshape(B, S, 3, H, d).permute(2, 0, 3, 1, 4)
    w = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, -1)
    return (w @ v).permute(0, 2, 1, 3).reshape(B * S, H * d).numpy()


@pytest.mark.parametrize("B,H,S", [(1, 1, 64), (2, 2, 48), (2, 1, 192), (1, 2, 200), (1, 1, 1), (2, 5, 768)])
def test_flash_attention(engine, B, H, S):
    rng = np.random.default_rng(S + H)
    qkv = rnd(rng, B * S, 3 * H * 64)
    assert_close(engine.op_flash_attn(qkv, B, H, S), attn_ref(qkv, B, S, H, 64), TOL, f"flash S={S}")


def test_flash_attention_online_softmax_rescale(engine):
    # a late key with a huge score forces the running-max rescale branch in a later KV tile
    rng = np.random.default_rng(9)
    B, H, S = 1, 1, 256
    qkv = rnd(rng, S, 192)
    qkv[:, 64:128][200] = h16(qkv[:, 0:64][5] * 6)       # key 200 aligned with query 5
    assert_close(engine.op_flash_attn(qkv, B, H, S), attn_ref(qkv, B, S, H, 64), TOL, "flash rescale")


@pytest.mark.parametrize("variant", [3, 7, 23, 87])
def test_flash_attention_variants(engine, variant):
    """Every launch form of the d = 64 flash attention (3 = 3-slot ring, 7 = 2-slot ring / 4 workgroups per CU, 23 = + lazy rescale and dot2
    row sums (the default), 87 = 8-wave ping-pong kernel) against the fp32 reference: ragged last tile, single tile, a late huge score
    (reference moved by more than the lazy threshold in a late tile) and a slowly growing maximum (moved by less than the threshold)."""
    try:
        engine.tune_flash(variant)
        for (B, H, S) in [(2, 2, 64), (1, 1, 100), (2, 3, 257), (1, 2, 1000), (3, 1, 129), (1, 1, 513), (2, 1, 1100)]:
            rng = np.random.default_rng(S + H)
            qkv = rnd(rng, B * S, 3 * H * 64)
            assert_close(engine.op_flash_attn(qkv, B, H, S), attn_ref(qkv, B, S, H, 64), TOL, f"flash variant {variant} S={S}")
        rng = np.random.default_rng(9)
        S = 256
        qkv = rnd(rng, S, 192)
        qkv[:, 64:128][200] = h16(qkv[:, 0:64][5] * 6)
        assert_close(engine.op_flash_attn(qkv, 1, 1, S), attn_ref(qkv, 1, S, 1, 64), TOL, f"flash variant {variant} late maximum")
        qkv = rnd(rng, 512, 192)
        qkv[:, 64:128] = h16(qkv[:, 64:128] * (1.0 + np.arange(512)[:, None] / 128.0))      # keys grow: the row maxima creep up tile by tile
        assert_close(engine.op_flash_attn(qkv, 1, 1, 512), attn_ref(qkv, 1, 512, 1, 64), TOL, f"flash variant {variant} creeping maximum")
    finally:
        engine.tune_flash(-1)


@pytest.mark.parametrize("T,HW,H", [(25, 12, 2), (5, 7, 1), (1, 4, 1), (32, 3, 2), (33, 5, 1), (50, 9, 2), (64, 4, 1),
                                    (65, 5, 1), (96, 3, 2), (97, 4, 1), (128, 3, 2)])   # NB = 3 (65..96 frames) and NB = 4 (97..128, 64 KiB of static LDS)
def test_temporal_attention(engine, T, HW, H):
    rng = np.random.default_rng(T)
    qkv = rnd(rng, T * HW, 3 * H * 64)
    got = engine.op_temporal_attn(qkv, T, HW, H)
    # sequence over frames for every pixel: [T,HW,...] -> batch = pixel
    x = qkv.reshape(T, HW, -1).transpose(1, 0, 2).reshape(HW * T, -1)
    ref = attn_ref(x, HW, T, H, 64).reshape(HW, T, -1).transpose(1, 0, 2).reshape(T * HW, -1)
    assert_close(got, ref, TOL, f"temporal attention T={T}")


@pytest.mark.parametrize("B,S,H,d", [(2, 257, 2, 80), (2, 48, 1, 512), (1, 64, 1, 64)])
def test_generic_attention(engine, B, S, H, d):
    rng = np.random.default_rng(S)
    qkv = rnd(rng, B * S, 3 * H * d)
    assert_close(engine.op_attention_generic(qkv, B, S, H, d), attn_ref(qkv, B, S, H, d), TOL, f"generic attn d={d}")


@pytest.mark.parametrize("B,S,H,d", [(2, 257, 2, 80), (3, 50, 1, 80), (1, 64, 2, 128), (2, 130, 3, 32), (1, 257, 16, 80), (2, 77, 2, 96)])
def test_flash_attention_other_head_dims(engine, B, S, H, d):
    """Fused self-attention for head dims other than 64 (flash_attn_dh_kernel; the CLIP ViT-H/14 tower: 16 heads of 80, S = 257): ragged last
    tile, padded d tile, against the fp32 reference and the four-launch path it replaces."""
    rng = np.random.default_rng(S + d)
    qkv = rnd(rng, B * S, 3 * H * d)
    got = engine.op_flash_attn_dh(qkv, B, S, H, d)
    assert_close(got, attn_ref(qkv, B, S, H, d), TOL, f"fused attention d={d} S={S}")
    assert_close(got, engine.op_attention_generic(qkv, B, S, H, d), TOL, f"fused vs four-launch attention d={d} S={S}")


def test_euler_step(engine):
    import sys, os
    from oracle.scheduler import EulerKarrasVPred
    rng = np.random.default_rng(0)
    sch = EulerKarrasVPred(); sch.set_timesteps(5)
    v, x = rnd(rng, 4096), rnd(rng, 4096) * 50
    for i in range(5):
        ref = sch.step(torch.from_numpy(v).half(), i, torch.from_numpy(x).half()).float().numpy()
        got = engine.op_euler_step(v, x, float(sch.sigmas[i]), float(sch.sigmas[i + 1]))
        assert_close(got, ref, 1e-3, f"euler step {i}")


# ---------------------------------------------------------------------------------------------------
# Full-size shapes of the real workload: these are the only sizes at which the 8-wave tile configurations
# (256x64, 256x256, 256x128), split-K and the two-launch/one-launch GroupNorm variants are selected, so parity is
# checked here on a random subset of output rows (the CPU reference of the whole output would take minutes).
# ---------------------------------------------------------------------------------------------------
def _rows(rng, M, n=96):
    return np.sort(rng.choice(M, size=n, replace=False))


@pytest.mark.parametrize("M,K,N,geglu,res", [
    (76800, 1280, 320, False, True),      # level-0 ff.net.2 (+residual): 256x64 tiles
    (76800, 320, 320, False, True),       # level-0 proj / to_out
    (76800, 320, 2560, True, False),      # level-0 GEGLU projection: 256x256 tiles
    (19200, 2560, 640, False, True),      # level-1 ff.net.2: 256x256 tiles (K >= 2048)
    (4800, 1280, 10240, True, False),     # level-2 GEGLU projection
    (1200, 11520, 1280, False, False),    # lowest level, long K: split-K path
    (1200, 1280, 1280, False, True),      # lowest level: 64x64 tiles
])
def test_linear_full_size_spot_check(engine, M, K, N, geglu, res):
    rng = np.random.default_rng(M + K + N)
    A, W, b = rnd(rng, M, K), rnd(rng, N, K, scale=K ** -0.5), rnd(rng, N)
    R = rnd(rng, M, N // 2 if geglu else N) if res else None
    got = engine.op_linear(A, W, b, R1=R, geglu=geglu)
    rows = _rows(rng, M)
    y = t(A[rows] @ W.T + b)
    if geglu:
        h, g = y.chunk(2, dim=-1)
        y = h * F.gelu(g)
    ref = y.numpy() + (R[rows] if res else 0)
    assert np.isfinite(got).all()
    assert_close(got[rows], ref, TOL, f"linear {M}x{K}x{N}")


@pytest.mark.parametrize("T,H,W,C,O,kt,k", [
    (25, 48, 64, 320, 320, 1, 3),     # UNet level 0 conv3x3: M = 76800 -> 256x64 tiles
    (2, 192, 256, 256, 256, 1, 3),    # VAE decoder 256-channel level: M = 98304, N = 256 -> 256x256 tiles
    (1, 384, 512, 128, 128, 1, 3),    # VAE full resolution, N = 128: 256x128 tiles
    (25, 48, 64, 320, 320, 3, 1),     # temporal conv, level 0
    (25, 6, 8, 1280, 1280, 1, 3),     # lowest level conv3x3: split-K
])
def test_conv_full_size_spot_check(engine, T, H, W, C, O, kt, k):
    rng = np.random.default_rng(T * H + C)
    x = rnd(rng, T, H, W, C)
    w = rnd(rng, O, C, kt, k, k, scale=(kt * k * k * C) ** -0.5)
    b = rnd(rng, O)
    got = engine.op_conv(x, w, b, kt=kt, k=k, pad_t=k // 2, pad_l=k // 2)
    assert np.isfinite(got).all()
    # reference on a handful of output pixels: gather the receptive field directly
    rs = np.random.default_rng(1)
    for _ in range(48):
        tt, yy, xx = rs.integers(T), rs.integers(H), rs.integers(W)
        acc = b.astype(np.float64).copy()
        for it in range(kt):
            for iy in range(k):
                for ix in range(k):
                    st, sy, sx = tt + it - kt // 2, yy + iy - k // 2, xx + ix - k // 2
                    if 0 <= st < T and 0 <= sy < H and 0 <= sx < W:
                        acc += w[:, :, it, iy, ix].astype(np.float64) @ x[st, sy, sx].astype(np.float64)
        assert_close(got[tt, yy, xx], acc, TOL, f"conv {T}x{H}x{W} C{C}->{O} at {(tt, yy, xx)}")


def test_groupnorm_full_size(engine):
    rng = np.random.default_rng(8)
    for (T, HW, C, temporal) in [(25, 3072, 320, False), (25, 3072, 320, True), (25, 48, 1280, False), (25, 192, 1280, True)]:
        x = rnd(rng, T, HW, C) + 0.25
        gm, bt = rnd(rng, C) + 1, rnd(rng, C)
        got = engine.op_groupnorm(x, 32, 1e-6, gm, bt, temporal=temporal, silu=True)
        xt = t(x)
        if temporal:
            y = F.group_norm(xt.permute(2, 0, 1)[None], 32, t(gm), t(bt), 1e-6)[0].permute(1, 2, 0)
        else:
            y = F.group_norm(xt.permute(0, 2, 1), 32, t(gm), t(bt), 1e-6).permute(0, 2, 1)
        assert_close(got, F.silu(y).numpy(), TOL, f"groupnorm T{T} HW{HW} C{C} temporal={temporal}")


@pytest.mark.parametrize("T,HW,C0,C1,temporal", [
    (25, 3072, 320, 0, False), (25, 3072, 320, 0, True), (25, 768, 640, 0, False), (25, 768, 640, 640, True),
    (25, 192, 1280, 0, False), (25, 192, 1280, 1280, False), (25, 48, 1280, 1280, True), (25, 48, 1280, 0, False),
    (3, 100, 64, 32, False), (64, 12, 32, 0, True), (25, 768, 640, 640, False), (1, 256, 1280, 0, False), (8, 768, 512, 0, False)])
def test_groupnorm_unet_shapes_two_sources(engine, T, HW, C0, C1, temporal):
    """Every (level, concat, pooled) GroupNorm shape of the UNet, both launch schemes' territory; repeated results must be
    bit-identical (fixed reduction order)."""
    rng = np.random.default_rng(T * HW + C0 + C1)
    C = C0 + C1
    x0 = rnd(rng, T, HW, C0) + 0.25
    x1 = rnd(rng, T, HW, C1) * 2 - 0.5 if C1 else None
    gm, bt = rnd(rng, C) + 1, rnd(rng, C)
    outs = [engine.op_groupnorm(x0, 32, 1e-6, gm, bt, temporal=temporal, silu=True, x1=x1) for _ in range(4)]
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    xt = t(np.concatenate([x0, x1], -1) if C1 else x0)
    if temporal:
        y = F.group_norm(xt.permute(2, 0, 1)[None], 32, t(gm), t(bt), 1e-6)[0].permute(1, 2, 0)
    else:
        y = F.group_norm(xt.permute(0, 2, 1), 32, t(gm), t(bt), 1e-6).permute(0, 2, 1)
    assert_close(outs[0], F.silu(y).numpy(), TOL, f"groupnorm T{T} HW{HW} C{C0}+{C1} temporal={temporal}")


def test_flash_attention_full_size_properties(engine):
    """S = 3072 (UNet level 0): spot-check rows against fp64 softmax attention, and the size-independent property that
    attention is invariant to a permutation of the keys/values."""
    rng = np.random.default_rng(21)
    B, H, S = 2, 5, 3072
    qkv = rnd(rng, B * S, 3 * H * 64)
    got = engine.op_flash_attn(qkv, B, H, S)
    q, k, v = qkv.reshape(B, S, 3, H, 64).transpose(2, 0, 3, 1, 4).astype(np.float64)
    for (b, h, i) in [(0, 0, 0), (1, 4, 3071), (0, 2, 1234), (1, 1, 77)]:
        sc = (k[b, h] @ q[b, h, i]) * 0.125
        p = np.exp(sc - sc.max()); p /= p.sum()
        assert_close(got[b * S + i, h * 64:(h + 1) * 64], p @ v[b, h], TOL, "flash row")
    perm = rng.permutation(S)
    x = qkv.reshape(B, S, 3, H * 64).copy()
    x[:, :, 1:] = x[:, perm][:, :, 1:]                       # permute K and V rows together, keep Q
    got2 = engine.op_flash_attn(x.reshape(B * S, -1), B, H, S)
    assert_close(got2, got, 1e-3, "key-permutation invariance")


# ---------------------------------------------------------------------------------------------------
# Cross-config race screen.  Every tile configuration accumulates K through the same 16x16x32 MFMA chain in the same
# order, so all of them must produce bit-identical outputs (split-K reorders the sum: its own screen, exact on integer data at every factor and on every
# kernel family, is tests/test_splitk_gpu.py); a pipeline race in one kernel variant
# (ring slot reuse, counted vmcnt, the asymmetric-loader kernels = configs 34 / 35 / 39, the producer / consumer kernels = 54 / 59 / 60) shows up as a difference.
# ---------------------------------------------------------------------------------------------------
def _force(engine, cfg):
    engine.tune_force(cfg, 1 if cfg >= 0 else -1)


@pytest.mark.parametrize("cfg", [0, 1, 3, 4, 8, 12, 14, 19, 34, 35, 39, 54, 59, 60, 61, 62, 63, 64])
def test_tile_configs_bitwise_identical_small_ragged(engine, cfg):
    rng = np.random.default_rng(100 + cfg)
    geglu = cfg in (0, 4, 8, 35, 54, 62, 64)
    M, K, N = 2049, 1352 if cfg < 30 else 1344, 640          # ragged M (and K where the flat-address path is taken)
    A, W, b, R = rnd(rng, M, K), rnd(rng, N, K, scale=K ** -0.5), rnd(rng, N), rnd(rng, M, N // 2 if geglu else N)
    x, x1 = rnd(rng, 5, 20, 28, 128), rnd(rng, 5, 20, 28, 64)
    w = rnd(rng, 192, 192, 1, 3, 3, scale=(9 * 192) ** -0.5)
    wt = rnd(rng, 192, 128, 3, 1, 1, scale=(3 * 128) ** -0.5)
    bc = rnd(rng, 192)
    w128 = np.ascontiguousarray(w[:, :128])

    def run():
        return (engine.op_linear(A, W, b, R1=R, geglu=geglu), engine.op_conv(x, w, bc, x1=x1), engine.op_conv(x, w128, bc, ups=2),
                engine.op_conv(x, wt, bc, kt=3, k=1, pad_t=0, pad_l=0), engine.op_conv(x, w128, bc, stride=2),
                engine.op_conv(x, w128, bc, stride=2, pad_t=0, pad_l=0))
    try:
        _force(engine, 15)
        ref = run()
        _force(engine, cfg)
        for rep in range(2):
            for i, (g_, r_) in enumerate(zip(run(), ref)):
                assert np.array_equal(g_, r_), f"cfg {cfg} output {i} run {rep}: max diff {np.abs(g_ - r_).max()}"
    finally:
        _force(engine, -1)
    rows = _rows(rng, M, 32)
    y = t(A[rows] @ W.T + b)
    if geglu:
        h, g2 = y.chunk(2, dim=-1)
        y = h * F.gelu(g2)
    assert_close(ref[0][rows], y.numpy() + R[rows], TOL, "config 15 reference itself")
    assert_close(ref[1], conv_ref(np.concatenate([x, x1], -1), w.reshape(192, 192, 3, 3), bc), TOL, "config 15 conv reference itself")


@pytest.mark.parametrize("M,K,N,geglu", [(76800, 320, 2560, True), (19200, 2560, 640, False), (4800, 5120, 1280, False)])
def test_loader_kernel_bitwise_full_size_dense(engine, M, K, N, geglu):
    rng = np.random.default_rng(M + K)
    A, W, b = rnd(rng, M, K), rnd(rng, N, K, scale=K ** -0.5), rnd(rng, N)
    try:
        _force(engine, 15)
        ref = engine.op_linear(A, W, b, geglu=geglu)
        _force(engine, 35)
        for rep in range(3):
            got = engine.op_linear(A, W, b, geglu=geglu)
            assert np.array_equal(got, ref), f"dense {M}x{K}x{N} run {rep}: {np.abs(got - ref).max()}"
    finally:
        _force(engine, -1)


@pytest.mark.parametrize("T,H,W,C,O,kt,k", [(25, 48, 64, 320, 320, 1, 3), (2, 192, 256, 256, 256, 1, 3), (8, 96, 128, 512, 512, 1, 3),
                                            (25, 24, 32, 640, 640, 3, 1)])
def test_loader_kernel_bitwise_full_size_conv(engine, T, H, W, C, O, kt, k):
    rng = np.random.default_rng(T * H + C)
    x = rnd(rng, T, H, W, C)
    w = rnd(rng, O, C, kt, k, k, scale=(kt * k * k * C) ** -0.5)
    b = rnd(rng, O)
    try:
        _force(engine, 15)
        ref = engine.op_conv(x, w, b, kt=kt, k=k, pad_t=k // 2, pad_l=k // 2)
        _force(engine, 34 if O == 320 else 35)
        for rep in range(3):
            got = engine.op_conv(x, w, b, kt=kt, k=k, pad_t=k // 2, pad_l=k // 2)
            assert np.array_equal(got, ref), f"conv run {rep}: {np.abs(got - ref).max()}"
    finally:
        _force(engine, -1)


@pytest.mark.parametrize("M,C", [(300, 64), (1000, 128), (4096, 192), (5000, 320), (77, 256)])
def test_ff_fused_vs_reference_and_two_launch_path(engine, M, C):
    """Fused GEGLU feed-forward (kernels/ff_fused.hip): c0 * (GEGLU(X W1^T + b1) W2^T + b2) + c1 * R1 against fp32 torch on fp16-rounded
    operands, and against the two-GEMM-launch path it replaces (same roundings: fp16 intermediate, fp32 accumulation)."""
    rng = np.random.default_rng(M + C)
    I = 4 * C
    X = h16(rng.standard_normal((M, C)))
    W1, b1 = h16(rng.standard_normal((2 * I, C)) / np.sqrt(C)), h16(rng.standard_normal(2 * I) * 0.1)
    W2, b2 = h16(rng.standard_normal((C, I)) / np.sqrt(I)), h16(rng.standard_normal(C) * 0.1)
    R1 = h16(rng.standard_normal((M, C)))
    got = engine.op_ff(X, W1, b1, W2, b2, R1=R1, c0=0.7, c1=1.3, fused=True)
    two = engine.op_ff(X, W1, b1, W2, b2, R1=R1, c0=0.7, c1=1.3, fused=False)
    h = t(X) @ t(W1).T + t(b1)
    mid = (h[:, :I] * torch.nn.functional.gelu(h[:, I:])).half().float()
    ref = (0.7 * (mid @ t(W2).T + t(b2)) + 1.3 * t(R1)).numpy()
    assert_close(got, ref, 2e-3, f"fused GEGLU feed-forward {M}x{C}")
    assert_close(got, two, 1.5e-3, f"fused vs two-launch feed-forward {M}x{C}")


@pytest.mark.parametrize("M,C,rpv", [(300, 64, 0), (1000, 128, 250), (5000, 320, 1250), (4100, 320, 4100), (77, 256, 0)])
def test_ff_fused_with_in_kernel_layernorm(engine, M, C, rpv):
    """Pre-norm inside the fused feed-forward kernel (FFusedP::ln_g): x' = fp16(X + row vector), LayerNorm(x') on the LDS tile, residual x'.
    Against fp32 torch on the fp16-rounded operands, and against the LayerNorm launch + fused / two-GEMM paths it replaces (the LayerNorm
    values are rounded to fp16 at the same point in all three, so they agree to fp32-summation-order effects)."""
    rng = np.random.default_rng(M + C)
    I = 4 * C
    X = h16(rng.standard_normal((M, C)) * 2.0 + 0.5)
    gamma, beta = h16(1.0 + 0.2 * rng.standard_normal(C)), h16(0.1 * rng.standard_normal(C))
    W1, b1 = h16(rng.standard_normal((2 * I, C)) / np.sqrt(C)), h16(rng.standard_normal(2 * I) * 0.1)
    W2, b2 = h16(rng.standard_normal((C, I)) / np.sqrt(I)), h16(rng.standard_normal(C) * 0.1)
    av = h16(rng.standard_normal(((M + rpv - 1) // rpv, C))) if rpv else None
    kw = dict(addvec=av, rows_per_vec=max(rpv, 1), eps=1e-5, c0=0.7, c1=1.3)
    got = engine.op_ln_ff(X, gamma, beta, W1, b1, W2, b2, mode=2, **kw)
    one = engine.op_ln_ff(X, gamma, beta, W1, b1, W2, b2, mode=1, **kw)
    two = engine.op_ln_ff(X, gamma, beta, W1, b1, W2, b2, mode=0, **kw)
    xs = t(X)
    if rpv:
        xs = (xs + t(av)[torch.arange(M) // rpv]).half().float()
    ln = torch.nn.functional.layer_norm(xs, (C,), t(gamma), t(beta), 1e-5).half().float()
    h = ln @ t(W1).T + t(b1)
    mid = (h[:, :I] * torch.nn.functional.gelu(h[:, I:])).half().float()
    ref = (0.7 * (mid @ t(W2).T + t(b2)) + 1.3 * xs).numpy()
    assert_close(got, ref, 2e-3, f"fused LayerNorm + feed-forward {M}x{C}")
    assert_close(got, one, 1e-3, f"in-kernel LayerNorm vs LayerNorm launch + fused feed-forward {M}x{C}")
    assert_close(got, two, 1.5e-3, f"in-kernel LayerNorm vs three launches {M}x{C}")


@pytest.mark.parametrize("M,N,bias,res,c0,c1", [
    (76800, 320, True, True, 1.0, 1.0),      # level-0 attention output / proj_out (+ residual)
    (76800, 960, False, False, 1.0, 1.0),    # level-0 fused Q | K | V projection: three column groups
    (19200, 320, True, True, 0.7, 0.3),      # scaled residual blend
    (16420, 640, True, False, 1.0, 1.0),     # ragged last tile (16420 = 513 x 32 + 4), two column groups
    (16384, 320, False, True, 1.0, 1.0),     # the smallest M the planner sends here
])
def test_stream_gemm_bitwise_and_reference(engine, M, N, bias, res, c0, c1):
    """Weight-stationary streaming GEMM of the short-K (K = 320) projections (kernels/gemm_stream.hip: W resident in registers, activation rows
    through a 4-slot LDS ring) against the tiled kernels it replaces (knob 65536 = off): same MFMA chain, same K order -> bit-identical;
    the tiled result against fp32 torch on sampled rows."""
    rng = np.random.default_rng(M + N)
    K = 320
    A, W = rnd(rng, M, K), rnd(rng, N, K, scale=K ** -0.5)
    b = rnd(rng, N) if bias else None
    R = rnd(rng, M, N) if res else None
    try:
        engine.tune_force(-100 - 65536, -1)
        ref = engine.op_linear(A, W, b, R1=R, c0=c0, c1=c1)
        engine.tune_force(-100 - 0, -1)
        got = [engine.op_linear(A, W, b, R1=R, c0=c0, c1=c1) for _ in range(2)]
    finally:
        engine.tune_force(-100 - 0, -1)
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(got[0], ref), f"streaming vs tiled GEMM: max diff {np.abs(got[0] - ref).max()}"
    rows = _rows(rng, M, 64)
    y = c0 * (t(A[rows]) @ t(W).T + (t(b) if bias else 0.0)) + (c1 * t(R[rows]) if res else 0.0)
    assert_close(ref[rows], y.numpy(), TOL, f"tiled reference itself {M}x{N}x{K}")


@pytest.mark.parametrize("T,H,W,C0,C1,O", [
    (1, 16, 16, 64, 0, 128),        # one 16 x 16 tile
    (2, 48, 64, 128, 0, 320),       # 320 columns: level-0 geometry (three 128-column tiles, the third half empty)
    (2, 24, 32, 128, 64, 160),      # two sources, 192-pixel tiles
    (2, 32, 48, 64, 0, 128),        # width 48: three 16-pixel tile columns
    (1, 32, 32, 192, 0, 256),       # three 64-channel chunks
    (2, 12, 16, 128, 0, 256),       # a 12 x 16 frame = one 192-pixel tile (UNet level 2)
    (3, 12, 16, 128, 128, 160),
    (25, 24, 32, 640, 0, 640),      # UNet level 1 at full size
    (2, 96, 128, 128, 0, 128),      # VAE decoder geometry, 128 channels
])
def test_conv_halo_bitwise_and_reference(engine, T, H, W, C0, C1, O):
    """Halo-staged 3x3 convolution (kernels/conv_halo.hip: the activation halo of a 64-channel chunk is fetched once for its nine taps) against the
    im2col GEMM it replaces (knob 16384 = halo off): same products, same K order -> bit-identical; the im2col result itself against torch.
    Knob 32768 keeps the 320-column (level-0) convolutions on the row-split im2col pair they ran on until round 3."""
    rng = np.random.default_rng(T * H * W + C0 + O)
    x0 = rnd(rng, T, H, W, C0)
    x1 = rnd(rng, T, H, W, C1) if C1 else None
    w, b = rnd(rng, O, C0 + C1, 3, 3, scale=(9 * (C0 + C1)) ** -0.5), rnd(rng, O)
    try:
        engine.tune_force(-100 - 16384, -1)
        ref = engine.op_conv(x0, w, b, x1=x1)
        engine.tune_force(-100 - 0, -1)
        got = engine.op_conv(x0, w, b, x1=x1)
        engine.tune_force(-100 - 32768, -1)
        got2 = engine.op_conv(x0, w, b, x1=x1)
    finally:
        engine.tune_force(-100 - 0, -1)
    assert np.array_equal(got, ref), f"halo vs im2col: max diff {np.abs(got - ref).max()}"
    assert np.array_equal(got2, ref), f"knob 32768 vs im2col: max diff {np.abs(got2 - ref).max()}"
    if T * H * W <= 8192:
        xx = np.concatenate([x0, x1], -1) if C1 else x0
        assert_close(ref, conv_ref(xx, w, b), TOL, "im2col reference itself")


@pytest.mark.parametrize("T,H,W,C,O,kt,k,temporal,res,want_rb", [
    (25, 24, 32, 640, 640, 1, 3, False, False, 48),    # UNet level 1, halo kernel on 192 x 128 tiles: blocks of 48 rows
    (25, 24, 32, 640, 640, 1, 3, True, True, 48),      # ... + residual, statistics pooled over the frames (the temporal block's first GroupNorm)
    (25, 48, 64, 320, 320, 1, 3, False, False, 64),    # level 0, halo kernel on 256 x 128 tiles (three column tiles, the third half empty)
    (25, 24, 32, 640, 640, 3, 1, True, True, -1),      # temporal convolution on the producer / consumer kernel (48- or 96-row blocks by wave layout)
    (25, 12, 16, 1280, 1280, 1, 3, False, True, 0),    # level 2: GroupNorm keeps its one-launch slab form there and ignores the partial sums - reported as 0 (round 5: launch_groupnorm says whether it consumed them)
    (2, 96, 128, 128, 128, 1, 3, False, False, 48),    # VAE decoder geometry
    (8, 96, 128, 512, 512, 3, 1, True, True, 128),     # VAE decoder temporal convolution on the 256 x 256 loader tile: 128-row blocks
    (2, 192, 256, 128, 128, 3, 1, True, False, -1),    # ... onto 128 columns (symmetric 256 x 128 or 256 x 64 tile by the planner's choice)
    (3, 20, 24, 64, 64, 1, 3, False, False, 0),        # ragged tiles: the planner's kernel declines, GroupNorm runs its statistics pass
])
def test_groupnorm_statistics_from_conv_epilogue(engine, T, H, W, C, O, kt, k, temporal, res, want_rb):
    """GroupNorm statistics from the producing convolution's epilogue (GemmP::stat_part, tile_epilogue_stats -> gn_finalize_cols) against the
    statistics pass over the stored tensor: the convolution's output is bit-identical (checked inside ug_op_conv_gn), the two GroupNorm outputs
    agree to fp32-summation-order effects on (mean, rstd) - a few fp16 ulps on isolated elements - and both match fp32 torch on the stored tensor."""
    rng = np.random.default_rng(T * H * W + C + kt)
    x = rnd(rng, T, H, W, C)
    w = rnd(rng, O, C, kt, k, k, scale=(kt * k * k * C) ** -0.5)
    b = rnd(rng, O)
    r = rnd(rng, T, H, W, O) if res else None
    gamma, beta = h16(1.0 + 0.2 * rng.standard_normal(O)), h16(0.1 * rng.standard_normal(O))
    co, y_pass, y_epi, rb = engine.op_conv_gn(x, w, b, 32, 1e-5, gamma, beta, res=r, kt=kt, k=k, temporal=temporal)
    if want_rb >= 0:
        assert rb == want_rb, f"rows per statistics block {rb}, expected {want_rb}"
    else:
        assert rb in (48, 64, 96, 128), rb
    xt = torch.from_numpy(co.reshape(T, H * W, O)).float()
    G, cpg = 32, O // 32
    xg = xt.reshape(T, H * W, G, cpg)
    dims = (0, 1, 3) if temporal else (1, 3)
    mean = xg.mean(dim=dims, keepdim=True)
    var = xg.var(dim=dims, keepdim=True, unbiased=False)
    yn = ((xg - mean) / torch.sqrt(var + 1e-5)).reshape(T, H * W, O) * t(gamma) + t(beta)
    ref = torch.nn.functional.silu(yn).numpy().reshape(T, H, W, O)
    assert_close(y_pass, ref, 2e-3, "GroupNorm with a statistics pass")
    assert_close(y_epi, ref, 2e-3, "GroupNorm with the statistics from the convolution's epilogue")
    d = np.abs(y_epi - y_pass)
    assert d.max() <= 4e-3 * max(1.0, float(np.abs(ref).max())), f"epilogue vs pass statistics: max diff {d.max()}"
    assert (d > 0).mean() < 0.02, f"epilogue vs pass statistics: {(d > 0).mean():.3%} of the elements differ"


# -1 = the planner's tiles, the others force one tile family each (tests/test_wide_gpu.py forces the same list on float32-output launches)
LEAN_EPILOGUE_CFGS = [-1, 0, 3, 14, 15, 19, 35, 54, 59, 61, 62, 63, 64]


@pytest.mark.parametrize("cfg", LEAN_EPILOGUE_CFGS)
def test_lean_epilogue_forms_equal_the_general_epilogue_bit_for_bit(engine, cfg):
    """Round 6: every GEMM-family kernel takes a compile-time form of its epilogue for the common cases (tile_epilogue_lean, tile_epilogue_geglu_lean, modes 1 / 2 of
    the statistics epilogue; kernels/gemm_common.h), chosen per launch from a launch-uniform test.  Knob 8388608 sends every launch through the general epilogue with
    its run-time variants instead: the outputs must be identical bit for bit - dense with / without bias and residual, GEGLU, ragged M, 3x3 convolutions on the
    halo-staged kernels with and without the GroupNorm statistics epilogue, a temporal convolution, a stride-2 convolution, and a residual scale c1 != 1 (general form
    on both sides).  cfg -1 = the planner's tiles (halo kernels, producer / consumer kernels), the others force one tile family each."""
    rng = np.random.default_rng(900 + cfg)
    M, K, N = 2049, 1344, 640
    A, Wd, b, R = rnd(rng, M, K), rnd(rng, N, K, scale=K ** -0.5), rnd(rng, N), rnd(rng, M, N)
    Rg = rnd(rng, M, N // 2)
    x = rnd(rng, 3, 48, 64, 128)
    w3 = rnd(rng, 256, 128, 1, 3, 3, scale=(9 * 128) ** -0.5)
    wt = rnd(rng, 128, 128, 3, 1, 1, scale=(3 * 128) ** -0.5)
    b3, bt = rnd(rng, 256), rnd(rng, 128)
    res = rnd(rng, 3, 48, 64, 256)
    gamma, beta = h16(1.0 + 0.2 * rng.standard_normal(256)), h16(0.1 * rng.standard_normal(256))
    geglu_ok = cfg in (-1, 0, 15, 35, 54, 62, 64)

    def run():
        outs = [engine.op_linear(A, Wd, b, R1=R), engine.op_linear(A, Wd, b), engine.op_linear(A, Wd), engine.op_linear(A, Wd, b, R1=R, c1=0.75),
                engine.op_conv(x, w3, b3), engine.op_conv(x, wt, bt, kt=3, k=1, pad_t=0, pad_l=0), engine.op_conv(x, w3, b3, stride=2)]
        if geglu_ok:
            outs.append(engine.op_linear(A, Wd, b, geglu=True))
        outs += list(engine.op_conv_gn(x, w3, b3, 32, 1e-5, gamma, beta, res=res)[:3])
        outs += list(engine.op_conv_gn(x, w3, b3, 32, 1e-5, gamma, beta)[:3])
        return outs
    try:
        _force(engine, cfg)
        engine.tune_force(-100 - 8388608, 0)
        ref = run()
        engine.tune_force(-100, 0)
        got = run()
        for i, (g_, r_) in enumerate(zip(got, ref)):
            assert np.array_equal(g_, r_), f"cfg {cfg} output {i}: lean vs general epilogue, max diff {np.abs(g_ - r_).max()}"
    finally:
        engine.tune_force(-100, 0)
        _force(engine, -1)
    y = t(A) @ t(Wd).T + t(b) + t(R)
    assert_close(got[0], y.numpy(), TOL, "dense + bias + residual")


@pytest.mark.parametrize("cfg,want_rb", [(14, 64), (19, 128), (35, 128), (54, 64), (59, 128), (63, 96), (64, 48)])
def test_statistics_epilogue_on_every_instantiated_tile(engine, cfg, want_rb):
    """Every general tile that is instantiated with the statistics epilogue, forced on one temporal convolution (the planner would pick one of them):
    block size as documented, convolution output unchanged (checked inside the op), GroupNorm equal to the statistics-pass form."""
    rng = np.random.default_rng(cfg)
    T, H, W, C = 4, 96, 128, 256
    x = rnd(rng, T, H, W, C)
    w = rnd(rng, C, C, 3, 1, 1, scale=(3 * C) ** -0.5)
    b, r = rnd(rng, C), rnd(rng, T, H, W, C)
    gamma, beta = h16(1.0 + 0.2 * rng.standard_normal(C)), h16(0.1 * rng.standard_normal(C))
    try:
        engine.tune_force(cfg, 1)
        co, y_pass, y_epi, rb = engine.op_conv_gn(x, w, b, 32, 1e-5, gamma, beta, res=r, kt=3, k=1, temporal=True)
    finally:
        engine.tune_force(-1, -1)
    assert rb == want_rb, f"config {cfg}: rows per statistics block {rb}, expected {want_rb}"
    d = np.abs(y_epi - y_pass)
    assert d.max() <= 4e-3 * max(1.0, float(np.abs(y_pass).max())) and (d > 0).mean() < 0.02, f"config {cfg}: max diff {d.max()}, {(d > 0).mean():.3%} differ"


@pytest.mark.parametrize("C1", [0, 320])
def test_conv_row_split_bitwise_full_size(engine, C1):
    """3x3 convolution onto 320 channels at the clip's level-0 size (25 x 48 x 64 = 76800 rows): launch_gemm runs the rows of the whole rounds
    on 256x160 tiles and the remaining 11264 rows as a second launch with a row offset (GemmP::m_off) - since round 4 only under knob 32768,
    the default being one launch of the halo kernel.  All three forms bit-identical (knob 1024 = im2col in a single launch), spot-checked against torch."""
    rng = np.random.default_rng(320 + C1)
    T, H, W, C0, O = 25, 48, 64, 320, 320
    x = rnd(rng, T, H, W, C0)
    x1 = rnd(rng, T, H, W, C1) if C1 else None
    w = rnd(rng, O, C0 + C1, 1, 3, 3, scale=(9 * (C0 + C1)) ** -0.5)
    b = rnd(rng, O)
    try:
        halo = engine.op_conv(x, w, b, x1=x1)                     # round 4 default: ONE launch of the halo kernel on 256 x 128 tiles
        engine.tune_force(-100 - 32768, 0)
        got = engine.op_conv(x, w, b, x1=x1)                      # knob 32768: the row-split im2col pair (the default until round 3)
        engine.tune_force(-100 - 32768 - 1024, 0)
        one = engine.op_conv(x, w, b, x1=x1)                      # + knob 1024: im2col in a single launch
    finally:
        engine.tune_force(-100, 0)
    assert np.array_equal(got, one), f"row split changes the result: max diff {np.abs(got - one).max()}"
    assert np.array_equal(halo, one), f"halo kernel vs im2col: max diff {np.abs(halo - one).max()}"
    xin = x if x1 is None else np.concatenate([x, x1], -1)
    for t_ in (0, 21, 24):        # frame 21 straddles the split row (65536 = 21 frames + 1024 rows)
        ref = conv_ref(xin[t_:t_ + 1], w.reshape(O, C0 + C1, 3, 3), b)
        assert_close(got[t_:t_ + 1], ref, TOL, f"row-split conv frame {t_}")
