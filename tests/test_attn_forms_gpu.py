"""The launch forms of the head-dim-64 attention kernels that packed self-attention of one video does not reach, op by op through the C ABI:

  * flash cross-attention (FlashP::Sk != 0, kv_shared, separate row strides; K and V side by side in one buffer) - what every StableNormal
    transformer block runs with 77 shared prompt tokens - under each launch form of the kernel (3 = 3-slot ring, 7 = 2-slot ring / 4 workgroups
    per CU, 23 = + lazy rescale and dot2 row sums (the default), 87 = 8-wave ping-pong kernel);
  * temporal attention over stacked videos (TemporalAttnP::nv > 1, grid dimension z) - the guided UNet pass.

Reference: tests/attn_oracle.py, plain float64 softmax attention on the fp16-rounded inputs.  Tolerance: test_ops_gpu.py's bound for
fp16-stored outputs after fp32 accumulation, max|err| / max|ref| < 2e-3; "bit-identical" is np.array_equal."""
import functools

import numpy as np
import pytest

import attn_oracle as ao
from util import assert_close, h16

pytestmark = pytest.mark.gpu
TOL = 2e-3
VARIANTS = [3, 7, 23, 87]


def rnd(rng, *shape, scale=1.0):
    return h16(rng.standard_normal(shape) * scale)


def run_cross(engine, q, k, v, B, H, S, Sk, kv_shared):
    """Tight buffers (ldq = ldo = C, ldkv = 2C, no guard) -> [B*S, C]."""
    C = H * 64
    return engine.op_flash_cross_attn(q, ao.pack_kv(k, v, 2 * C), ao.out_buffer(B * S, C), B, H, S, Sk, kv_shared)


# (B, H, S, Sk, kv_shared): every Sk of {1, 13 (one ragged tile), 64 (one full tile), 65, 77 (the prompt), 141 (more tiles than the 2-slot ring
# holds ahead), 200 (more than the 3-slot and ping-pong prologues stage)} and every S of {8, 100, 129 (one row in a second 128-row workgroup),
# 513 (one row in a second 512-row ping-pong workgroup)} meet at least twice, H in {1, 2, 5}, B in {1, 2, 3}, both kv_shared for B > 1; the
# last two have a workgroup count of 8, so the XCD-grouped order is taken (nqb = 1 and nqb = 2)
CROSS_CASES = [
    (1, 1, 8, 1, 0), (2, 2, 100, 13, 1), (3, 5, 129, 64, 0), (1, 2, 513, 65, 0), (2, 1, 8, 77, 0), (3, 2, 100, 141, 1), (1, 5, 129, 200, 0),
    (2, 1, 513, 13, 1), (2, 5, 8, 200, 1), (3, 1, 100, 65, 0), (1, 1, 129, 141, 0), (2, 2, 513, 77, 0), (3, 2, 8, 64, 1), (2, 1, 129, 1, 1),
    (2, 4, 100, 64, 1), (1, 4, 200, 77, 1),
]


@functools.lru_cache(maxsize=None)
def cross_case(B, H, S, Sk, kv_shared):
    """Inputs and float64 reference of one case, made once for the four variants (read-only)."""
    rng = np.random.default_rng(1000 * S + 10 * Sk + H + B)
    C, rows_kv = H * 64, (1 if kv_shared else B) * Sk
    q, k, v = rnd(rng, B * S, C), rnd(rng, rows_kv, C), rnd(rng, rows_kv, C)
    ref = ao.cross_attn_ref(q, k, v, B, H, S, Sk, kv_shared)
    for a in (q, k, v, ref):
        a.setflags(write=False)
    return q, k, v, ref


@pytest.mark.parametrize("variant", VARIANTS)
def test_cross_attention_against_float64(engine, variant):
    try:
        engine.tune_flash(variant)
        for (B, H, S, Sk, kv_shared) in CROSS_CASES:
            q, k, v, ref = cross_case(B, H, S, Sk, kv_shared)
            got = run_cross(engine, q, k, v, B, H, S, Sk, kv_shared)
            assert_close(got, ref, TOL, f"flash cross variant {variant} B={B} H={H} S={S} Sk={Sk} shared={kv_shared}")
    finally:
        engine.tune_flash(-1)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,H,S", [(2, 2, 100), (1, 3, 257)])
def test_cross_entry_with_own_keys_is_self_attention_bit_for_bit(engine, variant, B, H, S):
    """Sk = S, one context per batch, K and V copied out of a packed qkv: the same kernel and arithmetic as op_flash_attn, only the bases and
    strides differ.  Sk = 0 (production's spelling of self-attention) must be the same launch again."""
    C = H * 64
    qkv = rnd(np.random.default_rng(S + H), B * S, 3 * C)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    try:
        engine.tune_flash(variant)
        want = engine.op_flash_attn(qkv, B, H, S)
        assert_close(want, ao.cross_attn_ref(q, k, v, B, H, S, 0, 0), TOL, f"flash packed variant {variant} S={S}")
        assert np.array_equal(run_cross(engine, q, k, v, B, H, S, S, 0), want)
        assert np.array_equal(run_cross(engine, q, k, v, B, H, S, 0, 0), want)
    finally:
        engine.tune_flash(-1)


@pytest.mark.parametrize("variant", VARIANTS)
def test_kv_shared_is_the_context_repeated(engine, variant):
    B, H, S, Sk = 3, 2, 100, 77
    q, k, v, ref = cross_case(B, H, S, Sk, 1)
    try:
        engine.tune_flash(variant)
        shared = run_cross(engine, q, k, v, B, H, S, Sk, 1)
        assert_close(shared, ref, TOL, f"flash cross variant {variant} kv_shared, 3 batches")
        assert np.array_equal(run_cross(engine, q, np.tile(k, (B, 1)), np.tile(v, (B, 1)), B, H, S, Sk, 0), shared)
    finally:
        engine.tune_flash(-1)


@pytest.mark.parametrize("variant", VARIANTS)
def test_key_selector(engine, variant):
    """One-hot keys and queries: output row i of head h must BE row pi[h, i] of that head's V (tests/attn_oracle.py: the float64 reference
    leaves < 1e-6, shown on the CPU) - a wrong key row, head column or K / V swap cannot hide inside a tolerance as it can with random data.
    Bound: fp16 storage of V-scale values, 1e-3 of max|V|, as in test_linear_transpose_detecting."""
    q, k, v, pi = ao.selector_inputs()
    try:
        engine.tune_flash(variant)
        got = run_cross(engine, q, k, v, 1, ao.SEL_H, ao.SEL_S, ao.SEL_SK, 0)
        assert_close(got, ao.selector_expected(v, pi), 1e-3, f"flash cross variant {variant} key selector")
    finally:
        engine.tune_flash(-1)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("Sk", [13, 77, 128])
def test_nothing_outside_the_operands_is_read_or_written(engine, variant, Sk):
    """NaN in every element next to the operands (surplus columns of q and kv, 70 rows after the last K / V row - Sk = 128 has no ragged
    tile: only the buffer descriptor's bound keeps the prologue's extra tiles out), 7.0 around the output.  The poisoned memory is allocated."""
    B, H, S = 2, 2, 100
    C = H * 64
    try:
        engine.tune_flash(variant)
        for kv_shared in (0, 1):
            (qb, kvb, ob), (q, k, v) = ao.poisoned_inputs(np.random.default_rng(Sk + kv_shared), B, H, S, Sk, kv_shared)
            got = engine.op_flash_cross_attn(qb, kvb, ob, B, H, S, Sk, kv_shared, guard=ao.POISON_GUARD)
            assert got.shape == ob.shape
            assert np.isfinite(got).all()
            assert_close(got[:B * S, :C], ao.cross_attn_ref(q, k, v, B, H, S, Sk, kv_shared), TOL,
                         f"flash cross variant {variant} Sk={Sk} shared={kv_shared} poisoned surroundings")
            assert (ao.outside(got, B * S, C) == ao.POISON_SENTINEL).all()
    finally:
        engine.tune_flash(-1)


def test_bad_calls_are_errors_and_the_context_stays_usable(engine):
    B, H, S, Sk = 2, 2, 100, 77
    C = H * 64
    q, k, v, ref = cross_case(B, H, S, Sk, 1)
    kv = ao.pack_kv(k, v, 2 * C)
    z = lambda rows, cols: np.zeros((rows, cols), np.float32)
    with pytest.raises(RuntimeError):      # S = 0
        engine.op_flash_cross_attn(z(0, C), kv, z(0, C), B, H, 0, Sk, 1)
    with pytest.raises(RuntimeError):      # Sk < 0
        engine.op_flash_cross_attn(q, kv, z(B * S, C), B, H, S, -1, 1)
    with pytest.raises(RuntimeError):      # ldq not a multiple of 8
        engine.op_flash_cross_attn(ao.pack_q(q, C + 4), kv, z(B * S, C), B, H, S, Sk, 1)
    with pytest.raises(RuntimeError):      # ldkv < 2 * H * 64
        engine.op_flash_cross_attn(q, np.ascontiguousarray(kv[:, :2 * C - 8]), z(B * S, C), B, H, S, Sk, 1)
    assert_close(run_cross(engine, q, k, v, B, H, S, Sk, 1), ref, TOL, "flash cross after rejected calls")


VIDEO_SCALE = (1.0, 3.0, 0.25)


@pytest.mark.parametrize("nv,T,HW,H", [(2, 5, 5, 1), (3, 5, 7, 2), (3, 33, 5, 2), (2, 33, 7, 1), (2, 97, 5, 2), (3, 97, 7, 1)])
def test_temporal_attention_stacked_videos(engine, nv, T, HW, H):
    """T = 5 / 33 / 97: 1 / 2 / 4 blocks of 32 frames; HW = 5, 7: the last workgroup of 4 pixels has waves that leave early.  Each video has
    its own magnitude, so a row read from the neighbouring video moves the result by far more than TOL."""
    rng = np.random.default_rng(100 * T + 10 * HW + nv)
    M, C = T * HW, H * 64
    qkv = np.concatenate([rnd(rng, M, 3 * C, scale=VIDEO_SCALE[n]) for n in range(nv)])
    got = engine.op_temporal_attn_nv(qkv, nv, T, HW, H)
    ref = ao.temporal_attn_ref(qkv, nv, T, HW, H)
    for n in range(nv):
        rows = slice(n * M, (n + 1) * M)
        assert_close(got[rows], ref[rows], TOL, f"temporal attention nv={nv} T={T} HW={HW} H={H} video {n}")
        assert np.array_equal(got[rows], engine.op_temporal_attn(qkv[rows], T, HW, H))
