"""CPU: the general-head-dim attention oracle against torch's scaled_dot_product_attention in float64, the batched-GEMM reference against a plain
loop, and the preconditions of the structured inputs of tests/test_attn_general_gpu.py, shown on the float64 reference alone."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_general_oracle as go

FUSED_D = [32, 48, 80, 96, 112, 128]
GPU_TOL = 2e-3


@pytest.mark.parametrize("B,S,H,d", [(2, 77, 3, 80), (1, 130, 2, 48)])
def test_oracle_is_torch_sdpa_in_float64(B, S, H, d):
    qkv = go.scaled_qkv(np.random.default_rng(S), B, S, H, d)
    q, k, v = (torch.from_numpy(a) for a in go.split_heads(qkv, B, S, H, d))
    want = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(B * S, H * d).numpy()
    got = go.attn_ref(qkv, B, S, H, d)
    assert got.dtype == np.float64 and np.abs(got - want).max() < 1e-12 * np.abs(want).max()


def test_oracle_ignores_surplus_columns_and_rows():
    B, S, H, d = 2, 33, 2, 48
    qkv = go.scaled_qkv(np.random.default_rng(0), B, S, H, d)
    buf, out = go.poisoned_buffers(qkv, B, S, H, d)
    assert buf.shape == (B * S + go.POISON_GUARD, 3 * H * d + 8) and out.shape == (B * S + go.POISON_GUARD, H * d + 4)
    assert np.isnan(buf[:, 3 * H * d:]).all() and np.isnan(buf[B * S:]).all() and (out == go.POISON_SENTINEL).all()
    assert buf.shape[1] % 8 == 0 and out.shape[1] % 4 == 0
    assert np.array_equal(go.attn_ref(buf, B, S, H, d), go.attn_ref(qkv, B, S, H, d))


def test_scaled_inputs_tell_neighbours_apart():
    """Every block's neighbours along the batch and along the head axis have another magnitude."""
    B, S, H, d = 3, 64, 3, 32
    qkv = go.scaled_qkv(np.random.default_rng(1), B, S, H, d)
    q = qkv[:, :H * d]
    rms = np.array([[np.sqrt((go.head_block(q, b, h, S, d) ** 2).mean()) for h in range(H)] for b in range(B)])
    assert np.allclose(rms, [[go.BH_SCALE[(b + h) % 3] for h in range(H)] for b in range(B)], rtol=0.1)
    assert (np.abs(np.log(rms[1:] / rms[:-1])) > 1).all() and (np.abs(np.log(rms[:, 1:] / rms[:, :-1])) > 1).all()


@pytest.mark.parametrize("d,H,S,B", [(d, 2, d, 1) for d in FUSED_D] + [(128, 1, 128, 2), (512, 1, 257, 2), (80, 2, 80, 2), (48, 3, 48, 1), (64, 1, 64, 3)])
def test_selector_reference_is_the_selected_rows(d, H, S, B):
    qkv, pi = go.selector_inputs(d, H, S, B)
    assert np.array_equal(qkv, go.h16(qkv))
    want = go.selector_expected(qkv, pi, d)
    assert want.shape == (B * S, H * d)
    # the selected score: 256 / sqrt(d) >= 22.6 nats up to d = 128 (leakage 127 e^-22.6 = 2e-8), 1024 / sqrt(512) = 45 at d = 512
    assert go.selector_amp(d) ** 2 / np.sqrt(d) > 22.6
    assert np.abs(go.attn_ref(qkv, B, S, H, d) - want).max() < 1e-6
    # the expected rows differ from head to head, from batch to batch, and from the K columns
    for b in range(B):
        for h in range(1, H):
            assert not np.array_equal(go.head_block(want, b, h, S, d), go.head_block(want, b, h - 1, S, d))
    if B > 1:
        assert not np.array_equal(want[:S], want[S:2 * S])


@pytest.mark.parametrize("d", [48, 80, 128])
def test_rising_maxima_preconditions(d):
    S, H = go.RISE_S, go.RISE_H
    assert S > 128 and S % 32 == 0
    qkv = go.rising_inputs(d)
    assert np.array_equal(qkv, go.h16(qkv)) and np.isfinite(qkv).all()
    s = go.scores(qkv, 1, S, H, d)[0]                                   # [H, S, S]
    blockmax = s.reshape(H, S, S // 32, 32).max(-1)                     # [H, query, block]
    runmax = np.maximum.accumulate(blockmax, axis=-1)
    for b in range(1, S // 32):
        if b == go.RISE_DIP:      # lower than its predecessor, for every query: the running maximum stays (alpha = 1)
            assert (blockmax[..., b] < blockmax[..., b - 1]).all()
        else:                     # >= 8 nats above everything seen before, for every query: alpha <= e^-8
            assert (blockmax[..., b] - runmax[..., b - 1] >= 8.0).all()
    ref = go.attn_ref(qkv, 1, S, H, d)
    last = go.last_block_only_ref(qkv, S, H, d)
    assert np.abs(ref - last).max() > 10 * GPU_TOL * np.abs(ref).max()       # the early tiles matter
    assert np.abs(ref).max() < 100.0


def test_gemm_batched_reference_and_offsets():
    """The strided reference against a plain loop over (bo, bi) on the P V form: fp16-width output scattered into head columns."""
    rng = np.random.default_rng(3)
    B, H, S, d = 2, 3, 9, 16
    Sp = go.pad8(S)
    ldo = H * d + 4
    P, Vt = go.ternary(rng, B * H * S * Sp), go.ternary(rng, B * H * d * Sp)
    out = np.full((B * S, ldo), 7.0, np.float32)
    got = go.gemm_batched_ref(P, Sp, (H * S * Sp, S * Sp), Vt, Sp, (H * d * Sp, d * Sp), S, d, Sp, B * H, H, out, ldo, (S * ldo, d),
                              dtype=np.int64).reshape(B * S, ldo)
    assert got.dtype == np.int64 and (got[:, H * d:] == 7).all()
    Pm, Vm = P.reshape(B, H, S, Sp).astype(np.int64), Vt.reshape(B, H, d, Sp).astype(np.int64)
    for b in range(B):
        for h in range(H):
            assert np.array_equal(go.head_block(got, b, h, S, d), Pm[b, h] @ Vm[b, h].T)
    assert go.batch_offsets(6, 3, (100, 7)) == [0, 7, 14, 100, 107, 114]
    assert np.abs(got).max() <= Sp <= 2048
