"""CPU: the float64 attention references of tests/attn_oracle.py against torch.softmax, and the preconditions of the structured inputs that
tests/test_attn_forms_gpu.py feeds the kernels - shown by the reference alone, so a failure there is the kernel's."""
import numpy as np
import pytest
import torch

import attn_oracle as ao


def torch_cross(q, k, v, B, H, S, Sk, kv_shared):
    nb = 1 if kv_shared else B
    qt = torch.from_numpy(ao.h16(q)).double().reshape(B, S, H, 64).permute(0, 2, 1, 3)
    kt = torch.from_numpy(ao.h16(k)).double().reshape(nb, Sk, H, 64).permute(0, 2, 1, 3).expand(B, H, Sk, 64)
    vt = torch.from_numpy(ao.h16(v)).double().reshape(nb, Sk, H, 64).permute(0, 2, 1, 3).expand(B, H, Sk, 64)
    w = torch.softmax(qt @ kt.transpose(-1, -2) * 0.125, -1)
    return (w @ vt).permute(0, 2, 1, 3).reshape(B * S, H * 64).numpy()


@pytest.mark.parametrize("B,H,S,Sk,kv_shared", [(2, 2, 10, 77, 1), (3, 1, 37, 13, 0)])
def test_cross_reference_equals_torch_softmax(B, H, S, Sk, kv_shared):
    rng = np.random.default_rng(S + Sk)
    C, rows_kv = H * 64, (1 if kv_shared else B) * Sk
    q, k, v = (rng.standard_normal((r, C)) * 2 for r in (B * S, rows_kv, rows_kv))
    ref = ao.cross_attn_ref(q, k, v, B, H, S, Sk, kv_shared)
    assert ref.dtype == np.float64
    assert np.abs(ref - torch_cross(q, k, v, B, H, S, Sk, kv_shared)).max() < 1e-12
    if not kv_shared:      # Sk = 0 is self-attention over the same rows when Sk == S
        assert np.array_equal(ao.cross_attn_ref(q[:B * Sk], k, v, B, H, Sk, 0, 0), ao.cross_attn_ref(q[:B * Sk], k, v, B, H, Sk, Sk, 0))


@pytest.mark.parametrize("nv,T,HW,H", [(2, 5, 3, 2), (3, 33, 2, 1)])
def test_temporal_reference_equals_torch_softmax(nv, T, HW, H):
    rng = np.random.default_rng(T)
    C = H * 64
    qkv = rng.standard_normal((nv * T * HW, 3 * C))
    ref = ao.temporal_attn_ref(qkv, nv, T, HW, H).reshape(nv, T, HW, C)
    x = ao.h16(qkv).reshape(nv, T, HW, 3 * C)
    for n in range(nv):
        for p in range(HW):        # one plain attention per (video, pixel): the sequence is that video's T frames
            s = x[n, :, p]
            want = torch_cross(s[:, :C], s[:, C:2 * C], s[:, 2 * C:], 1, H, T, T, 0)
            assert np.abs(ref[n, :, p] - want).max() < 1e-12


def test_selector_reference_is_the_selected_value_row():
    q, k, v, pi = ao.selector_inputs()
    assert q.shape == (150, 128) and k.shape == v.shape == (61, 128) and pi.shape == (2, 150)
    for a in (q, k, v):
        assert np.array_equal(a, ao.h16(a))                  # exact in fp16: the kernel sees these numbers
    assert (pi[0] != pi[1]).any() and len(np.unique(pi)) > 50    # the heads select differently, nearly every key is selected
    ref = ao.cross_attn_ref(q, k, v, 1, ao.SEL_H, ao.SEL_S, ao.SEL_SK, 0)
    want = ao.selector_expected(v, pi)
    assert np.abs(ref - want).max() < 1e-6
    # what the test tells apart: a neighbouring key row, the other head's columns and K in V's place are all far outside its bound
    bound = 1e-3 * np.abs(v).max()
    assert np.abs(ao.selector_expected(v, (pi + 1) % ao.SEL_SK) - want).max() > 100 * bound
    assert np.abs(ao.selector_expected(v, pi[::-1]) - want).max() > 100 * bound
    assert np.abs(ao.selector_expected(k, pi) - want).max() > 100 * bound


@pytest.mark.parametrize("Sk", [13, 77, 128])
@pytest.mark.parametrize("kv_shared", [0, 1])
def test_poisoned_inputs_leave_the_reference_finite(Sk, kv_shared):
    B, H, S = 2, 2, 100
    C, rows_kv = H * 64, (1 if kv_shared else B) * Sk
    (qb, kvb, ob), (q, k, v) = ao.poisoned_inputs(np.random.default_rng(Sk), B, H, S, Sk, kv_shared)
    assert qb.shape == (B * S, C + 8) and kvb.shape == (rows_kv + 70, 2 * C + 8) and ob.shape == (B * S + 70, C + 4)
    # the poison is where it should be, and nowhere inside the operands
    assert np.isnan(ao.outside(qb, B * S, C)).all() and np.isnan(ao.outside(kvb, rows_kv, 2 * C)).all()
    assert (ao.outside(ob, B * S, C) == ao.POISON_SENTINEL).all() and ao.outside(ob, B * S, C).size == B * S * 4 + 70 * (C + 4)
    kk, vv = ao.unpack_kv(kvb, rows_kv, C)
    ref = ao.cross_attn_ref(qb[:, :C], kk, vv, B, H, S, Sk, kv_shared)
    assert np.isfinite(ref).all()
    assert np.array_equal(ref, ao.cross_attn_ref(q, k, v, B, H, S, Sk, kv_shared))
