"""Plain float64 softmax attention on fp16-rounded inputs for ANY head dim (test helper) - the yardstick of tests/test_attn_general_*.py for the two
attention paths that serve every head dim but 64 (the fused flash_attn_dh_kernel<DH> and the four-launch unfused_attention) and an exact
float64 / int64 reference of the batched GEMMs under the second.

out[b, i, h] = sum_j softmax_j(d^-0.5 * <q[b, i, h], k[b, j, h]>) v[b, j, h] on packed qkv [B*S, >= 3*H*d] (columns q | k | v), evaluated with the
row maximum subtracted, nothing else (attn_oracle._softmax_av; attn_oracle.D stays 64).  The builders of the structured inputs (key selector,
rising maxima, poisoned surroundings, integer GEMM operands) live here too, so that the CPU test can check their preconditions by the reference
alone and the GPU test uses the very same arrays.  Nothing here imports the package under test."""
import numpy as np

import attn_oracle as ao
from attn_oracle import POISON_GUARD, POISON_SENTINEL, h16, outside  # noqa: F401  (re-exported)

BH_SCALE = (1.0, 3.0, 0.25)     # magnitude of batch b, head h: BH_SCALE[(b + h) % 3], as VIDEO_SCALE of test_attn_forms_gpu.py


def split_heads(qkv, B, S, H, d):
    """qkv [>= B*S, >= 3*H*d] -> q, k, v float64 [B, H, S, d] of the fp16-rounded values."""
    x = h16(np.asarray(qkv)[:B * S, :3 * H * d]).astype(np.float64).reshape(B, S, 3, H, d).transpose(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def attn_ref(qkv, B, S, H, d):
    """-> float64 [B*S, H*d]."""
    q, k, v = split_heads(qkv, B, S, H, d)
    return ao._softmax_av(q, k, v, d ** -0.5).transpose(0, 2, 1, 3).reshape(B * S, H * d)


def scores(qkv, B, S, H, d):
    """-> float64 [B, H, S, S], the scaled scores (natural-log units)."""
    q, k, _ = split_heads(qkv, B, S, H, d)
    return np.einsum("nhqd,nhkd->nhqk", q, k) * d ** -0.5


def head_block(a, b, h, S, d):
    """The [S, d] block of batch b, head h of a [B*S, >= H*d] output."""
    return a[b * S:(b + 1) * S, h * d:(h + 1) * d]


def scaled_qkv(rng, B, S, H, d):
    """Gaussian qkv [B*S, 3*H*d], fp16-representable, batch b / head h scaled by BH_SCALE[(b + h) % 3] in q, k and v alike: a row taken from the
    neighbouring batch or a column from the neighbouring head has another magnitude and moves the result of that block far beyond the bound."""
    x = rng.standard_normal((B, S, 3, H, d))
    for b in range(B):
        for h in range(H):
            x[b, :, :, h] *= BH_SCALE[(b + h) % 3]
    return h16(x.reshape(B * S, 3 * H * d))


# ------------------------------------------------------------------ batched GEMM
def batch_offsets(batch, nb_inner, s):
    """Element offset of every batch b = (bo, bi) = (b // nb_inner, b % nb_inner): bo * s[0] + bi * s[1]."""
    return [(b // nb_inner) * s[0] + (b % nb_inner) * s[1] for b in range(batch)]


def gemm_batched_ref(A, lda, sA, W, ldw, sW, M, N, K, batch, nb_inner, out, ldo, sO, c0=1.0, dtype=np.float64):
    """Out[b] = c0 * A[b] W[b]^T written into a copy of the flat `out` (everything else keeps the caller's contents) -> flat array of `dtype`
    (np.int64 on integer data with an integer c0: exact)."""
    A, W = np.asarray(A).ravel(), np.asarray(W).ravel()
    res = np.array(out, dtype=dtype).ravel()
    rows_m, rows_n, cols = np.arange(M)[:, None], np.arange(N)[:, None], np.arange(K)[None, :]
    for oa, ow, oo in zip(batch_offsets(batch, nb_inner, sA), batch_offsets(batch, nb_inner, sW), batch_offsets(batch, nb_inner, sO)):
        a = A[oa + rows_m * lda + cols].astype(dtype)
        w = W[ow + rows_n * ldw + cols].astype(dtype)
        res[oo + rows_m * ldo + np.arange(N)[None, :]] = dtype(c0) * (a @ w.T)
    return res


def ternary(rng, *shape):
    """Entries in {-1, 0, 1}: every product and every partial sum of a K <= 2048 dot product is an integer that float32 and fp16 hold exactly."""
    return rng.integers(-1, 2, shape).astype(np.float32)


def pad8(n):
    return (n + 7) // 8 * 8


# ------------------------------------------------------------------ structured inputs
def selector_amp(d):
    """16 up to d = 128 (selected score 256 / sqrt(d) >= 22.6); 32 at d = 512, where 16 would leave 256 / sqrt(512) = 11.3 nats and a leakage of
    e^-11.3 per key.  Both are fp16 values whose squares float32 holds exactly."""
    return 16.0 if d <= 128 else 32.0


def selector_inputs(d, H, S, B=1, seed=61):
    """Key j of every batch and head is amp * e_j (S <= d), query i of batch b, head h is amp * e_pi[b, h, i]: the selected score is amp^2 / sqrt(d),
    every other one 0, so the output is row pi[b, h, i] of that batch's V.  V[r, c] = ((r * 64 + c) % 251) / 251 over the full width c < H * d and all
    rows r < B * S: rows, batches, heads and K against V are all told apart.  -> qkv [B*S, 3*H*d], pi [B, H, S]."""
    assert S <= d
    amp, C = selector_amp(d), H * d
    pi = np.random.default_rng(seed + d).integers(0, S, (B, H, S))
    q = np.zeros((B, S, H, d), np.float32)
    k = np.zeros((B, S, H, d), np.float32)
    for b in range(B):
        for h in range(H):
            q[b, np.arange(S), h, pi[b, h]] = amp
            k[b, np.arange(S), h, np.arange(S)] = amp
    v = h16(((np.arange(B * S)[:, None] * 64 + np.arange(C)[None, :]) % 251) / 251.0)
    return np.concatenate([q.reshape(B * S, C), k.reshape(B * S, C), v], axis=1), pi


def selector_expected(qkv, pi, d):
    """[B*S, H*d]: for every batch and head, the selected rows of that head's V columns."""
    B, H, S = pi.shape
    C = H * d
    v = qkv[:, 2 * C:3 * C]
    return np.concatenate([np.concatenate([v[b * S + pi[b, h], h * d:(h + 1) * d] for h in range(H)], axis=1) for b in range(B)], axis=0)


RISE_S, RISE_H = 160, 2                             # five 32-key blocks = three 64-key tiles, two 128-row workgroups
RISE_LEVELS = (0.0, 8.5, 17.0, 12.0, 25.5)          # score level of each block in nats; block 3 lies below block 2
RISE_DIP = 3
RISE_VSCALE = (2.0 ** 9, 2.0 ** 9, 2.0 ** 6, 2.0 ** 9, 2.0 ** -6)    # |V| per block: what the softmax takes from the early blocks, V gives back


def rising_inputs(d, seed=7):
    """One batch, RISE_H heads, S = 160.  q[i] = (8, noise), k[j] = (level(block of j) * sqrt(d) / 8, noise) with noise ~ 0.25 N(0, 1): the score of
    every query against key j is level(block) + N(0, ~0.06^2).  The running maximum of every query therefore rises by >= 8 nats at blocks 1, 2 and 4
    (alpha = e^-8 or less: every accumulator is rescaled) and stays where it is at block 3 (alpha = 1).  V is scaled per block so that block 2
    (weight e^-8.5 per key) and block 3 (e^-13.5) still carry a visible share of the output.  -> qkv [S, 3*H*d], fp16-representable."""
    rng = np.random.default_rng(seed + d)
    S, H = RISE_S, RISE_H
    x = rng.standard_normal((S, 3, H, d)) * 0.25
    blk = np.arange(S) // 32
    x[:, 0, :, 0] = 8.0
    x[:, 1, :, 0] = (np.asarray(RISE_LEVELS)[blk] * np.sqrt(d) / 8.0)[:, None]
    x[:, 2] = rng.standard_normal((S, H, d)) * np.asarray(RISE_VSCALE)[blk][:, None, None]
    return h16(x.reshape(S, 3 * H * d))


def last_block_only_ref(qkv, S, H, d):
    """What a kernel that forgot every block but the last would give: softmax attention over keys [S - 32, S) alone -> float64 [S, H*d]."""
    q, k, v = split_heads(qkv, 1, S, H, d)
    return ao._softmax_av(q, k[:, :, S - 32:], v[:, :, S - 32:], d ** -0.5).transpose(0, 2, 1, 3).reshape(S, H * d)


def poisoned_buffers(qkv, B, S, H, d):
    """Clean qkv [B*S, 3*H*d] inside buffers whose every other element would show: NaN in the surplus columns (ld = 3*H*d + 8) and in POISON_GUARD rows
    after the last row; POISON_SENTINEL in the surplus columns (ldo = H*d + 4) and guard rows of the output buffer, and in its corner too (the kernels
    must overwrite it).  -> qkv_buf [B*S + POISON_GUARD, ld], out_buf [B*S + POISON_GUARD, ldo]."""
    C = H * d
    buf = np.full((B * S + POISON_GUARD, 3 * C + 8), np.nan, np.float32)
    buf[:B * S, :3 * C] = qkv
    return buf, ao.out_buffer(B * S, C + 4, POISON_GUARD, POISON_SENTINEL)
