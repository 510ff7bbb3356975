"""Plain float64 softmax attention on fp16-rounded inputs (test helper) - the yardstick of tests/test_attn_forms_*.py for the launch forms of
the head-dim-64 kernels that packed self-attention does not reach:

  * cross-attention: S queries and Sk keys per batch, K and V side by side in one [rows, ldkv] buffer (K in columns [0, H*64), V in
    [H*64, 2*H*64)), either one context per batch (rows [b*Sk, (b+1)*Sk)) or one context shared by every batch (kv_shared);
  * temporal attention of nv videos stacked [nv][T][HW]: for every pixel and head, the sequence is the T frames of ITS video.

out[b, i, h] = sum_j softmax_j(scale * <q[b, i, h], k[b, j, h]>) v[b, j, h], evaluated with the row maximum subtracted, nothing else.
The builders of the structured inputs (key selector, poisoned surroundings) live here too, so that the CPU test can check their
preconditions by the reference alone and the GPU test uses the very same arrays.  Nothing here imports the package under test."""
import numpy as np

D = 64                      # head dim of both kernels
SCALE = D ** -0.5           # 0.125, what the engine passes


def h16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def _softmax_av(q, k, v, scale):
    """q [N,H,S,D], k, v [N,H,Sk,D] float64 -> [N,H,S,D]."""
    s = np.einsum("nhqd,nhkd->nhqk", q, k) * scale
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return np.einsum("nhqk,nhkd->nhqd", p, v)


def cross_attn_ref(q, k, v, B, H, S, Sk, kv_shared, scale=SCALE):
    """q [B*S, H*64]; k, v [(1 if kv_shared else B) * keys, H*64], keys = Sk or S (Sk = 0: self-attention) -> float64 [B*S, H*64]."""
    keys = Sk if Sk else S
    nb = 1 if kv_shared else B
    q = h16(q).astype(np.float64).reshape(B, S, H, D).transpose(0, 2, 1, 3)
    k = h16(k).astype(np.float64).reshape(nb, keys, H, D).transpose(0, 2, 1, 3)
    v = h16(v).astype(np.float64).reshape(nb, keys, H, D).transpose(0, 2, 1, 3)
    if kv_shared:
        k, v = np.broadcast_to(k, (B,) + k.shape[1:]), np.broadcast_to(v, (B,) + v.shape[1:])
    return _softmax_av(q, k, v, scale).transpose(0, 2, 1, 3).reshape(B * S, H * D)


def temporal_attn_ref(qkv, nv, T, HW, H, scale=SCALE):
    """qkv [nv*T*HW, 3*H*64] (row = (video, frame, pixel), columns q | k | v) -> float64 [nv*T*HW, H*64]; batch = (video, pixel)."""
    x = h16(qkv).astype(np.float64).reshape(nv, T, HW, 3, H, D).transpose(3, 0, 2, 4, 1, 5).reshape(3, nv * HW, H, T, D)
    o = _softmax_av(x[0], x[1], x[2], scale)
    return o.reshape(nv, HW, H, T, D).transpose(0, 3, 1, 2, 4).reshape(nv * T * HW, H * D)


# ------------------------------------------------------------------ buffers as the cross-attention entry point takes them
def pack_q(q, ldq, fill=0.0):
    """q [rows, C] -> [rows, ldq], `fill` in the surplus columns."""
    out = np.full((q.shape[0], ldq), fill, np.float32)
    out[:, :q.shape[1]] = q
    return out


def pack_kv(k, v, ldkv, guard=0, fill=0.0):
    """k, v [rows, C] -> [rows + guard, ldkv] = [k | v | fill], `fill` in the guard rows."""
    rows, C = k.shape
    out = np.full((rows + guard, ldkv), fill, np.float32)
    out[:rows, :C] = k
    out[:rows, C:2 * C] = v
    return out


def unpack_kv(kv, rows, C):
    return kv[:rows, :C], kv[:rows, C:2 * C]


def out_buffer(rows, ldo, guard=0, fill=0.0):
    return np.full((rows + guard, ldo), fill, np.float32)


def outside(buf, rows, C):
    """Everything of `buf` but its [rows, C] corner, flattened: surplus columns, then guard rows."""
    return np.concatenate([buf[:rows, C:].ravel(), buf[rows:].ravel()])


# ------------------------------------------------------------------ structured inputs
SEL_H, SEL_S, SEL_SK = 2, 150, 61


def selector_inputs():
    """Key j is 16 e_j, query i of head h is 16 e_pi[h, i]: the selected score is 0.125 * 256 = 32, every other one 0, so the softmax puts
    1 - 60 e^-32 on key pi[h, i] and the output is row pi[h, i] of V.  V[j, c] = ((j * 64 + c) % 251) / 251 over the full width c < H * 64:
    rows, heads and K against V are all told apart.  -> q [S, C], k, v [Sk, C], pi [H, S]."""
    H, S, Sk, C = SEL_H, SEL_S, SEL_SK, SEL_H * D
    pi = np.random.default_rng(61).integers(0, Sk, (H, S))
    q = np.zeros((S, H, D), np.float32)
    k = np.zeros((Sk, H, D), np.float32)
    for h in range(H):
        q[np.arange(S), h, pi[h]] = 16.0
        k[np.arange(Sk), h, np.arange(Sk)] = 16.0
    v = h16(((np.arange(Sk)[:, None] * 64 + np.arange(C)[None, :]) % 251) / 251.0)
    return q.reshape(S, C), k.reshape(Sk, C), v, pi


def selector_expected(v, pi):
    """[S, H*64]: for every head, the selected rows of that head's V columns."""
    H, S = pi.shape
    return np.concatenate([v[pi[h], h * D:(h + 1) * D] for h in range(H)], axis=1)


POISON_GUARD, POISON_SENTINEL = 70, 7.0


def poisoned_inputs(rng, B, H, S, Sk, kv_shared):
    """Random operands inside buffers whose every other element would show: NaN in the surplus columns of q and kv (ldq = C + 8,
    ldkv = 2C + 8) and in POISON_GUARD rows after the last K / V row, POISON_SENTINEL in the surplus columns (ldo = C + 4) and guard rows of
    the output buffer.  -> (q_buf, kv_buf, out_buf), (q, k, v) clean."""
    C = H * D
    rows_kv = (1 if kv_shared else B) * Sk
    q, k, v = (h16(rng.standard_normal((r, C))) for r in (B * S, rows_kv, rows_kv))
    bufs = (pack_q(q, C + 8, np.nan), pack_kv(k, v, 2 * C + 8, POISON_GUARD, np.nan), out_buffer(B * S, C + 4, POISON_GUARD, POISON_SENTINEL))
    return bufs, (q, k, v)
