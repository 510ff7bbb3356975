"""numpy restatement of the seeded device noise - the yardstick of tests/test_device_noise_*.py.

Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123): multipliers
0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds.  Key = the 64-bit seed (lo, hi); counter = (q lo, q hi, stream, 0)
with q = e >> 2 for the linear element index e of a tensor in its own layout (C order); stream 0 = noise_aug [T,3,H,W], 1 = noise_latents
[T,4,H/8,W/8].  The words x0..x3 of block q make elements 4q .. 4q+3:

    u(x) = ((x >> 9) + 0.5) * 2^-23        (exact in float32, strictly inside (0, 1))
    r = sqrt(-2 ln u(x0));  4q, 4q+1 = r cos(2 pi u(x1)), r sin(2 pi u(x1));  4q+2, 4q+3 likewise from (x2, x3)

so |z| <= sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.768.  Nothing here imports the package under test.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
STREAM_AUG, STREAM_LATENTS = 0, 1
MAX_ABS = float(np.sqrt(48.0 * np.log(2.0)))     # 5.7677...
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> four uint32 arrays."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]          # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def philox_blocks(seed, stream, q0, nblocks):
    """Words of blocks q0 .. q0 + nblocks - 1 -> [nblocks, 4] uint32."""
    seed = int(seed)
    q = (np.arange(int(nblocks), dtype=np.uint64) + np.uint64(int(q0) & 0xFFFFFFFFFFFFFFFF))
    x = philox4x32_10((q & _MASK, q >> np.uint64(32), np.uint64(int(stream)), np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(x, axis=1)


def uniform(x, dtype=np.float64):
    """u(x) = ((x >> 9) + 0.5) * 2^-23, evaluated in ``dtype`` (exact in float32 and float64 alike)."""
    x = np.asarray(x, dtype=np.uint32)
    return ((x >> np.uint32(9)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -23)


def normals_from_words(words, dtype=np.float64):
    """[nblocks, 4] uint32 -> [nblocks, 4] normals: the definition evaluated in ``dtype`` (float64: the reference; float32: the floor
    of what a float32 evaluation can reach)."""
    u = uniform(words, dtype)
    two_pi = dtype(2.0 * np.pi)
    out = np.empty(u.shape, dtype)
    for a in (0, 2):
        r = np.sqrt(dtype(-2.0) * np.log(u[:, a]))
        th = two_pi * u[:, a + 1]
        out[:, a] = r * np.cos(th)
        out[:, a + 1] = r * np.sin(th)
    return out


def randn(seed, stream, element_offset, n, dtype=np.float64):
    """Elements element_offset .. element_offset + n - 1 of (seed, stream)."""
    e0, n = int(element_offset), int(n)
    q0, q1 = e0 >> 2, (e0 + n + 3) >> 2
    z = normals_from_words(philox_blocks(seed, stream, q0, q1 - q0), dtype).reshape(-1)
    return z[e0 - 4 * q0: e0 - 4 * q0 + n]


def make_noise(T, H, W, seed, dtype=np.float64):
    """(noise_latents [T,4,H/8,W/8], noise_aug [T,3,H,W]) of the device mode, by the definition."""
    aug = randn(seed, STREAM_AUG, 0, T * 3 * H * W, dtype).reshape(T, 3, H, W)
    lat = randn(seed, STREAM_LATENTS, 0, T * 4 * (H // 8) * (W // 8), dtype).reshape(T, 4, H // 8, W // 8)
    return lat, aug


def moment_checks(lat, aug):
    """The statistical gates of the full-size test, each as (name, |value|, bound): mean within 5 / sqrt(N), variance within 5 sqrt(2 / N) of 1
    (five standard deviations of the estimators for N independent standard normals: Var[mean] = 1/N, Var[s^2] = 2/N), and the correlation of
    the latent stream with the first elements of the aug stream within 5 / sqrt(n) (Var[r] = 1/n for independent streams)."""
    out = []
    for name, z in (("aug", aug), ("latents", lat)):
        z = np.asarray(z, dtype=np.float64).reshape(-1)
        N = z.size
        out.append((f"{name} mean", abs(z.mean()), 5.0 / np.sqrt(N)))
        out.append((f"{name} variance - 1", abs(z.var() - 1.0), 5.0 * np.sqrt(2.0 / N)))
    a = np.asarray(lat, dtype=np.float64).reshape(-1)
    b = np.asarray(aug, dtype=np.float64).reshape(-1)[:a.size]
    r = float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std()))
    out.append(("latents x aug correlation", abs(r), 5.0 / np.sqrt(a.size)))
    return out
