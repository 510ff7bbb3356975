"""float64 references for kernels/norm.hip (GroupNorm, LayerNorm), the inputs and the case table of tests/test_norm_forms_gpu.py, and an fp32
emulation of the kernels' statistics schemes that tests/test_norm_oracle_cpu.py holds against the same bound the GPU tests assert.

The bound, elementwise:  |got - ref| <= F * (2^-10 |ref| + 2^-20 (mag + 1)),  mag = |x a| + |b|  (a = rstd gamma, b = beta - mean a), F = 2 on the GPU.
2^-10 |ref|: the fp16 rounding of the output (half an ulp is 2^-11 |ref|; the fp32 result may sit on the other side of a rounding boundary).
2^-20 (mag + 1): the fp32 cancellation in x a + b when the output is near zero.  F = 1 is what the fp32 emulation below must meet on every GroupNorm
input of the GPU file (summation order of one 256-thread workgroup, correctly rounded division / exp); F = 2 leaves the device its own summation order
and its rcp / exp.  The inputs stay inside what the sum / sum-of-squares scheme handles: group means of at most 2 standard deviations (make_groups).
"""
import numpy as np

BOUND_FACTOR_GPU = 2.0


def h16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def bound(ref, mag, factor=1.0):
    return factor * (2.0 ** -10 * np.abs(ref) + 2.0 ** -20 * (mag + 1.0))


def worst_ratio(got, ref, mag, factor=1.0):
    """max over the elements of |got - ref| / bound, and its flat index"""
    r = np.abs(np.asarray(got, np.float64) - ref) / bound(ref, mag, factor)
    i = int(np.argmax(r))
    return float(r.flat[i]), i


def _silu(y):
    return y / (1.0 + np.exp(-y))


def _concat(x0, x1):
    x0 = np.asarray(x0, np.float64)
    return x0 if x1 is None else np.concatenate([x0, np.asarray(x1, np.float64)], -1)


def groupnorm_f64(x0, x1, G, eps, gamma, beta, temporal, silu):
    """x0 [T,HW,C0] (+ x1 [T,HW,C1]: the virtual channel concat) -> (ref, mag) [T,HW,C]; statistics per (frame, group), or per group over all frames."""
    x = _concat(x0, x1)
    T, HW, C = x.shape
    xg = x.reshape(T, HW, G, C // G)
    ax = (0, 1, 3) if temporal else (1, 3)
    mean = xg.mean(ax, keepdims=True)
    var = ((xg - mean) ** 2).mean(ax, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    a = rstd * np.asarray(gamma, np.float64).reshape(1, 1, G, C // G)
    b = np.asarray(beta, np.float64).reshape(1, 1, G, C // G) - mean * a
    y = xg * a + b
    mag = np.abs(xg * a) + np.abs(b)
    if silu:
        y = _silu(y)
    return y.reshape(T, HW, C), mag.reshape(T, HW, C)


def layernorm_f64(x, eps, gamma, beta, addvec=None, rows_per_vec=1, row0=0):
    """x [M,C] -> (ref, mag, xout); with addvec the row m first becomes fp16(x[m] + addvec[(m + row0) // rows_per_vec]), as the kernels round it.
    mag = |xhat gamma| + |beta|."""
    x = np.asarray(x, np.float64)
    M, C = x.shape
    xout = None
    if addvec is not None:
        rows = (np.arange(M) + row0) // rows_per_vec
        xout = h16(x.astype(np.float32) + np.asarray(addvec, np.float32)[rows])     # one fp32 add of two fp16 values, rounded to fp16: exact in fp32
        x = xout.astype(np.float64)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    xh = (x - mean) / np.sqrt(var + eps)
    g, b = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    return xh * g + b, np.abs(xh * g) + np.abs(b), xout


def make_groups(rng, T, HW, G, cpg, temporal):
    """fp16-representable input [T,HW,G*cpg] in which every (frame, group) - every group, when temporal - has its own standard deviation 2^U(-2,1) and
    mean std * U(-2,2), with gamma = 1 + 0.3 N and beta = 0.5 N distinct per channel: a wrong group, frame or channel index fails by many ulps."""
    shape = (1 if temporal else T, 1, G, 1)
    std = 2.0 ** rng.uniform(-2, 1, shape)
    mean = std * rng.uniform(-2, 2, shape)
    x = h16(rng.standard_normal((T, HW, G, cpg)) * std + mean).reshape(T, HW, G * cpg)
    return x, h16(1 + 0.3 * rng.standard_normal(G * cpg)), h16(0.5 * rng.standard_normal(G * cpg))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the statistics schemes (one 256-thread workgroup per group: every thread sums its strided share in order, then a binary tree)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _block_sum32(v, nthreads=256):
    v = np.asarray(v, np.float32).ravel()
    pad = (-v.size) % nthreads
    v = np.concatenate([v, np.zeros(pad, np.float32)]).reshape(-1, nthreads)
    s = np.cumsum(v, axis=0, dtype=np.float32)[-1]           # cumsum adds in order: the thread's running fp32 sum
    while s.size > 1:
        s = (s[: s.size // 2] + s[s.size // 2:]).astype(np.float32)
    return np.float32(s[0])


def _rows_per_chunk(T, HW, C):
    """rows per workgroup of gn_stats (gn_chunks2 of kernels/norm.hip: ~1024 workgroups, >= 4 row iterations per thread, <= 128 chunks per frame)"""
    rpi = max(256 // (C // 8), 1)
    rpc = max(-(-HW // -(-1024 // T)), 4 * rpi)
    if -(-HW // rpc) > 128:
        rpc = -(-HW // 128)
    return rpc


def groupnorm_emulated(x0, x1, G, eps, gamma, beta, temporal, silu, scheme):
    """The statistics in fp32 as the kernels take them, scale / shift and the output expression in fp32 as the kernels write them, output rounded to fp16.
    'chunked' : gn_stats + gn_finalize - fp32 sum and sum of squares per chunk of rows, the chunks (and frames, when pooled) combined in fp64
    'small'   : gn_small - one workgroup's fp32 sum and sum of squares over the whole (frame, group); the kernel has no pooled form
    'twopass' : gn_slab, LayerNorm - fp32 mean, then the fp32 sum of squared deviations, over the whole slab"""
    x = _concat(x0, x1).astype(np.float32)
    T, HW, C = x.shape
    cpg = C // G
    assert scheme in ("chunked", "small", "twopass") and not (scheme == "small" and temporal)
    rpc = _rows_per_chunk(T, HW, C)
    out = np.empty((T, HW, C), np.float32)
    gm, bt = np.asarray(gamma, np.float32), np.asarray(beta, np.float32)
    for t in ([slice(None)] if temporal else range(T)):
        for g in range(G):
            cs = slice(g * cpg, (g + 1) * cpg)
            v = x[t, :, cs]
            n = float(v.size)
            if scheme == "twopass":
                mean = np.float32(float(_block_sum32(v)) / n)
                d = v - mean
                var = float(_block_sum32(d * d)) / n
            else:
                if scheme == "small":
                    s, q = float(_block_sum32(v)), float(_block_sum32(v * v))
                else:
                    s = q = 0.0
                    for f in v.reshape(-1, HW, cpg):
                        for r0 in range(0, HW, rpc):
                            s += float(_block_sum32(f[r0: r0 + rpc])); q += float(_block_sum32(f[r0: r0 + rpc] ** 2))
                mean = s / n
                var = max(q / n - mean * mean, 0.0)
                mean = np.float32(mean)
            rstd = np.float32(1.0 / np.sqrt(var + float(eps)))
            a = rstd * gm[cs]
            b = bt[cs] - mean * a
            y = v * a + b
            if silu:
                y = y / (np.float32(1) + np.exp(-y))
            out[t, :, cs] = y
    assert out.dtype == np.float32
    return h16(out)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the GroupNorm cases of tests/test_norm_forms_gpu.py: (id, C0, C1, G, T, HW, temporal, mode, want) with want = (scheme, slab threads, slab VMAX) and,
# for scheme 1, optionally the chunks per frame as a fourth entry; fin = the gn_finalize width the case is written for (1024 threads when
# (temporal ? T : 1) * chunks > 64, else 256 - the test derives the side from the reported chunk count).  SiLU alternates over the table.
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _c(id_, C, G, T, HW, temporal, mode, want, C1=0, fin=0):
    return dict(id=id_, C0=C - C1, C1=C1, G=G, T=T, HW=HW, temporal=temporal, mode=mode, want=want, fin=fin)


GN_CASES = [
    # every slab instantiation in each MODE that can run it
    _c("s4 256/4 one row", 8, 2, 1, 1, False, 0, (4, 256, 4)),
    _c("s4 256/8", 256, 2, 1, 33, False, 0, (4, 256, 8)),
    _c("s4 1024/4", 128, 2, 1, 130, False, 0, (4, 1024, 4)),
    _c("s4 1024/8", 2048, 16, 16, 130, False, 0, (4, 1024, 8)),
    _c("s6 256/4", 64, 16, 16, 1, True, 0, (6, 256, 4)),
    _c("s6 256/8", 2048, 16, 16, 33, True, 0, (6, 256, 8)),
    _c("s6 1024/4", 1024, 16, 16, 130, True, 0, (6, 1024, 4)),
    _c("s6 1024/8", 2048, 16, 16, 130, True, 0, (6, 1024, 8)),
    _c("s6 T65 256/4", 16, 4, 65, 1, True, 0, (6, 256, 4)),
    _c("s6 T65 256/8", 512, 4, 65, 33, True, 0, (6, 256, 8)),
    _c("s6 T65 1024/4", 256, 4, 65, 130, True, 0, (6, 1024, 4)),
    _c("s6 T65 1024/8", 512, 4, 65, 130, True, 0, (6, 1024, 8)),
    _c("mode4 256/8", 16, 2, 1, 528, False, 4, (4, 256, 8)),
    _c("mode4 1024/8", 8, 2, 1, 4100, False, 4, (4, 1024, 8)),
    _c("mode4 1024/16", 16, 2, 1, 4100, False, 4, (4, 1024, 16)),
    _c("mode4 1024/32", 256, 2, 1, 528, False, 4, (4, 1024, 32)),
    _c("mode4 1024/48", 128, 2, 1, 2100, False, 4, (4, 1024, 48)),
    _c("mode4 pooled 256/8", 8, 2, 8, 130, True, 4, (4, 256, 8)),
    _c("mode4 pooled 1024/4", 8, 2, 16, 130, True, 4, (4, 1024, 4)),
    _c("mode4 pooled 1024/16", 8, 2, 2, 4100, True, 4, (4, 1024, 16)),
    _c("mode4 pooled 1024/32", 16, 2, 2, 4100, True, 4, (4, 1024, 32)),
    _c("mode4 pooled 1024/48", 8, 2, 8, 4100, True, 4, (4, 1024, 48)),
    _c("mode6 1024/16", 16, 2, 3, 4100, True, 6, (6, 1024, 16)),
    _c("mode6 1024/32", 256, 2, 3, 528, True, 6, (6, 1024, 32)),
    _c("mode6 1024/48", 128, 2, 3, 2100, True, 6, (6, 1024, 48)),
    _c("mode6 T65 1024/16", 16, 2, 65, 4100, True, 6, (6, 1024, 16)),
    # scheme 6 at the readlane / serial switch and at the engine's window limit
    _c("s6 T64 256/4", 16, 4, 64, 1, True, 0, (6, 256, 4)),
    _c("s6 T128 256/4", 16, 4, 128, 1, True, 0, (6, 256, 4)),
    _c("s6 T128 1024/4", 128, 2, 128, 130, True, 0, (6, 1024, 4)),
    # slab edges: groups whose vector count does not divide the workgroup (5, 10, 15 lanes per row: the last thread(s) idle)
    _c("cpg20 256", 640, 32, 2, 100, False, 0, (4, 256, 4)),
    _c("cpg40 256", 1280, 32, 2, 48, False, 0, (4, 256, 4)),
    _c("cpg60 256", 1920, 32, 2, 48, False, 0, (4, 256, 4)),
    _c("cpg20 1024", 640, 32, 1, 450, False, 4, (4, 1024, 4)),
    _c("cpg60 1024", 1920, 32, 1, 150, False, 4, (4, 1024, 4)),
    _c("cpg40 pooled 1024", 1280, 32, 3, 100, True, 4, (4, 1024, 4)),
    _c("cpg20 s6", 640, 32, 8, 100, True, 0, (6, 256, 4)),
    # row counts R below, at and above k * rpi (cpg 32: rpi = 32 rows on 256 threads, 128 on 1024): tail rows stay out of the squared-deviation sum
    _c("R127", 64, 2, 1, 127, False, 4, (4, 256, 4)),
    _c("R128", 64, 2, 1, 128, False, 4, (4, 256, 4)),
    _c("R129", 64, 2, 1, 129, False, 4, (4, 256, 8)),
    _c("R255", 64, 2, 1, 255, False, 4, (4, 256, 8)),
    _c("R256", 64, 2, 1, 256, False, 4, (4, 256, 8)),
    _c("R257", 64, 2, 1, 257, False, 4, (4, 1024, 4)),
    _c("R511", 64, 2, 1, 511, False, 4, (4, 1024, 4)),
    _c("R512", 64, 2, 1, 512, False, 4, (4, 1024, 4)),
    _c("R513", 64, 2, 1, 513, False, 4, (4, 1024, 8)),
    _c("R6143", 64, 2, 1, 6143, False, 4, (4, 1024, 48)),
    _c("R6144", 64, 2, 1, 6144, False, 4, (4, 1024, 48)),
    _c("R6145 does not fit: gn_small", 64, 2, 1, 6145, False, 4, (2, 0, 0)),
    _c("R129 pooled", 64, 2, 3, 43, True, 4, (4, 256, 8)),
    _c("R129 per frame of 2", 64, 2, 2, 129, False, 4, (4, 256, 8)),
    # forced scheme 2 (gn_small)
    _c("mode2", 64, 16, 2, 100, False, 2, (2, 0, 0)),
    _c("mode2 straddle 96+48", 144, 4, 2, 50, False, 2, (2, 0, 0), C1=48),
    _c("mode2 straddle 1280+640 HW7", 1920, 32, 3, 7, False, 2, (2, 0, 0), C1=640),
    _c("mode2 temporal falls back to 1", 64, 16, 2, 100, True, 2, (1, 0, 0)),
    # scheme 1: three vectors per thread, the 128-chunk cap, both gn_finalize widths
    _c("s1 vpt3 C4104", 4104, 8, 2, 40, False, 0, (1, 0, 0)),
    _c("s1 vpt3 C4224 pooled", 4224, 32, 2, 24, True, 1, (1, 0, 0)),
    _c("s1 chunk cap", 2560, 32, 1, 520, False, 0, (1, 0, 0, 104), fin=1024),
    _c("s1 finalize 256: 8 chunks", 320, 32, 3, 192, False, 1, (1, 0, 0, 8), fin=256),
    _c("s1 finalize 256 pooled: 3 x 8", 320, 32, 3, 192, True, 1, (1, 0, 0, 8), fin=256),
    _c("s1 finalize 1024 pooled: 9 x 8", 320, 32, 9, 192, True, 1, (1, 0, 0, 8), fin=1024),
    _c("s1 two sources straddle", 144, 4, 2, 50, False, 1, (1, 0, 0), C1=48),
]
for _i, _case in enumerate(GN_CASES):
    _case["silu"] = bool(_i % 2)
    _case["seed"] = 1000 + _i

# one input per layout under every scheme that accepts it (0 = as the launcher picks)
GN_VERSUS = [
    dict(id="per frame", C0=64, C1=0, G=16, T=2, HW=100, temporal=False, silu=True, seed=2000, modes=(0, 1, 2, 4), schemes=(4, 1, 2, 4)),
    dict(id="pooled", C0=64, C1=0, G=4, T=64, HW=12, temporal=True, silu=False, seed=2001, modes=(0, 1, 4, 6), schemes=(6, 1, 4, 6)),
]

# the same tensors as two sources and as one concatenated source, every group inside one source
GN_TWO_SOURCE = [
    dict(id="96+96 G8", C0=96, C1=96, G=8, T=2, HW=50, temporal=False, silu=True, seed=2100),
    dict(id="1280+1280 HW12", C0=1280, C1=1280, G=32, T=2, HW=12, temporal=False, silu=False, seed=2101),
    dict(id="1280+1280 HW12 pooled", C0=1280, C1=1280, G=32, T=8, HW=12, temporal=True, silu=True, seed=2102),
]

# scheme 6 on both sides of T = 64: the same input, extended by one frame
GN_T64_65 = dict(id="T64|65", C0=64, C1=0, G=4, T=65, HW=33, temporal=True, silu=True, seed=2200)


def gn_inputs(case):
    """(x0, x1 or None, gamma, beta) of a case, deterministic in case['seed']"""
    rng = np.random.default_rng(case["seed"])
    C = case["C0"] + case["C1"]
    x, gm, bt = make_groups(rng, case["T"], case["HW"], case["G"], C // case["G"], case["temporal"])
    if case["C1"]:
        return np.ascontiguousarray(x[..., : case["C0"]]), np.ascontiguousarray(x[..., case["C0"]:]), gm, bt
    return x, None, gm, bt


def all_gn_inputs():
    """every GroupNorm input the GPU file runs: (id, x0, x1, G, temporal, silu, gamma, beta)"""
    for case in GN_CASES + GN_VERSUS + GN_TWO_SOURCE + [GN_T64_65]:
        x0, x1, gm, bt = gn_inputs(case)
        yield case["id"], x0, x1, case["G"], case["temporal"], case["silu"], gm, bt
