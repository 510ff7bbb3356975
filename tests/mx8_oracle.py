"""Inputs and references of the MX-fp8 op tests (tests/test_mx8_forms_gpu.py; pinned on the CPU by tests/test_mx8_oracle_cpu.py).

The reference of every check is util.mx8_quantise (OCP MX: e8m0 scale floor(log2 amax) - 8 per 32 K elements, e4m3 elements rounded to nearest even,
saturated at +-448 BEFORE the conversion - the project's definition, kernels/mx8.hip) followed by a float64 product of the dequantised operands.

Three kinds of data:
  * the quantiser edge matrix (edge_blocks / edge_matrix): per block a chosen maximum m * 2^t and, in the other slots, every e4m3 rounding tie at that
    block's scale with its fp16 neighbours, the saturation band, the e4m3 subnormals and signed zeros;
  * the exact screen (exact_operand / exact_case): small integers times a per-(row, block) power of two, for which the quantisation is lossless and the
    fp32 accumulation exact in any order, so that fp16(float64 reference) is the only admissible device output;
  * Gaussian rows of mixed scale (gauss_case) for the epilogues that cannot be exact; the bound is derived from the reference's own fp16 rounding.
"""
import numpy as np

from util import e4m3_encode, h16, mx8_quantise

# ---------------------------------------------------------------------------------------------------------------- e4m3 and the edge matrix
E4M3_POS = np.array(sorted({k * 2.0 ** -9 for k in range(8)} | {(1 + j / 8) * 2.0 ** E for E in range(-6, 9) for j in range(8) if (1 + j / 8) * 2.0 ** E <= 448}))
E4M3_TIES = (E4M3_POS[:-1] + E4M3_POS[1:]) / 2          # every midpoint of two neighbouring e4m3 values: both parities of the lower neighbour occur
EDGE_MANTISSAS = (1.0, 1.75, 2.0 - 2.0 ** -10)           # block maximum = m * 2^t: scaled to 256, 448 (the largest e4m3) and 511.75 (inside the saturation band)
EDGE_TS = tuple(range(-24, 16))                          # fp16-subnormal maxima (t < -14) up to 65504 = (2 - 2^-10) * 2^15


def fp16_exact(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return np.isfinite(x) & (x.astype(np.float16).astype(np.float64) == x)


def _neighbours(v):
    """v and the fp16 values one ulp either side of it (v fp16-exact)."""
    h = np.asarray(v, np.float64).astype(np.float16)
    with np.errstate(over="ignore"):                      # above 65504 there is no neighbour: inf, dropped by the caller
        return np.concatenate([h, np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(-np.inf))]).astype(np.float64)


def edge_candidates(m, t):
    """The values that fill the blocks of maximum m * 2^t, in real units: everything fp16 cannot hold, and everything above the block maximum, is dropped."""
    amax = m * 2.0 ** t
    s = 2.0 ** (t - 8)                                    # the block's scale: floor(log2 amax) - 8
    ties = E4M3_TIES * s
    ties = ties[fp16_exact(ties)]
    band = np.array([448 + 2.0 ** -3, 449, 456, 464, 472, 480, 496, 504, 511.75]) * s      # (448, 512) * 2^e: 464 is the tie towards the NaN encoding
    sub = np.concatenate([np.arange(1, 8) * 2.0 ** -9, [2.0 ** -10, 3 * 2.0 ** -10]]) * s    # e4m3 subnormals, half of the smallest (tie to zero), 1.5 of it
    pos = np.concatenate([_neighbours(ties), _neighbours(band[fp16_exact(band)]), sub[fp16_exact(sub)], E4M3_POS[fp16_exact(E4M3_POS * s)] * s])
    pos = np.unique(pos[(pos > 0) & (pos <= amax) & fp16_exact(pos)])
    return np.concatenate([pos, -pos, [0.0, -0.0]])


def edge_blocks():
    """All blocks [nblk, 32] of the edge matrix: per (m, t) as many blocks as its candidates need, slot 0 of every block = the block maximum (alternating
    sign), and one all-zero block at the end."""
    blocks = []
    for t in EDGE_TS:
        for m in EDGE_MANTISSAS:
            amax = m * 2.0 ** t
            if not fp16_exact(amax):
                continue
            c = edge_candidates(m, t)
            pad = (-len(c)) % 31
            c = np.concatenate([c, np.zeros(pad)]).reshape(-1, 31)
            sign = np.where(np.arange(len(c)) % 2 == 0, 1.0, -1.0)[:, None]
            blocks.append(np.concatenate([sign * amax, c], 1))
    blocks.append(np.zeros((1, 32)))
    b = np.concatenate(blocks)
    # the maximum moves through the block's 32 slots from block to block: every lane pair of the quantiser's shuffle sees it
    idx = np.arange(len(b))
    out = b.copy()
    out[idx, 0] = b[idx, idx % 32]
    out[idx, idx % 32] = b[idx, 0]
    return out.astype(np.float32)


def edge_matrix(K):
    """The edge blocks laid out as rows of K elements (zero blocks pad the last row): x [M, K] float32, fp16-exact.  The blocks are shuffled (fixed seed):
    the four blocks of a scale dword, and the rows next to each other, then carry unrelated exponents - in generation order neighbours share theirs, and
    an exponent gathered from the wrong block would go unseen."""
    b = edge_blocks()
    b = b[np.random.default_rng(27).permutation(len(b))]
    per = K // 32
    pad = (-len(b)) % per
    b = np.concatenate([b, np.zeros((pad, 32), np.float32)])
    return np.ascontiguousarray(b.reshape(-1, K))


def edge_classes(x):
    """How many elements of x [M, K] are exact e4m3 ties / saturate / are e4m3-subnormal after scaling / are -0.0, and how many blocks have an
    fp16-subnormal maximum: the CPU test requires each class to be non-empty."""
    x = np.asarray(x, np.float64)
    xb = x.reshape(x.shape[0], -1, 32)
    amax = np.abs(xb).max(-1)
    ex = np.where(amax > 0, np.floor(np.log2(np.maximum(amax, 1e-300))) - 8, 0.0)
    v = np.abs(xb) * 2.0 ** -ex[..., None]
    tie = np.isin(v, E4M3_TIES)
    lower = E4M3_POS[np.clip(np.searchsorted(E4M3_POS, v, side="right") - 1, 0, len(E4M3_POS) - 1)]
    k = e4m3_encode(lower) & 1                            # parity of the lower neighbour's code: the tie goes down when it is even, up when it is odd
    return {"ties": int(tie.sum()), "ties_lower_even": int((tie & (k % 2 == 0)).sum()), "ties_lower_odd": int((tie & (k % 2 == 1)).sum()),
            "saturated": int((v > 448).sum()), "e4m3_subnormal": int(((v > 0) & (v < 2.0 ** -6)).sum()),
            "negative_zero": int((np.signbit(x) & (x == 0)).sum()), "fp16_subnormal_blocks": int(((amax > 0) & (amax < 2.0 ** -14)).sum()),
            "zero_blocks": int((amax == 0).sum()), "max": float(np.abs(x).max())}


def scale_dwords(e, ld, fill=None):
    """Biased exponents e [M, K/32] -> the device layout [K/128][ld] of dwords (4 e8m0 per dword, block j in byte j); rows >= M keep `fill`."""
    M, nb = e.shape
    d = e.reshape(M, nb // 4, 4).astype(np.uint32)
    w = d[..., 0] | (d[..., 1] << 8) | (d[..., 2] << 16) | (d[..., 3] << 24)
    out = np.zeros((nb // 4, ld), np.uint32) if fill is None else np.array(fill, dtype=np.uint32)
    out[:, :M] = w.T
    return out


# ---------------------------------------------------------------------------------------------------------------- the exact screen
EXACT_INT = 4                 # elements are integers in [-4, 4] ...
EXACT_TS = (-2, -1, 0, 1, 2)  # ... times 2^t, t drawn per (row, block); every block holds a +-4, so its exponent is t + 2 - 8 and the scaled values are multiples of 64 <= 256
EXACT_KMAX = 1024             # worst case sum |a| |w| = K * 16 * 2^4 = 2^22 granules of 2^-4 at K = 1024: below 2^24 with room


def exact_operand(rng, rows, K):
    """[rows, K] float32 and the per-(row, block) t: small integers times 2^t with the block maximum forced to 4 * 2^t."""
    nb = K // 32
    t = rng.choice(EXACT_TS, size=(rows, nb))
    v = rng.integers(-EXACT_INT, EXACT_INT + 1, size=(rows, nb, 32)).astype(np.float64)
    slot = rng.integers(0, 32, size=(rows, nb))
    r, b = np.meshgrid(np.arange(rows), np.arange(nb), indexing="ij")
    v[r, b, slot] = EXACT_INT * rng.choice([-1.0, 1.0], size=(rows, nb))
    return (v * 2.0 ** t[..., None]).reshape(rows, K).astype(np.float32), t


def exact_case(M, N, K, seed=0, epilogue=False, wide=0):
    """Operands of an exact GEMM case and the float64 reference pieces.  epilogue: integer bias, R1, R2 (rows of N + wide columns)."""
    assert K % 128 == 0 and K <= EXACT_KMAX
    rng = np.random.default_rng([M, N, K, seed])
    A, ta = exact_operand(rng, M, K)
    W, tw = exact_operand(rng, N, K)
    c = {"A": A, "W": W, "ta": ta, "tw": tw, "prod": A.astype(np.float64) @ W.astype(np.float64).T}
    if epilogue:
        c["bias"] = rng.integers(-8, 9, N).astype(np.float32)
        c["R1"] = rng.integers(-64, 65, (M, N + wide)).astype(np.float32)
        c["R2"] = rng.integers(-64, 65, (M, N + wide)).astype(np.float32)
    return c


def exact_ref(c, bias=False, R1=False, R2=False, c0=1.0, c1=1.0, c2=1.0):
    """float64 value of c0 * (A W^T + bias) + c1 * R1 + c2 * R2 on an exact case (the flags pick the operands)."""
    N = c["W"].shape[0]
    y = c["prod"] + (c["bias"].astype(np.float64) if bias else 0.0)
    y = c0 * y
    if R1:
        y = y + c1 * c["R1"][:, :N].astype(np.float64)
    if R2:
        y = y + c2 * c["R2"][:, :N].astype(np.float64)
    return y


def exact_conditions(c, bias=False, R1=False, R2=False, c0=1.0, c1=1.0, c2=1.0):
    """The figures under which fp16(float64 reference) is the only admissible output: (every operand fp16-exact, the quantisation lossless, the largest sum of
    absolute terms of one output in units of the smallest granule any partial result can have, max |ref|).  fp32 arithmetic is exact in any order - MFMA
    accumulation, bias, the coefficient products and the residual sums - while that sum stays below 2^24."""
    A, W = c["A"], c["W"]
    N = W.shape[0]
    ok16 = bool(fp16_exact(A).all() and fp16_exact(W).all())
    lossless = bool(np.array_equal(mx8_quantise(A)[0], A) and np.array_equal(mx8_quantise(W)[0], W))
    gran = 2.0 ** (2 * min(EXACT_TS))                     # smallest product of two elements
    mag = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T
    coef = [abs(c0)]
    if bias:
        ok16 &= bool(fp16_exact(c["bias"]).all()); mag = mag + np.abs(c["bias"])
    mag = mag * abs(c0)
    if R1:
        ok16 &= bool(fp16_exact(c["R1"]).all()); mag = mag + abs(c1) * np.abs(c["R1"][:, :N]); coef.append(abs(c1))
    if R2:
        ok16 &= bool(fp16_exact(c["R2"]).all()); mag = mag + abs(c2) * np.abs(c["R2"][:, :N]); coef.append(abs(c2))
    for k in coef:
        assert k > 0 and np.log2(k) == np.round(np.log2(k)), "coefficients of the exact screen are powers of two"
    gran *= min(1.0, min(coef))
    ref = exact_ref(c, bias, R1, R2, c0, c1, c2)
    return ok16, lossless, float(mag.max() / gran), float(np.abs(ref).max())


# the GPU cases, shared with the CPU test that shows the conditions hold on exactly this data
EXACT_MS = (1, 127, 129, 191, 193, 255, 257, 385, 449)
EXACT_NS = (8, 120, 136, 264)
EXACT_KS = (128, 256, 384, 640)
EXACT_WALK = (4352, 4096, 128)      # 34 x 32 = 1088 tiles of 128 x 128 on 512 workgroups, 17 x 32 = 544 of 256 x 128 and 23 x 32 = 736 of 192 x 128 on 256: a second tile per workgroup
EXACT_GROUPED = (570, 4096, 1024)   # fp8 weights of 4 MiB > the L2 rule's 1.5 MiB: group_m = 2 against an odd tile-row count on every tile (3 x 256, 3 x 192, 5 x 128)
EPI_FORMS = {      # name -> (bias, R1, R2, c0, c1, c2): the forms transformer_forward sends through launch_gemm_mx8, on exact data with power-of-two coefficients
    "none": (False, False, False, 1.0, 1.0, 1.0),
    "bias": (True, False, False, 1.0, 1.0, 1.0),
    "R1": (True, True, False, 1.0, 1.0, 1.0),
    "R1_c1": (True, True, False, 1.0, 0.5, 1.0),
    "R1_R2": (True, True, True, 0.5, 0.25, 2.0),
}


# ---------------------------------------------------------------------------------------------------------------- Gaussian data, planted defects
def gauss_case(M, N, K, seed=0):
    """Rows of very different scale (activations) against 1 / sqrt(K) weights, with bias and two residuals, all fp16-exact."""
    rng = np.random.default_rng([M, N, K, seed, 7])
    A = h16(rng.standard_normal((M, K)) * np.exp(rng.normal(0, 1.5, (M, 1))))
    W = h16(rng.standard_normal((N, K)) / np.sqrt(K))
    return {"A": A, "W": W, "bias": h16(rng.standard_normal(N) * 0.1), "R1": h16(rng.standard_normal((M, N))), "R2": h16(rng.standard_normal((M, N)))}


def dequant(bytes_, e):
    """e4m3 bytes [M, K] and biased exponents [M, K/32] -> float64 [M, K] (the inverse of util.e4m3_encode, times the block scale)."""
    b = np.asarray(bytes_, np.int64)
    ef, mf = (b >> 3) & 15, b & 7
    mag = np.where(ef == 0, mf * 2.0 ** -9, (1 + mf / 8.0) * 2.0 ** (ef - 7.0))
    v = np.where(b & 128, -mag, mag)
    return v * np.repeat(2.0 ** (np.asarray(e, np.float64) - 127), 32, axis=1)


def planted(e, defect):
    """A biased-exponent array [rows, K/32] as a GEMM with a misplaced scale would read it."""
    rows, nb = e.shape
    if defect == "neighbour_block":          # a block's scale taken from its neighbour inside the dword
        return e.reshape(rows, nb // 4, 4)[..., [1, 0, 3, 2]].reshape(rows, nb)
    if defect == "dword_reversed":           # the four exponents of a dword reversed
        return e.reshape(rows, nb // 4, 4)[..., ::-1].reshape(rows, nb)
    if defect == "previous_kstep":           # a K step's scales taken from the step before
        return np.roll(e.reshape(rows, nb // 4, 4), 1, axis=1).reshape(rows, nb)
    raise ValueError(defect)


PLANTED = ("neighbour_block", "dword_reversed", "previous_kstep")
