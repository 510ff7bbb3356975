"""Plain float64 restatements of what every GEMM / implicit-GEMM launch of the engine ends in:

    Out = act(c0 * f(acc + bias + bias2) + c1 * R1 + c2 * R2),   f = GEGLU or the identity, Out stored in fp16

and of the GroupNorm statistics a launch may hand on with it (GemmP::stat_part): per block of rb output rows of one frame and per column the sum and the
sum of squares of the fp16 values stored.  Shared by tests/test_epilogue_forms_gpu.py (the kernels) and tests/test_epilogue_oracle_cpu.py (the screens
themselves, against a float32 model with planted defects).  Nothing in here knows a kernel's tile geometry except halo_block_of_row, which restates the
block numbering of the halo-staged convolution from kernels/conv_halo.hip."""
import numpy as np
import torch

from util import conv_f64, h16

U32 = 2.0 ** -23            # one unit in the last place of a float32 in [1, 2): the relative size of ONE fp32 rounding, however the adder rounds


# --------------------------------------------------------------------------------------------------- the expression
def act64(y, act):
    """act 0: identity, 1: SiLU, 2: GELU (erf form), in float64."""
    if act == 0:
        return y
    y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64))
    return (torch.nn.functional.silu(y) if act == 1 else torch.nn.functional.gelu(y)).numpy()


def cols(R, n):
    """The first n columns of a residual given with its leading dimension ([rows, ld], ld >= n); None stays None."""
    return None if R is None else np.asarray(R, np.float64)[:, :n]


def epilogue64(acc, bias=None, bias2=None, R1=None, R2=None, c0=1.0, c1=1.0, c2=1.0, act=0, geglu=False):
    """acc [M, N] float64 (the matrix product / convolution without bias) -> [M, N] or, with geglu, [M, N / 2]: columns [0, N / 2) are the values h,
    [N / 2, N) the gates g (checkpoint order), f = h * gelu(g).  R1 / R2 [M, ld >= output width]."""
    y = np.asarray(acc, np.float64).copy()
    for b in (bias, bias2):
        if b is not None:
            y = y + np.asarray(b, np.float64)
    if geglu:
        n = y.shape[1] // 2
        y = y[:, :n] * act64(y[:, n:], 2)
    o = c0 * y
    if R1 is not None:
        o = o + c1 * cols(R1, o.shape[1])
    if R2 is not None:
        o = o + c2 * cols(R2, o.shape[1])
    return act64(o, act)


def epilogue_mag(absacc, bias=None, bias2=None, R1=None, R2=None, c0=1.0, c1=1.0, c2=1.0):
    """|c0| (sum_k |a_k w_k| + |bias| + |bias2|) + |c1 R1| + |c2 R2|: the size of what the fp32 roundings of the accumulation and of the epilogue act on.
    absacc = the product of the absolute values, [M, N]."""
    m = np.asarray(absacc, np.float64).copy()
    for b in (bias, bias2):
        if b is not None:
            m = m + np.abs(np.asarray(b, np.float64))
    m = abs(c0) * m
    if R1 is not None:
        m = m + np.abs(c1 * cols(R1, m.shape[1]))
    if R2 is not None:
        m = m + np.abs(c2 * cols(R2, m.shape[1]))
    return m


def ulp16(x):
    """Spacing of fp16 at |x| (2^-24 in the subnormal range)."""
    a = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (np.maximum(e, -14.0) - 10.0)


def gauss_bound(ref64, mag, K):
    """|got - ref64| <= 0.5 ulp16(ref64) + (K + 8) 2^-23 mag, act = 0.  The first term is the one rounding to fp16.  The second: the K products are exact
    in fp32 (fp16 x fp16), the accumulator takes at most K additions, the epilogue at most 8 further operations (two bias additions, c0, two products and
    two additions of the residuals, one to spare), each with a relative error of at most one fp32 unit 2^-23 - twice the half unit of a round-to-nearest
    adder, since the rounding of the MFMA accumulator is not documented - of an intermediate that `mag` bounds.  No measured constant."""
    return 0.5 * ulp16(ref64) + (K + 8) * U32 * np.asarray(mag, np.float64)


def gauss_excess(got, ref64, mag, K):
    """max |got - ref64| / bound over the tensor: <= 1 passes."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "non-finite output"
    return float((np.abs(got - ref64) / gauss_bound(ref64, mag, K)).max())


# --------------------------------------------------------------------------------------------------- statistics
def frame_stats64(out16, T, HW):
    """out16 [T * HW, N]: per frame and column (sum, sum of squares) in float64 -> [T, N, 2]."""
    x = np.asarray(out16, np.float64).reshape(T, HW, -1)
    return np.stack([x.sum(1), (x * x).sum(1)], -1)


def consecutive_block_of_row(M, rb):
    """Block number of every output row where a block is rb consecutive rows (the tile_epilogue family)."""
    return np.arange(M) // rb


def halo_block_of_row(T, H, W, bm, lg, rb):
    """Block number of every output row of a halo-staged convolution (kernels/conv_halo.hip): a tile is TH x TW = bm pixels of one frame (TW = 1 << lg),
    tiles are numbered frame-major, then tile row, then tile column; inside a tile, tile row r = pixel (r >> lg, r & (TW - 1)) and wave wm owns the
    tile rows [wm * rb, (wm + 1) * rb): block (tile number) * (bm / rb) + wm."""
    tw, th = 1 << lg, bm >> lg
    assert th * tw == bm and H % th == 0 and W % tw == 0 and bm % rb == 0
    t, y, x = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    tile = (t * (H // th) + y // th) * (W // tw) + x // tw
    r = (y % th) * tw + x % tw
    return (tile * (bm // rb) + r // rb).reshape(-1)


def block_stats64(out16, block_of_row, nblocks):
    """(sum, sum of squares) of the rows filed under every block -> [nblocks, N, 2] float64, and the same of |x| for the error bound."""
    x = np.asarray(out16, np.float64)
    s = np.zeros((nblocks, x.shape[1], 2)); a = np.zeros((nblocks, x.shape[1]))
    np.add.at(s[:, :, 0], block_of_row, x)
    np.add.at(s[:, :, 1], block_of_row, x * x)
    np.add.at(a, block_of_row, np.abs(x))
    return s, a


def check_stats(part, rb, out16, T, HW, sentinel, exact, block_of_row=None, what="", strict=True):
    """part [nalloc, N, 2] float32 as the launch left it (it went up filled with the `sentinel` word), rb > 0 the rows per block it reported, out16 [T * HW, N]
    the fp16 output the SAME launch stored.  Asserts
      - every word of the blocks [0, M / rb) has lost the sentinel, every word beyond still has it;
      - per frame t and column n, the sum over the blocks [t HW / rb, (t + 1) HW / rb) equals the float64 (sum, sum of squares) of out16 over the frame's
        rows - the contract gn_finalize_cols consumes: exactly (exact=True: integer data, every partial sum an integer below 2^24), or within
        rb 2^-23 sum |x| (sum x^2) per block, summed over the frame's blocks (rb - 1 fp32 additions per column and block, one unit each; x * x of an fp16 x is
        exact in fp32);
      - with block_of_row (the block every output row belongs to), the same per block.
    Returns (frame excess, block excess): max |got - ref| / bound; on exact data the number of entries that differ.  strict=False: the sentinel checks
    only, the figures are returned without being asserted (tests/test_epilogue_oracle_cpu.py measures planted defects with it)."""
    out16 = np.asarray(out16, np.float64)
    M, N = out16.shape
    assert M == T * HW and rb > 0 and HW % rb == 0, (M, T, HW, rb)
    nb = M // rb
    bits = np.ascontiguousarray(part).view(np.uint32)
    assert part.shape[0] >= nb and part.shape[1:] == (N, 2), (part.shape, nb, N)
    kept = bits[:nb] == sentinel
    assert not kept.any(), f"{what}: {int(kept.sum())} statistics words of the blocks [0, {nb}) were not written, first block {int(np.argwhere(kept)[0][0])}"
    lost = bits[nb:] != sentinel
    assert not lost.any(), f"{what}: {int(lost.sum())} statistics words beyond block {nb} were written, first block {nb + int(np.argwhere(lost)[0][0])}"
    got = np.asarray(part[:nb], np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite statistics"
    ref_f = frame_stats64(out16, T, HW)
    got_f = got.reshape(T, HW // rb, N, 2).sum(1)
    absf = np.abs(out16).reshape(T, HW, N).sum(1)
    tol_f = rb * U32 * np.stack([absf, ref_f[..., 1]], -1)
    ex_f = ex_b = 0.0
    if exact:
        bad = np.argwhere(got_f != ref_f)
        ex_f = float(len(bad))
        assert not strict or not len(bad), f"{what}: per-frame totals differ at {len(bad)} (frame, column, sum | sumsq), first {tuple(bad[0])}: got {got_f[tuple(bad[0])]}, expected {ref_f[tuple(bad[0])]}"
    else:
        ex_f = float((np.abs(got_f - ref_f) / np.maximum(tol_f, 1e-300)).max())
        assert not strict or ex_f <= 1.0, f"{what}: per-frame totals off by {ex_f:.3g} x the bound"
    if block_of_row is not None:
        ref_b, abs_b = block_stats64(out16, block_of_row, nb)
        if exact:
            assert ref_b[..., 1].max() < 2 ** 24, f"{what}: a block's sum of squares leaves the exact fp32 integers"
            bad = np.argwhere(got != ref_b)
            ex_b = float(len(bad))
            assert not strict or not len(bad), f"{what}: per-block sums differ at {len(bad)} (block, column, sum | sumsq), first {tuple(bad[0])}: got {got[tuple(bad[0])]}, expected {ref_b[tuple(bad[0])]}"
        else:
            tol_b = rb * U32 * np.stack([abs_b, ref_b[..., 1]], -1)
            ex_b = float((np.abs(got - ref_b) / np.maximum(tol_b, 1e-300)).max())
            assert not strict or ex_b <= 1.0, f"{what}: per-block sums off by {ex_b:.3g} x the bound"
    return ex_f, ex_b


# --------------------------------------------------------------------------------------------------- data
def tri(rng, *shape):
    """{-1, 0, 1}: the matrix operands of the exact screens."""
    return rng.integers(-1, 2, shape).astype(np.float32)


def ints(rng, lim, *shape):
    return rng.integers(-lim, lim + 1, shape).astype(np.float32)


def evens(rng, lim, *shape):
    return (2 * rng.integers(-(lim // 2), lim // 2 + 1, shape)).astype(np.float32)


def gauss(rng, *shape, scale=1.0):
    """fp16-representable Gaussian data."""
    return h16(rng.standard_normal(shape) * scale)


# Exact operand screen: c0 = 2, c1 = -1, c2 = 0.5 with bias, bias2 in [-2, 2], R1 in [-8, 8], R2 even in [-8, 8].  Every operand has its own coefficient, so
# one dropped, doubled, swapped with another, applied on the wrong side of c0 or read from the wrong row / column run moves some output by a non-zero integer.
EXACT_COEF = dict(c0=2.0, c1=-1.0, c2=0.5)
# name -> operands present.  The first five are the subsets of the issue; the two "lean" ones (c0 = c1 = 1, no R2) reach the epilogues without run-time
# variants (tile_epilogue_lean, modes 1 / 2 of the statistics epilogue), which the coefficients above never select.
SUBSETS = {
    "all five": dict(bias=1, bias2=1, R1=1, R2=1),
    "bias2 alone": dict(bias2=1),
    "R2 alone": dict(R2=1),
    "R1 with R2": dict(R1=1, R2=1),
    "bias2 without bias": dict(bias2=1, R1=1),
    "lean bias + bias2": dict(bias=1, bias2=1, lean=1),
    "lean bias + bias2 + R1": dict(bias=1, bias2=1, R1=1, lean=1),
}


def exact_operands(rng, rows, n_bias, nout, ldr1=0, ldr2=0):
    """The full set of integer operands; residuals [rows, ld] (ld 0: nout), their surplus columns filled too (a kernel that reads them is wrong)."""
    return dict(bias=ints(rng, 2, n_bias), bias2=ints(rng, 2, n_bias), R1=ints(rng, 8, rows, ldr1 or nout), R2=evens(rng, 8, rows, ldr2 or nout))


def subset_kwargs(ops, name, coef=None):
    """Keyword arguments (operands + coefficients) of one subset, for epilogue64 and for the engine wrappers alike."""
    s = SUBSETS[name]
    kw = {k: ops[k] for k in ("bias", "bias2", "R1", "R2") if s.get(k)}
    kw.update(dict(c0=1.0, c1=1.0, c2=1.0) if s.get("lean") else (coef or EXACT_COEF))
    return kw


def exact_ref(acc, **kw):
    """epilogue64 on integer data as int64, with the preconditions of the exact screen asserted: the float64 evaluation is itself an integer (so it is
    exact) and below 2048 in size (so it is an exact fp16 number, as every intermediate is an exact fp32 one: |.| < 2^24)."""
    ref = epilogue64(acc, **kw)
    ri = np.rint(ref)
    assert np.array_equal(ri, ref), "the integer reference is not an integer"
    assert np.abs(ri).max() < 2048, f"the reference leaves the exact fp16 integers: max {np.abs(ri).max()}"
    return ri.astype(np.float32)


def conv_acc64(x, w, x1=None, **kw):
    """util.conv_f64 without bias as a [rows, O] matrix."""
    y = conv_f64(x, w, None, x1=x1, **kw)
    return y.reshape(-1, y.shape[-1])
