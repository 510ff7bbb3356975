"""The screens of tests/test_epilogue_forms_gpu.py must be able to see a wrong kernel.

A float32 numpy model of a GEMM launch - the K sum in 64-wide chunks from the last to the first, the epilogue in float32, one rounding to fp16, the
statistics in float32 from the last row of a block to the first - stands in for a kernel.  Without a defect it passes the exact screen and the bounds of the
Gaussian and the statistics tests (the very functions the GPU tests call: tests/epilogue_oracle.py).  With one planted defect each it fails the exact
screen and misses the Gaussian bound at least tenfold on some case.

One defect cannot fail an exact screen by construction: statistics taken of the UNROUNDED float32 values.  On integer data below 2048 the unrounded and the
rounded value are the same number.  It is seen by the Gaussian bound alone: 60 x the bound per block and 11 x per frame on independent Gaussian columns,
124 x on a column that is constant over a frame (zero weights: the rounding errors of its rows add up coherently).  Both sides are asserted below, so that
nobody takes the integer screen for more than it is."""
import numpy as np
import pytest

import epilogue_oracle as eo

SENT = 0x7FC5A5A5
EPI_DEFECTS = ["bias2 dropped", "bias2 shifted by one 16-column run", "c1 / c2 swapped", "c0 applied after the residuals", "R2 indexed with ldr1",
               "GEGLU residual columns at N instead of N / 2"]
STAT_DEFECTS = ["a block filed one frame late", "frame-fastest permutation left out of the block index", "statistics of the unrounded values"]


# --------------------------------------------------------------------------------------------------- the model kernel
def model_gemm(A, W, bias=None, bias2=None, R1=None, R2=None, c0=1.0, c1=1.0, c2=1.0, geglu=False, defect=None):
    """-> (fp16 output widened to float32, the unrounded float32 values).  R1 / R2 [M, ld]."""
    f = np.float32
    A, W = A.astype(f), W.astype(f)
    M, K = A.shape; N = W.shape[0]
    acc = np.zeros((M, N), f)
    for k0 in reversed(range(0, K, 64)):
        acc += A[:, k0:k0 + 64] @ W[:, k0:k0 + 64].T
    v = acc
    if bias is not None:
        v = v + bias.astype(f)
    if bias2 is not None and defect != "bias2 dropped":
        v = v + (np.roll(bias2, -16) if defect == "bias2 shifted by one 16-column run" else bias2).astype(f)
    nout = N
    if geglu:
        nout = N // 2
        v = (v[:, :nout] * eo.act64(v[:, nout:].astype(np.float64), 2).astype(f)).astype(f)
    if defect == "c1 / c2 swapped":
        c1, c2 = c2, c1
    col = np.arange(nout)
    if geglu and defect == "GEGLU residual columns at N instead of N / 2":
        col = col + 8 * (col // 8)        # a lane's first output column taken as nb (its first of 16 GEMM columns) instead of nb / 2
    res = np.zeros((M, nout), f)
    if R1 is not None:
        res = res + f(c1) * R1[:, col].astype(f)
    if R2 is not None:
        if defect == "R2 indexed with ldr1":
            flat = R2.ravel()
            r2 = flat[(np.arange(M)[:, None] * (nout if R1 is None else R1.shape[1]) + col[None, :])]
        else:
            r2 = R2[:, col]
        res = res + f(c2) * r2.astype(f)
    o = f(c0) * (v + res) if defect == "c0 applied after the residuals" else f(c0) * v + res
    o = o.astype(f)
    return o.astype(np.float16).astype(f), o


def model_stats(out16, raw32, rb, T, HW, bm, defect=None):
    """part [ceil(M / 48), N, 2] float32 as a launch with blocks of rb consecutive rows, tiles of bm rows and the frame-fastest tile walk would leave it."""
    f = np.float32
    M, N = out16.shape
    nb = M // rb
    src = raw32 if defect == "statistics of the unrounded values" else out16
    x = src.astype(f).reshape(nb, rb, N)[:, ::-1]
    s = np.zeros((nb, N), f); q = np.zeros((nb, N), f)
    for i in range(rb):
        s += x[:, i]; q += x[:, i] * x[:, i]
    blocks = np.stack([s, q], -1)
    at = np.arange(nb)
    if defect == "a block filed one frame late":
        first = at % (HW // rb) == 0                      # the first block of every frame lands in the next frame's slot (the last frame's in frame 0's)
        at = np.where(first, (at + HW // rb) % nb, at)
    if defect == "frame-fastest permutation left out of the block index":
        w, per, nbf = bm // rb, M // bm, HW // bm          # walk index i runs tile (i % T) * nbf + i // T; the defect files it under i
        i = np.arange(per)
        tile_of_walk = (i % T) * nbf + i // T
        at = np.empty(nb, np.int64)
        at[(tile_of_walk[:, None] * w + np.arange(w)[None, :]).ravel()] = (i[:, None] * w + np.arange(w)[None, :]).ravel()
    part = np.full(((M + 47) // 48, N, 2), SENT, np.uint32).view(f)
    part[at] = blocks
    return part


# --------------------------------------------------------------------------------------------------- the cases (small)
def _dense(rng, gen, M, K, N, geglu=False):
    nout = N // 2 if geglu else N
    A, W = gen(rng, M, K), gen(rng, N, K)
    if geglu:
        W[N // 2:] = 0                                     # gates: zero weights, see _geglu_gate
    return A, W, nout


def _exact_case(seed, geglu=False, gate=0.0):
    rng = np.random.default_rng(seed)
    M, K, N = 70, 192, 256 if geglu else 96
    A, W, nout = _dense(rng, eo.tri, M, K, N, geglu)
    ops = eo.exact_operands(rng, M, N, nout, ldr1=N if geglu else nout, ldr2=N if geglu else nout + 8)
    if geglu:
        ops["bias"][N // 2:] = gate; ops["bias2"][N // 2:] = 0
    acc = A.astype(np.float64) @ W.astype(np.float64).T
    return A, W, ops, acc


def _gauss_case(seed, geglu=False):
    rng = np.random.default_rng(seed)
    M, K, N = 70, 192, 256 if geglu else 96
    nout = N // 2 if geglu else N
    A, W = eo.gauss(rng, M, K), eo.gauss(rng, N, K, scale=K ** -0.5)
    ops = dict(bias=eo.gauss(rng, N), bias2=eo.gauss(rng, N), R1=eo.gauss(rng, M, N if geglu else nout), R2=eo.gauss(rng, M, N if geglu else nout + 8))
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    return A, W, ops, A64 @ W64.T, np.abs(A64) @ np.abs(W64).T, K


GCOEF = dict(c0=0.3, c1=0.3, c2=0.7)


def _exact_fails(defect):
    """Does the exact screen see the defect on some subset (dense), or on the GEGLU gate = 0 / saturated-gate cases?"""
    seen = []
    A, W, ops, acc = _exact_case(1)
    for name in eo.SUBSETS:
        kw = eo.subset_kwargs(ops, name)
        got, _ = model_gemm(A, W, defect=defect, **kw)
        seen.append(not np.array_equal(got, eo.exact_ref(acc, **kw)))
    for gate in (0.0, 16.0):
        A, W, ops, acc = _exact_case(2, geglu=True, gate=gate)
        kw = eo.subset_kwargs(ops, "all five")
        got, _ = model_gemm(A, W, geglu=True, defect=defect, **kw)
        seen.append(not np.array_equal(got, eo.exact_ref(acc, geglu=True, **kw)))
    return seen


def _gauss_excess(defect):
    A, W, ops, acc, absacc, K = _gauss_case(3)
    got, _ = model_gemm(A, W, defect=defect, **ops, **GCOEF)
    ex = [eo.gauss_excess(got, eo.epilogue64(acc, **ops, **GCOEF), eo.epilogue_mag(absacc, **ops, **GCOEF), K)]
    if defect is None or defect.startswith("GEGLU"):
        # GEGLU with residuals: against float64 at the project's TOL (the gate's erf / exp are not bounded by a derivation), expressed as error / TOL
        A, W, ops, acc, absacc, K = _gauss_case(4, geglu=True)
        got, _ = model_gemm(A, W, geglu=True, defect=defect, **ops, **GCOEF)
        ref = eo.epilogue64(acc, geglu=True, **ops, **GCOEF)
        ex.append(float(np.abs(got - ref).max() / np.abs(ref).max() / 2e-3))
    return ex


# --------------------------------------------------------------------------------------------------- tests
def test_preconditions_of_the_integer_data():
    """Reference below 2048 (asserted inside exact_ref for every subset) and block sums of squares below 2^24, at the K and block sizes of the GPU file."""
    for K in (192, 576, 1352, 1728):
        rng = np.random.default_rng(K)
        M, N = 512, 128
        A, W = eo.tri(rng, M, K), eo.tri(rng, N, K)
        ops = eo.exact_operands(rng, M, N, N)
        acc = A.astype(np.float64) @ W.astype(np.float64).T
        for name in eo.SUBSETS:
            ref = eo.exact_ref(acc, **eo.subset_kwargs(ops, name))
            for rb in (48, 128):
                sq, _ = eo.block_stats64(ref[:M // rb * rb], eo.consecutive_block_of_row(M // rb * rb, rb), M // rb)
                assert sq[..., 1].max() < 2 ** 24, (K, name, rb, sq[..., 1].max())
    assert np.array_equal(eo.ulp16(np.array([0.0, 1.0, 1.5, 2.0, 2047.0, 6e-8])), 2.0 ** np.array([-24.0, -10, -10, -9, 0, -24]))


def test_model_without_defect_passes_every_screen():
    assert not any(_exact_fails(None))
    ex = _gauss_excess(None)
    assert max(ex) <= 1.0, ex


@pytest.mark.parametrize("defect", EPI_DEFECTS)
def test_planted_epilogue_defect_is_seen(defect):
    seen = _exact_fails(defect)
    assert any(seen), f"{defect}: the exact screen passes"
    ex = _gauss_excess(defect)
    assert max(ex) >= 10.0, f"{defect}: misses the Gaussian bound by only {max(ex):.3g} x"


def _stat_cases():
    """(name, out16, raw32, exact) over T = 3 frames of HW = 768 rows, 64 columns: integer data, Gaussian data, and a column-constant output (zero weights:
    every row of a column is c0 * (bias + bias2), so the fp16 rounding errors of a frame add up coherently)."""
    T, HW, N, K = 3, 768, 64, 192
    rng = np.random.default_rng(7)
    A, W = eo.tri(rng, T * HW, K), eo.tri(rng, N, K)
    ops = eo.exact_operands(rng, T * HW, N, N)
    out = [("integer", *model_gemm(A, W, **eo.subset_kwargs(ops, "all five")), True)]
    A, W = eo.gauss(rng, T * HW, K), eo.gauss(rng, N, K, scale=K ** -0.5)
    g = dict(bias=eo.gauss(rng, N), bias2=eo.gauss(rng, N), R1=eo.gauss(rng, T * HW, N))
    out.append(("Gaussian", *model_gemm(A, W, c0=0.6, **g), False))
    out.append(("column-constant", *model_gemm(A, 0 * W, c0=0.6, bias=g["bias"], bias2=g["bias2"]), False))
    return T, HW, out


@pytest.mark.parametrize("rb,bm", [(48, 192), (64, 256), (128, 256)])
def test_statistics_model_without_defect_passes(rb, bm):
    T, HW, cases = _stat_cases()
    for name, o16, raw, exact in cases:
        part = model_stats(o16, raw, rb, T, HW, bm)
        eo.check_stats(part, rb, o16, T, HW, SENT, exact, eo.consecutive_block_of_row(T * HW, rb), what=name)


@pytest.mark.parametrize("defect", STAT_DEFECTS)
def test_planted_statistics_defect_is_seen(defect):
    T, HW, cases = _stat_cases()
    rb, bm = 48, 192
    res = {}
    for name, o16, raw, exact in cases:
        part = model_stats(o16, raw, rb, T, HW, bm, defect)
        res[name] = eo.check_stats(part, rb, o16, T, HW, SENT, exact, eo.consecutive_block_of_row(T * HW, rb), what=name, strict=False)
    if defect == "statistics of the unrounded values":
        assert res["integer"] == (0.0, 0.0)                    # invisible on exact data by construction (module docstring)
        assert min(res["column-constant"]) >= 10.0, res         # measured: 124 x per frame and per block
        assert max(res["Gaussian"]) >= 10.0, res                # measured: 60 x per block, 11 x per frame
    elif defect == "frame-fastest permutation left out of the block index":
        assert res["integer"][0] > 0 and res["integer"][1] > 0, res
        assert res["Gaussian"][0] >= 10.0 and res["Gaussian"][1] >= 10.0, res
    else:
        assert res["integer"][0] > 0 and res["integer"][1] > 0, res
        assert res["Gaussian"][0] >= 10.0, res


def test_halo_block_numbering_covers_each_frame_with_its_own_blocks():
    """The contract of the per-frame totals for the 2-D blocks of the halo tiles: frame t's rows fall into the blocks [t HW / rb, (t + 1) HW / rb), rb rows each."""
    for (H, W, bm, lg, rb) in [(32, 48, 256, 4, 64), (24, 64, 256, 5, 64), (20, 64, 256, 6, 64), (24, 32, 192, 4, 48)]:
        T, HW = 2, H * W
        blk = eo.halo_block_of_row(T, H, W, bm, lg, rb)
        assert np.array_equal(np.bincount(blk), np.full(T * HW // rb, rb))
        assert np.array_equal(blk // (HW // rb), np.arange(T * HW) // HW)
        if lg < 6 or rb > 64:
            assert not np.array_equal(blk, eo.consecutive_block_of_row(T * HW, rb))     # not consecutive rows
