"""The numpy restatements that tests/test_conv_bound_gpu.py compares the device against, checked here against the definition (no GPU needed).

phase_weights restates k_upsample_phase_w (kernels/misc.hip): a nearest-2x upsample followed by a zero-padded 3x3 convolution is four 2x2
convolutions on the source grid, one per output parity (a, b); rows 2y-1, 2y, 2y+1 of the upsampled image are source rows y-1, y, y (a = 0) or
y, y, y+1 (a = 1), so the three taps collapse to {w0, w1+w2} or {w0+w1, w2}, and the same along x.  bound_layout restates k_permute_conv_w and
k_rechunk_conv_w: the K order in which bind_conv (engine.hip) leaves a weight.  conv_phases_f64 evaluates the four-phase form in fp64, so that

1. on integer data the four-phase form with unrounded phase weights equals conv_f64(..., ups=2) exactly, at every shape of the GPU file;
2. on the GPU file's Gaussian data the ONE rounding of the phase weights to fp16 is measured against the definition: REF_ONLY_ERR, asserted here,
   so that a later change of shapes cannot let the reference's own error eat the GPU test's tolerance."""
import functools

import numpy as np
import pytest

from util import conv_f64, h16

TOL = 2e-3              # test_ops_gpu.TOL (asserted equal in the GPU file): the project's max|err| / max|ref| bound of an fp16-stored output

# (T, H, W, C, O) of the sub-pixel problems of tests/test_conv_bound_gpu.py
EXACT_SHAPES = [(5, 20, 28, 128, 192), (3, 7, 9, 192, 64), (2, 1, 1, 64, 64), (2, 1, 6, 64, 64), (2, 6, 1, 64, 64), (3, 5, 7, 40, 72)]
RANDOM_SHAPES = [(2, 6, 8, 128, 128), (3, 5, 7, 64, 64), (2, 3, 5, 40, 72), (1, 4, 4, 320, 320)]
# max|four-phase form in fp64, phase weights rounded once to fp16 - definition| / max|definition| on random_problem(shape): measured by
# test_reference_only_error_is_recorded_and_small, which asserts them
REF_ONLY_ERR = {(2, 6, 8, 128, 128): 2.084e-4, (3, 5, 7, 64, 64): 1.911e-4, (2, 3, 5, 40, 72): 2.224e-4, (1, 4, 4, 320, 320): 2.158e-4}


def pad8(n):
    return (n + 7) // 8 * 8


def phase_weights(w9, rounded=True):
    """w9 [O, I, 1, 3, 3] (or [O, I, 3, 3]) -> the sub-pixel weights [4][O][2*2][Ipad] in tap-major order: phase 2a + b, tap 2p + q, zero pad columns.
    rounded: inputs rounded to fp16, sums formed in fp32 in the kernel's order (iy, then ix, ascending) and rounded once to fp16 (returned as float32);
    otherwise the exact fp64 sums of w9 as given."""
    w = np.asarray(w9)
    O, I = w.shape[:2]
    w = w.reshape(O, I, 3, 3)
    w = h16(w) if rounded else w.astype(np.float64)
    out = np.zeros((4, O, 4, pad8(I)), w.dtype)
    for a in range(2):
        for b in range(2):
            for iy in range(3):
                for ix in range(3):
                    p = (0 if iy == 0 else 1) if a == 0 else (1 if iy == 2 else 0)
                    q = (0 if ix == 0 else 1) if b == 0 else (1 if ix == 2 else 0)
                    out[2 * a + b, :, 2 * p + q, :I] += w[:, :, iy, ix]
    return h16(out) if rounded else out


def rechunk(w, taps, cinp):
    """[rows][taps][cinp] -> [rows][cinp/64][taps][64], flattened per row (k_rechunk_conv_w)."""
    w = w.reshape(-1, taps, cinp // 64, 64)
    return np.ascontiguousarray(w.transpose(0, 2, 1, 3)).reshape(w.shape[0], taps * cinp)


def is_chunk_major(taps, cinp):
    return taps > 1 and cinp % 64 == 0


def bound_layout(w, kt, k, cinp):
    """Checkpoint-layout w [O, I, kt, k, k] -> the bound Conv::w as [O, taps * cinp] float32 of fp16 values: tap-major [O][taps][cinp] with zero pad
    columns, chunk-major [O][cinp/64][taps][64] when taps > 1 and cinp % 64 == 0."""
    w = h16(w)
    O, I = w.shape[:2]
    taps = kt * k * k
    out = np.zeros((O, taps, cinp), np.float32)
    out[:, :, :I] = w.reshape(O, I, taps).transpose(0, 2, 1)
    return rechunk(out, taps, cinp) if is_chunk_major(taps, cinp) else out.reshape(O, taps * cinp)


def bound_phase_layout(w9, cinp):
    """The bound Conv::wphase as [4, O, 4 * cinp]: phase_weights, re-chunked with taps = 4 over 4 * O rows where the weight itself is chunk-major."""
    w4 = phase_weights(w9)
    O = w4.shape[1]
    assert w4.shape[3] == cinp
    return (rechunk(w4, 4, cinp) if is_chunk_major(9, cinp) else w4).reshape(4, O, 4 * cinp)


def conv_phases_f64(x, w4, b):
    """The four-phase form in fp64: x [T,H,W,C], tap-major phase weights w4 [4][O][4][Cpad] -> [T,2H,2W,O].  Phase (a, b) is a 2x2 convolution on the
    source grid with pads (1 - a, 1 - b), written to the output pixels (2y + a, 2x + b); pixels no phase writes stay NaN."""
    T, H, W, C = x.shape
    O = w4.shape[1]
    out = np.full((T, 2 * H, 2 * W, O), np.nan)
    for a in range(2):
        for bb in range(2):
            wp = np.asarray(w4[2 * a + bb], np.float64)[:, :, :C].reshape(O, 2, 2, C).transpose(0, 3, 1, 2).reshape(O, C, 1, 2, 2)
            out[:, a::2, bb::2] = conv_f64(x, wp, b, k=2, pad_t=1 - a, pad_l=1 - bb)
    return out


@functools.lru_cache(maxsize=None)
def exact_problem(shape):
    """x, w in {-1, 0, 1}, bias in [-2, 2] and the integer reference conv_f64(x, w, b, ups=2) of one sub-pixel problem (T, H, W, C, O)."""
    T, H, W, C, O = shape
    rng = np.random.default_rng(sum(shape) + 7 * C)
    x = rng.integers(-1, 2, (T, H, W, C)).astype(np.float32)
    w = rng.integers(-1, 2, (O, C, 1, 3, 3)).astype(np.float32)
    b = rng.integers(-2, 3, O).astype(np.float32)
    ref = conv_f64(x, w, b, ups=2)
    for a in (x, w, b, ref):
        a.setflags(write=False)
    return x, w, b, ref


@functools.lru_cache(maxsize=None)
def random_problem(shape):
    """x ~ N(0, 1), w ~ N(0, 1 / (9 C)), b ~ N(0, 0.01), all rounded to fp16, and the definition conv_f64(x, w, b, ups=2) with the raw weights."""
    T, H, W, C, O = shape
    rng = np.random.default_rng(1000 + sum(shape))
    x = h16(rng.standard_normal((T, H, W, C)))
    w = h16(rng.standard_normal((O, C, 1, 3, 3)) * (9 * C) ** -0.5)
    b = h16(0.1 * rng.standard_normal(O))
    ref = conv_f64(x, w, b, ups=2)
    for a in (x, w, b, ref):
        a.setflags(write=False)
    return x, w, b, ref


# ---------------------------------------------------------------------------------------------------
def test_phase_weights_are_the_collapsed_taps():
    """Spelled out for one weight: phase (a, b) = (rows collapsed for a) x (columns collapsed for b), tap 2p + q, pad columns zero."""
    rng = np.random.default_rng(1)
    w = rng.integers(-1023, 1024, (3, 5, 1, 3, 3)) / 1024.0
    got = phase_weights(w, rounded=False)
    assert got.shape == (4, 3, 4, 8) and not got[..., 5:].any()
    w = w.reshape(3, 5, 3, 3)
    rows = {0: [w[:, :, 0], w[:, :, 1] + w[:, :, 2]], 1: [w[:, :, 0] + w[:, :, 1], w[:, :, 2]]}        # [p] -> [O, I, 3 (ix)]
    for a in range(2):
        for b in range(2):
            for p in range(2):
                r = rows[a][p]
                cols = [r[..., 0], r[..., 1] + r[..., 2]] if b == 0 else [r[..., 0] + r[..., 1], r[..., 2]]
                for q in range(2):
                    assert np.array_equal(got[2 * a + b, :, 2 * p + q, :5], cols[q]), (a, b, p, q)
    # multiples of 2^-10 in (-1, 1): every sum of up to four is a multiple of 2^-10 below 4 - exact in fp32, so the rounded form is ONE fp16 rounding of the exact sum
    assert np.array_equal(phase_weights(w), got.astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("shape", EXACT_SHAPES + RANDOM_SHAPES, ids=str)
def test_four_phases_equal_the_definition_on_integers(shape):
    T, H, W, C, O = shape
    x, w, b, ref = exact_problem(shape)
    assert np.array_equal(np.rint(ref), ref) and np.abs(ref).max() <= 9 * C + 2
    w4 = phase_weights(w, rounded=False)
    assert np.abs(w4).max() <= 4 and np.array_equal(np.rint(w4), w4)
    got = conv_phases_f64(x, w4, b)
    assert not np.isnan(got).any(), "a pixel no phase wrote"
    assert np.array_equal(got, ref)
    # integers up to 4 are fp16 numbers: the rounded phase weights are the same ones
    assert np.array_equal(phase_weights(w), w4)


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=str)
def test_integer_data_sees_the_errors_the_screen_is_for(shape):
    """The screen's data is not blind to the two mistakes named in its comments: phases scattered to the transposed parity, and a tap that ignores the
    frame edge (the clip evaluated as one tall frame of T * H rows: row y + 1 of a frame's last row is then the next frame's first)."""
    T, H, W, C, O = shape
    x, w, b, ref = exact_problem(shape)
    w4 = phase_weights(w, rounded=False)
    swapped = conv_phases_f64(x, w4[[0, 2, 1, 3]], b)
    assert not np.array_equal(swapped, ref)
    tall = conv_phases_f64(x.reshape(1, T * H, W, C), w4, b).reshape(ref.shape)
    assert not np.array_equal(tall, ref)
    assert np.array_equal(tall[:, 1:-1], ref[:, 1:-1])          # only the rows at the frame edges read across them


@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=str)
def test_reference_only_error_is_recorded_and_small(shape):
    x, w, b, ref = random_problem(shape)
    got = conv_phases_f64(x, phase_weights(w), b)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"reference-only error {shape}: {err:.4e}")
    rec = REF_ONLY_ERR[shape]
    assert abs(err - rec) <= 0.01 * rec, f"{shape}: measured {err:.4e}, recorded {rec:.4e}"
    # with the fp16 store of the output (2^-11 of max|ref| at the most) the reference side stays under half of the bound
    assert rec + 2.0 ** -11 < TOL / 2


LAYOUT_CASES = [(64, 64, 1, 3), (72, 192, 1, 3), (64, 40, 1, 3), (16, 4, 1, 3), (64, 128, 3, 1), (64, 128, 1, 1)]     # (O, I, kt, k) of the GPU file


@pytest.mark.parametrize("O,I,kt,k", LAYOUT_CASES)
def test_bound_layout_against_the_index_formula(O, I, kt, k):
    rng = np.random.default_rng(O + I + kt + k)
    w = (rng.integers(-1023, 1024, (O, I, kt, k, k)) / 1024.0).astype(np.float32)
    taps, cinp = kt * k * k, pad8(I)
    lay = bound_layout(w, kt, k, cinp)
    assert lay.shape == (O, taps * cinp)
    i, tp = np.meshgrid(np.arange(I), np.arange(taps), indexing="ij")
    pos = ((i // 64) * taps + tp) * 64 + i % 64 if is_chunk_major(taps, cinp) else tp * cinp + i
    assert np.array_equal(lay[:, pos], w.reshape(O, I, taps))
    rest = np.ones(taps * cinp, bool)
    rest[pos.ravel()] = False
    assert rest.sum() == taps * (cinp - I) and not lay[:, rest].any()


@pytest.mark.parametrize("O,I,kt,k", LAYOUT_CASES[:4])
def test_bound_phase_layout_against_the_index_formula(O, I, kt, k):
    rng = np.random.default_rng(O + I)
    w = (rng.integers(-1023, 1024, (O, I, 1, 3, 3)) / 1024.0).astype(np.float32)
    cinp = pad8(I)
    w4 = phase_weights(w)
    lay = bound_phase_layout(w, cinp)
    assert lay.shape == (4, O, 4 * cinp)
    i, tp = np.meshgrid(np.arange(cinp), np.arange(4), indexing="ij")
    pos = ((i // 64) * 4 + tp) * 64 + i % 64 if cinp % 64 == 0 else tp * cinp + i
    assert np.array_equal(lay[:, :, pos], w4.transpose(0, 1, 3, 2))
    assert sorted(pos.ravel()) == list(range(4 * cinp))
