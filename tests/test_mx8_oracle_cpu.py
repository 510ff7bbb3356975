"""CPU: the reference of the MX-fp8 op tests is pinned independently, and the generators of tests/mx8_oracle.py meet the conditions their checks rest on
(DESIGN.md section 27).

  * util.e4m3_rne / e4m3_encode against torch's float8_e4m3fn conversion on every finite fp16 value with |x| <= 448.  Saturation above 448 is the project's
    own definition (fminf / fmaxf before the conversion in kernels/mx8.hip): stated here, not borrowed.
  * the quantiser edge matrix really contains ties of both parities, saturated elements, e4m3 subnormals, -0.0, fp16-subnormal blocks, zero blocks, 65504.
  * the exact screen: fp16-exact operands, lossless quantisation, the sum of absolute terms below 2^24 granules, max |ref| < 65504 - on exactly the
    shapes and seeds the GPU test runs.
  * the planted scale defects move the reference by far more than any bound the GPU tests use.
"""
import numpy as np
import pytest
import torch

import mx8_oracle as mo
from util import e4m3_encode, e4m3_rne, h16, mx8_quantise, rel_err


def test_e4m3_reference_matches_torch_on_every_fp16_value_in_range():
    h = np.arange(65536, dtype=np.uint16).view(np.float16)
    h = h[np.isfinite(h) & (np.abs(h.astype(np.float32)) <= 448)]
    assert len(h) == 48642
    x = h.astype(np.float32)
    t8 = torch.from_numpy(x).to(torch.float8_e4m3fn)
    want_v, want_b = t8.to(torch.float32).numpy(), t8.view(torch.uint8).numpy()
    got_v = e4m3_rne(x)
    assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32))            # values, the sign of zero included
    assert np.array_equal(e4m3_encode(got_v), want_b)


def test_saturation_is_the_projects_definition():
    x = np.array([448.125, 464.0, 480.0, 511.75, 1e4, 65504.0, -449.0, -65504.0], np.float32)
    assert np.array_equal(e4m3_rne(x), np.copysign(448.0, x).astype(np.float32))
    assert np.array_equal(e4m3_encode(e4m3_rne(x)), np.where(x > 0, 0x7E, 0xFE).astype(np.uint8))


def test_dequant_inverts_the_encoding():
    x = mo.edge_matrix(128)
    deq, b, e = mx8_quantise(x)
    assert np.array_equal(mo.dequant(b, e).astype(np.float32).view(np.uint32), deq.view(np.uint32))


@pytest.mark.parametrize("K", [128, 256, 640])
def test_edge_matrix_holds_every_class(K):
    x = mo.edge_matrix(K)
    assert x.shape[1] == K and mo.fp16_exact(x).all()
    cls = mo.edge_classes(x)
    print("edge matrix", x.shape, cls)
    for k in ("ties_lower_even", "ties_lower_odd", "saturated", "e4m3_subnormal", "negative_zero", "fp16_subnormal_blocks", "zero_blocks"):
        assert cls[k] > 0, (k, cls)
    assert cls["ties"] > 10000 and cls["saturated"] > 100 and cls["max"] == 65504.0
    # the three block maxima at every exponent fp16 can hold them at
    amax = np.abs(x.reshape(x.shape[0], -1, 32)).max(-1)
    for t in mo.EDGE_TS:
        for m in mo.EDGE_MANTISSAS:
            if mo.fp16_exact(m * 2.0 ** t):
                assert (amax == np.float32(m * 2.0 ** t)).any(), (m, t)
    # and the reference puts the two tie parities on different sides
    deq, _, e = mx8_quantise(x)
    s = np.repeat(2.0 ** (e.astype(np.float64) - 127), 32, axis=1)
    v, q = np.abs(x) / s, np.abs(deq) / s
    tie = np.isin(v, mo.E4M3_TIES)
    assert (q[tie] < v[tie]).any() and (q[tie] > v[tie]).any()


def _exact_shapes():
    shapes = [(M, N, K) for M in (mo.EXACT_MS[0], mo.EXACT_MS[-1]) for N in (mo.EXACT_NS[0], mo.EXACT_NS[-1]) for K in mo.EXACT_KS]
    return shapes + [(257, 136, 384), mo.EXACT_GROUPED, mo.EXACT_WALK]


@pytest.mark.parametrize("M,N,K", _exact_shapes())
def test_exact_screen_conditions(M, N, K):
    c = mo.exact_case(M, N, K, epilogue=True)
    assert len(mo.EXACT_TS) >= 5
    for op, t in ((c["A"], c["ta"]), (c["W"], c["tw"])):           # the exponent of every block is known: t + 2 - 8
        assert np.array_equal(mx8_quantise(op)[2].astype(np.int64) - 127, t + 2 - 8)
    if M * K >= 32 * 128 * 4:
        assert len(np.unique(c["ta"])) == len(mo.EXACT_TS)
    for name, (bias, R1, R2, c0, c1, c2) in mo.EPI_FORMS.items():
        ok16, lossless, units, mx = mo.exact_conditions(c, bias, R1, R2, c0, c1, c2)
        print(f"exact screen {M}x{N}x{K} {name}: sum of |terms| = {units:.0f} granules (2^{np.log2(units):.1f}), max |ref| = {mx}")
        assert ok16 and lossless
        assert units < 2 ** 23                                        # room: half of what fp32 holds exactly
        assert mx < 65504 / 2


def test_exact_screen_worst_case_is_bounded_by_reasoning():
    """Whatever the draw: K * (4 * 2^2)^2 = K * 2^8 in real units = K * 2^12 granules of 2^-4; 2^22 at K = 1024."""
    assert mo.EXACT_KMAX * (mo.EXACT_INT * 2.0 ** max(mo.EXACT_TS)) ** 2 / 2.0 ** (2 * min(mo.EXACT_TS)) <= 2 ** 22
    assert max(max(mo.EXACT_KS), mo.EXACT_WALK[2], mo.EXACT_GROUPED[2]) <= mo.EXACT_KMAX


@pytest.mark.parametrize("defect", mo.PLANTED)
@pytest.mark.parametrize("side", ["A", "W"])
def test_planted_scale_defects_miss_by_far(defect, side):
    """A misplaced scale is a factor of at least 2 on a whole block: on the exact screen thousands of outputs change, and the error relative to max |ref|
    is orders of magnitude above both the exact check (0) and the Gaussian bound (< 1e-3)."""
    c = mo.exact_case(257, 136, 384)
    g = mo.gauss_case(257, 136, 384)
    for name, A, W in (("exact", c["A"], c["W"]), ("gauss", g["A"], g["W"])):
        (_, ab, ae), (_, wb, we) = mx8_quantise(A), mx8_quantise(W)
        ref = mo.dequant(ab, ae) @ mo.dequant(wb, we).T
        bad = mo.dequant(ab, mo.planted(ae, defect)) @ mo.dequant(wb, we).T if side == "A" else mo.dequant(ab, ae) @ mo.dequant(wb, mo.planted(we, defect)).T
        err = rel_err(bad, ref)
        frac = float((h16(bad) != h16(ref)).mean())
        print(f"planted {defect} on {side}, {name} data: rel err {err:.3e}, {frac:.1%} of the fp16 outputs differ")
        assert err > (0.05 if name == "exact" else 0.02) and frac > 0.5


def test_gaussian_bound_comes_from_the_reference_rounding():
    """The bound of the Gaussian checks: twice the error of fp16(ref64) against ref64 in the same metric (max |err| / max |ref|) - the reference's own
    output rounding, doubled for an fp32 summation order that tips a rounding the other way.  It can never exceed 2^-10."""
    g = mo.gauss_case(300, 256, 640)
    ref = mx8_quantise(g["A"])[0].astype(np.float64) @ mx8_quantise(g["W"])[0].astype(np.float64).T + g["bias"]
    r = rel_err(h16(ref), ref)
    print(f"reference rounding {r:.3e}, bound {2 * r:.3e}")
    assert 0 < r <= 2.0 ** -11 and 2 * r < 1e-3
