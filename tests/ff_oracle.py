"""float64 reference for the fused GEGLU feed-forward (kernels/ff_fused.hip), an fp32 emulation of the kernel's arithmetic, the elementwise bound and
the case table that tests/test_ff_oracle_cpu.py and tests/test_ff_forms_gpu.py share.

The operation:  out = c0 * (mid W2^T + b2) + c1 * r1 + c2 * R2,  mid = hv * GELU(hg),  [hv | hg] = xn W1^T + b1  (W1 [8C][C]: 4C value rows, then 4C gate rows),
xn = X, or with the pre-norm xn = LayerNorm(x') * gamma + beta on x' = fp16(X + addvec[row // rows_per_vec]); r1 is a tensor of its own or the stream x'.

The reference (ff_f64) is staged: float64 arithmetic, rounded to fp16 exactly where the kernel stores fp16 - x', the normalised tile, mid.  Those three
roundings belong to the operation as the project defines it (the two-launch path it replaces stores the same three tensors); everything between them is
float64 with the exact erfc GELU.  mag = |c0| (|mid| |W2|^T + |b2|) + |c1 r1| + |c2 R2| is the sum of the absolute values of the terms of one output.

The bound, elementwise:  |got - ref| <= F * (2^-10 |ref| + 2^-13 (mag + 1)),  F = 1 for the fp32 emulation below, F = 2 on the GPU.
  2^-10 |ref|   : the fp16 rounding of the output: half an ulp is at most 2^-11 |ref|, and a value that arrives on the other side of a rounding boundary
                  lands one whole ulp away.
  2^-13 (mag+1) : an fp32 evaluation does not reproduce the reference's fp16 `mid` bit for bit.  Where the fp32 value of hv * GELU(hg) and the float64
                  one lie on different sides of an fp16 rounding boundary, mid_j differs by one ulp, at most 2^-10 |mid_j|, and that enters output n
                  as c0 W2[n, j] ulp(mid_j).  Two mechanisms flip roundings (figures: the emulation below on the cases of this file):
                  (a) the fp32 value itself is off by about 2^-22 |mid_j| from the products and sums and, through Phi(hg), by the 1.5e-7 absolute error
                      of the Abramowitz-Stegun 7.1.26 polynomial and the fp32 cancellation in 0.5 - y e - a few 2^-23 / Phi(hg) relative, which for a
                      negative gate is not small against the ulp spacing of 2^-11 .. 2^-10 relative.  0.17 - 0.6 % of the elements flip, 1.5 % with
                      the gates pushed into the tails (ROW_CASES).
                  (b) with the pre-norm, the fp32 statistics flip the fp16 rounding of 0.015 - 0.11 % of the normalised values, which is one or more
                      in 1 - 12 % of the rows.  One flipped xn_k moves every hv_j and hg_j of its row by 2^-10 |xn_k W1[j, k]|: with |W1| about
                      1 / sqrt(C) that is 2^-13 .. 2^-14 relative to h, an eighth to a quarter of mid's ulp spacing - so 4 - 20 % of that row's mid
                      flips, all because of the same xn_k.
                  Neither set is a random subset with random signs (the polynomial's error is a smooth function of hg; the flips of (b) share one
                  cause), and at C = 64 a single term holds up to an eighth of an output's inner sum by weight.  The term therefore allows one ulp of
                  mid, all in one direction, on 1/8 of the inner sum by weight: 2^-10 * 2^-3 * |c0| |mid| |W2|^T <= 2^-13 mag.  Measured on the
                  emulation: the flips summed with their signs reach 2^-13.0 mag (summed without them, 2^-11.8 mag; every element flipped would be
                  2^-10 mag).  The fp32 accumulation of the two products (about 2^-24 sqrt(K) relative to the terms, K <= 1280: below 2^-19 mag) is
                  small against it and carried by the same term; `+ 1` keeps the bound from vanishing where every term of an output is tiny.
The emulation (ff_emulated) is held to F = 1 on every case of the table by tests/test_ff_oracle_cpu.py (worst case 0.69 of the bound; with 2^-14 in
place of 2^-13 it reaches 1.2): if it could not hold the bound, neither could a correct kernel.  F = 2 (BOUND_FACTOR_GPU, as for the norms) leaves the
device its own summation order inside the MFMA chain and in the LayerNorm, and its rcp / exp2.  With F = 1 the median element's bound is 2.2e-4 ..
2.8e-4 of max |ref| on these inputs (1.2e-3 at the largest outputs, where the rounding of the output itself dominates), against the 2e-3 of max |ref|
for every element in tests/test_ops_gpu.py.
"""
import numpy as np
import torch

BOUND_FACTOR_GPU = 2.0
REL_OUT = 2.0 ** -10          # fp16 rounding of the output
REL_MAG = 2.0 ** -13          # one fp16 ulp of mid (2^-10) on 1/8 of the inner sum by weight (2^-3)


def h16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def bound(ref, mag, factor=1.0):
    return factor * (REL_OUT * np.abs(ref) + REL_MAG * (mag + 1.0))


def worst_ratio(got, ref, mag, factor=1.0):
    """max over the elements of |got - ref| / bound, and its flat index"""
    r = np.abs(np.asarray(got, np.float64) - ref) / bound(ref, mag, factor)
    i = int(np.argmax(r))
    return float(r.flat[i]), i


def _phi64(g):
    """standard normal CDF in float64 by erfc (accurate in the lower tail)"""
    return 0.5 * torch.special.erfc(torch.from_numpy(-g / np.sqrt(2.0))).numpy()


def _vec_rows(rows, rows_per_vec):
    return rows // rows_per_vec


def ff_f64(inp, rows=None, stages=False):
    """The staged float64 reference on the rows `rows` (None: all M; guard rows of the inputs are never read) -> (ref, mag) [len(rows), C], with
    stages=True also a dict of the intermediate tensors (xs = x', xn_exact before its fp16 rounding, xn, mid_exact, mid)."""
    M, C = inp["M"], inp["C"]
    rows = np.arange(M) if rows is None else np.asarray(rows)
    I = 4 * C
    xs = np.asarray(inp["X"], np.float32)[rows]
    if inp["addvec"] is not None:
        xs = h16(xs + np.asarray(inp["addvec"], np.float32)[_vec_rows(rows, inp["rows_per_vec"])])     # one fp32 add of two fp16 values: exact before the rounding
    xs = xs.astype(np.float64)
    st = {"xs": xs}
    if inp["gamma"] is not None:
        mean = xs.mean(-1, keepdims=True)
        var = ((xs - mean) ** 2).mean(-1, keepdims=True)
        xn_exact = (xs - mean) / np.sqrt(var + inp["eps"]) * np.asarray(inp["gamma"], np.float64) + np.asarray(inp["beta"], np.float64)
        xn = h16(xn_exact).astype(np.float64)
    else:
        xn_exact = xn = xs
    W1, W2 = np.asarray(inp["W1"], np.float64), np.asarray(inp["W2"], np.float64)
    h = xn @ W1.T + np.asarray(inp["b1"], np.float64)
    hv, hg = h[:, :I], h[:, I:]
    mid_exact = hv * hg * _phi64(hg)
    mid = h16(mid_exact).astype(np.float64)
    b2 = np.zeros(C) if inp["b2"] is None else np.asarray(inp["b2"], np.float64)
    c0, c1, c2 = inp["c0"], inp["c1"], inp["c2"]
    ref = c0 * (mid @ W2.T + b2)
    mag = abs(c0) * (np.abs(mid) @ np.abs(W2).T + np.abs(b2))
    for coef, r in ((c1, inp["R1"]), (c2, inp["R2"])):
        if r is None:
            continue
        rr = xs if isinstance(r, str) else np.asarray(r, np.float64)[rows]
        ref = ref + coef * rr
        mag = mag + np.abs(coef * rr)
    if stages:
        st.update(xn_exact=xn_exact, xn=xn, mid_exact=mid_exact, mid=mid)
        return ref, mag, st
    return ref, mag


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernel
# ---------------------------------------------------------------------------------------------------------------------------------------------
def geglu32(h, g):
    """ff_geglu2 of kernels/ff_fused.hip in fp32, constant for constant: h * g * Phi(g), erfc by Abramowitz-Stegun 7.1.26 (rcp and exp2 correctly rounded
    here, about one ulp off on the device)"""
    f = np.float32
    h, g = np.asarray(h, f), np.asarray(g, f)
    ag = np.abs(g)
    u = ag * f(0.23164189) + f(1.0)
    t = f(1.0) / u
    y = t * f(0.5307027145) - f(0.7265760135)
    y = y * t + f(0.7107068705)
    y = y * t - f(0.142248368)
    y = y * t + f(0.127414796)
    y = y * t
    w = (g * g) * f(-0.72134752044)
    e = np.exp2(w)
    q = f(0.5) - y * e
    phi = f(0.5) + np.copysign(q, g)
    out = h * g * phi
    assert out.dtype == np.float32
    return out


def ff_emulated(inp, rows=None):
    """The kernel's arithmetic in fp32 on the rows `rows`: fp32 sums (numpy's order, not the MFMA chain's), two-pass fp32 LayerNorm statistics, the
    polynomial GELU, fp16 roundings of x', the normalised tile, mid and the output; the epilogue term by term as the kernel writes it."""
    f = np.float32
    M, C = inp["M"], inp["C"]
    rows = np.arange(M) if rows is None else np.asarray(rows)
    I = 4 * C
    xs = np.asarray(inp["X"], f)[rows]
    if inp["addvec"] is not None:
        xs = h16(xs + np.asarray(inp["addvec"], f)[_vec_rows(rows, inp["rows_per_vec"])])
    xn = xs
    if inp["gamma"] is not None:
        mean = (xs.sum(-1, keepdims=True, dtype=f) / f(C)).astype(f)
        d = xs - mean
        var = ((d * d).sum(-1, keepdims=True, dtype=f) / f(C)).astype(f)
        rstd = (f(1.0) / np.sqrt(var + f(inp["eps"]))).astype(f)
        xn = h16(d * rstd * np.asarray(inp["gamma"], f) + np.asarray(inp["beta"], f))
    h = xn @ np.asarray(inp["W1"], f).T + np.asarray(inp["b1"], f)
    mid = h16(geglu32(h[:, :I], h[:, I:]))
    acc = mid @ np.asarray(inp["W2"], f).T
    if inp["b2"] is not None:
        acc = acc + np.asarray(inp["b2"], f)
    out = f(inp["c0"]) * acc
    for coef, r in ((inp["c1"], inp["R1"]), (inp["c2"], inp["R2"])):
        if r is not None:
            out = out + f(coef) * (xs if isinstance(r, str) else np.asarray(r, f)[rows])
    assert out.dtype == np.float32
    return h16(out)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs and the case table
# ---------------------------------------------------------------------------------------------------------------------------------------------
FORMS = ("plain", "ln", "lnvec", "nob2", "nor1", "r2", "ln_sepr1", "rows")
C0, C1, C2, EPS = 0.7, 1.3, -0.5, 1e-5


def _case(id_, M, C, form, seed, rpv=0, rows=None, **kw):
    assert form in FORMS and C % 64 == 0 and (rpv > 0) == (form == "lnvec" or kw.get("vec", False))
    return dict(id=id_, M=M, C=C, form=form, seed=seed, rpv=rpv, rows=rows, **kw)


def ff_inputs(case, in_guard=0, guard_value=0.0):
    """The operands of a case, deterministic in case['seed'], all exact in fp16.  X, R1 and R2 get in_guard rows of guard_value behind row M - 1 and
    addvec, with in_guard > 0, one more vector of it: the first M rows (and ceil(M / rpv) vectors) do not depend on in_guard.
      plain    : no pre-norm, a residual tensor of its own            nob2 : plain without b2          nor1 : plain without a residual
      ln       : pre-norm, the stream as residual                      r2   : plain with a second residual R2, c2 = -0.5
      lnvec    : pre-norm on fp16(X + addvec[row // rpv]), stream      ln_sepr1 : pre-norm without addvec, a residual tensor of its own
      rows     : one tile of rows a LayerNorm can get wrong and gates in the GELU's tails (ROW_CASES)"""
    rng = np.random.default_rng(case["seed"])
    M, C, form, rpv = case["M"], case["C"], case["form"], case["rpv"]
    I = 4 * C
    pre = form in ("ln", "lnvec", "ln_sepr1", "rows")
    if pre:      # rows of distinct scale and mean: a wrong row, or a wrong row's statistics, fails by many ulps
        X = h16(rng.standard_normal((M, C)) * 2.0 ** rng.uniform(-2, 1, (M, 1)) + rng.uniform(-2, 2, (M, 1)))
    else:
        X = h16(rng.standard_normal((M, C)))
    W1, b1 = h16(rng.standard_normal((2 * I, C)) / np.sqrt(C)), h16(rng.standard_normal(2 * I) * 0.1)
    W2, b2 = h16(rng.standard_normal((C, I)) / np.sqrt(I)), h16(rng.standard_normal(C) * 0.1)
    gamma = h16(1 + 0.3 * rng.standard_normal(C)) if pre else None
    beta = h16(0.5 * rng.standard_normal(C)) if pre else None
    R = h16(rng.standard_normal((M, C)))
    R2 = h16(rng.standard_normal((M, C))) if form == "r2" else None
    nvec = (M + rpv - 1) // rpv if rpv else 0
    addvec = h16(rng.standard_normal((nvec, C)) * 2) if rpv else None       # two standard deviations of the stream: a wrong vector index cannot hide
    if form == "rows":
        X[0] = 0.75                                                           # constant row: zero variance
        X[1] = 0.0                                                            # all-zero row
        X[2] = h16(1000.0 + rng.standard_normal(C))                           # a large offset over unit noise
        X[3, C // 2] = 3e4                                                    # one outlier that owns the variance
        X[4] = h16(2.0 ** -14 * (1 + rng.uniform(0, 1, C)))                   # the smallest normal fp16 values
        gates = np.arange(64) * (I // 64)                                     # one gate column in every 64-column chunk at C = 320, every fourth at C = 64
        b1[I + gates] = np.tile([3.0, -3.0, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0], 8)
    inp = dict(M=M, C=C, X=X, W1=W1, b1=b1, W2=W2, b2=None if form == "nob2" else b2,
               R1=None if form == "nor1" else ("x" if form in ("ln", "lnvec", "rows") else R), R2=R2, c0=C0, c1=C1, c2=C2,
               gamma=gamma, beta=beta, eps=EPS, addvec=addvec, rows_per_vec=max(rpv, 1))
    if in_guard:
        pad = np.full((in_guard, C), guard_value, np.float32)
        for k in ("X", "R1", "R2"):
            if isinstance(inp[k], np.ndarray):
                inp[k] = np.concatenate([inp[k], pad])
        if addvec is not None:
            inp["addvec"] = np.concatenate([addvec, pad[:1]])
    return inp


WALK_M = 421            # three full 128-row tiles and 37 rows
WALK_CASES = [_case(f"walk C{C} {form}", WALK_M, C, form, 3000 + C + i, rpv=100 if form == "lnvec" else 0)
              for C in (64, 128, 192, 256, 320) for i, form in enumerate(("plain", "ln", "lnvec"))]


def _real_rows(M, two_tile_wgs, seed):
    """the tiles of the workgroups that walk two tiles at 256 workgroups, and 256 sampled rows of the rest"""
    head, tail = np.arange(two_tile_wgs * 128), np.arange(32768, M)
    rest = np.random.default_rng(seed).choice(np.arange(two_tile_wgs * 128, 32768), 256, replace=False)
    return np.unique(np.concatenate([head, tail, rest]))


# the product's launch geometry: more tiles than the 256 workgroups of the grid
REAL_CASES = [_case("real C320 M33485", 33485, 320, "lnvec", 3100, rpv=1339, rows=_real_rows(33485, 6, 1)),
              _case("real C192 M32901", 32768 + 128 + 5, 192, "lnvec", 3101, rpv=1339, rows=_real_rows(32901, 2, 2)),
              _case("real C256 M32901", 32768 + 128 + 5, 256, "lnvec", 3102, rpv=1339, rows=_real_rows(32901, 2, 3))]


def _split_rows(M, M1, seed):
    edge = np.arange(max(M1 - 64, 0), min(M1 + 64, M))
    rest = np.random.default_rng(seed).choice(M, 192, replace=False)
    return np.unique(np.concatenate([np.arange(64), edge, np.arange(M - 37, M), rest]))


# the whole-rounds row split of the engine's ln_ff (ff_fused_rows): a last round of <= 160 tiles goes through LayerNorm + two GEMMs.  m1 = the rows the
# fused kernel must report
SPLIT_CASES = [dict(REAL_CASES[0], id="split M33485", m1=32768, rows=np.arange(32768, 33485)),
               _case("split 160 tiles over", 32768 + 160 * 128, 320, "lnvec", 3110, rpv=1339, m1=32768, rows=_split_rows(32768 + 160 * 128, 32768, 4)),
               _case("split 161 tiles over", 32768 + 161 * 128, 320, "lnvec", 3111, rpv=1339, m1=32768 + 161 * 128, rows=_split_rows(32768 + 161 * 128, 32768, 5))]

EDGE_CASES = [_case(f"edge M{M} C{C} {form}{rpv or ''}", M, C, form, 3200 + M + C + rpv, rpv=rpv)
              for M in (1, 17, 128, 129, 255) for C in (64, 192, 320) for form, rpv in (("plain", 0), ("lnvec", 1), ("lnvec", 7))]

OPT_CASES = [_case(f"opt C{C} {form}", 300, C, form, 3300 + C + i) for C in (64, 320) for i, form in enumerate(("nob2", "nor1", "r2", "ln_sepr1"))]

ROW_CASES = [_case(f"rows C{C}", 128, C, "rows", 3400 + C) for C in (320, 64)]

ALL_CASES = WALK_CASES + REAL_CASES + SPLIT_CASES[1:] + EDGE_CASES + OPT_CASES + ROW_CASES
