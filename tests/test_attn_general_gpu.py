"""The two attention paths for every head dim but 64, and the batched GEMMs under the second, op by op through the C ABI:

  * flash_attn_dh_kernel<DH> (kernels/attn.hip; DH in {32, 48, 80, 96, 112, 128}) - the attention of the CLIP ViT-H/14 tower;
  * unfused_attention (engine.hip): Q K^T batched GEMM with float32 output, softmax_rows_kernel, transpose_kernel, P V batched GEMM - the VAE
    decoder's mid-block attention (one head of 512) and the tower's fall-back;
  * one batched GEMM (ug_op_gemm_batched) in the two forms that path launches, under the planner's tile and under every forced tile config.

Reference: tests/attn_general_oracle.py, plain float64 softmax attention on the fp16-rounded inputs, and an int64 matrix product.  Tolerances:
test_ops_gpu.py's bound for fp16-stored outputs after fp32 accumulation, max|err| / max|ref| < 2e-3, taken per (batch, head) block where the blocks
have magnitudes of their own; 1e-3 of max|V| for the key selector; "bit-identical" and "exact" are np.array_equal."""
import functools

import numpy as np
import pytest

import attn_general_oracle as go
from util import assert_close, where_differ

pytestmark = pytest.mark.gpu
TOL = 2e-3
FUSED_D = [32, 48, 80, 96, 112, 128]
# every 32-key block, 64-key tile, 32-row wave and 128-row workgroup boundary from both sides, one key, one ragged block, the tower's 257
FUSED_S = [1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 257]
BH = [(1, 1), (2, 3), (3, 2)]
CFGS = [0, 1, 3, 4, 8, 12, 14, 15, 19, 34, 35, 39, 54, 59, 60, 61, 62, 63, 64]


def tight_out(B, S, H, d):
    return np.zeros((B * S, H * d), np.float32)


def run_fused(engine, qkv, B, S, H, d):
    return engine.op_flash_attn_dh_ex(qkv, tight_out(B, S, H, d), B, S, H, d)


def run_generic(engine, qkv, B, S, H, d):
    return engine.op_attention_generic_ex(qkv, tight_out(B, S, H, d), B, S, H, d)[0]


def assert_blocks_close(got, ref, B, S, H, d, what):
    """The bound on every (batch, head) block against that block's own maximum."""
    for b in range(B):
        for h in range(H):
            assert_close(go.head_block(got, b, h, S, d), go.head_block(ref, b, h, S, d), TOL, f"{what} B={B} H={H} d={d} S={S} block ({b},{h})")


@functools.lru_cache(maxsize=None)
def gauss_case(B, S, H, d):
    """Inputs and float64 reference of one case, made once (read-only)."""
    qkv = go.scaled_qkv(np.random.default_rng(1000 * S + 10 * d + H + B), B, S, H, d)
    ref = go.attn_ref(qkv, B, S, H, d)
    qkv.setflags(write=False); ref.setflags(write=False)
    return qkv, ref


# ------------------------------------------------------------------ the fused kernel
@pytest.mark.parametrize("d", FUSED_D)
def test_fused_against_float64(engine, d):
    """Every S of FUSED_S meets this d once; (B, H) cycles through BH with an offset per d, so each pair appears four times per d."""
    for i, S in enumerate(FUSED_S):
        B, H = BH[(i + FUSED_D.index(d)) % 3]
        qkv, ref = gauss_case(B, S, H, d)
        assert_blocks_close(run_fused(engine, qkv, B, S, H, d), ref, B, S, H, d, "fused attention")


@pytest.mark.parametrize("d", FUSED_D)
def test_fused_key_selector(engine, d):
    """One-hot keys and queries, S = d: output row i of batch b, head h must BE row pi[b, h, i] of that head's V (the float64 reference leaves
    < 1e-6, shown on the CPU).  d = 80 crosses a 64-key tile, d = 128 fills a workgroup."""
    qkv, pi = go.selector_inputs(d, 2, d)
    assert_close(run_fused(engine, qkv, 1, d, 2, d), go.selector_expected(qkv, pi, d), 1e-3, f"fused attention d={d} key selector")


def test_fused_key_selector_two_workgroups(engine):
    qkv, pi = go.selector_inputs(128, 1, 128, B=2)
    assert_close(run_fused(engine, qkv, 2, 128, 1, 128), go.selector_expected(qkv, pi, 128), 1e-3, "fused attention d=128 key selector, two batches")


@pytest.mark.parametrize("d", [48, 80, 128])
def test_fused_rising_maxima(engine, d):
    """The running maximum of every query rises by >= 8 nats at blocks 1, 2 and 4 and stays at block 3 (shown on the CPU): alpha, m_run, l_run."""
    qkv = go.rising_inputs(d)
    got = run_fused(engine, qkv, 1, go.RISE_S, go.RISE_H, d)
    assert_close(got, go.attn_ref(qkv, 1, go.RISE_S, go.RISE_H, d), TOL, f"fused attention d={d} rising maxima")


@functools.lru_cache(maxsize=None)
def poisoned_case(B, S, H, d):
    qkv, ref = gauss_case(B, S, H, d)
    buf, out = go.poisoned_buffers(qkv, B, S, H, d)
    buf.setflags(write=False); out.setflags(write=False)
    return qkv, ref, buf, out


def check_poisoned(got, ref, out, B, S, H, d, what):
    assert got.shape == out.shape
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    assert_blocks_close(got[:B * S, :H * d], ref, B, S, H, d, what)
    assert (go.outside(got, B * S, H * d) == go.POISON_SENTINEL).all(), f"{what}: sentinel overwritten"


@pytest.mark.parametrize("d", FUSED_D)
def test_fused_poisoned_surroundings_and_tight_buffers(engine, d):
    """NaN in the surplus columns of qkv and in 70 rows after its last row, 7.0 around the output: finite, within the bound, the sentinels bit for bit.
    The same inputs through tight buffers (ld = 3*H*d, no guard) give the corner's bits: strides and bases alone differ."""
    for i, S in enumerate((33, 64, 130)):
        B, H = BH[(i + FUSED_D.index(d)) % 3]
        qkv, ref, buf, out = poisoned_case(B, S, H, d)
        got = engine.op_flash_attn_dh_ex(buf, out, B, S, H, d, guard=go.POISON_GUARD)
        check_poisoned(got, ref, out, B, S, H, d, "fused attention, poisoned surroundings")
        assert np.array_equal(run_fused(engine, qkv, B, S, H, d), got[:B * S, :H * d])


def test_fused_bad_calls_are_errors_and_the_context_stays_usable(engine):
    B, S, H, d = 2, 33, 3, 80
    qkv, ref = gauss_case(B, S, H, d)
    C = H * d
    z = lambda rows, cols: np.zeros((rows, cols), np.float32)
    with pytest.raises(RuntimeError):      # head dim 40: no instantiation
        engine.op_flash_attn_dh_ex(z(B * S, 3 * H * 40), z(B * S, H * 40), B, S, H, 40)
    with pytest.raises(RuntimeError):      # ld not a multiple of 8
        engine.op_flash_attn_dh_ex(z(B * S, 3 * C + 4), z(B * S, C), B, S, H, d)
    with pytest.raises(RuntimeError):      # ld < 3 * H * d
        engine.op_flash_attn_dh_ex(z(B * S, 3 * C - 8), z(B * S, C), B, S, H, d)
    with pytest.raises(RuntimeError):      # S = 0
        engine.op_flash_attn_dh_ex(z(0, 3 * C), z(0, C), B, 0, H, d)
    for bad in (lambda: engine.op_attention_generic_ex(z(B * S, 3 * C + 4), z(B * S, C), B, S, H, d),
                lambda: engine.op_attention_generic_ex(z(B * S, 3 * C - 8), z(B * S, C), B, S, H, d),
                lambda: engine.op_attention_generic_ex(z(0, 3 * C), z(0, C), B, 0, H, d)):
        with pytest.raises(RuntimeError):
            bad()
    assert_blocks_close(run_fused(engine, qkv, B, S, H, d), ref, B, S, H, d, "fused attention after rejected calls")
    assert_blocks_close(run_generic(engine, qkv, B, S, H, d), ref, B, S, H, d, "four-launch attention after rejected calls")


# ------------------------------------------------------------------ the four-launch path
GENERIC_BHD = [(2, 1, 512), (2, 2, 80), (1, 3, 48), (3, 1, 64)]
# pad8 edges (7, 8, 9; 63, 64, 65), one key, partial 32 x 32 transpose tiles, K = Spad a multiple of 64 (64, 257 -> 264 is not, 63 -> 64 is) and not
GENERIC_S = [1, 7, 8, 9, 48, 63, 64, 65, 130, 257]


@pytest.mark.parametrize("B,H,d", GENERIC_BHD)
def test_four_launch_against_float64_and_the_fused_kernel(engine, B, H, d):
    for S in GENERIC_S:
        qkv, ref = gauss_case(B, S, H, d)
        got = run_generic(engine, qkv, B, S, H, d)
        assert_blocks_close(got, ref, B, S, H, d, "four-launch attention")
        if d in FUSED_D:
            assert_blocks_close(run_fused(engine, qkv, B, S, H, d), got, B, S, H, d, "fused vs four-launch attention")


@pytest.mark.parametrize("B,H,d", GENERIC_BHD)
def test_four_launch_key_selector(engine, B, H, d):
    S = min(d, 257)
    qkv, pi = go.selector_inputs(d, H, S, B)
    assert_close(run_generic(engine, qkv, B, S, H, d), go.selector_expected(qkv, pi, d), 1e-3, f"four-launch attention B={B} H={H} d={d} key selector")


@pytest.mark.parametrize("B,H,d", GENERIC_BHD)
def test_four_launch_poisoned_surroundings_and_tight_buffers(engine, B, H, d):
    """As for the fused kernel.  The surplus columns right of the last head keep their sentinel: the P V tile's masked N tail stays inside its head."""
    for S in (9, 64, 130):
        qkv, ref, buf, out = poisoned_case(B, S, H, d)
        got, _ = engine.op_attention_generic_ex(buf, out, B, S, H, d, guard=go.POISON_GUARD)
        check_poisoned(got, ref, out, B, S, H, d, "four-launch attention, poisoned surroundings")
        assert np.array_equal(run_generic(engine, qkv, B, S, H, d), got[:B * S, :H * d])


def test_four_launch_pad_columns_do_not_depend_on_stale_workspace(engine):
    """The P V product runs over K = Spad: the columns [S, Spad) of P and of V^T must be zeros that the softmax and the transpose WRITE, not whatever the
    workspace held.  Every entry's buffers are stacked from the same workspace base, so a small batched GEMM whose A buffer carries a long NaN tail
    leaves NaN where the next call's scores, P and V^T will lie."""
    B, H, d = 2, 2, 80
    nan_tail = np.full(4 << 20, np.nan, np.float32)                 # 8 MiB of fp16 NaN on the device: more than the attention calls below stack up
    nan_tail[:64] = 1.0
    eye = np.eye(8, dtype=np.float32).ravel()
    for S in (9, 65, 257):
        qkv, ref = gauss_case(B, S, H, d)
        got, _ = engine.op_gemm_batched(nan_tail, 8, (0, 0), eye, 8, (0, 0), 8, 8, 8, 1, 1, np.zeros(64, np.float32), 8, (0, 0))
        assert np.array_equal(got, np.ones(64, np.float32))
        assert_blocks_close(run_generic(engine, qkv, B, S, H, d), ref, B, S, H, d, "four-launch attention over a NaN-filled workspace")


def _force(engine, cfg):
    engine.tune_force(cfg, 1 if cfg >= 0 else -1)


@pytest.mark.parametrize("B,H,d,S", [(2, 1, 512, 65), (2, 2, 80, 257), (1, 3, 64, 65)])
def test_four_launch_bit_identical_across_tile_configs(engine, B, H, d, S):
    """Every tile config accumulates K through the same MFMA chain in the same order: both GEMMs forced onto each config of CFGS give config 15's bits.
    The third case has several heads AND K % 64 == 0, so the buffer-addressed loader and producer / consumer kernels run with an inner batch index."""
    qkv, ref = gauss_case(B, S, H, d)
    try:
        _force(engine, 15)
        want, plan = engine.op_attention_generic_ex(qkv, tight_out(B, S, H, d), B, S, H, d)
        assert plan == ((15, 1), (15, 1)), plan
        assert_blocks_close(want, ref, B, S, H, d, "four-launch attention on config 15")
        for cfg in CFGS:
            _force(engine, cfg)
            for rep in range(2):
                got, plan = engine.op_attention_generic_ex(qkv, tight_out(B, S, H, d), B, S, H, d)
                assert plan == ((cfg, 1), (cfg, 1)), plan
                assert np.array_equal(got, want), f"cfg {cfg} run {rep}: {where_differ(got, want)}"
    finally:
        _force(engine, -1)


# ------------------------------------------------------------------ one batched GEMM, exact on integer data
SENT = 7.0
BATCHES = [(2, 1), (6, 1), (6, 3)]           # (batch, nb_inner): batch in {2, 6}, nb_inner in {1, 3}; nb_inner divides batch
QK_SHAPES = [(65, 512), (64, 64), (257, 80), (130, 48)]                  # (M = N = S, K = d)
PV_SHAPES = [(64, 512, 64), (257, 80, 264), (65, 48, 72)]                # (M = S, N = d, K = Spad)


@functools.lru_cache(maxsize=None)
def qk_case(S, d, batch, nb_inner):
    """The Q K^T form: A and W are the Q and K column blocks of head bi, frame bo of ONE qkv buffer (inner stride d, outer stride S * ld); the V columns
    and eight surplus columns hold NaN; float32 output [batch, S, Spad] full of sentinels plus a guard row - the columns [S, Spad) keep theirs."""
    H, B = nb_inner, batch // nb_inner
    C, Sp = H * d, go.pad8(S)
    ld = 3 * C + 8
    rng = np.random.default_rng(S + d + 7 * batch + nb_inner)
    qkv = np.full((B * S, ld), np.nan, np.float32)
    qkv[:, :2 * C] = go.ternary(rng, B * S, 2 * C)
    out = np.full(batch * S * Sp + Sp, SENT, np.float32)
    args = dict(lda=ld, sA=(S * ld, d), ldw=ld, sW=(S * ld, d), M=S, N=S, K=d, batch=batch, nb_inner=nb_inner, ldo=Sp, sO=(H * S * Sp, S * Sp))
    flat = qkv.ravel()
    ref = go.gemm_batched_ref(flat, args["lda"], args["sA"], flat[C:], args["ldw"], args["sW"], S, S, d, batch, nb_inner, out, Sp, args["sO"], dtype=np.int64)
    for a in (flat, out, ref):
        a.setflags(write=False)
    return flat, flat[C:], out, args, ref


@functools.lru_cache(maxsize=None)
def pv_case(S, d, Sp, batch, nb_inner):
    """The P V form: P [batch, S, Spad] and V^T [batch, d, Spad], fp16 output scattered into the head columns of [B*S + guard, ldo] (inner stride d),
    ldo = H * d + 4 with sentinels to the right of the last head and in a guard row."""
    H, B = nb_inner, batch // nb_inner
    ldo = H * d + 4
    rng = np.random.default_rng(S + d + 11 * batch + nb_inner)
    P, Vt = go.ternary(rng, batch * S * Sp), go.ternary(rng, batch * d * Sp)
    out = np.full((B * S + 1) * ldo, SENT, np.float32)
    args = dict(lda=Sp, sA=(H * S * Sp, S * Sp), ldw=Sp, sW=(H * d * Sp, d * Sp), M=S, N=d, K=Sp, batch=batch, nb_inner=nb_inner, ldo=ldo, sO=(S * ldo, d))
    ref = go.gemm_batched_ref(P, Sp, args["sA"], Vt, Sp, args["sW"], S, d, Sp, batch, nb_inner, out, ldo, args["sO"], dtype=np.int64)
    for a in (P, Vt, out, ref):
        a.setflags(write=False)
    return P, Vt, out, args, ref


def gemm_cases():
    for (batch, nb_inner) in BATCHES:
        for (S, d) in QK_SHAPES:
            yield f"QK^T S={S} d={d} batch={batch} nb_inner={nb_inner}", True, qk_case(S, d, batch, nb_inner)
        for (S, d, Sp) in PV_SHAPES:
            assert Sp == go.pad8(S)
            yield f"PV S={S} d={d} batch={batch} nb_inner={nb_inner}", False, pv_case(S, d, Sp, batch, nb_inner)


def run_gemm_case(engine, f32, case):
    A, W, out, args, _ = case
    a = dict(args)
    return engine.op_gemm_batched(A, a.pop("lda"), a.pop("sA"), W, a.pop("ldw"), a.pop("sW"), a.pop("M"), a.pop("N"), a.pop("K"), a.pop("batch"),
                                  a.pop("nb_inner"), out, a.pop("ldo"), a.pop("sO"), c0=1.0, out_f32=f32)


@pytest.mark.parametrize("cfg", [-1] + CFGS)
def test_batched_gemm_exact_on_integer_data(engine, cfg):
    """Entries in {-1, 0, 1}, c0 = 1: every output is an integer of magnitude <= K <= 512, exact in float32 and in fp16, so the kernel must return the int64
    product and every sentinel - under the planner's tile (cfg -1) and under each forced tile config with the split factor forced to 1, twice each.
    A wrong per-batch base gives integers of the right size from the wrong head or frame; the data differ from batch to batch."""
    try:
        _force(engine, cfg)
        for rep in range(2):
            for name, f32, case in gemm_cases():
                got, plan = run_gemm_case(engine, f32, case)
                assert plan[1] == 1 and (cfg < 0 or plan[0] == cfg), (name, plan)
                ref = case[4]
                assert np.array_equal(got.astype(np.int64), ref) and np.array_equal(got, ref.astype(np.float32)), \
                    f"cfg {cfg} run {rep} {name}: {where_differ(got, ref.astype(np.float32))}"
    finally:
        _force(engine, -1)


def test_forced_split_k_with_a_batch_runs_unsplit(engine):
    """gemm_plan's plain_epi demands batch == 1: a forced split factor must not reach a batched launch (run_gemm sizes `partial` for one batch only)."""
    M, N, K, batch = 64, 128, 512, 2
    rng = np.random.default_rng(5)
    A, W = go.ternary(rng, batch * M * K), go.ternary(rng, batch * N * K)
    out = np.full(batch * M * N + N, SENT, np.float32)
    ref = go.gemm_batched_ref(A, K, (M * K, 0), W, K, (N * K, 0), M, N, K, batch, 1, out, N, (M * N, 0), dtype=np.int64)
    try:
        engine.tune_force(3, 4)
        for f32 in (False, True):
            got, plan = engine.op_gemm_batched(A, K, (M * K, 0), W, K, (N * K, 0), M, N, K, batch, 1, out, N, (M * N, 0), out_f32=f32)
            assert plan == (3, 1), plan
            assert np.array_equal(got.astype(np.int64), ref), where_differ(got, ref.astype(np.float32))
        # the same problem as ONE batch does split: the override is live
        got, plan = engine.op_gemm_batched(A, K, (0, 0), W, K, (0, 0), M, N, K, 1, 1, out, N, (0, 0), out_f32=False)
        assert plan == (3, 4), plan
        ref1 = go.gemm_batched_ref(A, K, (0, 0), W, K, (0, 0), M, N, K, 1, 1, out, N, (0, 0), dtype=np.int64)
        assert np.array_equal(got.astype(np.int64), ref1), where_differ(got, ref1.astype(np.float32))
    finally:
        engine.tune_force(-1, -1)


def test_batched_gemm_rejects_operands_that_leave_their_buffers(engine):
    A, W, out, args, ref = qk_case(64, 64, 2, 1)
    a = dict(args)
    slack = a["ldw"] - 2 * 64      # W is the buffer from its K columns on: what follows the last K row (the V and surplus columns)
    with pytest.raises(RuntimeError):      # the last batch's last row would end one element past the buffer
        engine.op_gemm_batched(A, a["lda"], a["sA"], W[:W.size - slack - 1], a["ldw"], a["sW"], 64, 64, 64, 2, 1, out, a["ldo"], a["sO"])
    with pytest.raises(RuntimeError):      # the output's last batch would
        engine.op_gemm_batched(A, a["lda"], a["sA"], W, a["ldw"], a["sW"], 64, 64, 64, 2, 1, out[:2 * 64 * 64 - 1], a["ldo"], a["sO"])
    with pytest.raises(RuntimeError):      # nb_inner does not divide batch
        engine.op_gemm_batched(A, a["lda"], a["sA"], W, a["ldw"], a["sW"], 64, 64, 64, 2, 3, out, a["ldo"], a["sO"])
    got, _ = run_gemm_case(engine, True, (A, W, out, args, ref))
    assert np.array_equal(got.astype(np.int64), ref)
