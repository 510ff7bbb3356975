"""References for the pipeline glue kernels of kernels/misc.hip (tests/test_glue_gpu.py): each operation restated in plain numpy, in float64
where the kernel does float32 arithmetic, in explicit float32 / float16 steps where the kernel reproduces a rounding sequence bit for bit.
tests/test_glue_oracle_cpu.py pins every restatement to the project's oracle and shows that the chosen cases and bounds tell a wrong kernel from a
right one.  The `defect` arguments evaluate a restatement with one planted mistake; nothing but that CPU test passes them."""
import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
F32, F16 = np.float32, np.float16


def h16(a):
    return np.asarray(a, F32).astype(F16).astype(F32)


def r16(a):
    """One float32 result rounded to fp16, widened again: the (float)(f16)(...) of the kernels."""
    assert a.dtype == F32, a.dtype
    return a.astype(F16).astype(F32)


def ulp16(x):
    """Spacing of fp16 numbers at |x| (2^-24 below the smallest normal)."""
    a = np.abs(np.asarray(x, np.float64))
    return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -14))) - 10)


def f16_excess(got, ref64, slack=0.0):
    """The shared bound of kernels that evaluate in float32 and store fp16: |got - ref64| <= 0.5 * ulp16(ref64) + slack, slack being the float32
    evaluation error of the expression.  Returns max (|got - ref64| - slack) / ulp16(ref64); the bound holds iff that is <= 0.5."""
    got = np.asarray(got, np.float64); ref64 = np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert np.isfinite(got).all(), "non-finite output"
    return float(((np.abs(got - ref64) - slack) / ulp16(ref64)).max())


def ulps16_apart(got, ref):
    """max |got - ref| in units of ref's fp16 spacing."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), "non-finite output"
    return float((np.abs(got - ref) / ulp16(ref)).max())


# ---------------------------------------------------------------------------------------------------- CLIP / DINO pre-processing
def antialias_taps(src, dst, extra=0):
    """Kernel size and normalised taps of the Gaussian pre-blur of one axis (diffusers' _resize_with_antialiasing)."""
    sigma = max((src / dst - 1.0) / 2.0, 0.001)
    ks = int(max(2.0 * 2 * sigma, 3))
    if ks % 2 == 0:
        ks += 1
    ks += extra
    x = np.arange(ks, dtype=np.float64) - ks // 2
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    return ks, g / g.sum()


def _blur_axis(x, g, axis, border):
    r, n = len(g) // 2, x.shape[axis]
    pad = [(0, 0)] * x.ndim
    pad[axis] = (r, r)
    xp = np.pad(x, pad, mode=border)
    out = np.zeros_like(x)
    for u in range(len(g)):
        out += x.dtype.type(g[u]) * np.take(xp, np.arange(u, u + n), axis=axis)
    return out


def _cubic_w(t):
    A = t.dtype.type(-0.75)
    one, two, three, four, five, eight = (t.dtype.type(v) for v in (1, 2, 3, 4, 5, 8))

    def near(x):
        return ((A + two) * x - (A + three)) * x * x + one

    def far(x):
        return ((A * x - five * A) * x + eight * A) * x - four * A
    return [far(t + one), near(t), near(one - t), far(two - t)]


def _bicubic_axis(x, out, axis, half_pixel):
    n, dt = x.shape[axis], x.dtype.type
    o = np.arange(out).astype(x.dtype)
    if half_pixel:
        src = (o + dt(0.5)) * dt(n / out) - dt(0.5)
    else:
        src = (dt(n - 1) / dt(out - 1)) * o if out > 1 else np.zeros(out, x.dtype)
    i0 = np.floor(src)
    w = _cubic_w(src - i0)
    shape = [1] * x.ndim
    shape[axis] = out
    res = None
    for a in range(4):
        term = w[a].reshape(shape) * np.take(x, np.clip(i0.astype(np.int64) - 1 + a, 0, n - 1), axis=axis)
        res = term if res is None else res + term
    return res


def resize_antialias(video, S, dtype=np.float64, defect=None):
    """video [T,H,W,3] -> [T,S,S,3]: separable Gaussian pre-blur with reflect borders, then bicubic (A = -0.75, aligned corners, indices clamped)."""
    x = np.asarray(video, dtype)
    _, H, W, _ = x.shape
    extra = 2 if defect == "taps" else 0
    border = "edge" if defect == "clamp" else "reflect"
    _, gy = antialias_taps(H, S, extra)
    _, gx = antialias_taps(W, S, extra)
    x = _blur_axis(x, gx.astype(dtype), 2, border)
    x = _blur_axis(x, gy.astype(dtype), 1, border)
    x = _bicubic_axis(x, S, 1, defect == "half_pixel")
    return _bicubic_axis(x, S, 2, defect == "half_pixel")


def patch_matrix(pixels, P, Kpad, fill, defect=None):
    """pixels [T,S,S,3] -> [T*(S/P)^2, Kpad], row (t, patch row, patch column), column c*P*P + py*P + px; the rest of a row keeps `fill`."""
    T, S, _, _ = pixels.shape
    npp = S // P
    v = pixels.reshape(T, npp, P, npp, P, 3)                        # t, pr, py, pc, px, c
    v = v.transpose(0, 1, 3, 5, 4, 2) if defect == "transpose" else v.transpose(0, 1, 3, 5, 2, 4)
    out = np.full((T * npp * npp, Kpad), fill, pixels.dtype)
    out[:, :3 * P * P] = v.reshape(T * npp * npp, 3 * P * P)
    return out


def clip_patchify(video, S, P, Kpad, imagenet=False, fill=0.0, dtype=np.float64, defect=None):
    """What k_clip_patchify stores, before the rounding to fp16."""
    if defect == "norm_swap":
        imagenet = not imagenet
    mean, std = (IMAGENET_MEAN, IMAGENET_STD) if imagenet else (CLIP_MEAN, CLIP_STD)
    r = resize_antialias(video, S, dtype, defect)
    one, half = dtype(1.0), dtype(0.5)
    # the constants are float32 numbers in the oracle (torch.tensor(CLIP_MEAN)) and in the kernel: the exact operation divides by float32(std)
    v = ((r + one) * half - np.asarray(mean, F32).astype(dtype)) / np.asarray(std, F32).astype(dtype)
    return patch_matrix(v, P, Kpad, fill, defect)


def clip_slack(floor, S, P, Kpad, imagenet=False):
    """The slack of the shared bound per patch-matrix column, 2 * floor / std_c (0 in the columns the kernel leaves alone)."""
    std = IMAGENET_STD if imagenet else CLIP_STD
    s = np.zeros(Kpad)
    for c in range(3):
        s[c * P * P:(c + 1) * P * P] = 2.0 * floor / std[c]
    return s[None, :]


def clip_case_input(rng, T, H, W):
    """fp16-representable noise in (-1, 1) plus a ramp over rows, columns and frames: the borders and the coordinate map both matter."""
    yy, xx, tt = np.arange(H)[None, :, None, None] / H, np.arange(W)[None, None, :, None] / W, np.arange(T)[:, None, None, None]
    ramp = 0.4 * yy - 0.3 * xx + 0.1 * tt + 0.05 * np.arange(3)[None, None, None, :]
    return h16(h16(rng.uniform(-1, 1, (T, H, W, 3))) + ramp)


def bound_ratio(got, ref64, slack=0.0):
    """max |got - ref64| / (0.5 * ulp16(ref64) + slack): how many times the shared bound an evaluation misses it by (<= 1: it holds)."""
    got = np.asarray(got, np.float64); ref64 = np.asarray(ref64, np.float64)
    return float((np.abs(got - ref64) / (0.5 * ulp16(ref64) + slack)).max())


# (id, T, H, W, S, P, Kpad, ImageNet constants, (ky, kx)): tests/test_glue_gpu.py runs them all, tests/test_glue_oracle_cpu.py plants its defects on the small ones
CLIP_CASES = [
    ("scale1", 1, 28, 28, 28, 14, 592, False, (3, 3)),            # sigma clamps to 0.001: taps (0, 1, 0), the output is the normalised input
    ("up_x3", 1, 20, 45, 28, 14, 592, False, (3, 3)),             # rows up-scaled, columns blurred
    ("5x5", 1, 90, 100, 28, 14, 592, False, (5, 5)),
    ("7x3", 1, 120, 30, 28, 14, 592, False, (7, 3)),
    ("3x9", 1, 29, 160, 28, 14, 592, False, (3, 9)),
    ("9x3", 1, 167, 57, 28, 14, 592, False, (9, 3)),              # factor 5.96, the last size below the refusal
    ("imagenet", 3, 64, 100, 42, 14, 640, True, (3, 3)),          # three patches per side, the frame stride, surplus columns
    ("576x1024", 1, 576, 1024, 224, 14, 592, False, (3, 7)),
    ("384x512", 1, 384, 512, 224, 14, 592, False, (3, 3)),
    ("lap2", 21, 64, 128, 224, 14, 592, False, (3, 3)),           # 1,053,696 output pixels: a second lap of the 1,048,576-thread grid
]


def time_conv_case(rng, T, HW=300, Cs=8):
    """Inputs of k_time_conv_out with the accumulator inside (-4, 4) and both clamps reached: output channel 0 has weights in [0.35, 0.4] and no
    bias, pixel 1 is +1 and pixel 2 is -1 in every frame (|acc| >= 1.05 there, <= 3.6 anywhere); channels 3.. hold 1e4."""
    x = np.full((T, HW, Cs), 1e4, F32)
    x[:, :, :3] = h16(rng.uniform(-1, 1, (T, HW, 3)))
    x[:, 1, :3], x[:, 2, :3] = 1.0, -1.0
    w = h16(rng.uniform(-0.4, 0.4, (3, 3, 3)))
    w[0] = h16(rng.uniform(0.35, 0.4, (3, 3)))
    b = h16(rng.uniform(-0.3, 0.3, 3))
    b[0] = 0.0
    return x, w, b


# ---------------------------------------------------------------------------------------------------- input preparation
def prep_video(frames, noise, aug):
    """k_prep_video: frames [T,H,W,3] in [0,1], noise [T,3,H,W] -> (clip_src [T*H*W,3], vae_in [T*H*W,8]); every step one float32 operation
    rounded to fp16 (x.half(); x * 2; - 1; aug * noise.half(); the sum), aug a float32 scalar."""
    f = np.asarray(frames, F32); T, H, W, _ = f.shape
    x = r16(f)
    v = r16(r16(x * F32(2.0)) - F32(1.0))
    nz = r16(np.asarray(noise, F32)).transpose(0, 2, 3, 1)          # planar -> channels-last
    an = r16(F32(aug) * nz)
    vin = np.zeros((T * H * W, 8), F32)
    vin[:, :3] = r16(v + an).reshape(-1, 3)
    return v.reshape(-1, 3), vin


# ---------------------------------------------------------------------------------------------------- sampler
def init_latents(noise_tchw, sigma0):
    """fp16(fp16(noise) * sigma0), [T,4,h,w] -> channels-last [T*h*w, 4]."""
    nz = np.asarray(noise_tchw, F32); T, ch, h, w = nz.shape
    return r16(r16(nz) * F32(sigma0)).transpose(0, 2, 3, 1).reshape(T * h * w, ch)


def unet_input64(lat, cond, den, guided=False):
    """(lat / den | cond) per pixel in float64 (den the float32 divisor the launch is given); guided: the second video (lat / den | 0) below."""
    lat = np.asarray(lat, np.float64); cond = np.asarray(cond, np.float64)
    scaled = lat / np.float64(F32(den))
    a = np.concatenate([scaled, cond], 1)
    return np.concatenate([a, np.concatenate([scaled, np.zeros_like(cond)], 1)], 0) if guided else a


def guided_v(vc, vu, g):
    """noise_pred = v_u + g * (v_c - v_u) on fp16 tensors: the difference, the product and the sum each rounded to fp16 (g in float32)."""
    vc, vu = np.asarray(vc, F32), np.asarray(vu, F32)
    return r16(vu + r16(F32(g) * r16(vc - vu)))


# ---------------------------------------------------------------------------------------------------- latent sliding windows
def renoise64(prev, cur, coef):
    """Overlap frames of a later window: previous result + (sigma_0 / init_noise_sigma) * the window's noise; coef the float32 factor of the launch."""
    return np.asarray(prev, np.float64) + np.float64(F32(coef)) * np.asarray(cur, np.float64)


def crossfade64(cur, prev, defect=None):
    """all[f] = cur[f] * w_f + all[f] * (1 - w_f), w = linspace(0, 1, overlap) (0 alone at overlap = 1); cur, prev [overlap, frame_elems]."""
    cur, prev = np.asarray(cur, np.float64), np.asarray(prev, np.float64)
    overlap = cur.shape[0]
    f = np.arange(overlap, dtype=np.float64)
    if defect == "weights":
        w = f / overlap
    else:
        w = f / (overlap - 1) if overlap > 1 else np.zeros(1)
    w = w[:, None]
    return cur * w + prev * (1.0 - w)


# ---------------------------------------------------------------------------------------------------- decoder tail, post-processing
def time_conv_acc64(x, w, b, defect=None):
    """The accumulator of k_time_conv_out before its rounding to fp16: Conv3d(3, 3, (3,1,1)) over frames, zero padded in time, on channels 0..2 of
    x [T,HW,Cs]; w [out, in, tap], b [3] -> [T*HW, 3]."""
    x = np.asarray(x, np.float64)[:, :, :3]; w = np.asarray(w, np.float64); b = np.asarray(b, np.float64)
    T, HW, _ = x.shape
    acc = np.tile(b, (T, HW, 1))
    for kt in range(3):
        wk = w[:, :, 2 - kt] if defect == "reversed" else w[:, :, kt]
        for t in range(T):
            tt = t + kt - 1
            if 0 <= tt < T:
                acc[t] += x[tt] @ wk.T
    return acc.reshape(T * HW, 3)


def time_conv_frames64(acc):
    """(x / 2 + 0.5).clamp(0, 1) of the accumulator."""
    return np.clip(np.asarray(acc, np.float64) * 0.5 + 0.5, 0.0, 1.0)


def depth_post32(frames):
    """k_depth_minmax / k_depth_apply / k_disparity_from_frames in float32, the same expressions in the same order: frames [n,3] ->
    (depth, disparity, (min, max))."""
    f = np.asarray(frames, F32)
    d = ((f[:, 0] + f[:, 1]) + f[:, 2]) / F32(3.0)
    lo, hi = d.min(), d.max()
    x = (d - lo) / (hi - lo)
    return F32(1.0) / (x + F32(0.1)), x, np.array([lo, hi], F32)


# ---------------------------------------------------------------------------------------------------- StableNormal glue
def add_grid_nearest(x, grid):
    """x [B,h,w,C] + grid [B,g,g,C] gathered at (y*g // h, x*g // w), rounded to fp16 -> [B*h*w, C]."""
    x, grid = np.asarray(x, F32), np.asarray(grid, F32)
    B, h, w, C = x.shape; g = grid.shape[1]
    iy, ix = (np.arange(h) * g) // h, (np.arange(w) * g) // w
    return r16(x + grid[:, iy][:, :, ix]).reshape(B * h * w, C)


def sn_normals64(dec):
    """Columns 0..2 of dec clipped to [-1,1] and divided by max(norm, 1e-6)."""
    v = np.clip(np.asarray(dec, np.float64)[:, :3], -1.0, 1.0)
    return v / np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), 1e-6)


def clip_assemble(patches, cls, pos, T):
    """tokens [T*(np+1), d] = fp16(cat[cls, patches of frame t] + pos)."""
    p, c, q = np.asarray(patches, F32), np.asarray(cls, F32), np.asarray(pos, F32)
    d = p.shape[1]; npp = p.shape[0] // T
    base = np.concatenate([np.broadcast_to(c, (T, 1, d)), p.reshape(T, npp, d)], 1)
    return r16(base + q[None]).reshape(T * (npp + 1), d)
