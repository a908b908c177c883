"""Independent numpy restatement of the reference's runtime image comparison, written from the reference text:
shaders/image_compare_metric.comp.slang (MSE, FLIP approx, FLIP reference with the brute-force (2r+1)^2 Gaussian exactly as the
shader loops), shaders/image_compare_composite.comp.slang (all six display modes), the colour helpers of shaders/color.h.slang and
ImageCompare::collectMetricsResult (src/image_compare.cpp:869-906).  Not a port of the library's kernels: no separable passes, no
tiles, one array operation per shader statement.

Every function takes dt (np.float64 or np.float32: the arithmetic type) and, where a sum's order is the shader's to choose, order
(0 = as written, 1 = reversed) so that the tests can measure what another order of the same operations changes.
Images are [H, W, 4] arrays, row 0 first, as the library stores them.  The sampler (unpinned in the reference) is clamp-to-edge
bilinear, the rule include/mgs.h documents; loads outside an image give 0."""
import math

import numpy as np

FREQS = (0.5, 1.0, 2.0, 4.0, 8.0)
LUM = (0.2126, 0.7152, 0.0722)


def _dot3(a, b, c, k, dt, order=0):
    t = [a * dt(k[0]), b * dt(k[1]), c * dt(k[2])]
    return (t[0] + t[1]) + t[2] if order == 0 else (t[2] + t[1]) + t[0]


def luminance(img, dt, order=0):
    img = img.astype(dt)
    return _dot3(img[..., 0], img[..., 1], img[..., 2], LUM, dt, order)


def bilinear(img, u, v, dt):
    """SampleLevel(linearSampler, uv, 0), clamp to edge; u, v broadcastable arrays"""
    img = img.astype(dt)
    H, W = img.shape[:2]
    fx, fy = u * dt(W) - dt(0.5), v * dt(H) - dt(0.5)
    x0f, y0f = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0f)[..., None], (fy - y0f)[..., None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.clip(x0 + 1, 0, W - 1), np.clip(y0 + 1, 0, H - 1)
    x0, y0 = np.clip(x0, 0, W - 1), np.clip(y0, 0, H - 1)
    sx, sy = dt(1) - tx, dt(1) - ty
    return (img[y0, x0] * sx + img[y0, x1] * tx) * sy + (img[y1, x0] * sx + img[y1, x1] * tx) * ty


def _uv(W, H, dt):
    u = (np.arange(W, dtype=dt) + dt(0.5)) / dt(W)
    v = (np.arange(H, dtype=dt) + dt(0.5)) / dt(H)
    return np.broadcast_to(u[None, :], (H, W)), np.broadcast_to(v[:, None], (H, W))


def current_at_capture(cap, cur, dt):
    """the shader's curColor: Load at equal sizes, the sampler at (p + 0.5) / captureSize otherwise"""
    H, W = cap.shape[:2]
    if cur.shape[:2] == (H, W):
        return cur.astype(dt)
    u, v = _uv(W, H, dt)
    return bilinear(cur, u, v, dt)


def load_at(img, W, H, dt):
    """Load(coord) for every coord of a W x H grid; 0 outside the image"""
    out = np.zeros((H, W, 4), dt)
    h, w = min(H, img.shape[0]), min(W, img.shape[1])
    out[:h, :w] = img[:h, :w].astype(dt)
    return out


def squared_error(cap, cur, dt, order=0):
    d = cap.astype(dt)[..., :3] - current_at_capture(cap, cur, dt)[..., :3]
    sq = [d[..., 0] * d[..., 0], d[..., 1] * d[..., 1], d[..., 2] * d[..., 2]]  # dot(diff, diff)
    return (sq[0] + sq[1]) + sq[2] if order == 0 else (sq[2] + sq[1]) + sq[0]


def csf_luminance(f, dt):
    f = dt(f)
    s = dt(1) / np.sqrt(dt(1) + np.power(f / dt(4), dt(2)))
    return dt(s * np.exp(dt(-0.5) * f))


def srgb_to_linear(c, dt):
    c = c.astype(dt)
    hi = np.power((np.maximum(c, dt(0.04045)) + dt(0.055)) / dt(1.055), dt(2.4))
    return np.where(c <= dt(0.04045), c / dt(12.92), hi)


def hunt_factor(dt):
    k = dt(5.0) * dt(1.0)
    kc = np.power(k, dt(1.0) / dt(3.0))
    return dt(dt(0.2) * kc * (dt(1) - np.exp(dt(-0.42) * kc)))


def srgb_to_ycxcz(rgb, dt, order=0):
    lin = srgb_to_linear(rgb[..., :3], dt)
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    L = _dot3(r, g, b, (0.31670331, 0.70299344, -0.01969366), dt, order)
    M = _dot3(r, g, b, (0.10938715, 0.87060437, 0.01990658), dt, order)
    S = _dot3(r, g, b, (0.01840087, 0.10476914, 0.87470614), dt, order)
    F = hunt_factor(dt)
    L, M, S = L * F, M * F, S * F
    return M, L - M, M - S


def color_error(ref, cur, dt, order=0):
    p, q = srgb_to_ycxcz(ref, dt, order), srgb_to_ycxcz(cur, dt, order)
    csf_y = csf_luminance(1.0, dt)
    csf_c = dt(csf_y * dt(0.4))
    t = [np.abs(p[0] - q[0]) * csf_y, np.abs(p[1] - q[1]) * csf_c, np.abs(p[2] - q[2]) * csf_c]
    return (t[0] + t[1]) + t[2] if order == 0 else (t[2] + t[1]) + t[0]


def sobel_feature(img, dt, order=0):
    """3 x 3 Sobel magnitude of the luminance; 0 on the one-pixel border of the image's own size"""
    L = luminance(img, dt, order)
    H, W = L.shape
    out = np.zeros((H, W), dt)
    if H < 3 or W < 3:
        return out
    tl, tc, tr = L[:-2, :-2], L[:-2, 1:-1], L[:-2, 2:]
    ml, mr = L[1:-1, :-2], L[1:-1, 2:]
    bl, bc, br = L[2:, :-2], L[2:, 1:-1], L[2:, 2:]
    two = dt(2)
    gx = ((((-tl + tr) - two * ml) + two * mr) - bl) + br
    gy = ((((-tl - two * tc) - tr) + bl) + two * bc) + br
    out[1:-1, 1:-1] = np.sqrt(gx * gx + gy * gy)
    return out


def flip_approx_powered(cap, cur, dt, order=0):
    """computeFLIPApprox per capture pixel: both images are loaded at the capture's coordinate"""
    H, W = cap.shape[:2]
    ce = color_error(cap.astype(dt), load_at(cur, W, H, dt), dt, order)
    rf = sobel_feature(cap, dt, order)
    cf = np.zeros((H, W), dt)
    s = sobel_feature(cur, dt, order)
    h, w = min(H, s.shape[0]), min(W, s.shape[1])
    cf[:h, :w] = s[:h, :w]
    fe = np.abs(rf - cf) * csf_luminance(4.0, dt)
    total = ce + fe * dt(3.83)
    return np.power(np.clip(total, dt(0), dt(1)), dt(3))


def sigma_radius(ppd, f, dt=np.float32):
    """sigma and r = int(ceil(3 sigma)); the shader computes them in fp32"""
    sigma = max(dt(ppd) / (dt(f) * dt(6.28)), dt(0.5))
    return sigma, int(math.ceil(dt(3.0) * sigma))


def gauss_weights(sigma, r, dt):
    x = np.arange(-r, r + 1).astype(dt)
    return np.exp(-(x * x) / (dt(2.0) * dt(sigma) * dt(sigma)))


def blur_2d(L, sigma, r, dt, order=0):
    """applyGaussianFilter for every pixel: the brute-force double loop over dx (outer) and dy (inner), as the shader loops;
    a pixel within r of any border returns its own luminance"""
    H, W = L.shape
    out = L.copy()
    if H <= 2 * r or W <= 2 * r:
        return out
    w = gauss_weights(sigma, r, dt)
    acc = np.zeros((H - 2 * r, W - 2 * r), dt)
    wsum = dt(0)
    rng = range(-r, r + 1) if order == 0 else range(r, -r - 1, -1)
    for dx in rng:
        for dy in rng:
            wt = dt(w[dx + r] * w[dy + r])
            acc += L[r + dy:H - r + dy, r + dx:W - r + dx] * wt
            wsum = dt(wsum + wt)
    out[r:H - r, r:W - r] = acc / wsum
    return out


def blur_separable(L, sigma, r, dt):
    """the same mean as a row pass and a column pass, normalised by the square of the 1-D weight sum (what the library evaluates)"""
    H, W = L.shape
    out = L.copy()
    if H <= 2 * r or W <= 2 * r:
        return out
    w = gauss_weights(sigma, r, dt)
    wsum = dt(0)
    for d in range(-r, r + 1):
        wsum = dt(wsum + w[d + r])
    rows = np.zeros((H, W - 2 * r), dt)
    for d in range(-r, r + 1):
        rows += L[:, r + d:W - r + d] * w[d + r]
    acc = np.zeros((H - 2 * r, W - 2 * r), dt)
    for d in range(-r, r + 1):
        acc += rows[r + d:H - r + d, :] * w[d + r]
    out[r:H - r, r:W - r] = acc / dt(wsum * wsum)
    return out


def spatial_features(img, ppd, dt, order=0, blur=blur_2d):
    """computeSpatialFeatures for every pixel of img: [5, H, W]"""
    L = luminance(img, dt, order)
    feats = []
    for f in FREQS:
        sigma, r = sigma_radius(ppd, f)
        b = blur(L, dt(sigma), r, dt, order) if blur is blur_2d else blur(L, dt(sigma), r, dt)
        feats.append(np.abs(L - b) * csf_luminance(f, dt))
    return np.stack(feats)


def flip_reference_powered(cap, cur, ppd, dt, order=0, blur=blur_2d):
    H, W = cap.shape[:2]
    curc = current_at_capture(cap, cur, dt)
    ce = color_error(cap.astype(dt), curc, dt, order)
    rf = spatial_features(cap, ppd, dt, order, blur)
    cf = spatial_features(cur, ppd, dt, order, blur)
    if cur.shape[:2] != (H, W):
        h, w = cur.shape[:2]
        # int2(uv * float2(currentSize)) is a discrete choice the shader makes in fp32 (at 160 -> 320 the product is an integer in
        # exact arithmetic): it is evaluated in float32 whatever dt is, like sigma_radius
        u, v = _uv(W, H, np.float32)
        cx = np.clip((u * np.float32(w)).astype(np.int64), 0, w - 1)
        cy = np.clip((v * np.float32(h)).astype(np.int64), 0, h - 1)
        cf = cf[:, cy, cx]
    fe = np.zeros((H, W), dt)
    for i in (range(5) if order == 0 else range(4, -1, -1)):
        fe = fe + np.abs(rf[i] - cf[i])
    total = ce + fe
    return np.power(np.clip(total, dt(0), dt(1)), dt(3))


def to_fixed(v):
    """uint(v) with the library's defined saturation"""
    v = np.nan_to_num(np.asarray(v, np.float64), nan=0.0, posinf=4294967295.0, neginf=0.0)
    return np.floor(np.clip(v, 0.0, 4294967295.0)).astype(np.uint64)


def contributions(cap, cur, flip_mode, ppd, dt, order=0, blur=blur_2d):
    """per capture pixel: (squared error, MSE contribution in fixed-point units before truncation, FLIP powered error or None,
    FLIP contribution in units or None)"""
    H, W = cap.shape[:2]
    divider = dt(np.float32(W * H * 3))
    se = squared_error(cap, cur, dt, order)
    mc = (se / divider) * dt(1e9)
    if flip_mode == 0:
        return se, mc, None, None
    p = flip_approx_powered(cap, cur, dt, order) if flip_mode == 1 else flip_reference_powered(cap, cur, ppd, dt, order, blur)
    fc = (p / (divider / dt(3.0))) * dt(1e9)
    return se, mc, p, fc


def collect(mse_fixed, flip_fixed):
    """ImageCompare::collectMetricsResult: (mse, psnr, flip) as float32 from the two uint32 sums"""
    mse = np.float32(np.float32(np.uint32(mse_fixed)) / np.float32(1e9))
    if mse < np.float32(1e-10):
        psnr = np.float32(99.99)
    else:
        psnr = min(np.float32(10.0) * np.log10(np.float32(1.0) / mse).astype(np.float32), np.float32(99.99))
    flip = np.float32(math.pow(float(np.uint32(flip_fixed)) / 1e9, 1.0 / 3.0))
    return mse, np.float32(psnr), flip


def metrics(cap, cur, flip_mode=2, ppd=67.0, dt=np.float64, order=0):
    """everything mgs_compare_metrics returns, from the restatement"""
    H, W = cap.shape[:2]
    se, mc, p, fc = contributions(cap, cur, flip_mode, ppd, dt, order)
    mse_fixed = int(to_fixed(mc).sum() & 0xFFFFFFFF)
    flip_fixed = int(to_fixed(fc).sum() & 0xFFFFFFFF) if fc is not None else 0
    mse, psnr, flip = collect(mse_fixed, flip_fixed)
    mse_exact = float(se.astype(np.float64).sum()) / (W * H * 3.0)
    psum = float(p.astype(np.float64).sum()) if p is not None else 0.0
    return dict(mse_fixed=mse_fixed, flip_fixed=flip_fixed, mse=mse, psnr=psnr, flip=flip, mse_exact=mse_exact,
                psnr_exact=(10.0 * math.log10(1.0 / mse_exact) if mse_exact > 0 else math.inf), flip_powered_sum=psum,
                flip_exact=math.pow(psum / (W * H), 1.0 / 3.0) if p is not None else 0.0, mse_units=mc, flip_units=fc)


# ---- the composite shader ------------------------------------------------------------------------------------------------------
def sample_image(img, outW, outH, dt):
    if img.shape[:2] == (outH, outW):
        return img.astype(dt)
    u, v = _uv(outW, outH, dt)
    return bilinear(img, u, v, dt)


def multi_scale_contrast(img, outW, outH, dt):
    """computeMultiScaleContrast at every OUTPUT pixel's coordinate, in the image's own size (0 within 2 of its border or outside)"""
    L = luminance(img, dt)
    H, W = L.shape
    c = np.zeros((H, W), dt)
    if H > 4 and W > 4:
        m = L[2:-2, 2:-2]

        def at(ox, oy):
            return L[2 + oy:H - 2 + oy, 2 + ox:W - 2 + ox]
        gx, gy = np.abs(at(1, 0) - at(-1, 0)), np.abs(at(0, -1) - at(0, 1))
        t = np.zeros_like(m) + np.sqrt(gx * gx + gy * gy) * dt(0.5)
        gx, gy = np.abs(at(2, 0) - at(-2, 0)) * dt(0.5), np.abs(at(0, -2) - at(0, 2)) * dt(0.5)
        t = t + np.sqrt(gx * gx + gy * gy) * dt(0.3)
        g1, g2 = np.abs(at(1, -1) - at(-1, 1)), np.abs(at(-1, -1) - at(1, 1))
        t = t + np.sqrt(g1 * g1 + g2 * g2) * dt(0.2)
        c[2:-2, 2:-2] = t
    out = np.zeros((outH, outW), dt)
    h, w = min(H, outH), min(W, outW)
    out[:h, :w] = c[:h, :w]
    return out


def opponent(rgb, dt):
    lin = srgb_to_linear(rgb[..., :3], dt)
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    X = _dot3(r, g, b, (0.4124564, 0.3575761, 0.1804375), dt)
    Y = _dot3(r, g, b, (0.2126729, 0.7151522, 0.0721750), dt)
    Z = _dot3(r, g, b, (0.0193339, 0.1191920, 0.9503041), dt)
    ystar = np.where(Y > dt(0.008856), np.power(np.maximum(Y, dt(1e-30)), dt(1.0) / dt(3.0)), dt(7.787) * Y + dt(16.0) / dt(116.0))
    return ystar, (X - Y) * dt(0.5), (Y - Z) * dt(0.3)


def turbo(x, dt):
    x = np.clip(x, dt(0), dt(1))
    v = [np.ones_like(x), x, x * x, x * x * x]
    a, b = v[2] * v[2], v[3] * v[2]

    def chan(k4, k2):
        d4 = ((v[0] * dt(k4[0]) + v[1] * dt(k4[1])) + v[2] * dt(k4[2])) + v[3] * dt(k4[3])
        return d4 + (a * dt(k2[0]) + b * dt(k2[1]))
    return np.stack([chan((0.13572138, 4.61539260, -42.66032258, 132.13108234), (-152.94239396, 59.28637943)),
                     chan((0.09140261, 2.19418839, 4.84296658, -14.18503333), (4.27729857, 2.82956604)),
                     chan((0.10667330, 12.64194608, -60.58204836, 110.36276771), (-89.90310912, 27.34824973))], axis=-1)


def display_color(mode, cap, cur, outW, outH, amplify, dt):
    one = np.ones((outH, outW, 1), dt)
    if mode == 0:
        return sample_image(cap, outW, outH, dt)
    if mode == 1:
        return sample_image(cur, outW, outH, dt)
    ref, c = sample_image(cap, outW, outH, dt), sample_image(cur, outW, outH, dt)
    diff = np.abs(ref - c)
    amp = dt(amplify)
    if mode == 2:
        return np.concatenate([np.minimum(diff[..., :3] * amp, dt(1)), one], axis=-1)
    if mode in (3, 4):
        inten = _dot3(diff[..., 0], diff[..., 1], diff[..., 2], (0.299, 0.587, 0.114), dt)
        inten = np.minimum(inten * amp, dt(1))
        if mode == 4:
            z = np.zeros_like(inten)
            return np.stack([inten, z, z, one[..., 0]], axis=-1)
        gray = _dot3(c[..., 0], c[..., 1], c[..., 2], (0.299, 0.587, 0.114), dt)
        return np.stack([gray + (dt(1) - gray) * inten, gray + (dt(0) - gray) * inten, gray + (dt(0) - gray) * inten, one[..., 0]], axis=-1)
    rc, cc = multi_scale_contrast(cap, outW, outH, dt), multi_scale_contrast(cur, outW, outH, dt)
    p, q = opponent(ref, dt), opponent(c, dt)
    lum_diff = np.abs(p[0] - q[0])
    dy, dz = p[1] - q[1], p[2] - q[2]
    chroma = np.sqrt(dy * dy + dz * dz)
    ce = lum_diff * dt(0.75) + chroma * dt(0.25)
    sens = dt(1) / (dt(1) + ((rc + cc) * dt(0.5)) * dt(8.0))
    mask = dt(1) - np.clip(np.maximum(rc, cc) * dt(4.0), dt(0), dt(1))
    e = (ce * (dt(0.4) + dt(0.6) * sens)) * (dt(0.3) + dt(0.7) * mask)
    e = np.power(np.clip(e, dt(0), dt(1)), dt(0.75))
    return np.concatenate([turbo(e, dt), one], axis=-1)


def composite(cap, cur, split=0.5, left=0, right=1, amplify=5.0, width=0, height=0, dt=np.float64):
    outH, outW = (height, width) if width else cur.shape[:2]
    split_pos = int(np.float32(split) * np.float32(outW))
    out = np.zeros((outH, outW, 4), dt)
    lc = display_color(left, cap, cur, outW, outH, amplify, dt)
    rc = lc if right == left else display_color(right, cap, cur, outW, outH, amplify, dt)
    x = np.arange(outW)
    out[:, x < split_pos] = lc[:, x < split_pos]
    out[:, x >= split_pos] = rc[:, x >= split_pos]
    dist = np.abs(x - split_pos)
    out[:, dist <= 2] = np.array([0, 0, 0, 1], dt)
    out[:, dist <= 0] = np.array([1, 1, 1, 1], dt)
    return out
