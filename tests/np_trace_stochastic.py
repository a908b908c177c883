"""Float64 restatement of the two stochastic trace strategies of mgs_render_traced (MgsTraceParams::trace_strategy 1 and 2).

Test infrastructure only.  Brute force over all particles per ray, as np_trace.py, whose rays, particle preparation and response it
calls; the per-hit quantities of a walk (t, alpha, radiance, normal, acceptance and their fp32 margins) are restated here because
np_trace.trace does not hand them out.  As written in
  shaders/threedgrt_raytrace.rgen.slang:615-819    the passes, with Russian roulette on a pass's opacity (:669-673, :684-687, :765-801)
  shaders/threedgrt_raytrace.rgen.slang:823-961    the stochastic any-hit's pixel, PARTICLES_SPP == 1
  shaders/threedgrt_raytrace.rahit.slang:94-150    a hit before the slot is kept with probability alpha
  shaders/threedgrt_raytrace.rgen.slang:228,848    seedRayPass / rngSeed = xxhash32(pixel, frameSampleId)

Per pixel it gives (a) one SAMPLE for a frame_sample_id, with the draws the device makes, and (b) the exact OUTCOME DISTRIBUTION, a
list of (probability, rgba): a pass is the pixel with probability opacity_k * prod_{j<k} (1 - opacity_j), a hit of the any-hit
strategy with probability alpha_i * prod_{j<i} (1 - alpha_j), and what is left is the untouched pixel (0, 0, 0, 0).

Fragile pixels: np_trace's rules (proxy, range, thresholds, order, transmittance against min_transmittance and the iso threshold,
iso-normal branches), restated with the same margins, and for a sample one more:
  * a draw against an opacity.  Pass-stochastic: opacity = float(1 - T); T carries the relative uncertainty relT + 4 u of np_trace's
    transmittance rule, the subtraction in double is exact to 2^-53 and the rounding to fp32 adds at most u (opacity <= 1), so a draw
    within T (relT + 4 u) + u of the opacity makes the pixel fragile.  Any-hit: a draw inside [alpha_lo, alpha_hi], the interval np_trace
    puts around a hit's alpha.  The draws themselves are exact: integers times 2^-23.
The any-hit draw hashes the bits of the fp32 t; the device's t differs from float32(float64 t) in the last bits, so its stream is
another one of the same distribution and a sample of strategy 2 is compared in distribution only."""
import numpy as np

import np_reference as npr
import np_trace
from np_trace import U, T_MIN, T_MAX, EPS_T, INVALID


def xxhash32(px, py, pz):
    m = 0xFFFFFFFF
    p0, p1, p2, p3 = 2246822519, 3266489917, 668265263, 374761393
    h = (pz + p3 + px * p1) & m
    h = (p2 * (((h << 17) | (h >> 15)) & m)) & m
    h = (h + py * p1) & m
    h = (p2 * (((h << 17) | (h >> 15)) & m)) & m
    h = (p0 * (h ^ (h >> 15))) & m
    h = (p1 * (h ^ (h >> 13))) & m
    return h ^ (h >> 16)


def rand(state):
    """pcg step: (new state, uniform in [0, 1) with 23 bits)"""
    m = 0xFFFFFFFF
    prev = (state * 747796405 + 2891336453) & m
    word = (((prev >> ((prev >> 28) + 4)) ^ prev) * 277803737) & m
    r = ((word >> 22) ^ word) & m
    return prev, (r >> 9) / 8388608.0


def _normal(ps, li, om, dm, Ri, thin, method, d_d):
    """normalWorld of a hit and whether a branch of it lies within the fp32 margin (threedgrt.h.slang:358-537, :218)"""
    s, R, p = ps["s"][li], ps["R"][li], ps["pos"][li]
    local = om - p
    iso = method == 1
    th = max(0.02 * s.max(), float(np.float32(thin))) if iso else float(np.float32(thin))
    small = s < th
    frag = bool((np.abs(s - th) <= 8.0 * U * th).any())
    n = -dm / np.linalg.norm(dm)
    if small.sum() == 0 and not iso:
        g = R @ ((R.T @ local) / (s * s))
        n = g / np.linalg.norm(g)
        n = -n if n @ local < 0 else n
    elif small.sum() == 0:
        oc, dc = (R.T @ local) / s, (R.T @ dm) / s
        dn = dc / np.linalg.norm(dc)
        b = oc @ dn
        cr = np.cross(dn, oc)
        rem = 9.0 - cr @ cr
        m_rem = 2.0 * np.sqrt(cr @ cr) * d_d + d_d * d_d + 16.0 * U * 9.0
        frag = frag or abs(rem) <= m_rem
        if rem >= 0.0:
            half = np.sqrt(rem)
            m_t = d_d + m_rem / max(2.0 * half, 1e-300) + 16.0 * U * (abs(b) + half)
            t1, t2 = -b - half, -b + half
            frag = frag or abs(t1) <= m_t or (t1 < 0.0 and abs(t2) <= m_t)
            tq = t1 if t1 >= 0.0 else t2
            if tq >= 0.0:
                h = oc + tq * dn
                g = R @ (h / np.linalg.norm(h) / s)
                n = g / np.linalg.norm(g)
    elif small.sum() == 1:
        n = R[:, int(np.argmax(small))]
        n = -n if n @ local < 0 else n
    wn = Ri.T @ n
    return wn / np.linalg.norm(wn), frag


def ray_hits(instances, V, P, W, H, adaptive_clamping=True, kernel_degree=2, kernel_min_response=0.0113, alpha_clamp=0.99, alpha_cull=1.0 / 255.0,
             sh_degree=3, fisheye=False, fov_rad=None, dof=None, thin=1e-6, sh_only=False, no_gauss=False, normal_method=0):
    """every ray's candidate hits in walk order (t, caller's global id): dict(O, D, OK, V, P, hits[y][x] = [hit], fragile[H,W]) with
    hit = dict(t, gid, acc, alpha, a_lo, a_hi, col, nrm, d_t).  fragile: a proxy, range, threshold, order or normal-branch decision
    of the ray lies within its fp32 margin (np_trace's margins); bit-identical copies within one instance are an exact tie."""
    V, P = np.asarray(V, np.float64), np.asarray(P, np.float64)
    kmr, acull, aclamp = float(np.float32(kernel_min_response)), float(np.float32(alpha_cull)), float(np.float32(alpha_clamp))
    O, D, OK = np_trace.rays(V, P, W, H, fisheye, fov_rad, dof)
    fragile = np.zeros((H, W), bool)
    hits = [[[] for _ in range(W)] for _ in range(H)]
    base = 0
    for k, (ps, M) in enumerate(instances):
        M = np.asarray(M, np.float64)
        Mi, Ri = np.linalg.inv(M), np.linalg.inv(M[:3, :3])
        dens = ps["rgba"][:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            thr = np.minimum(kmr / dens if adaptive_clamping else np.full_like(dens, kmr), 0.97)
        alive = (dens > acull) & np.isfinite(ps["s"]).all(1) & np.isfinite(ps["pos"]).all(1) & np.isfinite(ps["R"]).all((1, 2))
        idx = np.nonzero(alive)[0]
        gbase, base = base, base + ps["n"]
        if idx.size == 0:
            continue
        pos, s, R = ps["pos"][idx], ps["s"][idx], ps["R"][idx]
        for y in range(H):
            om = O[y] @ Mi[:3, :3].T + Mi[:3, 3]
            dm = D[y] @ Ri.T
            x = om[:, None, :] - pos[None, :, :]
            oc = np.einsum("wnj,njc->wnc", x, R) / s[None]
            dc = np.einsum("wj,njc->wnc", dm, R) / s[None]
            dd = (dc * dc).sum(-1)
            t = -(oc * dc).sum(-1) / dd
            cr = np.cross(dc, oc)
            dist = np.sqrt((cr * cr).sum(-1) / dd)
            l1 = np.abs(om).sum(-1)[:, None] + np.abs(pos).sum(-1)[None] + np.abs(x).sum(-1)
            d_oc = 8.0 * U * l1[..., None] / s[None]
            d_d = np.sqrt((d_oc * d_oc).sum(-1)) + 16.0 * U * np.sqrt((oc * oc).sum(-1))
            d_t = d_d / np.sqrt(dd)
            r_mid = np_trace.response(kernel_degree, dist)
            r_hi = np_trace.response(kernel_degree, dist - d_d) * (1.0 + 16.0 * U)
            r_lo = np_trace.response(kernel_degree, dist + d_d) * (1.0 - 16.0 * U)
            th = thr[idx][None]
            is_c = (t > T_MIN + EPS_T) & (t < T_MAX + EPS_T) & (r_mid > th)
            maybe = ((t + d_t > T_MIN) & (t - d_t < T_MAX + EPS_T)) & (r_hi > th) & ~((t - d_t > T_MIN + EPS_T) & (t + d_t < T_MAX) & (r_lo > th))
            fragile[y] |= maybe.any(1)
            for lim in (np.full_like(th, kmr), acull / dens[idx][None]):
                fragile[y] |= (is_c & (r_lo <= lim) & (r_hi >= lim)).any(1)
            for a, b in zip(*np.nonzero(is_c)):
                if not OK[y, a]:
                    continue
                li, den = idx[b], dens[idx[b]]
                resp = float(r_mid[a, b])
                alpha = min(aclamp, resp * den)
                acc = alpha > acull and resp > kmr
                a_hi, a_lo = min(aclamp, float(r_hi[a, b]) * den), min(aclamp, float(r_lo[a, b]) * den)
                col, nrm = np.zeros(3), np.zeros(3)
                if acc:
                    if no_gauss:
                        alpha = a_hi = a_lo = 1.0
                    v = ps["pos"][li] - om[a]
                    v = v / np.linalg.norm(v)
                    col = np.full(3, 0.5) if sh_only else ps["rgba"][li, :3].copy()
                    deg = min(ps["degree"], sh_degree)
                    if deg > 0:
                        col = col + npr.sh_radiance(ps["sh"][li:li + 1], deg, v[None])[0]
                    nrm, nfrag = _normal(ps, li, om[a], dm[a], Ri, thin, normal_method, d_d[a, b])
                    fragile[y, a] |= nfrag
                hits[y][a].append(dict(t=float(t[a, b]), gid=int(gbase + li), inst=k, shape=int(ps["shape"][li]), acc=bool(acc), alpha=alpha, a_lo=a_lo,
                                       a_hi=a_hi, col=col, nrm=nrm, d_t=float(d_t[a, b])))
    for y in range(H):
        for x in range(W):
            c = hits[y][x] = sorted(hits[y][x], key=lambda e: (e["t"], e["gid"]))
            for e, f in zip(c, c[1:]):
                if f["t"] - e["t"] <= e["d_t"] + f["d_t"] and not (e["inst"] == f["inst"] and e["shape"] == f["shape"]):
                    fragile[y, x] = True
    return dict(O=O, D=D, OK=OK, V=V, P=P, W=W, H=H, hits=hits, fragile=fragile)


def _ndc_z(R, y, x, t):
    clip = R["P"] @ (R["V"] @ np.append(R["O"][y, x] + t * R["D"][y, x], 1.0))
    return clip[2] / clip[3], clip


def depth_and_tol(R, y, x, t, d_t):
    """ndc z of origin + t * direction and what fp32 may move it by (np_trace's rule for the picked depth)"""
    z, clip = _ndc_z(R, y, x, t)
    V, P = R["V"], R["P"]
    dt = d_t + 8.0 * U * (np.abs(R["O"][y, x]).sum() + t + np.abs(V[:3, 3]).sum())
    tol = (max(abs(_ndc_z(R, y, x, t + dt)[0] - z), abs(_ndc_z(R, y, x, t - dt)[0] - z))
           + 8.0 * U * (np.abs(P[2]) @ np.abs(V @ np.append(R["O"][y, x] + t * R["D"][y, x], 1.0))) / abs(clip[3]))
    return z, tol


class _Pixel:
    """PixelData as far as the strategies touch it"""

    def __init__(self):
        self.T, self.relT = 1.0, 0.0
        self.rad, self.nrm, self.wsum = np.zeros(3), np.zeros(3), 0.0
        self.hc, self.pick, self.iso_d, self.pick_dt = 0, INVALID, 0.0, 0.0

    def copy(self):
        q = _Pixel()
        q.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()})
        return q


def _pass_chain(c, K, max_passes, minT, isoT):
    """the passes of one ray as long as every pass is REJECTED, literally: snapshot, walk, restore (rgen.slang:634-818).  Yields per
    pass that found a hit (pixel after the walk = what an accepted pass leaves before the division, last valid slot, fragile: a
    transmittance test of the walk within its margin, accepted-at-pass index, fallback slot accepted?)"""
    pixel = _Pixel()
    tmin = T_MIN
    rest = c
    for _ in range(max_passes):
        if not (tmin <= T_MAX and pixel.T > minT):
            break
        rest = [e for e in rest if e["t"] > tmin + EPS_T]
        if not rest:
            break
        old = pixel.copy()                      # const PixelData oldPixel = pixel (:671)
        slots = rest[:K]
        last, frag = slots[0], False
        for e in slots:
            near = lambda lim: abs(pixel.T - lim) <= pixel.T * (pixel.relT + 4.0 * U)
            frag |= near(minT)
            if not pixel.T > minT:
                continue
            last = e
            if e["acc"]:
                w = e["alpha"] * pixel.T
                pixel.rad = pixel.rad + e["col"] * w
                pixel.T *= 1.0 - e["alpha"]
                pixel.relT += (e["a_hi"] - e["a_lo"]) / max(1.0 - e["alpha"], 1e-30) + 4.0 * U
                pixel.hc += 1
                pixel.nrm = pixel.nrm + e["nrm"] * w
                pixel.wsum += w
                if pixel.iso_d == 0.0:
                    frag |= near(isoT)
                    if pixel.T < isoT:
                        pixel.iso_d, pixel.pick, pixel.pick_dt = e["t"], e["gid"], e["d_t"]
            tmin = max(tmin, e["t"])
        yield pixel, last, frag
        pixel = old                             # pixel = oldPixel (:798)


def pass_stochastic(R, sample_id, samples_per_pass=18, max_passes=200, min_transmittance=0.01, depth_iso_threshold=0.7):
    """strategy 1, one sample: dict(image, hits, id, depth, depth_tol, normal, fragile, accepted_pass [H,W] (0 = never), fallback [H,W]:
    the pick is the lastValidHitIdx slot, fallback_rejected [H,W]: and that slot's hit was not accepted by particleProcessHit)"""
    W, H = R["W"], R["H"]
    minT, isoT = float(np.float32(min_transmittance)), float(np.float32(depth_iso_threshold))
    out = dict(image=np.zeros((H, W, 4)), hits=np.zeros((H, W), np.int64), id=np.full((H, W), INVALID, np.int64), depth=np.zeros((H, W)),
               depth_tol=np.zeros((H, W)), normal=np.zeros((H, W, 4)), fragile=R["fragile"].copy(), accepted_pass=np.zeros((H, W), np.int64),
               fallback=np.zeros((H, W), bool), fallback_rejected=np.zeros((H, W), bool))
    for y in range(H):
        for x in range(W):
            if not R["OK"][y, x]:
                out["image"][y, x] = (0, 0, 0, 1)
                continue
            seed = xxhash32(x, y, sample_id)
            for k, (px, last, frag) in enumerate(_pass_chain(R["hits"][y][x], samples_per_pass, max_passes, minT, isoT)):
                out["fragile"][y, x] |= frag
                opacity = 1.0 - px.T
                seed, u = rand(seed)
                if abs(u - opacity) <= px.T * (px.relT + 4.0 * U) + U:
                    out["fragile"][y, x] = True
                if u < opacity:
                    pick, t, d_t = px.pick, px.iso_d, px.pick_dt
                    if px.iso_d == 0.0:
                        pick, t, d_t = last["gid"], last["t"], last["d_t"]
                        out["fallback"][y, x], out["fallback_rejected"][y, x] = True, not last["acc"]
                    out["image"][y, x] = (*(px.rad / opacity), 1.0)
                    out["hits"][y, x], out["id"][y, x] = px.hc, pick
                    out["depth"][y, x], out["depth_tol"][y, x] = depth_and_tol(R, y, x, t, d_t)
                    out["normal"][y, x] = (*px.nrm, px.wsum)
                    out["accepted_pass"][y, x] = k + 1
                    break
    return out


def pass_distribution(R, samples_per_pass=18, max_passes=200, min_transmittance=0.0):
    """strategy 1: per pixel the list of (probability, rgba); [H][W]"""
    minT = float(np.float32(min_transmittance))
    dist = [[None] * R["W"] for _ in range(R["H"])]
    for y in range(R["H"]):
        for x in range(R["W"]):
            if not R["OK"][y, x]:
                dist[y][x] = [(1.0, np.array([0, 0, 0, 1.0]))]
                continue
            left, o = 1.0, []
            for px, _, _ in _pass_chain(R["hits"][y][x], samples_per_pass, max_passes, minT, 0.7):
                opacity = 1.0 - px.T
                if opacity > 0.0:
                    o.append((left * opacity, np.append(px.rad / opacity, 1.0)))
                left *= 1.0 - opacity
            o.append((left, np.zeros(4)))
            dist[y][x] = o
    return dist


def anyhit_distribution(R):
    """strategy 2: per pixel the list of (probability, rgba); [H][W]"""
    dist = [[None] * R["W"] for _ in range(R["H"])]
    for y in range(R["H"]):
        for x in range(R["W"]):
            if not R["OK"][y, x]:
                dist[y][x] = [(1.0, np.array([0, 0, 0, 1.0]))]
                continue
            left, o = 1.0, []
            for e in R["hits"][y][x]:
                if e["acc"]:
                    o.append((left * e["alpha"], np.append(e["col"], 1.0)))
                    left *= 1.0 - e["alpha"]
            o.append((left, np.zeros(4)))
            dist[y][x] = o
    return dist


def anyhit(R, sample_id):
    """strategy 2, one sample with the draws of the fp32-rounded t: dict(image, hits, id, depth, depth_tol, normal, fragile, not_nearest
    [H,W]: the kept hit is not the ray's nearest candidate)"""
    W, H = R["W"], R["H"]
    out = dict(image=np.zeros((H, W, 4)), hits=np.zeros((H, W), np.int64), id=np.full((H, W), INVALID, np.int64), depth=np.zeros((H, W)),
               depth_tol=np.zeros((H, W)), normal=np.zeros((H, W, 4)), fragile=R["fragile"].copy(), not_nearest=np.zeros((H, W), bool))
    for y in range(H):
        for x in range(W):
            if not R["OK"][y, x]:
                out["image"][y, x] = (0, 0, 0, 1)
                continue
            rng_seed = xxhash32(x, y, sample_id)
            for i, e in enumerate(R["hits"][y][x]):
                if not e["acc"]:
                    continue
                bits = int(np.float32(e["t"]).view(np.uint32))
                _, u = rand(xxhash32(rng_seed, e["gid"] ^ bits, 0))
                if e["a_lo"] <= u <= e["a_hi"] and e["a_lo"] < e["a_hi"]:
                    out["fragile"][y, x] = True
                if u < e["alpha"]:
                    out["image"][y, x] = (*e["col"], 1.0)
                    out["hits"][y, x], out["id"][y, x] = 1, e["gid"]
                    out["depth"][y, x], out["depth_tol"][y, x] = depth_and_tol(R, y, x, e["t"], e["d_t"])
                    out["normal"][y, x] = (*e["nrm"], 1.0)
                    out["not_nearest"][y, x] = i > 0
                    break
    return out


def moments(dist):
    """mean, variance and range R = max |outcome - mean| per pixel and channel of an outcome distribution: three [H,W,4]"""
    H, W = len(dist), len(dist[0])
    mu, var, rng = np.zeros((H, W, 4)), np.zeros((H, W, 4)), np.zeros((H, W, 4))
    for y in range(H):
        for x in range(W):
            p = np.array([a for a, _ in dist[y][x]])
            v = np.array([b for _, b in dist[y][x]])
            assert abs(p.sum() - 1.0) <= 1e-12
            mu[y, x] = p @ v
            var[y, x] = p @ (v - mu[y, x]) ** 2
            rng[y, x] = np.abs(v[p > 0] - mu[y, x]).max(0)
    return mu, var, rng


BERNSTEIN_L = 20.0


def bernstein_ok(mean, mu, var, rng, ok, N, slack=1e-4):
    """bounds (a) per pixel and channel and (b) per channel of the frame-wide average of mean - mu, over the pixels `ok`, by
    Bernstein's inequality with failure probability <= 2 exp(-L) per comparison.  Returns (a holds, b holds, worst ratios)"""
    L = BERNSTEIN_L
    bound = np.sqrt(2.0 * var * L / N) + 2.0 * rng * L / (3.0 * N) + slack
    err = np.abs(mean - mu)
    n = int(ok.sum())
    a = bool((err[ok] <= bound[ok]).all())
    avg = (mean - mu)[ok].mean(0)
    bound_b = np.sqrt(2.0 * (var[ok].sum(0) / n ** 2) * L / N) + 2.0 * (rng[ok].max(0) / n) * L / (3.0 * N) + slack
    b = bool((np.abs(avg) <= bound_b).all())
    tiny = 1e-300  # (a pixel without noise has bound 0 and error 0)
    return a, b, float((err[ok] / (bound[ok] + tiny)).max()), float((np.abs(avg) / (bound_b + tiny)).max())
