"""The blend of the 3DGS rasteriser as a float64 INTERVAL per pixel and channel: the counterpart of np_gut.GutFragments.blend for
k_composite (and for the oracle, which tests/test_blend_cpu.py holds to the same interval without the kernel).

Inputs: a splat table as np_fragments.splat_table builds it (id, c, b1, b2, opacity, z per drawn splat), the per-splat colours and
opacities as the implementation under test holds them, and the frame's draw order, nearest first (the sorted stream: ties are not
open, test_depth_keys_cull_and_sort_bit_exact holds it bit for bit).  The table is built from the RECORDS OF THE IMPLEMENTATION UNDER
TEST (the oracle's orc_project, the device's mgs_frame_download_projected), taken as exact: what a projection in fp32 leaves open
(fragment_cases.EPS_FRAG, 1e-4 per fragment) is forty times what the blend leaves open, is tested by the projection's own tests, and
would otherwise be the whole interval.  This is the one rounding the issue's list had missed; it is removed, not allowed for.

Exact value.  Fragments f = 1, 2, ... of a pixel, nearest first, alpha_f = opacity * exp(-A_f / 2) where A_f <= 8 and
alpha_f > 1/255 (np_fragments._eval, _rule):  T_0 = 1, w_f = alpha_f T_{f-1}, C = sum w_f c_f, T_f = T_{f-1} - w_f; the default alpha
is 1 - T, the additive alpha (MGS_ALPHA_SUM) sum alpha_f.

The allowance, derived (nothing here is fitted to an output).  U = 2^-24, the unit roundoff of fp32.
  * alpha_f, relative:  EXP_ULPS = 16 fp32 ulps (2^-23 each) for the hardware exponential and the product with the opacity — the
    allowance np_trace.py gives v_exp_f32 —, plus ln2 * dq, the rounding of the exponent q = (A / 2) log2 e (|d alpha| / alpha <=
    ln2 |dq|).  dq has three parts:
      - Q_ROUNDINGS = 8 roundings of magnitude <= q + |log2 opacity| (the folded form log2 a - s^2 - u^2: two squares, two sums, the
        logarithm, the scaling of the axes by sqrt(log2 e));
      - the axes of the record: s = d.p1, u = d.p2 with p = b sqrt8 / |b|^2 scaled, AXIS_ROUNDINGS = 4 roundings each, relative to
        the terms of the dot product (next item);
      - the dot products are taken about the REGION centre (k_composite: s = lx p1x + (ly p1y + k1), k1 = -(r . p1), r = centre -
        region centre, |l| <= 17.2 px): their terms are as large as |p| (|r| + |l|) <= |p| (|d| + 35), not as |s|.  So
        ds <= AXIS_ROUNDINGS U |p1| (|d| + 35), du likewise, and dq <= 2 (|s| ds + |u| du).  For a splat near its region this is
        the issue's "magnitude <= |q|"; for a large splat it is the cancellation the issue's count had left out.
    A fragment within `delta` of A = 8 or of alpha = 1/255 (np_fragments._rule) may or may not exist: alpha in [0, alpha (1 + eps)].
  * the transmittance chain: CHAIN = 3 roundings per fragment on T (w = alpha T, T - w; back to front: 1 - alpha, the product),
    relative; `t_abs` adds an ABSOLUTE rounding per fragment for an implementation that accumulates A = 1 - T (the oracle's
    front-to-back blend, A' = a (1 - A) + A: one rounding of a number near 1 per fragment, which (1 - a) damps like T itself).
  * one rounding per accumulate of C: n U sum w |c| for n fragments (`acc_u` = U; 2^-11 for an fp16 target that is rounded after
    every blend).  Stated for the total and not per step because the oracle adds the same terms from the other end; the partial
    sums of either direction are bounded by sum w |c|.  The additive alpha: one relative `acc_u` per add.
  Everything is pushed through as interval arithmetic in float64.

Saturation.  k_composite stops a WAVE when all 128 pixels of its 16x8 quarter have T < 1e-4; a saturated pixel of a live wave keeps
taking fragments.  The reference's blend never stops.  Instead of re-enacting batches, the interval is the envelope over every
stopping time at or after the pixel's own first T < 1e-4 (T_lo < 1e-4 (1 + delta) counts as open): the running minimum of the lower
and the running maximum of the upper bound of C (+ T * the caller's colour under an occluder) and of 1 - T from that fragment on.
Any correct retirement lies inside; a wave that retires while one of its pixels is above 1e-4 does not.  The additive alpha never
stops and has its own interval.

Surface outputs.  The pick fires at the first existing fragment after which T < depth_iso_threshold.  Admissible are all fragments at
which T_lo < threshold while no certain fragment has had T_hi < threshold before; `none` (no pick) while no such certain fragment
exists.  Up to PICK_SLOTS per pixel; a pixel with more is `pick_open` (not compared, counted as excluded).
The integrated normal is sum w_f n_f with the SAME weights w_f as the colour (and 1 - T in its fourth channel), under the same
envelope rule; n_f is the splat's world normal as the implementation holds it, each component within `normal_err` of the value
given (0 for the implementation that supplied the normals; for another fp32 evaluation see normal_allowance).

simulate() is a float64 POINT evaluation of the same frame with the kernel's retirement as parameters (threshold, share of the quarter
that has to be saturated, a record dropped from a region's staged list, the cutoff, a late pick, an additive alpha that stops): the
honest setting must lie in the interval, each wrong one must not (tests/test_blend_cpu.py).

Test infrastructure only."""
import numpy as np

import np_fragments as nf

U = 2.0 ** -24
EXP_ULPS = 16
Q_ROUNDINGS = 8
AXIS_ROUNDINGS = 4
CHAIN = 3
T_SAT = 1.0e-4
LOG2E = 1.4426950408889634
PICK_SLOTS = 4
NONE_ID = 0xFFFFFFFF
DEPTH_TOL = 16 * U   # a picked depth against the float64 ndc z of its splat: clip z and clip w are 4-term dot products whose terms
                     # are about |view z| each, their quotient lies in [0, 1]: 8 roundings of magnitude <= 2


NORMAL_ROUNDINGS = 32   # camera into model space, the canonical vector, 1 / s^2, back through the rotation, two normalisations, the
                        # model matrix: 16 roundings of a unit-size term per evaluation, two fp32 evaluations apart


def normal_allowance(scales, local):
    """How far two fp32 evaluations of a splat's world normal (the gradient R S^-2 R^T (camera - centre), normalised) may lie apart
    per component: NORMAL_ROUNDINGS U, times the cancellation in the canonical vector — a component of R^T local is good to
    U |local|, and after the division by s_c^2 that error stands against |S^-2 R^T local|.  scales [n,3] (linear), local [n,3]
    = R^T (camera - centre) in float64."""
    w = 1.0 / np.asarray(scales, np.float64) ** 2
    lo = np.asarray(local, np.float64)
    kappa = np.linalg.norm(lo, axis=1) * w.max(axis=1) / np.maximum(np.linalg.norm(lo * w, axis=1), 1e-300)
    return NORMAL_ROUNDINGS * U * np.maximum(kappa, 1.0)


def table_from_records(ids, centre, b1, b2, opacity, z=None):
    """a splat table (np_fragments.splat_table's layout) from an implementation's own projected records, rows in the order given"""
    n = len(ids)
    return dict(id=np.asarray(ids, np.int64), c=np.asarray(centre, np.float64).reshape(n, 2), b1=np.asarray(b1, np.float64).reshape(n, 2),
                b2=np.asarray(b2, np.float64).reshape(n, 2), opacity=np.asarray(opacity, np.float64).reshape(n), theta=np.zeros(n),
                z=np.zeros(n) if z is None else np.asarray(z, np.float64).reshape(n))


def _windows(t, W, H, delta):
    ex = np.abs(t["b1"][:, 0]) + np.abs(t["b2"][:, 0])
    ey = np.abs(t["b1"][:, 1]) + np.abs(t["b2"][:, 1])
    pad = 1.0 + 8.0 * delta
    x0 = np.maximum(0, np.floor(t["c"][:, 0] - pad * ex - 0.5)).astype(np.int64)
    x1 = np.minimum(W - 1, np.ceil(t["c"][:, 0] + pad * ex - 0.5)).astype(np.int64)
    y0 = np.maximum(0, np.floor(t["c"][:, 1] - pad * ey - 0.5)).astype(np.int64)
    y1 = np.minimum(H - 1, np.ceil(t["c"][:, 1] + pad * ey - 0.5)).astype(np.int64)
    return x0, x1, y0, y1


def _fragment(t, i, xx, yy, delta, alpha_min=nf.ALPHA_MIN):
    """(alpha, exists, borderline, eps) of splat row i at the pixels (xx, yy); eps: the relative allowance of alpha (module docstring)"""
    c, b1, b2, op = t["c"][i], t["b1"][i], t["b2"][i], t["opacity"][i]
    dx, dy = xx + 0.5 - c[0], yy + 0.5 - c[1]
    n1, n2 = b1[0] ** 2 + b1[1] ** 2, b2[0] ** 2 + b2[1] ** 2
    u, v = (dx * b1[0] + dy * b1[1]) / n1, (dx * b2[0] + dy * b2[1]) / n2
    A = 8.0 * (u * u + v * v)
    alpha = np.exp(-0.5 * A) * op
    keep = (A <= 8.0) & (alpha > alpha_min)
    # borderline: within delta of either threshold while the other rule could still let the fragment through
    maybe = (A <= 8.0 * (1.0 + delta)) & (alpha > alpha_min * (1.0 - delta))
    edge = maybe & ~((A <= 8.0 * (1.0 - delta)) & (alpha > alpha_min * (1.0 + delta)))
    k = 2.0 * np.sqrt(LOG2E)           # s = k u, |p1| = k / |b1|: q = s^2 + u'^2 = (A / 2) log2 e
    reach = np.hypot(dx, dy) + 35.0
    ds = AXIS_ROUNDINGS * U * k / np.sqrt(n1) * reach
    du = AXIS_ROUNDINGS * U * k / np.sqrt(n2) * reach
    q = 0.5 * A * LOG2E
    dq = Q_ROUNDINGS * U * (q + abs(np.log2(max(op, 1e-300)))) + 2.0 * (np.abs(k * u) * ds + np.abs(k * v) * du)
    eps = EXP_ULPS * 2.0 * U + np.log(2.0) * dq
    return alpha, keep, edge, eps


class Blend:
    """lo, hi [H,W,4]: the default mode (alpha = 1 - T); sum_lo, sum_hi [H,W]: the additive alpha; n [H,W]: fragments (borderline
    ones included); with iso: pick_ids [H,W,PICK_SLOTS] (-1: unused), pick_none [H,W] (no pick is admissible), pick_open [H,W]"""

    def image(self, alpha_sum=False):
        """(lo, hi) [H,W,4] of the frame in the given alpha mode (the colour is the same in both)"""
        if not alpha_sum:
            return self.lo, self.hi
        lo, hi = self.lo.copy(), self.hi.copy()
        lo[..., 3], hi[..., 3] = self.sum_lo, self.sum_hi
        return lo, hi


def blend(table, order, colours, W, H, delta=1e-4, acc_u=U, t_abs=0.0, depth_level=None, bg=None, iso=None, normals=None, normal_err=None):
    """table: see table_from_records; order: global ids nearest first; colours: [n, 3] by global id; depth_level: a constant occluder
    depth D (a splat is drawn iff its table z <= D) and bg [H,W,4], the caller's colour image under it; iso: depth_iso_threshold
    (surface outputs) or None; normals [n, 3] by global id and normal_err [n] (or None: exact): the integrated normal's interval
    nlo, nhi [H,W,4].  Returns Blend."""
    row = {int(g): r for r, g in enumerate(table["id"])}
    x0, x1, y0, y1 = _windows(table, W, H, delta)
    T_lo, T_hi = np.ones((H, W)), np.ones((H, W))
    C_lo, C_hi, Cabs = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 3))
    S_lo, S_hi = np.zeros((H, W)), np.zeros((H, W))
    n = np.zeros((H, W), np.int32)
    bgc = np.zeros((H, W, 3)) if bg is None else np.asarray(bg, np.float64)[..., :3]
    env_lo, env_hi = np.full((H, W, 3), np.inf), np.full((H, W, 3), -np.inf)
    aenv_lo, aenv_hi = np.full((H, W), np.inf), np.full((H, W), -np.inf)
    N_lo, N_hi, Nabs = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 3))
    nenv_lo, nenv_hi = np.full((H, W, 3), np.inf), np.full((H, W, 3), -np.inf)
    pick_ids = np.full((H, W, PICK_SLOTS), -1, np.int64)
    pick_n = np.zeros((H, W), np.int32)
    picked = np.zeros((H, W), bool)
    thr = T_SAT * (1.0 + delta)
    for g in order:
        i = row.get(int(g))
        if i is None or x1[i] < x0[i] or y1[i] < y0[i] or (depth_level is not None and table["z"][i] > depth_level):
            continue
        win = (slice(y0[i], y1[i] + 1), slice(x0[i], x1[i] + 1))
        yy, xx = np.mgrid[win]
        alpha, keep, edge, eps = _fragment(table, i, xx, yy, delta)
        a_hi = np.where(keep | edge, alpha * (1.0 + eps), 0.0)
        if not a_hi.any():
            continue
        a_lo = np.where(keep & ~edge, alpha * (1.0 - eps), 0.0)
        tl, th = T_lo[win], T_hi[win]
        w_lo = np.where(tl < 0.0, a_hi, a_lo) * tl * (1.0 - U)
        w_hi = a_hi * th * (1.0 + U)
        c = colours[int(g)]
        p, q = w_lo[..., None] * c, w_hi[..., None] * c
        C_lo[win] += np.minimum(p, q)
        C_hi[win] += np.maximum(p, q)
        Cabs[win] += w_hi[..., None] * np.abs(c)
        n[win] += a_hi > 0
        if normals is not None:
            e = 0.0 if normal_err is None else float(normal_err[int(g)])
            nl, nh = normals[int(g)] - e, normals[int(g)] + e
            cand = np.stack([w_lo[..., None] * nl, w_lo[..., None] * nh, w_hi[..., None] * nl, w_hi[..., None] * nh])
            N_lo[win] += cand.min(axis=0)
            N_hi[win] += cand.max(axis=0)
            Nabs[win] += w_hi[..., None] * np.maximum(np.abs(nl), np.abs(nh))
        S_lo[win] = (S_lo[win] + a_lo) * (1.0 - acc_u)
        S_hi[win] = (S_hi[win] + a_hi) * (1.0 + acc_u)
        tl = np.where(tl < 0.0, tl * (1.0 - a_lo), tl * (1.0 - a_hi))
        tl = tl - CHAIN * U * np.abs(tl) - np.where(a_hi > 0, t_abs, 0.0)
        th = th * (1.0 - a_lo) * (1.0 + CHAIN * U) + np.where(a_hi > 0, t_abs, 0.0)
        T_lo[win], T_hi[win] = tl, th
        m = tl < thr
        if m.any():   # the pixel may be saturated from here on: a wave may retire after this record (or any later one)
            el, eh = env_lo[win], env_hi[win]
            bl, bh = bgc[win] * tl[..., None], bgc[win] * th[..., None]
            el[m] = np.minimum(el[m], (C_lo[win] + np.minimum(bl, bh))[m])
            eh[m] = np.maximum(eh[m], (C_hi[win] + np.maximum(bl, bh))[m])
            if normals is not None:
                ql, qh = nenv_lo[win], nenv_hi[win]
                ql[m] = np.minimum(ql[m], N_lo[win][m])
                qh[m] = np.maximum(qh[m], N_hi[win][m])
            al, ah = aenv_lo[win], aenv_hi[win]
            al[m] = np.minimum(al[m], 1.0 - th[m])
            ah[m] = np.maximum(ah[m], 1.0 - tl[m])
        if iso is not None:
            can = (a_hi > 0) & ~picked[win] & (tl < iso)
            if can.any():
                ys, xs = yy[can], xx[can]
                k = pick_n[ys, xs]
                ok = k < PICK_SLOTS
                pick_ids[ys[ok], xs[ok], k[ok]] = int(g)
                pick_n[ys, xs] = k + 1
            picked[win] |= (a_lo > 0) & (th < iso)
    bl, bh = bgc * T_lo[..., None], bgc * T_hi[..., None]
    env_lo = np.minimum(env_lo, C_lo + np.minimum(bl, bh))
    env_hi = np.maximum(env_hi, C_hi + np.maximum(bl, bh))
    aenv_lo, aenv_hi = np.minimum(aenv_lo, 1.0 - T_hi), np.maximum(aenv_hi, 1.0 - T_lo)
    acc = (n[..., None] + 2) * acc_u * (Cabs + np.abs(bgc) * np.maximum(T_hi, 0.0)[..., None])
    out = Blend()
    out.W, out.H, out.n = W, H, n
    out.lo = np.concatenate([env_lo - acc, (aenv_lo - acc_u * (1 + np.abs(aenv_lo)))[..., None]], 2)
    out.hi = np.concatenate([env_hi + acc, (aenv_hi + acc_u * (1 + np.abs(aenv_hi)))[..., None]], 2)
    bga = 0.0 if bg is None else np.asarray(bg, np.float64)[..., 3]
    if normals is not None:
        nacc = (n[..., None] + 2) * acc_u * Nabs
        out.nlo = np.concatenate([np.minimum(nenv_lo, N_lo) - nacc, out.lo[..., 3:]], 2)
        out.nhi = np.concatenate([np.maximum(nenv_hi, N_hi) + nacc, out.hi[..., 3:]], 2)
    out.sum_lo, out.sum_hi = (S_lo + bga) * (1.0 - acc_u), (S_hi + bga) * (1.0 + acc_u)
    out.T_lo, out.T_hi = T_lo, T_hi
    out.pick_ids, out.pick_none, out.pick_open = pick_ids, ~picked, pick_n > PICK_SLOTS
    out.fragments = nf.Fragments(W, H, table, True, delta, None if depth_level is None else np.full((H, W), float(depth_level)))
    return out


def simulate(table, order, colours, W, H, t_sat=T_SAT, share=1.0, drop=None, alpha_min=nf.ALPHA_MIN, iso=None, late_pick=False,
             sum_stops=False, depth_level=None, bg=None):
    """A float64 point evaluation with k_composite's retirement: a 16x8 quarter stops taking fragments once at least `share` of its
    128 pixels (those outside the image count as saturated, as in the kernel) have T < t_sat; share = 0 stands for "any one pixel
    inside the image".  drop = k: record k (0-based) of the staged list of every 32x16 region is lost (staged: the footprint box
    reaches one of the region's pixel centres).  late_pick: the depth pick fires one fragment late.  sum_stops: the additive alpha
    stops with its wave.  Returns (image [H,W,4] with alpha = 1 - T, additive alpha [H,W], picked ids [H,W] (NONE_ID: none))."""
    row = {int(g): r for r, g in enumerate(table["id"])}
    x0, x1, y0, y1 = _windows(table, W, H, 0.0)
    QH, QW = (H + 7) // 8, (W + 15) // 16
    Tp = np.zeros((QH * 8, QW * 16))   # padded to whole quarters: outside the image T = 0 (saturated from the start)
    Tp[:H, :W] = 1.0
    inside = np.zeros(Tp.shape, bool)
    inside[:H, :W] = True
    done = np.zeros((QH, QW), bool)
    C, S = np.zeros((H, W, 3)), np.zeros((H, W))
    pid = np.full((H, W), NONE_ID, np.int64)
    armed = np.zeros((H, W), bool)   # late_pick: the threshold is crossed, the next fragment is picked
    staged = np.zeros(((H + 15) // 16, (W + 31) // 32), np.int64)
    ex, ey = np.hypot(table["b1"][:, 0], table["b2"][:, 0]), np.hypot(table["b1"][:, 1], table["b2"][:, 1])
    rcx, rcy = np.arange(staged.shape[1]) * 32 + 16.0, np.arange(staged.shape[0]) * 16 + 8.0
    for g in order:
        i = row.get(int(g))
        if i is None or (depth_level is not None and table["z"][i] > depth_level):
            continue
        lost = None
        if drop is not None:
            reach = (np.abs(table["c"][i, 1] - rcy) <= ey[i] + 7.5)[:, None] & (np.abs(table["c"][i, 0] - rcx) <= ex[i] + 15.5)[None, :]
            lost = reach & (staged == drop)
            staged += reach
        if x1[i] < x0[i] or y1[i] < y0[i]:
            continue
        win = (slice(y0[i], y1[i] + 1), slice(x0[i], x1[i] + 1))
        yy, xx = np.mgrid[win]
        alpha, keep, _, _ = _fragment(table, i, xx, yy, 0.0, alpha_min)
        a = np.where(keep, alpha, 0.0)
        if lost is not None and lost.any():
            a = np.where(lost[yy // 16, xx // 32], 0.0, a)
        stopped = done[yy // 8, xx // 16]
        S[win] += np.where(stopped & sum_stops, 0.0, a)
        a = np.where(stopped, 0.0, a)
        if not a.any():
            continue
        T = Tp[win]
        w = a * T
        C[win] += w[..., None] * colours[int(g)]
        T = T - w
        Tp[win] = T
        if iso is not None:
            hit = (a > 0) & (pid[win] == NONE_ID)
            fire = hit & (armed[win] if late_pick else (T < iso))
            pw = pid[win]
            pw[fire] = int(g)
            armed[win] |= hit & (T < iso)
        qy0, qy1, qx0, qx1 = y0[i] // 8, y1[i] // 8 + 1, x0[i] // 16, x1[i] // 16 + 1
        blk = Tp[qy0 * 8:qy1 * 8, qx0 * 16:qx1 * 16].reshape(qy1 - qy0, 8, qx1 - qx0, 16)
        ins = inside[qy0 * 8:qy1 * 8, qx0 * 16:qx1 * 16].reshape(qy1 - qy0, 8, qx1 - qx0, 16)
        if share > 0:
            done[qy0:qy1, qx0:qx1] |= (blk < t_sat).sum(axis=(1, 3)) >= share * 128
        else:
            done[qy0:qy1, qx0:qx1] |= ((blk < t_sat) & ins).any(axis=(1, 3))
    T = Tp[:H, :W]
    if bg is not None:
        C = C + T[..., None] * np.asarray(bg, np.float64)[..., :3]
        S = S + np.asarray(bg, np.float64)[..., 3]
    return np.concatenate([C, (1.0 - T)[..., None]], 2), S, pid


# ---- the comparison both test modules use --------------------------------------------------------------------------------------------
EXCLUDE_FACTOR = 10.0   # a pixel whose interval is wider than this many median intervals of the case is borderline-dominated
EXCLUDE_CAP = 0.01      # at most this share of a case's pixels, and never a whole quarter


def excluded(lo, hi, n):
    """the borderline-dominated pixels: (mask [H,W], the case's median width); width = the widest channel, median over the pixels
    that have a fragment"""
    width = (hi - lo).max(axis=2)
    has = n > 0
    med = float(np.median(width[has])) if has.any() else 0.0
    return has & (width > EXCLUDE_FACTOR * med), med


def whole_quarter_excluded(mask):
    H, W = mask.shape
    m = np.ones(((H + 7) // 8 * 8, (W + 15) // 16 * 16), bool)   # pixels outside the image do not save a quarter
    m[:H, :W] = mask
    return bool(m.reshape(m.shape[0] // 8, 8, m.shape[1] // 16, 16).all(axis=(1, 3)).any())


def compare(lo, hi, n, img):
    """img [H,W,4] against the interval: (bad [H,W]: a non-excluded pixel with a channel outside; excluded [H,W]; the largest
    distance from the interval's midpoint as a fraction of the half-width over the non-excluded pixels; the widest interval there)"""
    img = np.asarray(img, np.float64)
    ex, _ = excluded(lo, hi, n)
    out = ((img < lo) | (img > hi) | ~np.isfinite(img)).any(axis=2)
    half = 0.5 * (hi - lo)
    frac = np.abs(img - 0.5 * (hi + lo)) / np.maximum(half, 1e-300)
    frac = np.where(half > 0, frac, np.where(img == lo, 0.0, np.inf))
    keep = ~ex
    return out & keep, ex, float(frac[keep].max()), float((hi - lo)[keep].max())


def compare_picks(b, ids, depth, z_of_id):
    """picked ids [H,W] (NONE_ID: none) and depths [H,W] against the admissible sets of Blend b; z_of_id: float64 ndc z by global id.
    Returns bad [H,W] (pixels that are pick_open are not compared)."""
    ids = np.asarray(ids, np.int64)
    none = ids == NONE_ID
    ok = (none & b.pick_none & (np.asarray(depth) == 0)) | ((b.pick_ids == ids[..., None]).any(axis=2) & ~none)
    z = np.asarray(z_of_id, np.float64)[np.where(none, 0, ids)]
    ok &= none | (np.abs(np.asarray(depth, np.float64) - z) <= DEPTH_TOL)
    return ~ok & ~b.pick_open


def describe(b, img, lo, hi, bad, order, limit=4, ids=16):
    """the first few pixels of `bad`: the frame's value, the interval, where the pixel lies and its fragments in draw order"""
    rank = {int(g): r for r, g in enumerate(order)}
    ys, xs = np.nonzero(bad)
    lines = [f"{ys.size} pixels outside their interval; the first {min(limit, ys.size)}:"]
    for y, x in list(zip(ys, xs))[:limit]:
        cov = sorted(b.fragments.covering(int(x), int(y)), key=lambda f: rank.get(f[0], 1 << 30))
        txt = ", ".join(f"{i}{'*' if e else ''}(a={al:.5f})" for i, _, al, e in cov[:ids]) + (" ..." if len(cov) > ids else "")
        lines.append(f"  pixel ({x},{y}) {nf.where(int(x), int(y))}: frame {np.asarray(img[y, x]).tolist()}, lo {lo[y, x].tolist()}, "
                     f"hi {hi[y, x].tolist()}; {len(cov)} fragments nearest first (* = borderline): {txt}")
    return "\n".join(lines)
