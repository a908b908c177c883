"""Float64 restatement of the ray queries (mgs_trace_rays): arbitrary rays, each with its own [t_min, t_max], through the walk of the
traced pipeline's strategy 0.

Test infrastructure only.  Brute force over all particles per ray, no hierarchy.  Everything follows np_trace.py, whose functions it
uses and whose module docstring has the sources and the derivation of every margin: the response, the proxy threshold, the tie rule
(t, caller's global id), the pass structure as written, and the fragile mask with its ulp bounds.  What differs from np_trace.trace:
  * the rays are given (origin, direction as they are: the direction is NOT normalised, t is the parameter along it); none of
    np_trace's margins assumes a unit direction: d_d is a distance in the canonical frame, d_t = d_d / |dc| carries the direction's
    length, and the relative terms are relative;
  * the window of the first pass is (max(t_min, 0) + EPS_T, t_max + EPS_T) per ray, and the order margin's "a hit within d_t of tMin
    or tMax" uses the ray's own bounds;
  * a ray with a non-finite component, a zero direction or t_min > t_max is invalid: the empty result, passes 0;
  * there is no camera: instead of the picked depth the result carries t_iso and its fp32 tolerance t_iso_tol (the hit's own d_t plus
    4 u of t), and the number of passes started.
With O, D from np_trace.rays and the window (np_trace.T_MIN, np_trace.T_MAX), processed in chunks of one image row, it is
np_trace.trace operation for operation (test_rays_cpu.py asserts the equality)."""
import numpy as np

import np_reference as npr
import np_trace
from np_trace import EPS_T, INVALID, U, response


def ray_valid(O, D, tmin, tmax):
    O, D = np.asarray(O, np.float64).reshape(-1, 3), np.asarray(D, np.float64).reshape(-1, 3)
    tmin, tmax = np.broadcast_to(np.asarray(tmin, np.float64), O.shape[:1]), np.broadcast_to(np.asarray(tmax, np.float64), O.shape[:1])
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(O).all(1) & np.isfinite(D).all(1) & np.isfinite(tmin) & np.isfinite(tmax)
        return fin & (D != 0.0).any(1) & (tmin <= tmax)


def trace_rays(instances, O, D, tmin, tmax, samples_per_pass=18, max_passes=200, min_transmittance=0.01, adaptive_clamping=True,
               depth_iso_threshold=0.7, kernel_degree=2, kernel_min_response=0.0113, alpha_clamp=0.99, alpha_cull=1.0 / 255.0, sh_degree=3,
               thin=1e-6, sh_only=False, no_gauss=False, normal_method=0, exact_ties=(), chunk=64):
    """instances: [(prepared set, M 4x4 math)] in creation order; O, D [n,3]; tmin, tmax scalars or [n].  Returns dict(radiance [n,3],
    transmittance [n], transmittance_tol [n], hits [n], id [n], t_iso [n], t_iso_tol [n], normal [n,4], passes [n], fragile [n], valid [n], candidates [n]).
    exact_ties: np_trace's declared ties with (chunk row, index in the chunk) in place of the pixel.  chunk: rays evaluated
    together (the arithmetic of a ray does not depend on it beyond what the matrix products' blocking may do)."""
    O, D = np.asarray(O, np.float64).reshape(-1, 3), np.asarray(D, np.float64).reshape(-1, 3)
    n = O.shape[0]
    tmin_a = np.broadcast_to(np.asarray(tmin, np.float64), (n,)).copy()
    tmax_a = np.broadcast_to(np.asarray(tmax, np.float64), (n,)).copy()
    valid = ray_valid(O, D, tmin_a, tmax_a)
    kmr = float(np.float32(kernel_min_response))
    acull, aclamp = float(np.float32(alpha_cull)), float(np.float32(alpha_clamp))
    minT, isoT = float(np.float32(min_transmittance)), float(np.float32(depth_iso_threshold))
    rad_out = np.zeros((n, 3))
    trans = np.ones(n)
    hits = np.zeros(n, np.int64)
    ids = np.full(n, INVALID, np.int64)
    t_iso = np.zeros(n)
    t_iso_tol = np.zeros(n)
    trans_tol = np.zeros(n)
    nrm = np.zeros((n, 4))
    passes = np.zeros(n, np.int64)
    fragile = np.zeros(n, bool)
    ncand = np.zeros(n, np.int64)
    per_inst = []
    base = 0
    for ps, M in instances:
        M = np.asarray(M, np.float64)
        Mi, Ri = np.linalg.inv(M), np.linalg.inv(M[:3, :3])
        dens = ps["rgba"][:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            thr = np.minimum(kmr / dens if adaptive_clamping else np.full_like(dens, kmr), 0.97)
        alive = dens > acull  # a particle at or below the cull threshold has no leaf and is never a hit
        alive &= np.isfinite(ps["s"]).all(1) & np.isfinite(ps["pos"]).all(1) & np.isfinite(ps["R"]).all((1, 2))
        per_inst.append((ps, M, Mi, Ri, dens, thr, alive, base))
        base += ps["n"]
    for row, c0 in enumerate(range(0, n, chunk)):
        sl = slice(c0, min(c0 + chunk, n))
        W = sl.stop - sl.start
        ok_row = valid[sl]
        # invalid rays are evaluated on a harmless stand-in and their candidates dropped
        o_row = np.where(ok_row[:, None], O[sl], 0.0)
        d_row = np.where(ok_row[:, None], D[sl], np.array([0.0, 0.0, 1.0]))
        lo_row = np.where(ok_row, np.maximum(tmin_a[sl], 0.0), 0.0)   # a ray has no hits behind its origin
        hi_row = np.where(ok_row, tmax_a[sl], 0.0)
        cand = [[] for _ in range(W)]  # per ray: (t, global id, instance, local, d, d_d, d_t, om, dm)
        frag_row = np.zeros(W, bool)
        for k, (ps, M, Mi, Ri, dens, thr, alive, gbase) in enumerate(per_inst):
            idx = np.nonzero(alive)[0]
            if idx.size == 0:
                continue
            pos, s, R = ps["pos"][idx], ps["s"][idx], ps["R"][idx]
            om = o_row @ Mi[:3, :3].T + Mi[:3, 3]            # [W,3]
            dm = d_row @ Ri.T                                 # [W,3] unnormalised: t stays the world ray's parameter
            x = om[:, None, :] - pos[None, :, :]             # [W,n,3]
            oc = np.einsum("wnj,njc->wnc", x, R) / s[None]   # R^T x / s
            dc = np.einsum("wj,njc->wnc", dm, R) / s[None]
            dd = (dc * dc).sum(-1)
            t = -(oc * dc).sum(-1) / dd
            cr = np.cross(dc, oc)
            dist = np.sqrt((cr * cr).sum(-1) / dd)
            l1 = np.abs(om).sum(-1)[:, None] + np.abs(pos).sum(-1)[None] + np.abs(x).sum(-1)
            d_oc = 8.0 * U * l1[..., None] / s[None]
            ocn = np.sqrt((oc * oc).sum(-1))
            d_d = np.sqrt((d_oc * d_oc).sum(-1)) + 16.0 * U * ocn
            d_t = d_d / np.sqrt(dd)
            r_mid = response(kernel_degree, dist)
            r_hi = response(kernel_degree, dist - d_d) * (1.0 + 16.0 * U)
            r_lo = response(kernel_degree, dist + d_d) * (1.0 - 16.0 * U)
            th = thr[idx][None]
            lo, hi = lo_row[:, None], hi_row[:, None]
            inr = (t > lo + EPS_T) & (t < hi + EPS_T)
            is_c = inr & (r_mid > th)
            maybe = ((t + d_t > lo) & (t - d_t < hi + EPS_T)) & (r_hi > th) & ~((t - d_t > lo + EPS_T) & (t + d_t < hi) & (r_lo > th))
            frag_row |= maybe.any(1)  # a proxy or range decision that rounding could flip
            for lim in (np.full_like(th, kmr), acull / dens[idx][None]):
                frag_row |= (is_c & (r_lo <= lim) & (r_hi >= lim)).any(1)
            wi, ni = np.nonzero(is_c)
            for a, b in zip(wi, ni):
                cand[a].append((t[a, b], gbase + idx[b], k, idx[b], dist[a, b], d_d[a, b], d_t[a, b], om[a], dm[a]))
        for xp in range(W):
            if not ok_row[xp]:
                continue
            gi = c0 + xp
            c = sorted(cand[xp], key=lambda e: (e[0], e[1]))
            ncand[gi] = len(c)
            fr = bool(frag_row[xp])

            def same_bits(e, f):  # one instance, bit-identical centre, log-scale and quaternion: bit-identical t on the device
                if e[2] == f[2] and per_inst[e[2]][0]["shape"][e[3]] == per_inst[e[2]][0]["shape"][f[3]]:
                    return True
                for ty, tx, tk, tids in exact_ties:
                    if (ty, tx) == (row, xp) and e[2] == f[2] == tk and e[3] in tids and f[3] in tids:
                        assert e[0] == f[0], "a declared exact tie has different t in the restatement"
                        return True
                return False

            for i in range(len(c) - 1):
                if c[i + 1][0] - c[i][0] <= c[i][6] + c[i + 1][6] and not same_bits(c[i], c[i + 1]):
                    fr = True
            T, relT = 1.0, 0.0
            rad = np.zeros(3)
            n_acc = np.zeros(3)
            wsum, iso_d, pick, hc, pick_dt = 0.0, 0.0, INVALID, 0, 0.0
            t_lo, t_hi = float(lo_row[xp]), float(hi_row[xp])

            def near(Tv, lim):
                return abs(Tv - lim) <= Tv * (relT + 4.0 * U)

            def walk(e):
                nonlocal T, relT, rad, n_acc, wsum, iso_d, pick, pick_dt, hc, fr
                tt, gid, k, li, dist, d_d, d_t, om, dm = e
                ps, M, Mi, Ri, dens, thr, alive, gbase = per_inst[k]
                den = dens[li]
                resp = float(response(kernel_degree, dist))
                alpha = min(aclamp, resp * den)
                if not (alpha > acull and resp > kmr):
                    return
                a_hi = min(aclamp, float(response(kernel_degree, dist - d_d)) * den * (1 + 16 * U))
                a_lo = min(aclamp, float(response(kernel_degree, dist + d_d)) * den * (1 - 16 * U))
                if no_gauss:
                    alpha = a_hi = a_lo = 1.0
                v = ps["pos"][li] - om
                v = v / np.linalg.norm(v)
                col = np.full(3, 0.5) if sh_only else ps["rgba"][li, :3].copy()
                deg = min(ps["degree"], sh_degree)
                if deg > 0:
                    col = col + npr.sh_radiance(ps["sh"][li:li + 1], deg, v[None])[0]
                w = alpha * T
                rad += col * w
                T *= 1.0 - alpha
                relT += (a_hi - a_lo) / max(1.0 - alpha, 1e-30) + 4.0 * U
                hc += 1
                nw, n_frag = np_trace._normal_world(ps, li, om, dm, Ri, thin, normal_method, d_d)
                fr = fr or n_frag
                n_acc += nw * w
                wsum += w
                if iso_d == 0.0:
                    if near(T, isoT):
                        fr = True
                    if T < isoT:
                        iso_d, pick, pick_dt = tt, gid, d_t

            rest = c
            for _ in range(max_passes):
                if near(T, minT):
                    fr = True
                if not (t_lo <= t_hi and T > minT):
                    break
                passes[gi] += 1
                rest = [e for e in rest if e[0] > t_lo + EPS_T]
                if not rest:
                    break
                for e in rest[:samples_per_pass]:
                    if near(T, minT):
                        fr = True
                    if T > minT:
                        walk(e)
                        t_lo = max(t_lo, e[0])
            rad_out[gi] = rad
            trans[gi] = T
            trans_tol[gi] = T * (relT + 4.0 * U) + U   # np_trace's bound of T (its `near`), and the result's rounding to fp32
            hits[gi] = hc
            nrm[gi] = (n_acc[0], n_acc[1], n_acc[2], wsum)
            if pick != INVALID:
                t_iso[gi], ids[gi] = iso_d, pick
                t_iso_tol[gi] = pick_dt + 4.0 * U * abs(iso_d)
            fragile[gi] = fr
    return dict(radiance=rad_out, transmittance=trans, hits=hits, id=ids, t_iso=t_iso, t_iso_tol=t_iso_tol, transmittance_tol=trans_tol, normal=nrm, passes=passes,
                fragile=fragile, valid=valid, candidates=ncand)
