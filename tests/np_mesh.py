"""Independent restatement of the mesh pass (mgs_meshes_render) in numpy.

Written from shaders/threedmesh_raster.vert.slang:53-62, shaders/threedmesh_raster.frag.slang:67-103 and the rasterisation rules
of include/mgs.h: vertex stage, near-plane and guard-band clipping on the weights of the three vertices, snap to 1/256 pixel,
coverage in 64-bit integers with the top-left rule, depth LESS in primitive order, perspective-correct attributes of the winning
fragment, shading through np_lighting._shade_direct.  `dtype` selects float32 or float64 for every floating-point operation
(the CPU test measures one against the other to set the GPU bar); the integer part is the same in both.

Conventions: matrices are 4x4 numpy arrays in math (row, col) convention; images are [H, W, ...] with row 0 = NDC y -1; a mesh is a
dict(positions [V,3], normals [V,3], indices [T,3], material_ids [T], materials [list of np_lighting material dicts],
transform 4x4 or None, visible bool); primitive ids count the triangles of all instances in order, visible or not.
"""
from collections import namedtuple

import numpy as np

import np_lighting as nl

NONE = 0xFFFFFFFF
GUARD = 256.0
SMALL = 8
Result = namedtuple("Result", "depth color prim fragments triangles_in")


def default_material():
    """the loader's default (src/obj_loader.cpp:72-81)"""
    return dict(ambient=(0.1, 0.1, 0.1), diffuse=(0.7, 0.7, 0.7), specular=(1.0, 1.0, 1.0), emission=(0.0, 0.0, 0.0), shininess=32.0)


def generate_normals(positions, indices, normals=None, visited=None):
    """src/obj_loader.cpp:98-151, literally: faces in order, the first face at a vertex sets its normal, every later one replaces
    it by mix(old, n, 0.5); float32 like glm"""
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    idx = np.asarray(indices).reshape(-1, 3)
    if normals is None:
        normals, visited = np.zeros((pos.shape[0], 3), np.float32), np.zeros(pos.shape[0], bool)
    half = np.float32(0.5)
    for i0, i1, i2 in idx:
        a, b = pos[i1] - pos[i0], pos[i2] - pos[i0]
        n = np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]], np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            n = n * (np.float32(1.0) / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2], dtype=np.float32))
        for v in (i0, i1, i2):
            if visited[v]:
                normals[v] = normals[v] * half + n * half
            else:
                normals[v] = n
                visited[v] = True
    return normals


def _mulv(v, M):
    """mul(v, M) of the shaders on a glm matrix == M v, summed in the order of v's components"""
    return ((v[:, 0:1] * M[:, 0] + v[:, 1:2] * M[:, 1]) + v[:, 2:3] * M[:, 2]) + v[:, 3:4] * M[:, 3]


def _plane(pl, c, dt):
    G = dt(GUARD)
    x, y, z, w = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    return [z, x + G * w, G * w - x, y + G * w, G * w - y][pl]


def _combine(b, a0, a1, a2):
    return (b[0] * a0 + b[1] * a1) + b[2] * a2


def _clip_polygon(c, dt):
    """Sutherland-Hodgman on the weights of the three vertices (c: [3,4] clip coordinates); returns the polygon's weights"""
    poly = [np.array(e, dt) for e in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    for pl in range(5):
        if len(poly) < 3:
            break
        out = []
        n = len(poly)
        for v in range(n):
            cur, nxt = poly[v], poly[(v + 1) % n]
            dc = _plane(pl, _combine(cur, c[0], c[1], c[2]), dt)
            dn = _plane(pl, _combine(nxt, c[0], c[1], c[2]), dt)
            in_c, in_n = dc >= 0, dn >= 0
            if in_c and len(out) < 8:
                out.append(cur)
            if in_c != in_n and len(out) < 8:
                (di, do, bi, bo) = (dc, dn, cur, nxt) if in_c else (dn, dc, nxt, cur)
                t = di / (di - do)
                out.append(bi + t * (bo - bi))
        poly = out
    return poly if len(poly) >= 3 else []


def _to_window(c, W, H, dt):
    """clip [n,4] -> (ok, X, Y int64 in 1/256 pixel, z, 1/w)"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = c[:, 3]
        wx = ((c[:, 0] / w) * dt(0.5) + dt(0.5)) * dt(W)
        wy = ((c[:, 1] / w) * dt(0.5) + dt(0.5)) * dt(H)
        z, invw = c[:, 2] / w, dt(1.0) / w
        ok = (w > 0) & (np.abs(wx) <= 2097152.0) & (np.abs(wy) <= 2097152.0) & np.isfinite(z) & np.isfinite(invw)
        X = np.where(ok, np.rint(np.where(ok, wx, 0) * dt(256.0)), 0).astype(np.int64)
        Y = np.where(ok, np.rint(np.where(ok, wy, 0) * dt(256.0)), 0).astype(np.int64)
    return ok, X, Y, z, invw


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _bias(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return np.where((dy < 0) | ((dy == 0) & (dx > 0)), 0, -1).astype(np.int64)


def _orient(X, Y, extra):
    """swap vertices 1 and 2 where the area is negative; extra: arrays [n,3,...] swapped along"""
    area2 = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    sw = area2 < 0
    for a in [X, Y] + extra:
        t = a[sw, 1].copy()
        a[sw, 1] = a[sw, 2]
        a[sw, 2] = t
    return np.abs(area2)


def _weights(X, Y, area2, sx, sy, dt):
    e0 = _edge(X[..., 1], Y[..., 1], X[..., 2], Y[..., 2], sx, sy)
    e1 = _edge(X[..., 2], Y[..., 2], X[..., 0], Y[..., 0], sx, sy)
    e2 = _edge(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1], sx, sy)
    fa = area2.astype(dt)
    return (e0, e1, e2), (e0.astype(dt) / fa, e1.astype(dt) / fa, e2.astype(dt) / fa)


def render(meshes, view, proj, camera_pos, W, H, lighting_mode=0, lights=(), dtype=np.float64):
    dt = np.dtype(dtype).type
    V, P = np.asarray(view, np.float32).astype(dt), np.asarray(proj, np.float32).astype(dt)
    origin = np.linalg.inv(np.asarray(view, np.float32).astype(np.float64))[:3, 3].astype(np.float32).astype(dt)

    # ---- vertex stage, per instance; sub-triangles of all primitives in one flat list
    S = dict(X=[], Y=[], z=[], invw=[], bary=[], ref=[], inst=[], tri=[])
    inst_data, prim0, tris_in = [], 0, 0
    for k, m in enumerate(meshes):
        idx = np.asarray(m["indices"], np.int64).reshape(-1, 3)
        T = idx.shape[0]
        M32 = np.eye(4, dtype=np.float32) if m.get("transform") is None else np.asarray(m["transform"], np.float32)
        M = M32.astype(dt)
        pos = np.asarray(m["positions"], np.float32).reshape(-1, 3).astype(dt)
        nrm = np.asarray(m["normals"], np.float32).reshape(-1, 3).astype(dt)
        with np.errstate(all="ignore"):
            wp = _mulv(np.concatenate([pos, np.ones((pos.shape[0], 1), dt)], 1), M)[:, :3]
            clip = _mulv(_mulv(np.concatenate([wp, np.ones((pos.shape[0], 1), dt)], 1), V), P)
            R = np.linalg.inv(M32[:3, :3].astype(np.float64)).astype(np.float32).astype(dt)  # transformRotScaleInverse
            wn = (nrm[:, 0:1] * R[0, :] + nrm[:, 1:2] * R[1, :]) + nrm[:, 2:3] * R[2, :]     # transpose(R) n
            wn = wn * (dt(1.0) / np.sqrt((wn[:, 0] * wn[:, 0] + wn[:, 1] * wn[:, 1]) + wn[:, 2] * wn[:, 2]))[:, None]
        inst_data.append(dict(wp=wp, wn=wn, vd=wp - origin, idx=idx, mesh=m))
        if m.get("visible", True):
            tris_in += T
            c = clip[idx]  # [T,3,4]
            finite = np.isfinite(c).all(axis=(1, 2))
            with np.errstate(invalid="ignore"):
                inside = np.stack([_plane(pl, c, dt) >= 0 for pl in range(5)], 0)  # [5,T,3]
            all_in = finite & inside.all(axis=(0, 2))
            reject = (~inside).all(axis=2).any(axis=0)
            t_in = np.nonzero(all_in)[0]
            if t_in.size:
                ok, X, Y, z, invw = _to_window(c[t_in].reshape(-1, 4), W, H, dt)
                ok = ok.reshape(-1, 3).all(axis=1)
                sel = t_in[ok]
                S["X"].append(X.reshape(-1, 3)[ok]); S["Y"].append(Y.reshape(-1, 3)[ok]); S["z"].append(z.reshape(-1, 3)[ok])
                S["invw"].append(invw.reshape(-1, 3)[ok])
                S["bary"].append(np.broadcast_to(np.eye(3, dtype=dt), (sel.size, 3, 3)).copy())
                S["ref"].append(((prim0 + sel) << 3).astype(np.int64)); S["inst"].append(np.full(sel.size, k)); S["tri"].append(sel)
            for t in np.nonzero(finite & ~all_in & ~reject)[0]:
                with np.errstate(all="ignore"):
                    poly = _clip_polygon(c[t], dt)
                    if not poly:
                        continue
                    bar = np.array([[poly[0], poly[s + 1], poly[s + 2]] for s in range(len(poly) - 2)], dt)  # [subs,3,3]
                    cc = np.array([[_combine(b, c[t, 0], c[t, 1], c[t, 2]) for b in tri] for tri in bar], dt)
                ok, X, Y, z, invw = _to_window(cc.reshape(-1, 4), W, H, dt)
                if not ok.all():
                    continue
                ns = bar.shape[0]
                S["X"].append(X.reshape(-1, 3)); S["Y"].append(Y.reshape(-1, 3)); S["z"].append(z.reshape(-1, 3)); S["invw"].append(invw.reshape(-1, 3))
                S["bary"].append(bar); S["ref"].append(((prim0 + t) << 3) + np.arange(ns, dtype=np.int64))
                S["inst"].append(np.full(ns, k)); S["tri"].append(np.full(ns, t))
        prim0 += T

    depth = np.ones((H, W), np.float32)
    color = np.zeros((H, W, 4), np.float32)
    prim = np.full((H, W), NONE, np.uint32)
    if not S["ref"]:
        return Result(depth, color, prim, 0, tris_in)
    S = {k: np.concatenate(v) for k, v in S.items()}
    X, Y, z, invw, bary = S["X"], S["Y"], S["z"].copy(), S["invw"].copy(), S["bary"].copy()
    area2 = _orient(X, Y, [z, invw, bary])

    # ---- coverage: fragments as (pixel, z, sub-triangle)
    px0 = np.maximum((X.min(1) - 128 + 255) >> 8, 0)
    px1 = np.minimum((X.max(1) - 128) >> 8, W - 1)
    py0 = np.maximum((Y.min(1) - 128 + 255) >> 8, 0)
    py1 = np.minimum((Y.max(1) - 128) >> 8, H - 1)
    live = (area2 != 0) & (px0 <= px1) & (py0 <= py1)
    b = [_bias(X[:, 1], Y[:, 1], X[:, 2], Y[:, 2]), _bias(X[:, 2], Y[:, 2], X[:, 0], Y[:, 0]), _bias(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1])]
    frag_pix, frag_z, frag_sub = [], [], []

    def sample(sel, px, py):
        """sel: sub-triangle indices [n]; px, py: [n] or [n, m] pixel coordinates"""
        ex = (lambda a: a[sel]) if px.ndim == 1 else (lambda a: a[sel][:, None])
        Xs, Ys = X[sel] if px.ndim == 1 else X[sel][:, None, :], Y[sel] if px.ndim == 1 else Y[sel][:, None, :]
        (e0, e1, e2), (w0, w1, w2) = _weights(Xs, Ys, ex(area2), px * 256 + 128, py * 256 + 128, dt)
        inside = (e0 + ex(b[0]) >= 0) & (e1 + ex(b[1]) >= 0) & (e2 + ex(b[2]) >= 0)
        zz = (ex(z[:, 0]) + w1 * (ex(z[:, 1]) - ex(z[:, 0]))) + w2 * (ex(z[:, 2]) - ex(z[:, 0]))
        with np.errstate(invalid="ignore"):
            keep = inside & (zz >= 0) & (zz < 1)
        subs = np.broadcast_to(sel if px.ndim == 1 else sel[:, None], px.shape)
        frag_pix.append((py * W + px)[keep]); frag_z.append(zz[keep]); frag_sub.append(subs[keep])

    small = live & (px1 - px0 < SMALL) & (py1 - py0 < SMALL)
    ids = np.nonzero(small)[0]
    for oy in range(SMALL):
        for ox in range(SMALL):
            sel = ids[(px0[ids] + ox <= px1[ids]) & (py0[ids] + oy <= py1[ids])]
            if sel.size:
                sample(sel, px0[sel] + ox, py0[sel] + oy)
    for i in np.nonzero(live & ~small)[0]:
        gy, gx = np.mgrid[py0[i]:py1[i] + 1, px0[i]:px1[i] + 1]
        sample(np.array([i]), gx.reshape(1, -1), gy.reshape(1, -1))
    pix, zz, sub = np.concatenate(frag_pix), np.concatenate(frag_z), np.concatenate(frag_sub)
    fragments = int(pix.size)
    if fragments == 0:
        return Result(depth, color, prim, 0, tris_in)
    order = np.lexsort((S["ref"][sub], zz, pix))  # LESS in primitive order: smallest z, then the earliest primitive
    first = np.ones(order.size, bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    win = order[first]
    wp_, wz, ws = pix[win], zz[win], sub[win]
    ys, xs = wp_ // W, wp_ % W
    depth[ys, xs] = np.abs(wz).astype(np.float32)
    prim[ys, xs] = (S["ref"][ws] >> 3).astype(np.uint32)

    # ---- resolve: attributes of the winning fragments, shading
    _, (w0, w1, w2) = _weights(X[ws], Y[ws], area2[ws], xs * 256 + 128, ys * 256 + 128, dt)
    pw = [w0 * invw[ws, 0], w1 * invw[ws, 1], w2 * invw[ws, 2]]
    tot = (pw[0] + pw[1]) + pw[2]
    n = ws.size
    attr = {k: np.zeros((n, 3, 3), dt) for k in ("wp", "wn", "vd")}  # the primitive's three vertices
    mat = {k: np.zeros((n, 3), dt) for k in ("ambient", "diffuse", "specular", "emission")}
    mat["shininess"], needs = np.zeros(n, dt), np.zeros(n, bool)
    for k, D in enumerate(inst_data):
        selk = np.nonzero(S["inst"][ws] == k)[0]
        if not selk.size:
            continue
        tri = S["tri"][ws][selk]
        vi = D["idx"][tri]
        for a in attr:
            attr[a][selk] = D[a][vi]
        mats = D["mesh"].get("materials") or [default_material()]
        mid = np.asarray(D["mesh"].get("material_ids") if D["mesh"].get("material_ids") is not None else np.zeros(D["idx"].shape[0]), np.int64)[tri]
        mid = np.where(mid >= len(mats), 0, mid)
        for f in ("ambient", "diffuse", "specular", "emission"):
            mat[f][selk] = np.array([np.asarray(mm[f], np.float32) for mm in mats], np.float32).astype(dt)[mid]
        mat["shininess"][selk] = np.array([np.float32(mm["shininess"]) for mm in mats], np.float32).astype(dt)[mid]
        needs[selk] = np.array([nl.need_shading(mm) for mm in mats], bool)[mid]
    bw = bary[ws]  # [n, vertex of the sub-triangle, weight]
    with np.errstate(all="ignore"):
        def interp(a):
            sv = [(bw[:, j, 0:1] * a[:, 0] + bw[:, j, 1:2] * a[:, 1]) + bw[:, j, 2:3] * a[:, 2] for j in range(3)]
            return ((sv[0] * pw[0][:, None] + sv[1] * pw[1][:, None]) + sv[2] * pw[2][:, None]) * (dt(1.0) / tot)[:, None]
        world, nrm_i, vdir = interp(attr["wp"]), interp(attr["wn"]), interp(attr["vd"])
        if lighting_mode == 0:
            col = (mat["emission"] + mat["ambient"]) + mat["diffuse"]
        else:
            lit = mat["emission"].copy()
            for L in (list(lights) if len(lights) else [nl.headlight(np.asarray(camera_pos, np.float32))]):
                nl._shade_direct(L, world, nrm_i, mat, vdir, lit, dt, False)
            col = np.where(needs[:, None], lit, mat["emission"])
    color[ys, xs, :3] = col.astype(np.float32)
    color[ys, xs, 3] = 1.0
    return Result(depth, color, prim, fragments, tris_in)


def boundary(prim):
    """pixels whose 8-neighbourhood in the primitive-id image holds another id or none"""
    p = np.pad(prim, 1, mode="edge")
    H, W = prim.shape
    out = np.zeros((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= p[dy:dy + H, dx:dx + W] != prim
    return out
