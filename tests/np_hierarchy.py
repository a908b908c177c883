"""What the two device-built hierarchies (k_bvh.hip, k_mesh_bvh.hip) must hold, stated in float64 from their contract and not from the
kernels' formulas.  The inputs are what the device holds, taken as exact fp32 values and lifted to float64: the splat planes in storage
order (centres, log-scales, quaternions (w, x, y, z), density), the mesh arrays, the instance matrices (row-major 4 x 4 as capi takes
them), and the fp32 parameters of the proxy (kernel_min_response, alpha_cull_threshold, the clamp 0.97f).

  ellipsoid_boxes   the exact AABB of the affine image of the proxy ellipsoid: A = mat3(M) R(q / |q|) diag(r exp(scale)), centre M p,
                    half extent sqrt(sum_j A_aj^2); r = the inverse of the kernel response at min(kmr [/ density], 0.97)
  splat_valid       a leaf iff density > alpha_cull and the box is finite (in fp32's range: the nodes are fp32)
  world_vertices    worldVertex's documented order of operations in fp32 (the ONE restated formula besides the cross product: the leaf
                    rule is defined on these float values), and the float64 transform with the bound of its difference
  triangle_valid    a leaf iff the three world vertices are finite and the float cross product, without contraction, is not (0, 0, 0)
  tree_shape        level_count[0] = leaves, level_count[l] = ceil(level_count[l - 1] / 8) down to 1, offsets = running sums
  morton / near_cell_boundary   the 30-bit code of a leaf centre in the build's frame, in float64, and which leaves may floor differently
                    in fp32
  check_nodes / check_order     the assertions every download must pass, shared by the GPU test and the CPU emulation"""
import numpy as np

DEGREES = (0, 1, 2, 3, 4, 5, 8)          # what validateTrace accepts (shaderio.h:112-119)
CLAMP = float(np.float32(0.97))          # the device's constant is the fp32 value
S0 = 0.329630334487                      # degree 0: response = max(1 - S0 d, 0)
EPS = 2.0 ** -24                         # half an ulp of 1.0f: the unit of the bounds below
FMAX = float(np.finfo(np.float32).max)
MAX_LEVELS = 11
NEAR = 2.0 ** -10                        # a quantised coordinate this close to a cell boundary may floor differently in fp32


def response(degree, d):
    """the generalised-Gaussian response at the canonical DISTANCE d (particleRayMaxKernelResponse, threedgrt.h.slang:83-127)"""
    d = np.asarray(d, np.float64)
    if degree == 0:
        return np.maximum(1.0 - S0 * d, 0.0)
    return np.exp(-4.5 / 3.0 ** degree * d ** degree)


def proxy_threshold(kmr, density, adaptive, dtype=np.float64):
    kmr, density = dtype(np.float32(kmr)), np.asarray(density, np.float32).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.minimum(kmr / density if adaptive else np.full_like(density, kmr), dtype(np.float32(0.97)))


def proxy_radius(degree, thr, dtype=np.float64):
    """the canonical distance at which response(degree, .) falls to thr"""
    thr = np.asarray(thr, dtype)
    if degree == 0:
        return (1 - thr) / dtype(S0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.log(thr) / (dtype(-4.5) / dtype(3) ** degree)) ** (dtype(1) / dtype(degree))


def rotations(q, dtype=np.float64):
    """R [n, 3, 3] of the normalised quaternions q [n, 4] = (w, x, y, z): world = R canonical"""
    q = np.asarray(q, np.float32).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = q / np.sqrt((q * q).sum(1, keepdims=True))
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def ellipsoid_boxes(centers, scales, quats, density, M, degree, kmr, adaptive, dtype=np.float64):
    """-> (c [n, 3], h [n, 3], T [n, 3]) float64: centre and half extent of the exact box, and T_a = |M_a0 p0| + |M_a1 p1| + |M_a2 p2| +
    |M_a3|, the sum of the absolute terms of the centre's transform (the magnitude its fp32 evaluation rounds at).  dtype: the
    precision it is evaluated in (np.longdouble: the reference of the reference, test_hierarchy_cpu.py)"""
    p = np.asarray(centers, np.float32).astype(dtype).reshape(-1, 3)
    M = np.asarray(M, np.float32).astype(dtype)
    r = proxy_radius(degree, proxy_threshold(kmr, density, adaptive, dtype), dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.exp(np.asarray(scales, np.float32).astype(dtype).reshape(-1, 3)) * r[:, None]
        A = (M[:3, :3][None, :, :, None] * rotations(quats, dtype)[:, None, :, :]).sum(2) * s[:, None, :]
        h = np.sqrt((A * A).sum(2))
        c = p @ M[:3, :3].T + M[:3, 3]
        T = np.abs(p) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3])
    return c, h, T


def splat_valid(density, alpha_cull, c, h):
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(c).all(1) & np.isfinite(h).all(1) & (np.abs(c - h) <= FMAX).all(1) & (np.abs(c + h) <= FMAX).all(1)
        return (np.asarray(density, np.float32) > np.float32(alpha_cull)) & fin


def scene_splats(sets, degree, kmr, adaptive, alpha_cull):
    """sets: [(dict(centers, scales, quats, density) in storage order, M)] in instance order -> dict of the concatenated c, h, T, valid"""
    parts = []
    for a, M in sets:
        c, h, T = ellipsoid_boxes(a["centers"], a["scales"], a["quats"], a["density"], M, degree, kmr, adaptive)
        parts.append((c, h, T, splat_valid(a["density"], alpha_cull, c, h)))
    if not parts:
        z = np.zeros((0, 3))
        return dict(c=z, h=z, T=z, valid=np.zeros(0, bool))
    return dict(zip(("c", "h", "T", "valid"), (np.concatenate(x) for x in zip(*parts))))


def world_vertices(positions, M):
    """(w32 [V, 3] fp32 = ((x m0 + y m4) + z m8) + m12 with every product and sum rounded where it stands; w64 the float64 transform;
    bound [V, 3] = 4 * 2^-24 * (|x m0| + |y m4| + |z m8| + |m12|), which holds the difference of the two)"""
    p = np.asarray(positions, np.float32).reshape(-1, 3)
    M = np.asarray(M, np.float32)
    w32 = np.empty_like(p)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(3):
            w32[:, r] = ((p[:, 0] * M[r, 0] + p[:, 1] * M[r, 1]) + p[:, 2] * M[r, 2]) + M[r, 3]
        pd, Md = p.astype(np.float64), M.astype(np.float64)
        w64 = pd @ Md[:3, :3].T + Md[:3, 3]
        bound = 4.0 * EPS * (np.abs(pd) @ np.abs(Md[:3, :3]).T + np.abs(Md[:3, 3]))
    return w32, w64, bound


def triangle_valid(tri32):
    """tri32 [N, 3, 3] fp32 world vertices"""
    e1, e2 = tri32[:, 1] - tri32[:, 0], tri32[:, 2] - tri32[:, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    return np.isfinite(tri32).all((1, 2)) & np.isfinite(c).all(1) & ~(c == 0).all(1)


def scene_triangles(meshes):
    """meshes: dicts of mesh_cases.mesh -> dict(tri32 [N, 3, 3], tri64, bound, inst [N], mat [N], valid [N]); N counts every instance's
    triangles in creation order, visible or not"""
    t32, t64, bd, inst, mat = [], [], [], [], []
    for k, m in enumerate(meshes):
        M = np.eye(4, dtype=np.float32) if m.get("transform") is None else m["transform"]
        w32, w64, b = world_vertices(m["positions"], M)
        idx = np.asarray(m["indices"]).reshape(-1, 3).astype(np.int64)
        t32.append(w32[idx]), t64.append(w64[idx]), bd.append(b[idx])
        inst.append(np.full(idx.shape[0], k, np.uint32))
        mid = m.get("material_ids")
        mat.append(np.zeros(idx.shape[0], np.uint32) if mid is None else np.asarray(mid, np.uint32))
    if not t32:
        z = np.zeros((0, 3, 3))
        return dict(tri32=z.astype(np.float32), tri64=z, bound=z, inst=np.zeros(0, np.uint32), mat=np.zeros(0, np.uint32), valid=np.zeros(0, bool))
    tri32 = np.concatenate(t32)
    return dict(tri32=tri32, tri64=np.concatenate(t64), bound=np.concatenate(bd), inst=np.concatenate(inst), mat=np.concatenate(mat),
                valid=triangle_valid(tri32))


def tree_shape(leaves):
    """-> (levels, total_nodes, level_offset[11], level_count[11])"""
    off, cnt = np.zeros(MAX_LEVELS, np.uint32), np.zeros(MAX_LEVELS, np.uint32)
    levels, total, c = 0, 0, int(leaves)
    while c > 0:
        assert levels < MAX_LEVELS
        off[levels], cnt[levels] = total, c
        total += c
        levels += 1
        if c == 1:
            break
        c = (c + 7) // 8
    return levels, total, off, cnt


def quantised(centre, box_lo, box_inv_ext):
    """the centre's coordinates in the Morton frame, [n, 3] in [0, 1023], float64"""
    lo, inv = np.asarray(box_lo, np.float32).astype(np.float64), np.asarray(box_inv_ext, np.float32).astype(np.float64)
    return np.clip((np.asarray(centre, np.float64) - lo) * inv, 0.0, 1.0) * 1023.0


def morton(q):
    qi = np.floor(q).astype(np.int64)
    code = np.zeros(qi.shape[0], np.int64)
    for b in range(10):
        for ax in range(3):
            code |= ((qi[:, ax] >> b) & 1) << (3 * b + ax)
    return code


def near_cell_boundary(q):
    """a leaf with a coordinate within NEAR of a cell boundary at which fp32 and float64 can floor differently (the clamp at 0 leaves
    no such boundary below the first cell)"""
    n = np.rint(q)
    return ((np.abs(q - n) < NEAR) & (n >= 1)).any(1)


def f64(bits):
    """uint32 raw bits -> the fp32 values lifted to float64"""
    return np.ascontiguousarray(bits, np.uint32).view(np.float32).astype(np.float64)


def check_nodes(info, nodes, leaves_expected):
    """the hard assertions on info and the node array (uint32 [total_nodes, 8] raw bits) that need no geometry: the tree's shape, no
    NaN, the .w words, every upper node bit for bit the min / max of its children"""
    levels, total, off, cnt = tree_shape(leaves_expected)
    assert (info["levels"], info["total_nodes"], info["leaves"]) == (levels, total, leaves_expected), (info, levels, total, leaves_expected)
    assert np.array_equal(info["level_offset"], off) and np.array_equal(info["level_count"], cnt)
    assert nodes.shape == (total, 8)
    v = nodes.view(np.float32)
    assert not np.isnan(v[:, [0, 1, 2, 4, 5, 6]]).any()
    assert not nodes[:, 7].any() and not nodes[int(cnt[0]):, 3].any()
    for l in range(1, levels):
        below = v[int(off[l - 1]):int(off[l - 1]) + int(cnt[l - 1])]
        pad = (-below.shape[0]) % 8
        lo = np.concatenate([below[:, 0:3], np.full((pad, 3), np.inf, np.float32)]).reshape(-1, 8, 3).min(1)
        hi = np.concatenate([below[:, 4:7], np.full((pad, 3), -np.inf, np.float32)]).reshape(-1, 8, 3).max(1)
        mine = v[int(off[l]):int(off[l]) + int(cnt[l])]
        assert lo.tobytes() == np.ascontiguousarray(mine[:, 0:3]).tobytes() and hi.tobytes() == np.ascontiguousarray(mine[:, 4:7]).tobytes(), l


def check_order(centre, box_lo, box_inv_ext, ids=None):
    """level 0's order: float64 codes non-decreasing except for pairs with a leaf near a cell boundary; among equal, unexcused codes the
    ids (splats: storage ids) ascend.  centre [leaves, 3] in leaf order.  -> (excused pairs, pairs)"""
    n = centre.shape[0]
    if n < 2:
        return 0, 0
    q = quantised(centre, box_lo, box_inv_ext)
    code, near = morton(q), near_cell_boundary(q)
    excused = near[:-1] | near[1:]
    assert (code[1:] >= code[:-1])[~excused].all(), "leaves out of Morton order"
    if ids is not None:
        tie = (code[1:] == code[:-1]) & ~excused
        assert (ids[1:].astype(np.int64) > ids[:-1].astype(np.int64))[tie].all(), "equal codes not in ascending id (the sort is stable)"
    return int(excused.sum()), n - 1


def splat_containment(nodes, ref):
    """leaf boxes against the float64 ellipsoid boxes.  nodes: the download; ref: scene_splats().  -> dict(ids, margin [leaves, 6] =
    how far each face lies outside the exact box (negative: the exact box sticks out), h, bound = the tightness bound per face)"""
    nl = int(ref["valid"].sum())
    ids = nodes[:nl, 3].astype(np.int64)
    lo, hi = f64(nodes[:nl, 0:3]), f64(nodes[:nl, 4:7])
    c, h, T = ref["c"][ids], ref["h"][ids], ref["T"][ids]
    margin = np.concatenate([(c - h) - lo, hi - (c + h)], 1)
    bound = np.tile(32.0 * EPS * (h + T), (1, 2))
    return dict(ids=ids, margin=margin, h=np.tile(h, (1, 2)), bound=bound)
