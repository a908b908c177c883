"""Which splats leave a fragment at which pixel: a float64 restatement of the fragment rule of
shaders/threedgs_raster.frag.slang:236-262 on top of np_reference.project (per splat) and np_reference.dist_cull (the dist stage).

With the opacity gaussian disabled every fragment has alpha 1 and the only rule is A <= 8, so the additive alpha of a frame is the
integer NUMBER of fragments of the pixel: `count` below.  A fragment whose A (or, with the gaussian on, whose alpha) lies within
`delta` of its threshold may fall on either side in fp32: such pixels are `borderline`, and `borderline_count` says by how many
fragments they may differ.

Test infrastructure only."""
import numpy as np

ALPHA_MIN = 1.0 / 255.0


class Fragments:
    """count[H,W] int32, alpha_sum[H,W] float64, borderline[H,W] bool, borderline_count[H,W] int32, and the table of the splats that
    were drawn (global ids: instances concatenated in creation order), which covering() evaluates at one pixel"""

    def __init__(self, W, H, table, gaussian, delta, depth):
        self.W, self.H, self.table, self.gaussian, self.delta, self.depth = W, H, table, gaussian, delta, depth
        self.count = np.zeros((H, W), np.int32)
        self.alpha_sum = np.zeros((H, W), np.float64)
        self.borderline_count = np.zeros((H, W), np.int32)

    @property
    def borderline(self):
        return self.borderline_count > 0

    def covering(self, x, y):
        """[(global id, A, alpha, borderline)] of the fragments (and near misses) of pixel (x, y), in id order"""
        t = self.table
        A, alpha = _eval(t["c"], t["b1"], t["b2"], t["opacity"], x + 0.5, y + 0.5, self.gaussian)
        keep, edge = _rule(A, alpha, self.gaussian, self.delta, _turn(t["c"], t["b1"], t["b2"], t["theta"], x + 0.5, y + 0.5))
        if self.depth is not None:
            seen = t["z"] <= self.depth[y, x]
            keep, edge = keep & seen, edge & seen
        return [(int(t["id"][i]), float(A[i]), float(alpha[i]), bool(edge[i])) for i in np.flatnonzero(keep | edge)]


def _eval(c, b1, b2, opacity, px, py, gaussian):
    """A = dot(fragPos, fragPos) (frag.slang:236) and the fragment's alpha; c, b1, b2 broadcast against the pixel centres px, py"""
    dx, dy = px - c[..., 0], py - c[..., 1]
    u = (dx * b1[..., 0] + dy * b1[..., 1]) / (b1[..., 0] ** 2 + b1[..., 1] ** 2)  # pixel = centre + u b1 + v b2, b1 orthogonal to b2
    v = (dx * b2[..., 0] + dy * b2[..., 1]) / (b2[..., 0] ** 2 + b2[..., 1] ** 2)
    A = 8.0 * (u * u + v * v)
    alpha = np.exp(-0.5 * A) * opacity if gaussian else np.ones_like(A)
    return A, alpha


def _turn(c, b1, b2, theta, px, py):
    """how far A moves when the basis is turned by theta (radians, 0 = not at all): with u = d.e1 / l1, v = d.e2 / l2 a turn
    gives du = v l2 / l1, dv = -u l1 / l2 per radian, so dA = 16 u v (l2 / l1 - l1 / l2) theta"""
    dx, dy = px - c[..., 0], py - c[..., 1]
    n1, n2 = b1[..., 0] ** 2 + b1[..., 1] ** 2, b2[..., 0] ** 2 + b2[..., 1] ** 2
    u, v = (dx * b1[..., 0] + dy * b1[..., 1]) / n1, (dx * b2[..., 0] + dy * b2[..., 1]) / n2
    return np.abs(16.0 * u * v * (np.sqrt(n2 / n1) - np.sqrt(n1 / n2))) * theta


def _rule(A, alpha, gaussian, delta, dA=0.0):
    """(fragment exists, fragment is within delta — plus dA, what the basis direction leaves open — of a threshold)"""
    keep = A <= 8.0
    edge = np.abs(A - 8.0) <= 8.0 * delta + dA
    if gaussian:
        keep &= alpha > ALPHA_MIN
        edge |= (A <= 8.0 * (1.0 + delta) + dA) & (np.abs(alpha * 255.0 - 1.0) <= delta + 127.5 * alpha * dA)
    return keep, edge


def basis_turn(pr, ulps):
    """The angle (radians) by which an fp32 evaluation of the reference's extent basis may be off, per splat; 0 for ulps = 0.
    threedgs.h.slang:84-100 takes the eigenvector as normalize((b, ev1 - a)) (x := 1 where |b| < 0.001).  For a nearly axis-aligned
    ellipse ev1 - a is the difference of two nearly equal numbers: whatever its true size, fp32 leaves it an absolute error of
    `ulps` steps of ev1, i.e. the direction an error of ulps * 2^-23 * ev1 / |(b, ev1 - a)| — the reference's shader, the oracle and
    the kernel each land somewhere inside.  A splat whose |b| is that close to 0.001 may take the other branch: any direction."""
    a, b, ev1 = pr["cov2"][:, 0], pr["cov2"][:, 1], pr["ev"][:, 0]
    if not ulps:
        return np.zeros(a.shape[0])
    step = ulps * 2.0 ** -23 * np.maximum(ev1, np.abs(a))
    x = np.where(np.abs(b) < 0.001, 1.0, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = step / np.hypot(x, ev1 - a)
    theta = np.where(np.abs(np.abs(b) - 0.001) <= step, np.pi, theta)
    return np.minimum(np.nan_to_num(theta, nan=np.pi, posinf=np.pi), np.pi)


def splat_table(projected, survivors, key_depth=None, basis_ulps=0):
    """the splats that are drawn, over all instances: projected = [np_reference.project(...)] and survivors = [dist-stage mask] per
    instance, key_depth = the key depth per GLOBAL id (only needed with an occluder), basis_ulps: see basis_turn"""
    rows, off = [], 0
    for pr, sv in zip(projected, survivors):
        n = pr["valid"].shape[0]
        idx = np.flatnonzero(pr["valid"] & np.asarray(sv, bool))
        rows.append(dict(id=idx + off, c=pr["center_px"][idx], b1=pr["b1"][idx], b2=pr["b2"][idx], opacity=pr["rgba"][idx, 3],
                         theta=basis_turn(pr, basis_ulps)[idx]))
        off += n
    t = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
    t["z"] = np.zeros(t["id"].shape[0]) if key_depth is None else np.asarray(key_depth, np.float64)[t["id"]]
    return t


def fragments(projected, survivors, W, H, gaussian=False, delta=1e-4, depth=None, key_depth=None, basis_ulps=0):
    """projected / survivors: per instance (see splat_table).  depth: occluder depth image [H,W] or None; a splat is then drawn at
    a pixel only where its key depth (key_depth[global id]) is <= depth.  basis_ulps > 0: a fragment that a turn of its splat's basis
    by basis_turn() could carry across a threshold is borderline too.  Returns Fragments."""
    t = splat_table(projected, survivors, key_depth if depth is not None else None, basis_ulps)
    D = None if depth is None else np.asarray(depth, np.float64)
    out = Fragments(W, H, t, gaussian, delta, D)
    ex = np.abs(t["b1"][:, 0]) + np.abs(t["b2"][:, 0])  # the quad's bounding box (A <= 8 lies inside the quad)
    ey = np.abs(t["b1"][:, 1]) + np.abs(t["b2"][:, 1])
    turned = t["theta"] > 0   # (a turned quad stays inside the box of half size l1 + l2)
    reach = np.hypot(t["b1"][:, 0], t["b1"][:, 1]) + np.hypot(t["b2"][:, 0], t["b2"][:, 1])
    ex, ey = np.where(turned, reach, ex), np.where(turned, reach, ey)
    pad = 1.0 + 8.0 * delta
    x0 = np.maximum(0, np.floor(t["c"][:, 0] - pad * ex - 0.5)).astype(np.int64)
    x1 = np.minimum(W - 1, np.ceil(t["c"][:, 0] + pad * ex - 0.5)).astype(np.int64)
    y0 = np.maximum(0, np.floor(t["c"][:, 1] - pad * ey - 0.5)).astype(np.int64)
    y1 = np.minimum(H - 1, np.ceil(t["c"][:, 1] + pad * ey - 0.5)).astype(np.int64)
    # a stack of identical splats is evaluated once.  `row` below holds every per-splat quantity the loop body reads (centre, basis,
    # opacity, theta, depth; the window follows from them): extend it if another one enters the loop
    same, last = None, None
    for i in np.flatnonzero((x1 >= x0) & (y1 >= y0)):
        row = (t["c"][i].tobytes(), t["b1"][i].tobytes(), t["b2"][i].tobytes(), float(t["opacity"][i]), float(t["theta"][i]), float(t["z"][i]))
        if row != same:
            yy, xx = np.mgrid[y0[i]:y1[i] + 1, x0[i]:x1[i] + 1]
            A, alpha = _eval(t["c"][i], t["b1"][i], t["b2"][i], t["opacity"][i], xx + 0.5, yy + 0.5, gaussian)
            keep, edge = _rule(A, alpha, gaussian, delta, _turn(t["c"][i], t["b1"][i], t["b2"][i], t["theta"][i], xx + 0.5, yy + 0.5) if t["theta"][i] else 0.0)
            win = (slice(y0[i], y1[i] + 1), slice(x0[i], x1[i] + 1))
            if D is not None:
                seen = t["z"][i] <= D[win]
                keep, edge = keep & seen, edge & seen
            same, last = row, (keep, edge, alpha, win)
        keep, edge, alpha, win = last
        out.count[win] += keep
        out.alpha_sum[win] += np.where(keep, alpha, 0.0)
        out.borderline_count[win] += edge
    return out


def where(x, y):
    """the compositor's names for the place of pixel (x, y): its 32x16-px region and the 16x8-px quarter (wave) inside it"""
    return f"region ({x // 32},{y // 16}) quarter ({(x % 32) // 16},{(y % 16) // 8})"


def describe(ref, got, expected, bad, limit=5, ids=12):
    """the first few pixels of the mask `bad`: the value the frame holds, the expected one, where the pixel lies and which splats
    cover it — enough to start looking from"""
    ys, xs = np.nonzero(bad)
    lines = [f"{ys.size} pixels differ; the first {min(limit, ys.size)}:"]
    for y, x in list(zip(ys, xs))[:limit]:
        cov = ref.covering(int(x), int(y))
        txt = ", ".join(f"{i}{'*' if e else ''}(A={A:.5f})" for i, A, _, e in cov[:ids]) + (" ..." if len(cov) > ids else "")
        lines.append(f"  pixel ({x},{y}) {where(int(x), int(y))}: frame {got[y, x]!r}, expected {expected[y, x]!r}, "
                     f"{ref.borderline_count[y, x]} borderline; {len(cov)} covering splats (* = borderline): {txt}")
    return "\n".join(lines)
