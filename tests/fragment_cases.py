"""The scenes of the fragment-count tests, shared by tests/test_fragments_cpu.py (which holds the oracle to the float64 count of
tests/np_fragments.py and establishes the borderline share and EPS_FRAG from the CPU side alone), tests/test_gpu_fragments.py (which
holds the compositor to the same counts), tests/_child_fragments.py and tests/_child_fragment_grids.py.

The compositor works on 32x16-px regions (one workgroup), 16x8-px quarters (one wave) and, in the additive-alpha mode, 128x64-px
bins (one depth-ordered list each).  Every case is chosen for a place where a fragment can get lost or counted twice."""
import functools

import numpy as np

from vk_gaussian_splatting_amd import synth
import np_fragments as nf
import np_reference as npr

# A fragment within DELTA (relative) of A = 8, or within DELTA of alpha * 255 = 1, may fall on either side in fp32: a CONDITION on the
# comparison, not a measurement.  fp32 evaluation of q about the region centre (operands <= 16 px) sits a few 1e-6 relative from the
# float64 value; 1e-4 is about forty times that.
DELTA = 1e-4
# At most this share of a case's pixels may be borderline, so that the mask cannot hide a failure (test_fragments_cpu.py shows it
# for every case from the restatement alone).
BORDERLINE_CAP = 0.01
# The oracle's worst per-fragment alpha error against float64 over the gaussian cases (EPS_CASES below): MEASURED by
# test_fragments_cpu.py::test_eps_frag_is_the_oracles_own_error (each splat drawn alone by the oracle into an fp32 additive-alpha
# target, compared fragment by fragment with np_fragments; the test fails if the measurement leaves [EPS_FRAG / 2, EPS_FRAG]).
EPS_FRAG = 1.0e-4   # measured 8.93e-5 (opaque_gaussian), 7.90e-5 (dense)

FOV, NEAR, FAR = 55.0, 0.1, 2000.0
EYE = (3.5, 1.2, 0.8)
W, H = 333, 217   # no multiple of 16 or 32: 3 x 4 bins of 128x64 px, ragged last region column and row


def lookat(eye, c, up=(0, 1, 0)):
    eye, c, up = (np.asarray(a, np.float32) for a in (eye, c, up))
    f = c - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    V = np.eye(4, dtype=np.float32)
    V[0, :3], V[1, :3], V[2, :3] = s, u, -f
    V[0, 3], V[1, 3], V[2, 3] = -s @ eye, -u @ eye, f @ eye
    return V


def persp(tan_half_fov, aspect, n, f):
    t = np.float64(tan_half_fov)
    P = np.zeros((4, 4), np.float32)
    P[0, 0], P[1, 1], P[2, 2], P[3, 2], P[2, 3] = 1 / (aspect * t), 1 / t, f / (n - f), -1, -(f * n) / (f - n)
    return P


def orbit_camera(w, h):
    return lookat(EYE, (0, 0, 0)), persp(np.tan(np.radians(FOV) / 2), w / h, NEAR, FAR), np.asarray(EYE, np.float32)


def _trs(scale, axis, angle, t):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = R @ np.diag(scale)
    M[:3, 3] = t
    return M.astype(np.float32)


SECOND_INSTANCE = _trs([0.8, 1.2, 1.0], [0.1, 1.0, 0.3], -0.6, [1.0, 0.1, -0.5])


# ---- hand-made: splats placed in window space ------------------------------------------------------------------------------------
HW, HH = 192, 112   # 6 x 7 regions, 2 x 2 bins of 128x64 px (both ragged)
HAND_EYE_Z = 5.0
STACKS = [(449, (48.0, 88.0), 4.0), (512, (112.0, 88.0), 4.2), (513, (144.0, 24.0), 4.4)]  # (splats, centre px, distance)


def hand_camera():
    """eye on +z looking down -z, tan(fov / 2) = 1/2: the focal length is HH pixels, one world unit at distance d is HH / d pixels"""
    eye = np.array([0.0, 0.0, HAND_EYE_Z], np.float32)
    return lookat(eye, (0, 0, 0)), persp(0.5, HW / HH, 0.1, 100.0), eye


def hand_made(clamped=True):
    """flat discs facing the camera: (centre px, sigma px along / across, angle, distance) -> position, log scale, rotation about z"""
    sp = []   # (x px, y px, sigma1 px, sigma2 px, angle, distance)
    sig = [(1.3, 1.3), (2.7, 1.1), (1.9, 3.1)]
    # centres exactly on region (32x16), quarter (16x8) and bin (128x64) edges, and half a pixel to either side
    for ex, ey in ((32.0, 16.0), (48.0, 24.0), (128.0, 64.0)):
        for i, dx in enumerate((0.0, -0.5, 0.5)):
            for j, dy in enumerate((0.0, -0.5, 0.5)):
                s1, s2 = sig[(i + j) % 3]
                sp.append((ex + dx, ey + dy, s1, s2, 0.37 * (i + 3 * j), 5.0))
    # thin ellipses at 45 degrees that cross a region corner: the footprint box covers the regions around the corner, the ellipse does
    # not reach most of them (what the bound in the ellipse's own frame is for)
    for cx, cy, ang, off in ((64.0, 32.0, np.pi / 4, 0.9), (64.0, 32.0, -np.pi / 4, -1.3), (96.0, 48.0, np.pi / 4, 2.1), (96.0, 80.0, -np.pi / 4, 0.2)):
        sp.append((cx + 7.0 + off * 0.7071, cy + 7.0 * np.sign(ang) - off * 0.7071 * np.sign(ang), 9.0, 1.0, ang, 5.2))
    # larger than the frame, both axes at the 2048-px clamp.  (Not a thin one: the smaller eigenvalue of a strongly anisotropic
    # Sigma2D is a difference of two large fp32 numbers in every implementation, the reference's shader included — at 2000 x 5 px
    # it is good to 1e-2, and A with it.  The ellipses of this case stay below an eigenvalue ratio of 100.)
    if clamped:
        sp.append((90.0, 60.0, 900.0, 800.0, 0.17, 6.0))
    # centres outside the frame whose footprints reach in (the dist stage keeps a centre up to 20 % outside)
    sp.append((-6.0, 40.0, 5.0, 3.0, 0.3, 5.0))
    sp.append((150.0, HH + 5.0, 4.0, 4.5, 1.1, 5.0))
    # sub-pixel splats, on a pixel centre and between four pixel centres: the 0.3-px^2 dilation is nearly all of their extent, and the
    # 0.1 floor under the discriminant (threedgs.h.slang:79) leaves them a short axis of 0.44 px.  (Below sigma = 0.127 px that floor
    # makes the smaller eigenvalue negative and the splat is culled.)
    sp.append((70.5, 40.5, 0.2, 0.2, 0.0, 5.0))
    sp.append((90.0, 50.0, 0.2, 0.2, 0.0, 5.0))
    # identical footprints stacked over one region, nearest in their bins' lists: 449 = MGS_SUM_CAP + 1 staged records,
    # 512 = one stage-A round of 256 * MGS_SUM_ENTRIES entries, 513 = one more
    for n, (cx, cy), d in STACKS:
        sp += [(cx, cy, 1.9, 1.6, 0.5, d)] * n
    return _discs(sp, HW, HH, HAND_EYE_Z)


def _discs(sp, w, h, eye_z):
    """(x px, y px, sigma1 px, sigma2 px, angle, distance) rows -> the arrays of a splat set: flat discs facing a camera on +z whose
    focal length is h pixels (hand_camera, grid_camera)"""
    a = np.asarray(sp, np.float64)
    d = a[:, 5]
    unit = d / h   # world units per pixel at distance d
    pos = np.stack([(a[:, 0] - w / 2) * unit, (a[:, 1] - h / 2) * unit, eye_z - d], 1)
    scale = np.log(np.stack([a[:, 2] * unit, a[:, 3] * unit, np.full(d.shape, 1e-4)], 1))
    rot = np.stack([np.cos(a[:, 4] / 2), np.zeros_like(d), np.zeros_like(d), np.sin(a[:, 4] / 2)], 1)
    n = a.shape[0]
    r = np.random.default_rng(9)
    return dict(positions=pos.astype(np.float32), f_dc=r.standard_normal((n, 3)).astype(np.float32), f_rest=np.zeros((n, 0), np.float32),
                opacity=np.full(n, 2.0, np.float32), scale=scale.astype(np.float32), rotation=rot.astype(np.float32))


# ---- bin grids: one frame per regime of the binning stage (k_dbin_count / k_dbin_scan / k_dbin_emit, the record path of k_bin) ----
GRID_EYE_Z = 5.0
OVERSIZED = (900.0, 800.0, 0.17)   # sigma px along / across, angle: both axes at the 2048-px clamp, as in hand_made


def grid_camera(w, h):
    """hand_camera for a frame of w x h px: the focal length is h pixels"""
    eye = np.array([0.0, 0.0, GRID_EYE_Z], np.float32)
    return lookat(eye, (0, 0, 0)), persp(0.5, w / h, 0.1, 100.0), eye


def _box(s1, s2, angle):
    """half width and half height in px of the footprint box of a disc (sigma px along / across, angle), as the reference builds its
    extent basis (threedgs.h.slang:60-121): 0.3 px^2 of dilation, and the 0.1 floor under the discriminant, which gives a small round
    splat axes of sqrt(8 (sigma^2 + 0.3 +- 0.316)) along (1, 0.316) and across"""
    c, n = np.cos(angle), np.sin(angle)
    a, b, d = s1 * s1 * c * c + s2 * s2 * n * n + 0.3, (s1 * s1 - s2 * s2) * c * n, s1 * s1 * n * n + s2 * s2 * c * c + 0.3
    half = 0.5 * (a + d)
    t = np.sqrt(max(0.1, half * half - (a * d - b * b)))
    ev1, ev2 = half + t, half - t
    e = np.array([1.0 if abs(b) < 0.001 else b, ev1 - a])
    e /= np.hypot(*e)
    l1, l2 = min(np.sqrt(8.0 * ev1), 2048.0), min(np.sqrt(8.0 * ev2), 2048.0)
    return float(np.hypot(e[0] * l1, e[1] * l2)), float(np.hypot(e[1] * l1, e[0] * l2))


def grid_case(bins_x, bins_y, bin_w, bin_h, ragged):
    """A frame of bins_x x bins_y bins of bin_w x bin_h px (ragged: 5 px narrower and 3 px lower, or a (dw, dh) pair: the last bin,
    region column and tile row are partial) with flat camera-facing discs placed for the binning stage: a splat inside each of a
    bin (at its centre, and three more layers off it), splats on bin corners and edges and half a pixel to either side
    (the coded 2x1, 1x2, 2x2 rectangles) and footprints that end between the last pixel centre of a bin and the first of the next,
    escapes (3x1, 1x3, 3x3, a rectangle over every bin column, one over every bin row, one splat larger than the frame) and centres
    outside the frame on all four sides.  Every group lies at a distance of its own.  Sizes scale with the bins (bin_h / 16).
    Returns dict(arrays, W, H, bins, bin_px, tags: group name -> splat indices)."""
    cut = (5, 3) if ragged is True else (tuple(ragged) if ragged else (0, 0))
    w, h = bins_x * bin_w - cut[0], bins_y * bin_h - cut[1]
    s, nb = bin_h / 16.0, bins_x * bins_y
    sp, tags = [], {}

    def add(tag, *rows):
        tags.setdefault(tag, []).extend(range(len(sp), len(sp) + len(rows)))
        sp.extend(rows)

    def mid_x(i):   # the centre of what the frame holds of bin column i
        return (i * bin_w + min((i + 1) * bin_w, w)) / 2.0

    def mid_y(j):
        return (j * bin_h + min((j + 1) * bin_h, h)) / 2.0

    # inside every bin (layer 0: at its centre, one bin each), and three more layers a fifth of a bin off the centre, which reach
    # into the neighbours: four waves of rounds on the larger grids, and a second chunk on those of 256 bins and more
    sig = [(1.6, 1.6), (2.2, 1.2), (1.4, 2.3)]
    for layer, (fx, fy) in enumerate(((0.0, 0.0), (0.22, 0.2), (-0.22, 0.15), (0.18, -0.2))):
        for b in range(nb):
            s1, s2 = sig[(b + layer) % 3]
            add("inside" if layer == 0 else "layers", (mid_x(b % bins_x) + fx * bin_w, mid_y(b // bins_x) + fy * bin_h, s1 * s, s2 * s,
                                                       0.3 + 0.31 * ((b + layer) % 4), 5.0 - 0.02 * layer))
    # bin corners: 2x2
    sig = [(1.3, 1.3), (2.7, 1.1), (1.9, 3.1)]
    corners = sorted({(i, j) for i, j in ((1, 1), (bins_x - 1, bins_y - 1), (bins_x // 2, bins_y // 2)) if 1 <= i < bins_x and 1 <= j < bins_y})
    for ci, cj in corners:
        for i, dx in enumerate((0.0, -0.5, 0.5)):
            for j, dy in enumerate((0.0, -0.5, 0.5)):
                s1, s2 = sig[(i + j) % 3]
                add("corner", (ci * bin_w + dx, cj * bin_h + dy, s1 * s, s2 * s, 0.37 * (i + 3 * j), 5.1))
    # bin edges: 2x1 and 1x2, and footprints that end 0.25 px short of / 0.75 px past the pixel centres on either side of an edge
    lx, ly = _box(1.3 * s, 1.3 * s, 0.0)
    if bins_x >= 2:
        for i in sorted({1, bins_x - 1}):
            for dx in (0.0, -0.5, 0.5):
                add("edge_x", (i * bin_w + dx, mid_y(bins_y // 2), 1.3 * s, 1.3 * s, 0.0, 5.2))
        e, y = float(bin_w), mid_y(bins_y - 1)
        add("ends_x_1", (e - lx - 0.25, y, 1.3 * s, 1.3 * s, 0.0, 5.25), (e + lx + 0.25, y, 1.3 * s, 1.3 * s, 0.0, 5.25))
        add("ends_x_2", (e - lx + 0.75, y, 1.3 * s, 1.3 * s, 0.0, 5.25), (e + lx - 0.75, y, 1.3 * s, 1.3 * s, 0.0, 5.25))
    if bins_y >= 2:
        for j in sorted({1, bins_y - 1}):
            for dy in (0.0, -0.5, 0.5):
                add("edge_y", (mid_x(bins_x // 2), j * bin_h + dy, 1.3 * s, 1.3 * s, 0.0, 5.3))
        e, x = float((bins_y - 1) * bin_h), mid_x(bins_x - 1)
        add("ends_y_1", (x, e - ly - 0.25, 1.3 * s, 1.3 * s, 0.0, 5.35), (x, e + ly + 0.25, 1.3 * s, 1.3 * s, 0.0, 5.35))
        add("ends_y_2", (x, e - ly + 0.75, 1.3 * s, 1.3 * s, 0.0, 5.35), (x, e + ly - 0.75, 1.3 * s, 1.3 * s, 0.0, 5.35))
    # escapes (more than 2 x 2 bins).  The long ones are tilted off the axes (no BASIS_ULPS needed) and keep sigma1 / sigma2 < 10.
    i0, j0 = min(bins_x - 3, bins_x // 2), min(bins_y - 3, bins_y // 2)
    if bins_x >= 3:
        add("3x1", ((i0 + 1.5) * bin_w, mid_y(min(1, bins_y - 1)), 0.45 * bin_w, 0.05 * bin_w, 0.1, 5.4))
    if bins_y >= 3:
        add("1x3", (mid_x(min(1, bins_x - 1)), (j0 + 1.5) * bin_h, 0.45 * bin_h, 0.06 * bin_h, np.pi / 2 - 0.1, 5.5))
    if bins_x >= 3 and bins_y >= 3:
        add("3x3", ((i0 + 1.5) * bin_w, (j0 + 1.5) * bin_h, np.sqrt(50.0 * s * s - 0.3), np.sqrt(50.0 * s * s - 0.3), 0.0, 5.6))
    # every bin column / every bin row: an axis of 0.56 of the frame (the other a tenth of it: on a wide grid the rectangle is
    # several bin rows high — an eigenvalue ratio under 100 allows no less)
    if bins_x >= 2:
        add("all_columns", (w / 2.0 + 1.3, mid_y(bins_y // 2), 0.56 * w / np.sqrt(8.0), 0.56 * w / np.sqrt(8.0) / 9.6, 0.04, 5.7))
    if bins_y >= 2:
        add("all_rows", (mid_x(bins_x // 2), h / 2.0 + 1.3, 0.56 * h / np.sqrt(8.0), 0.56 * h / np.sqrt(8.0) / 9.6, np.pi / 2 - 0.04, 5.8))
    add("oversized", (w / 2.0 + 3.0, h / 2.0 + 2.0) + OVERSIZED + (6.0,))
    # centres outside the frame whose footprints reach in (the dist stage keeps a centre up to 20 % of the half frame outside)
    ox, oy = min(5.0, 0.06 * w), min(5.0, 0.06 * h)
    add("outside", (-ox, 0.4 * h, 5.0 * s, 3.0 * s, 0.3, 4.9), (w + ox, 0.6 * h, 4.0 * s, 4.5 * s, 1.1, 4.9),
        (0.3 * w, -oy, 3.0 * s, 5.0 * s, 0.5, 4.9), (0.7 * w, h + oy, 4.5 * s, 4.0 * s, 0.8, 4.9))
    return dict(arrays=_discs(sp, w, h, GRID_EYE_Z), W=w, H=h, bins=(bins_x, bins_y), bin_px=(bin_w, bin_h), tags=tags)


# name -> (bins_x, bins_y, ragged): 32x16-px bins (MGS_BIN_SHIFT=1,0; tests/_child_fragment_grids.py).  21x12 (252 bins) is the one
# grid of sum 33 — the first that takes the ballots by default — which the direct binning takes (17x16 goes to the records)
GRIDS = {}
for _bx, _by in ((32, 8), (8, 32), (25, 10), (21, 12), (17, 16), (16, 16), (17, 15), (31, 1), (1, 31), (33, 4), (1, 1)):
    GRIDS[f"grid_{_bx}x{_by}"] = (_bx, _by, False)
    GRIDS[f"grid_{_bx}x{_by}_ragged"] = (_bx, _by, (12, 7) if (_bx, _by) == (1, 1) else True)   # (1x1 ragged: 20x9 px)
RECORD_GRIDS = ("grid_17x16", "grid_33x4")   # no direct binning: 272 bins; 33 bin columns (plain and ragged alike)
# the stage's default 128x64-px additive-alpha bins, rendered by the default process
DEFAULT_BIN_GRIDS = {"bins128_16x16": (16, 16), "bins128_32x8": (32, 8)}

# chunks of kDbChunk = 1024 sorted splats and k_dbin_emit's stage of kDbStage = 3072 entries, on the 16x16 grid: stacks of identical
# footprints, each at a distance of its own (far to near = the sorted stream)
SW, SH = 512, 256
_OVER = (SW / 2 + 3.0, SH / 2 + 2.0) + OVERSIZED


def _one_bin(bx, by):
    return (bx * 32 + 16.0, by * 16 + 8.0, 1.6, 1.6, 0.0)


def _three_bins(bx, by):   # bins bx .. bx + 2 of row by
    return ((bx + 1.5) * 32, by * 16 + 8.0, 14.4, 1.6, 0.1)


def _four_bins(i, j):      # the bins around corner (i, j)
    return (i * 32.0, j * 16.0, 1.3, 1.3, 0.0)


# name -> [(splats, footprint, distance)], far to near
STACK_CASES = {
    # 1 + 400 + 300 + 200 + 123 = 1024 sorted splats: one full chunk; one more, the nearest, is a last chunk of one splat
    "chunks_1024": [(1, _OVER, 6.0), (400, _one_bin(3, 2), 5.8), (300, _four_bins(9, 5), 5.6), (200, _three_bins(6, 11), 5.4), (123, _one_bin(13, 14), 5.2)],
    "chunks_1025": [(1, _OVER, 6.0), (400, _one_bin(3, 2), 5.8), (300, _four_bins(9, 5), 5.6), (200, _three_bins(6, 11), 5.4), (123, _one_bin(13, 14), 5.2),
                    (1, _one_bin(15, 15), 4.6)],
    "chunks_4097": [(1, _OVER, 6.0), (1500, _one_bin(3, 2), 5.8), (1200, _four_bins(9, 5), 5.6), (800, _three_bins(6, 11), 5.4), (595, _one_bin(13, 14), 5.2),
                    (1, _one_bin(15, 15), 4.6)],
    # chunk 0: 1024 x 256 entries (unstaged, every bin's run 1024 long); chunk 1: 1024 x 3 = 3072 = kDbStage (the last staged size,
    # all escapes); chunk 2: 1023 x 3 + 4 = 3073 (the first unstaged size); chunk 3: 1024 x 1
    "stage_edge": [(1024, _OVER, 6.0), (1024, _three_bins(2, 3), 5.6), (1023, _three_bins(7, 8), 5.2), (1, _four_bins(12, 12), 5.19),
                   (1024, _one_bin(5, 12), 4.8)],
}
STAGE_EDGE_ENTRIES = [1024 * 256, 3072, 3073, 1024]   # list entries per chunk of "stage_edge"


def stack_case(name):
    sp = []
    for n, foot, d in STACK_CASES[name]:
        sp += [foot + (d,)] * n
    return dict(arrays=_discs(sp, SW, SH, GRID_EYE_Z), W=SW, H=SH, bins=(16, 16), bin_px=(32, 16), tags={"oversized": [0]})


GRID_CASES = list(GRIDS) + list(STACK_CASES)   # what tests/_child_fragment_grids.py renders, with 32x16-px bins


def bin_rects(table, w, h, bin_w, bin_h):
    """the bin rectangle (x0, y0, x1, y1) per row of a Fragments.table, from the footprint box alone (the pixel centres inside
    centre +- the ellipse's bounding box, clipped to the frame), and whether the box has such a pixel at all"""
    ex, ey = np.hypot(table["b1"][:, 0], table["b2"][:, 0]), np.hypot(table["b1"][:, 1], table["b2"][:, 1])
    x0, x1 = np.ceil(table["c"][:, 0] - ex - 0.5), np.floor(table["c"][:, 0] + ex - 0.5)
    y0, y1 = np.ceil(table["c"][:, 1] - ey - 0.5), np.floor(table["c"][:, 1] + ey - 0.5)
    hit = (x1 >= x0) & (y1 >= y0) & (x1 >= 0) & (x0 <= w - 1) & (y1 >= 0) & (y0 <= h - 1)
    r = np.stack([np.clip(x0, 0, w - 1) // bin_w, np.clip(y0, 0, h - 1) // bin_h, np.clip(x1, 0, w - 1) // bin_w, np.clip(y1, 0, h - 1) // bin_h], 1)
    return r.astype(np.int64), hit


def unpack_rects(rect):
    """download_projected's packed rectangles -> int64[n, 4] (x0, y0, x1, y1) in bins"""
    r = np.asarray(rect, np.uint32).astype(np.int64)
    return np.stack([r & 255, (r >> 8) & 255, (r >> 16) & 255, r >> 24], 1)


def rect_entries(r):
    """list entries per rectangle: (x1 - x0 + 1) (y1 - y0 + 1)"""
    return (r[:, 2] - r[:, 0] + 1) * (r[:, 3] - r[:, 1] + 1)


def direct_binning_takes(bx, by):
    """the grids k_dbin_* take (directBinningSupported): at most 32 bins along an axis, 256 bins, binsX + binsY <= 40"""
    return bx <= 32 and by <= 32 and bx * by <= 256 and bx + by <= 40


def bin_grid(w, h, shift_x, shift_y):
    """the frame's bin grid: bins of (16 << shift_x) x (16 << shift_y) px over 16-px tiles"""
    tx, ty = (w + 15) // 16, (h + 15) // 16
    return (tx + (1 << shift_x) - 1) >> shift_x, (ty + (1 << shift_y) - 1) >> shift_y


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# "crowded" / "crowded_opaque" are there because of what test_fragments_cpu.py::test_staged_records_per_region finds: no region of
# "dense" stages more than MGS_SUM_GO = 192 records, so each walks ONE batch and the all-saturated batches' polynomial walk never
# runs for it.  12 000 smaller splats put 31 regions above 192 staged records and 2 above MGS_SUM_CAP = 448, at 0.4 % borderline.
COUNT_CASES = ["dense", "sparse", "hand_made", "two_instances", "crowded"]   # the count mode (opacity gaussian disabled)
GAUSSIAN_CASES = ["opaque_gaussian", "dense", "crowded_opaque"]              # the additive alpha with the gaussian on
# The cases added here (not the issue's five) also set aside the fragments that the DIRECTION of the extent basis leaves open, because
# the first GPU run of "crowded" found one: pixel (251,81), splat 6286, A = 8.00287 in float64 (3.6 DELTA outside), counted by the kernel.
# The splat is nearly axis-aligned (Sigma2D = (132.18, -0.031, 57.05)), and the reference's eigenvector (b, ev1 - a) is then
# (-0.031, 1.3e-5) with the second component below one fp32 step of ev1 (1.5e-5): its direction is open by 5e-4 rad per step in ANY
# fp32 evaluation.  The oracle's own fp32 projection moves this fragment's A by 6.6e-5 relative and that of splat 3452 at the same
# pixel by 1.1e-4, more than DELTA, with centre and axis lengths good to 2e-7 (it stayed on float64's side by luck).
# np_fragments.basis_turn models the angle as `ulps` fp32 steps of ev1 over |(b, ev1 - a)|, np_fragments._turn turns it into a
# per-fragment dA, all in float64.  BASIS_ULPS is the oracle's own worst error in those units over the drawn splats of "crowded"
# (the rounding of Sigma2D's entries counts too, and weighs most where a is close to d): MEASURED by
# test_fragments_cpu.py::test_basis_direction_of_nearly_axis_aligned_splats (fails outside [BASIS_ULPS / 2, BASIS_ULPS]); measured 14.05.
# The kernel gets BASIS_MARGIN times that: its front end takes reciprocals, square roots and the normalisation from the 1-ulp hardware
# instructions where the oracle's are correctly rounded and lets the compiler fuse the products, so each step's error at most doubles.
BASIS_ULPS = 16
BASIS_MARGIN = 2
BASIS_CASES = ("crowded", "crowded_opaque")
EPS_CASES = ["opaque_gaussian", "dense"]   # EPS_FRAG is measured on these; "crowded_opaque" (1.93e-4 of its own) is held to the same figure
COVERAGE_CASES = ["dense", "sparse", "hand_made_open", "two_instances", "crowded"]   # the default alpha mode: where is there a fragment at all
CHILD_CASES = ["dense", "hand_made"]                                 # what tests/_child_fragments.py renders


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> dict(sets=[(arrays, transform or None)], cam=(V, P, eye), W, H)"""
    if name in GRIDS or name in DEFAULT_BIN_GRIDS or name in STACK_CASES:
        if name in STACK_CASES:
            g = stack_case(name)
        elif name in GRIDS:
            g = grid_case(GRIDS[name][0], GRIDS[name][1], 32, 16, GRIDS[name][2])
        else:
            g = grid_case(DEFAULT_BIN_GRIDS[name][0], DEFAULT_BIN_GRIDS[name][1], 128, 64, False)
        return dict(sets=[(g["arrays"], None)], cam=grid_camera(g["W"], g["H"]), W=g["W"], H=g["H"], bins=g["bins"], bin_px=g["bin_px"], tags=g["tags"])
    if name in ("hand_made", "hand_made_open"):   # "open": without the splat that covers the whole frame, for the coverage test
        return dict(sets=[(hand_made(clamped=name == "hand_made"), None)], cam=hand_camera(), W=HW, H=HH)
    crowded = name in ("crowded", "crowded_opaque")
    sc = synth.make_scene(12000 if crowded else 3000, seed=5)
    if crowded:
        sc["scale"] = (sc["scale"] + 0.4).astype(np.float32)
    if name in ("dense", "opaque_gaussian"):   # several hundred to a thousand entries per bin: a region goes through several batches
        sc["scale"] = (sc["scale"] + 1.0).astype(np.float32)
    if name in ("opaque_gaussian", "crowded_opaque"):   # waves saturate after a few fragments, the real-valued tail is summed by the saturated walks
        sc["opacity"] = (sc["opacity"] + 5.0).astype(np.float32)
    sets = [(sc, None), (sc, SECOND_INSTANCE)] if name == "two_instances" else [(sc, None)]
    assert crowded or name in ("dense", "opaque_gaussian", "sparse", "two_instances"), name
    return dict(sets=sets, cam=orbit_camera(W, H), W=W, H=H)


class Reference:
    """what the float64 restatement says about one case: built once per process and shared (never modified)"""

    def __init__(self, ob, name):
        c = case(name)
        self.name, self.c = name, c
        V, P, eye = c["cam"]
        self.prepared = {id(a): ob.PreparedSet(a) for a, _ in c["sets"]}
        self.inst = ob.make_instances([(self.prepared[id(a)], m) for a, m in c["sets"]])
        self.frame_kw = dict(view=V, proj=P, camera_pos=eye, width=c["W"], height=c["H"])
        self.projected, self.survivors, total = [], [], 0
        for a, m in c["sets"]:
            ps = self.prepared[id(a)]
            n = ps.count
            M = np.eye(4) if m is None else m
            self.projected.append(npr.project(ps.positions, ps.cov6, ps.rgba, ps.sh.reshape(n, -1) if ps.sh_stride else np.zeros((n, 45)),
                                              ps.sh_degree, M, V, P, eye, c["W"], c["H"]))
            self.survivors.append(npr.dist_cull(ps.positions, M, V, P, c["W"], c["H"], 0.2)[0])
            total += n
        self.total = total
        # the key depth of every splat the oracle's dist stage keeps (back-to-front keys hold -ndc.z), by global id
        import occluder_levels as ol
        keys, ids = ob.key_cull(ob.make_frame(**self.frame_kw), self.inst)
        self.oracle_survivors = np.zeros(total, bool)
        self.oracle_survivors[ids] = True
        self.key_depth = np.full(total, np.inf, np.float32)
        self.key_depth[ids] = ol.depths_of_btf_keys(keys)
        self._memo = {}

    def fragments(self, gaussian=False, depth_level=None):
        """the counts; depth_level: a constant occluder depth (fp32) or None"""
        key = (bool(gaussian), None if depth_level is None else float(depth_level))
        if key not in self._memo:
            depth = None if depth_level is None else np.full((self.c["H"], self.c["W"]), np.float32(depth_level), np.float32)
            self._memo[key] = nf.fragments(self.projected, self.survivors, self.c["W"], self.c["H"], gaussian, DELTA, depth, self.key_depth,
                                              basis_ulps=BASIS_MARGIN * BASIS_ULPS if self.name in BASIS_CASES else 0)
        return self._memo[key]

    def staged_per_region(self):
        """how many records stage A of the compositor keeps per 32x16-px region: the splats whose footprint box (the ellipse's
        bounding box) reaches one of the region's pixel centres"""
        t = self.fragments().table
        ex, ey = np.hypot(t["b1"][:, 0], t["b2"][:, 0]), np.hypot(t["b1"][:, 1], t["b2"][:, 1])
        return np.array([[int(((np.abs(t["c"][:, 0] - (rx + 16)) <= ex + 15.5) & (np.abs(t["c"][:, 1] - (ry + 8)) <= ey + 7.5)).sum())
                          for rx in range(0, self.c["W"], 32)] for ry in range(0, self.c["H"], 16)])

    def median_level(self):
        """an occluder depth in a gap of the key depths next to their median (occluder_levels.pick_level: no splat within 16 fp32 steps)"""
        import occluder_levels as ol
        return ol.pick_level(self.key_depth[np.isfinite(self.key_depth)], 0.5)


_references = {}


def reference(ob, name):
    if name not in _references:
        _references[name] = Reference(ob, name)
    return _references[name]
