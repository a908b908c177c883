"""The scenes of the fragment-count tests, shared by tests/test_fragments_cpu.py (which holds the oracle to the float64 count of
tests/np_fragments.py and establishes the borderline share and EPS_FRAG from the CPU side alone), tests/test_gpu_fragments.py (which
holds the compositor to the same counts) and tests/_child_fragments.py.

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
    a = np.asarray(sp, np.float64)
    d = a[:, 5]
    unit = d / HH   # world units per pixel at distance d
    pos = np.stack([(a[:, 0] - HW / 2) * unit, (a[:, 1] - HH / 2) * unit, HAND_EYE_Z - d], 1)
    scale = np.log(np.stack([a[:, 2] * unit, a[:, 3] * unit, np.full(d.shape, 1e-4)], 1))
    rot = np.stack([np.cos(a[:, 4] / 2), np.zeros_like(d), np.zeros_like(d), np.sin(a[:, 4] / 2)], 1)
    n = a.shape[0]
    r = np.random.default_rng(9)
    return dict(positions=pos.astype(np.float32), f_dc=r.standard_normal((n, 3)).astype(np.float32), f_rest=np.zeros((n, 0), np.float32),
                opacity=np.full(n, 2.0, np.float32), scale=scale.astype(np.float32), rotation=rot.astype(np.float32))


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
