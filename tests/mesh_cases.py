"""The inputs of the mesh tests, shared by tests/test_mesh_cpu.py (which establishes the coverage cap and the float32-vs-float64
differences on the numpy restatement alone) and tests/test_gpu_mesh.py (which holds the kernels to them)."""
import os

import numpy as np

import lighting_cases as lc
import np_lighting as nl
import np_mesh as nm

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes", "fixture.obj")
W, H = 128, 96

# At most 0.5 % of the pixels the float64 restatement covers may be left out of a comparison, each of them a boundary pixel
# (np_mesh.boundary): a condition on the cases.  float32 against float64 of the restatement alone must stay within a quarter of it.
COVERAGE_CAP = 0.005
# Largest float32-vs-float64 difference of np_mesh over all cases below, on the pixels where both agree on the primitive: MEASURED by
# test_mesh_cpu.py::test_cap_and_tolerance_from_the_reference_alone (which fails if a measurement leaves [X / 2, X]).
DEPTH_F32_VS_F64 = 1.0e-6   # absolute; measured 8.94e-7 (both_paths: the clipped triangle and the distant quad), 1.19e-7 elsewhere
COLOR_F32_VS_F64 = 1.5e-5   # relative to max(1, value); measured 1.37e-5 (shading_moved: a specular highlight), 6.12e-6 (shading_mixed), 5.42e-6 (shading_headlight)
GPU_DEPTH_BAR, GPU_COLOR_BAR = 4.0 * DEPTH_F32_VS_F64, 4.0 * COLOR_F32_VS_F64  # the margin the lighting tests give, for the same reason


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


def persp(fov, aspect, n, f):
    t = np.tan(np.radians(fov) / 2)
    P = np.zeros((4, 4), np.float32)
    P[0, 0], P[1, 1], P[2, 2], P[3, 2], P[2, 3] = 1 / (aspect * t), 1 / t, f / (n - f), -1, -(f * n) / (f - n)
    return P


def camera(eye=(2.2, 1.6, 3.0), center=(0, 0.1, 0)):
    return lookat(eye, center), persp(55.0, W / H, 0.1, 50.0), np.asarray(eye, np.float32)


def mesh(positions, indices, normals=None, material_ids=None, materials=None, transform=None, visible=True):
    positions = np.asarray(positions, np.float32).reshape(-1, 3)
    indices = np.asarray(indices, np.uint32).reshape(-1, 3)
    if normals is None:
        normals = nm.generate_normals(positions, indices)
    return dict(positions=positions, indices=indices, normals=np.asarray(normals, np.float32).reshape(-1, 3),
                material_ids=None if material_ids is None else np.asarray(material_ids, np.uint32), materials=materials,
                transform=transform, visible=visible)


# ---- exact fill rule: 64 x 64, view = identity, proj = identity (clip = position, w = 1), vertices on multiples of 1/256 pixel ----
FW = FH = 64


def _ndc(px, size=64):
    return np.float32(px) / np.float32(size / 2) - np.float32(1.0)


def fill_mesh():
    """window-space triangles (x, y in pixels, z) -> one mesh.  Listed in primitive order."""
    tris = [
        [(2.5, 2.5, .5), (10.5, 2.5, .5), (2.5, 10.5, .5)],          # edges through pixel centres, a vertex on a pixel centre
        [(10.5, 2.5, .5), (10.5, 10.5, .5), (2.5, 10.5, .5)],        # shares the diagonal, opposite direction
        [(20, 4, .4), (20, 14, .4), (30, 4, .4)],                    # the other winding
        [(30, 4, .4), (20, 14, .4), (30, 14, .4)],                   # shared edge traversed the same way round
        [(40.5, 5.5, .3), (50.5, 5.5, .3), (45.5, 5.5, .3)],         # zero area
        [(4, 20, .6), (28, 20, .6), (4, 44, .6)],                    # two coplanar triangles at equal depth:
        [(4, 20, .6), (28, 20, .6), (4, 44, .6)],                    # the lower primitive id wins
        [(36, 20, 1.0), (60, 20, 1.0), (36, 44, 1.0)],               # depth exactly 1.0: nothing
        [(36.5 + 1 / 256, 48.5, .2), (59.25, 50.75 + 3 / 256, .2), (40.125, 61.5, .2)],  # off-centre vertices
        [(8.5, 50.5, .7), (8.5, 58.5, .7), (16.5, 58.5, .7)],        # horizontal bottom edge and vertical left edge on centres
    ]
    pos = np.array([[_ndc(x), _ndc(y), np.float32(z)] for t in tris for (x, y, z) in t], np.float32)
    return mesh(pos, np.arange(pos.shape[0]).reshape(-1, 3), normals=np.tile(np.float32([0, 0, 1]), (pos.shape[0], 1)))


def grid_mesh(seed=3, n=33):
    """a jittered n x n grid in the plane z = 0 that more than covers the frame of grid_camera()"""
    r = np.random.default_rng(seed)
    g = np.linspace(-4.0, 4.0, n, dtype=np.float32)
    x, y = np.meshgrid(g, g)
    jit = (r.random((n, n, 2), dtype=np.float32) - 0.5) * np.float32(0.4 * 8.0 / (n - 1))
    jit[0, :], jit[-1, :], jit[:, 0], jit[:, -1] = 0, 0, 0, 0
    pos = np.stack([x + jit[..., 0], y + jit[..., 1], np.zeros_like(x)], -1).reshape(-1, 3)
    a = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).reshape(-1)
    idx = np.concatenate([np.stack([a, a + 1, a + n + 1], 1), np.stack([a, a + n + 1, a + n], 1)], 0)
    return mesh(pos, idx, normals=np.tile(np.float32([0, 0, 1]), (pos.shape[0], 1)))


def grid_camera():
    return camera(eye=(0.6, -0.8, 2.2), center=(0, 0, 0))


def both_paths_meshes(seed=5, count=20000):
    """one triangle larger than the frame with a vertex behind the near plane, one full-frame quad, `count` sub-pixel triangles"""
    V, P, eye = camera()
    r = np.random.default_rng(seed)
    big = mesh([[-6, -1.0, -4], [6, -1.2, -4], [2.0, 1.4, 3.2]], [[0, 1, 2]])  # the third vertex lies behind the camera
    quad = mesh([[-300, -200, -12], [300, -200, -12], [300, 200, -12], [-300, 200, -12]], [[0, 1, 2], [0, 2, 3]],
                materials=[nl.default_material(ambient=(0.1, 0.1, 0.1), diffuse=(0.2, 0.3, 0.6), specular=(0.2, 0.2, 0.2), emission=(0, 0, 0), shininess=8.0)])
    c = (r.random((count, 1, 3), dtype=np.float32) - 0.5) * np.float32([5.0, 3.0, 3.0])
    tri = c + (r.random((count, 3, 3), dtype=np.float32) - 0.5) * np.float32(0.03)
    small = mesh(tri.reshape(-1, 3), np.arange(3 * count).reshape(-1, 3), material_ids=r.integers(0, 2, count),
                 materials=[nl.default_material(ambient=(0.05, 0.05, 0.05), diffuse=(0.9, 0.4, 0.2), specular=(0.4, 0.4, 0.4), emission=(0, 0, 0), shininess=16.0),
                            nl.default_material(emission=(0.1, 0.8, 0.3))])
    return [big, quad, small], (V, P, eye)


def worklist_meshes():
    """the scene of both_paths_meshes() plus two grids of 512 triangles of about 13 pixels, some 150 of each inside the frame with a box
    above 8 x 8 pixels (one chunk of the work list each, spread over 16 waves of the set-up pass): more than 300 chunks in all"""
    meshes, cam = both_paths_meshes()
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] *= np.float32(1.4)
    T[2, 3] = np.float32(-1.5)
    T2 = T.copy()
    T2[2, 3] = np.float32(-2.5)
    g = grid_mesh(seed=11, n=17)
    return meshes + [dict(g, transform=T), dict(g, transform=T2)], cam


SCALE = np.array([[1.6, 0, 0, -0.9], [0, 0.6, 0, 0.1], [0, 0, 1.1, 0.2], [0, 0, 0, 1]], np.float32)   # non-uniform: the normal matrix matters
_c, _s = np.float32(np.cos(0.7)), np.float32(np.sin(0.7))
ROTATE = np.array([[_c, 0, _s, 1.3], [0, 1, 0, 0.0], [-_s, 0, _c, -0.6], [0, 0, 0, 1]], np.float32)
MOVED = ROTATE.copy()
MOVED[1, 3] = np.float32(0.45)  # the second instance lifted: what set_transform is tested with
LIGHTS3 = [lc.LIGHTS_MIXED[0], lc.LIGHTS_MIXED[2], lc.LIGHTS_MIXED[3]]  # one directional, one point, one spot


def fixture_meshes(view_of_fixture):
    """view_of_fixture: capi.Mesh.load_obj(FIXTURE).view()"""
    v = view_of_fixture
    base = dict(positions=v["positions"], indices=v["indices"], normals=v["normals"], material_ids=v["material_ids"], materials=v["materials"])
    return [dict(base, transform=SCALE, visible=True), dict(base, transform=ROTATE, visible=True)]


def cases(view_of_fixture):
    """name -> (meshes, (V, P, eye), width, height, lighting_mode, lights)"""
    ident = (np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), np.zeros(3, np.float32))
    bp, bcam = both_paths_meshes()
    fx = fixture_meshes(view_of_fixture)
    return {
        "fill": ([fill_mesh()], ident, FW, FH, 0, []),
        "grid": ([grid_mesh()], grid_camera(), W, H, 0, []),
        "both_paths": (bp, bcam, W, H, 1, []),
        "shading_unlit": (fx, camera(), W, H, 0, []),
        "shading_headlight": (fx, camera(), W, H, 1, []),
        "shading_mixed": (fx, camera(), W, H, 1, LIGHTS3),
        "shading_moved": ([fx[0], dict(fx[1], transform=MOVED)], camera(), W, H, 1, []),
    }


def compare(got, ref, name=""):
    """(left-out share of the covered pixels, all left-out pixels are boundary pixels, max depth difference, max colour difference
    relative to max(1, value)) of got = (depth, colour, prim) against the float64 result `ref`"""
    gd, gc, gp = got
    covered = ref.prim != nm.NONE
    differ = gp != ref.prim
    agree = ~differ & covered
    share = differ.sum() / max(int(covered.sum()), 1)
    on_boundary = bool((nm.boundary(ref.prim) | ~differ).all())
    dd = float(np.abs(gd.astype(np.float64) - ref.depth.astype(np.float64))[agree].max()) if agree.any() else 0.0
    with np.errstate(invalid="ignore"):
        rel = np.abs(gc.astype(np.float64) - ref.color) / np.maximum(1.0, np.abs(ref.color))
    dc = float(rel[agree].max()) if agree.any() else 0.0
    return share, on_boundary, dd, dc
