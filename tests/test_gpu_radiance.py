"""Per-splat radiance at every shading site against float64 (-m gpu).

addShRadiance<SHF> (csrc/sh_eval.h) is called from six sites, each with its own instance look-up, view direction and
min(set degree, frame degree): the rasteriser's compositor, the two 3DGUT compositors ("packed", and "tile" which the surface outputs
select), the traced K-buffer walk, shadeHit of the stochastic trace strategies, and the ray queries.  Every other test sees shading
only after it was blended into a frame, at the frames' tolerance (2.5e-2 per channel); here the shaded colour of every single splat is
read out and held to a few units of fp32 rounding.

The read-out (radiance_cases.py has the construction): MGS_DEBUG_OPACITY_GAUSSIAN_DISABLED, an RGBA32F target and footprints that do
not overlap, so the pixel under a splat's centre is 1 * 1 * colour + 0.  Each test asserts what makes that valid: alpha == 1.0 at every
read pixel and == 0 on every pixel outside the cells' interiors (a ray batch: exactly one accepted hit and transmittance 0 per ray).
Every splat of the scene is read; none is left out.

Tolerance: K * u per value with u = 2^-23 (|base| + sum_k |c_k| BMAX_k) over the coefficients of the effective degree.  K_REF = 1.5 is
the oracle's fp32 shading against the same float64 reference in these units (measured 1.400 and held by
test_radiance_cpu.py::test_oracle_fp32_against_float64); K = 8 is 4 * K_REF rounded up to a power of two, the margin for fused
multiply-adds, v_rsq_f32 and the kernel's summation order (measured on an MI355X: 2.2 u at the traced sites, 1.7 u in the compositors, 1.2 u
for the ray batch).  One uint8 SH step is 2/255, about 6e4 u of a unit coefficient.

One child process per storage format renders everything (tests/_child_radiance.py); the tests compare what it left."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import radiance_cases as rc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SITES = ("raster", "gut_packed", "gut_tile", "trace", "shade_hit")


@pytest.fixture(scope="module", params=list(rc.FORMATS))
def frames(request):
    """(storage format, what its child process left): one child per format"""
    fmt = request.param
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "radiance.npz")
        e = {k: v for k, v in os.environ.items() if not k.startswith("MGS_") or k in ("MGS_LIB", "MGS_RCCL_LIB")}
        r = subprocess.run([sys.executable, os.path.join(HERE, "_child_radiance.py"), fmt, out], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
        return fmt, dict(np.load(out))


def check_frame(got, key, want, u, label):
    """the read-out's premises and the bar, for one frame; returns the worst error in units of u"""
    px, border = got[key + "/px"], got[key + "/border"]
    assert px.shape == (want.shape[0], 4) and px.shape[0] == rc.N, "a splat was left out"
    assert np.array_equal(px[:, 3], np.ones(rc.N, np.float32)), f"{label}: alpha != 1 at the read pixels of splats {np.flatnonzero(px[:, 3] != 1)[:8]}"
    assert not border.any(), f"{label}: {int(np.count_nonzero(border))} pixels outside the cells' interiors are covered"
    k = rc.in_units(np.abs(px[:, :3].astype(np.float64) - want), u)
    worst = float(k.max())
    i, c = np.unravel_index(int(np.argmax(k)), k.shape)
    print(f"{label}: worst {worst:.3f} u (splat {i}, channel {c}: got {px[i, c]!r}, float64 {want[i, c]!r})")
    assert worst <= rc.K, f"{label}: {worst:.2f} u at splat {i} channel {c}, {int((k > rc.K).sum())} values over {rc.K} u"
    return worst


@pytest.mark.parametrize("site", SITES)
def test_site_all_poses_and_degrees(frames, site):
    """eight poses x frame sh_degree 0..3 over set degrees 3, 0, 1, 2 under four transforms: all 16 clamp combinations per pose"""
    fmt, got = frames
    worst = 0.0
    for pose in rc.POSE_NAMES:
        for deg in range(4):
            want, u = rc.reference("four", pose, fmt, deg)
            worst = max(worst, check_frame(got, f"four/{pose}/{site}/{deg}", want, u, f"{site} {fmt} {pose} sh_degree {deg}"))
    print(f"{site} {fmt}: worst of all poses and degrees {worst:.3f} u, bar {rc.K} u")


@pytest.mark.parametrize("site", SITES)
def test_sh_only(frames, site):
    """MGS_DEBUG_SH_ONLY: the base colour is 0.5"""
    fmt, got = frames
    want, u = rc.reference("four", rc.EXTRAS_POSE, fmt, 3, True)
    check_frame(got, f"four/{rc.EXTRAS_POSE}/{site}/3/sh_only", want, u, f"{site} {fmt} SH only")
    plain, _ = rc.reference("four", rc.EXTRAS_POSE, fmt, 3)
    assert np.abs(want - plain).max() > 0.4                      # (the flag is visible)


@pytest.mark.parametrize("variant", ["surface", "occluder", "occluder_surface", "strips"])
def test_rasteriser_instantiations(frames, variant):
    """the shading phase of k_composite's other instantiations: surface outputs, a bound occluder that hides nothing (with and without
    the surface outputs), and one frame rendered as two strips (the boundary, pixel row 96, crosses a row of cells)"""
    fmt, got = frames
    want, u = rc.reference("four", rc.EXTRAS_POSE, fmt, 3)
    check_frame(got, f"four/{rc.EXTRAS_POSE}/raster/3/{variant}", want, u, f"raster {fmt} {variant}")
    assert np.array_equal(got[f"four/{rc.EXTRAS_POSE}/raster/3/{variant}/px"], got[f"four/{rc.EXTRAS_POSE}/raster/3/px"])   # the same code: bit for bit


@pytest.mark.parametrize("site", ["raster", "gut_packed", "gut_tile", "trace"])
def test_twenty_instances(frames, site):
    """above the compositor's inline table of 16 instances; every instance's first and last splat is read (all are)"""
    fmt, got = frames
    for deg in range(4):
        want, u = rc.reference("twenty", rc.TWENTY_POSE, fmt, deg)
        check_frame(got, f"twenty/{rc.TWENTY_POSE}/{site}/{deg}", want, u, f"{site} {fmt} twenty instances sh_degree {deg}")


def test_ray_queries(frames):
    """mgs_trace_rays: one ray per splat from an origin of the test's choosing; the model-space directions include the six axes and
    the eight octant diagonals exactly"""
    fmt, got = frames
    for tag, deg, sh_only in (("0", 0, False), ("1", 1, False), ("2", 2, False), ("3", 3, False), ("3/sh_only", 3, True)):
        want, u = rc.ray_reference(fmt, deg, sh_only)
        rad = got[f"rays/{tag}/radiance"].astype(np.float64)
        assert rad.shape == (rc.N, 3), "a splat was left out"
        assert np.array_equal(got[f"rays/{tag}/hits"], np.ones(rc.N, np.uint32)) and not got[f"rays/{tag}/transmittance"].any()
        k = rc.in_units(np.abs(rad - want), u)
        worst = float(k.max())
        print(f"rays {fmt} {tag}: worst {worst:.3f} u, on the 14 exact directions {float(k[rc.rays()['exact']].max()):.3f} u")
        assert worst <= rc.K, (tag, worst, int((k > rc.K).sum()))
