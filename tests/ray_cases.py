"""The ray batch of the ray-query tests (test_rays_cpu.py, test_gpu_rays.py, _child_rays.py), numpy only: about 4 000 arbitrary rays
through the scene of trace_cases' c_two_instances (two instances, one with a non-uniform scale), and its float64 restatement
(np_trace_rays.py), computed once per process.

The batch, in fp32 as the device receives it (SEED chosen on the CPU so that the restatement's fragile share stays within the cap
test_trace_cpu.py holds the frames' cases to; test_rays_cpu.py asserts it):
  * origins inside the scene box, on a shell outside it, and far outside (15 units: the fp32 margins of a ray grow with its origin's distance);
  * directions towards a random point of the scene or fully random; every tenth ray has length 0.5, every tenth 3.0 (its window is
    given in its own parameter); a group is axis-parallel with two exactly zero components;
  * windows: the primary rays' (0.001, 10000); t_min at the scene's centre (the near half is skipped); t_max at the scene's centre
    (the scene is cut in half); a negative t_min; and t_min == t_max;
  * eight invalid rays spread through the batch (NaN, inf, zero direction, t_min > t_max)."""
import functools

import numpy as np

import np_trace
import np_trace_rays
import trace_cases as tc

SCENE = "c_two_instances"
SEED = 7
N = 4000
INVALID_AT = (5, 300, 1023, 1024, 2047, 2500, 3333, 3999)


@functools.lru_cache(maxsize=None)
def batch(seed=SEED):
    """(O [N,3], D [N,3], tmin [N], tmax [N]) float32; do not modify the result"""
    rng = np.random.Generator(np.random.PCG64(seed))
    kind = rng.integers(0, 100, N)
    O = np.empty((N, 3))
    inside, far = kind < 55, kind >= 97
    shell = ~inside & ~far
    O[inside] = rng.uniform(-1.0, 1.0, (int(inside.sum()), 3)) * (1.6, 0.9, 1.0)
    u = rng.standard_normal((N, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    O[shell] = (u * rng.uniform(3.0, 3.6, (N, 1)))[shell]
    O[far] = (u * 15.0)[far]
    target = rng.uniform(-0.9, 0.9, (N, 3))
    D = target - O
    free = rng.random(N) < 0.15                       # fully random directions: most of them miss from outside
    D[free] = rng.standard_normal((int(free.sum()), 3))
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    axis = np.arange(N) % 25 == 7                      # axis-parallel, two exactly zero components, through the scene
    ax = rng.integers(0, 3, N)
    for i in np.nonzero(axis)[0]:
        O[i] = rng.uniform(-0.7, 0.7, 3)
        sign = 1.0 if rng.random() < 0.5 else -1.0
        O[i, ax[i]] = -3.5 * sign
        D[i] = 0.0
        D[i, ax[i]] = sign
    centre = np.abs((O * D).sum(1))                    # the parameter of the point closest to the scene's centre (unit direction)
    length = np.ones(N)
    length[np.arange(N) % 10 == 3] = 0.5
    length[np.arange(N) % 10 == 6] = 3.0
    D *= length[:, None]
    tmin, tmax = np.full(N, 0.001), np.full(N, 10000.0)
    w = rng.integers(0, 10, N)
    tmin[w == 0] = (centre / length)[w == 0]          # starts at the scene's centre
    tmax[w == 1] = (centre / length)[w == 1]          # ends there
    both = w == 2                                      # a slab of the scene
    tmin[both], tmax[both] = (centre / length * 0.8)[both], (centre / length * 1.1)[both]
    tmin[w == 3] = -2.0                                # taken as 0
    same = (w == 4) & (np.arange(N) % 4 == 0)
    tmax[same] = tmin[same] = (centre / length)[same]  # an empty window that is still valid
    O, D, tmin, tmax = (a.astype(np.float32) for a in (O, D, tmin, tmax))
    bad = list(INVALID_AT)
    O[bad[0], 1] = np.nan
    D[bad[1], 0] = np.inf
    D[bad[2]] = 0.0
    tmin[bad[3]], tmax[bad[3]] = 2.0, 1.0
    tmax[bad[4]] = np.inf
    D[bad[5], 2] = np.nan
    O[bad[6], 0] = -np.inf
    tmin[bad[7]] = np.nan
    return O, D, tmin, tmax


def prepared():
    case = tc.cases()[SCENE]
    return [(np_trace.prepare_set(a), M) for a, M in case["sets"]]


@functools.lru_cache(maxsize=None)
def restate():
    """np_trace_rays.trace_rays of the batch with the defaults of the frame and trace parameters; do not modify the result"""
    O, D, tmin, tmax = batch()
    return np_trace_rays.trace_rays(prepared(), O, D, tmin, tmax)
