"""child process of test_gpu_mesh.py: one mesh pass with the work-list capacity the environment gives (MGS_MESH_WORK_ITEMS is read
when the library starts).   usage: _child_mesh_worklist.py OUT.npz"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import mesh_cases as mc  # noqa: E402

meshes, (V, P, eye) = mc.worklist_meshes()
scene = mgs.Scene(0)
keep = [mgs.Mesh.from_arrays(m["positions"], m["indices"], m["normals"], m.get("material_ids"),
                             [capi.make_material(**mm) for mm in (m.get("materials") or [])] or None) for m in meshes]
for m, cm in zip(meshes, keep):
    scene.add_mesh_instance(cm, m.get("transform"))
p = capi.default_params(mc.W, mc.H)
capi.set_camera(p, V, P, eye)
p.lighting_mode = 0  # unlit: the test is about coverage
res = {}
for rep in range(2):  # the second pass finds the list as the first one left it
    out = scene.render_meshes(p, want_stats=True)
    depth, color, prim = scene.download_meshes()
    res.update({f"depth{rep}": depth, f"color{rep}": color, f"prim{rep}": prim,
                f"stats{rep}": np.array([out.triangles_in, out.triangles_rasterised, out.fragments, out.flags], np.uint64)})
np.savez(sys.argv[1], **res)
scene.close()
print("CHILD_DONE", flush=True)
