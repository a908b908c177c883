"""child process of test_gpu_fragments.test_binning_paths_give_the_same_counts: libmgs reads MGS_DIRECT_BIN / MGS_BIN_SHIFT once per
process, so every setting renders in its own interpreter.  Renders the cases of fragment_cases.CHILD_CASES in the count mode (additive
alpha, opacity gaussian disabled, RGBA32F target) and prints the SHA-1 of each alpha plane."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fragment_cases as fc  # noqa: E402
import gpu_fragments as gf  # noqa: E402

for name in fc.CHILD_CASES:
    scene = gf.build_scene(name)
    alpha, out = gf.render_alpha(scene, name, alpha_mode=gf.capi.ALPHA_SUM, debug_flags=4)
    assert out.error_flags == 0
    print("ALPHA_SHA1", name, gf.sha1(alpha), flush=True)
    scene.close()
print("CHILD_DONE", flush=True)
