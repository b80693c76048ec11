"""Register/scratch/LDS budget of ipp_pipe_scene_map's kernels (ipp_label.hip
k_scene_map, k_scene_table): read from the amdhsa metadata of their ISA
(tests/kernel_isa.py, CPU only); a resource check only."""
from tests.kernel_isa import clean, isa, needs_hipcc

pytestmark = needs_hipcc


def test_scene_map_kernels_no_spills_no_scratch():
    _, text, ks = isa("ipp_label")
    want = ("k_scene_map", "k_scene_table")
    seen = {}
    for k in ks:
        hit = [w for w in want if w in (k.get("name") or "")]
        if hit:
            seen[hit[0]] = k
            clean(k, text)
    assert set(seen) == set(want)
    m = seen["k_scene_map"]
    # no LDS, and few enough registers for 8 waves per SIMD (<= 64 per lane):
    # the kernel is a stream of 16-B stores, its occupancy hides the byte loads
    assert int(m["group_segment_fixed_size"]) == 0
    assert int(m["vgpr_count"]) + int(m.get("agpr_count", 0)) <= 64
