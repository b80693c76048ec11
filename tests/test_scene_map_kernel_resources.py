"""Register/scratch/LDS budget of ipp_pipe_scene_map's kernels (ipp_label.hip
k_scene_map, k_scene_table): compiled to ISA (CPU only) and read from the
amdhsa metadata as tests/test_scene_kernel_resources.py does; a resource check
only."""
import os

import pytest

from tests.test_scene_kernel_resources import HIPCC, _clean, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_scene_map_kernels_no_spills_no_scratch(tmp_path):
    ks, text = _kernels("ipp_label", tmp_path)
    want = ("k_scene_map", "k_scene_table")
    seen = {}
    for k in ks:
        hit = [w for w in want if w in (k.get("name") or "")]
        if hit:
            seen[hit[0]] = k
            _clean(k, text)
    assert set(seen) == set(want)
    m = seen["k_scene_map"]
    # no LDS, and few enough registers for 8 waves per SIMD (<= 64 per lane):
    # the kernel is a stream of 16-B stores, its occupancy hides the byte loads
    assert int(m["group_segment_fixed_size"]) == 0
    assert int(m["vgpr_count"]) + int(m.get("agpr_count", 0)) <= 64
