"""Register/scratch/LDS budget of the contour kernels (ipp_contour.hip
k_contour_*): compiled to ISA (CPU only) and read from the amdhsa metadata
alone through tools/kernel_res; a resource check only."""
import os

import pytest

from tests.test_scene_kernel_resources import HIPCC, LDS_MAX, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

WANT = ("k_contour_emit", "k_contour_link", "k_contour_jump", "k_contour_select", "k_contour_header",
        "k_contour_pack")


def test_contour_kernels_no_spills_no_private_segment(tmp_path):
    ks, _ = _kernels("ipp_contour", tmp_path)
    seen = {}
    for k in ks:
        name = k.get("name") or ""
        if "k_contour_" not in name:
            continue
        seen[[w for w in WANT if w in name][0]] = k
        assert int(k.get("vgpr_spill_count", 0)) == 0, name
        assert int(k.get("sgpr_spill_count", 0)) == 0, name
        assert int(k.get("private_segment_fixed_size", 0)) == 0, name
        assert int(k.get("group_segment_fixed_size", 0)) <= LDS_MAX, name
    assert set(seen) == set(WANT)
