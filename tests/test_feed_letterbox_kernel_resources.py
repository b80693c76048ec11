"""Register/scratch/LDS budget of the letterboxing training-batch kernels
(ipp_feed_resize.hip k_letterbox_images and k_letterbox_index_map, ipp_feed.hip
k_letterbox_targets): read from the amdhsa metadata of their ISA alone
(tests/kernel_isa.py, CPU only); a resource check only.  k_letterbox_images
carves all of its LDS from the dynamic segment, sized by the launch from the
rectangle's geometry up to IPP_FEED_RESIZE_LDS_BYTES exactly as k_feed_resize's
(the extents are swept in tests/test_feed_resize_cpu.py), so its static segment
must be empty: static plus dynamic then stays within the stated budget."""
from tests.kernel_isa import clean, isa, needs_hipcc
from tests.test_feed_resize_kernel_resources import LDS_BUDGET, LDS_CEILING, _define

pytestmark = needs_hipcc


def test_letterbox_kernels_no_spills_no_private_segment_lds_within_budget():
    _, text, ks = isa("ipp_feed_resize")
    images = [k for k in ks if "k_letterbox_images" in (k.get("name") or "")]
    index_map = [k for k in ks if "k_letterbox_index_map" in (k.get("name") or "")]
    assert len(images) == 2 and len(index_map) == 1          # the 2- and the 4-byte instance
    for k in images + index_map:
        clean(k, text)
    assert _define("IPP_FEED_RESIZE_LDS_BYTES") == LDS_BUDGET <= LDS_CEILING
    for k in images:
        assert int(k["group_segment_fixed_size"]) == 0, k["name"]
        assert int(k["group_segment_fixed_size"]) + LDS_BUDGET <= LDS_CEILING
        assert int(k["vgpr_count"]) <= 128, k["name"]        # two workgroups of 256 threads per CU need no more
    assert int(index_map[0]["group_segment_fixed_size"]) == 256
    _, text, ks = isa("ipp_feed")
    targets = [k for k in ks if "k_letterbox_targets" in (k.get("name") or "")]
    assert len(targets) == 1
    clean(targets[0], text)
    assert 0 < int(targets[0]["group_segment_fixed_size"]) <= 256
