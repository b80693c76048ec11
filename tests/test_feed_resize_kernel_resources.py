"""Register/scratch/LDS budget of the resizing training-batch kernels
(ipp_feed_resize.hip): read from the amdhsa metadata of its ISA alone
(tests/kernel_isa.py, CPU only); a resource check only.  k_feed_resize carves
all of its LDS from the dynamic segment, which the launch sizes from the
geometry up to IPP_FEED_RESIZE_LDS_BYTES (the extents themselves
are swept in tests/test_feed_resize_cpu.py), so its static segment must be
empty: static plus dynamic then stays within the stated budget."""
import re

from tests.kernel_isa import ROOT, clean, isa, needs_hipcc

pytestmark = needs_hipcc

LDS_BUDGET = 64 * 1024          # two workgroups share a CU's 160 KiB
LDS_CEILING = 80 * 1024


def _define(name):
    text = (ROOT / "include" / "ipp.h").read_text()
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


def test_feed_resize_kernels_no_spills_no_private_segment_lds_within_budget():
    _, text, ks = isa("ipp_feed_resize")
    resize = [k for k in ks if "k_feed_resize" in (k.get("name") or "")]
    sampled = [k for k in ks if "k_feed_index_map_sampled" in (k.get("name") or "")]
    assert len(resize) == 2 and len(sampled) == 1            # the 2- and the 4-byte instance
    for k in resize + sampled:
        clean(k, text)
    assert _define("IPP_FEED_RESIZE_LDS_BYTES") == LDS_BUDGET <= LDS_CEILING
    for k in resize:
        assert int(k["group_segment_fixed_size"]) == 0, k["name"]
        assert int(k["group_segment_fixed_size"]) + LDS_BUDGET <= LDS_CEILING
        assert int(k["vgpr_count"]) <= 128, k["name"]        # two workgroups of 256 threads per CU need no more
    assert int(sampled[0]["group_segment_fixed_size"]) == 256
