"""Register/scratch/LDS budget of the training-batch kernels (ipp_feed.hip
k_feed_*): read from the amdhsa metadata of its ISA alone (tests/kernel_isa.py,
CPU only); a resource check only."""
from tests.kernel_isa import isa, needs_hipcc

pytestmark = needs_hipcc

WANT = ("k_feed_images", "k_feed_targets", "k_feed_index_map")
TABLE_BYTES = 3 * 256 * 4       # the widest table of the images kernel
FEW_WORDS = 64


def test_feed_kernels_no_spills_no_private_segment_small_lds():
    _, _, ks = isa("ipp_feed")
    seen = {w: [] for w in WANT}
    for k in ks:
        name = k.get("name") or ""
        if "k_feed_" not in name:
            continue
        seen[[w for w in WANT if w in name][0]].append(k)
        assert int(k.get("vgpr_spill_count", 0)) == 0, name
        assert int(k.get("sgpr_spill_count", 0)) == 0, name
        assert int(k.get("private_segment_fixed_size", 0)) == 0, name
    assert len(seen["k_feed_images"]) == 2 and len(seen["k_feed_targets"]) == 1 and len(seen["k_feed_index_map"]) == 1
    # the table lives in LDS: 3·256 elements of 2 and of 4 bytes for the two instances, 256 bytes for the index map
    lds = sorted(int(k["group_segment_fixed_size"]) for k in seen["k_feed_images"])
    assert TABLE_BYTES // 2 <= lds[0] <= TABLE_BYTES // 2 + FEW_WORDS and TABLE_BYTES <= lds[1] <= TABLE_BYTES + FEW_WORDS
    assert 256 <= int(seen["k_feed_index_map"][0]["group_segment_fixed_size"]) <= TABLE_BYTES + FEW_WORDS
    assert 0 < int(seen["k_feed_targets"][0]["group_segment_fixed_size"]) <= 256
