"""Register/scratch/LDS budget of the run-length kernels (ipp_rle.hip
k_rle_*): read from the amdhsa metadata of its ISA alone (tests/kernel_isa.py,
CPU only); a resource check only."""
from tests.kernel_isa import LDS_MAX, isa, needs_hipcc

pytestmark = needs_hipcc

WANT = ("k_rle_count", "k_rle_scan", "k_rle_pack")


def test_rle_kernels_no_spills_no_private_segment():
    _, _, ks = isa("ipp_rle")
    seen = {}
    for k in ks:
        name = k.get("name") or ""
        if "k_rle_" not in name:
            continue
        seen[[w for w in WANT if w in name][0]] = k
        assert int(k.get("vgpr_spill_count", 0)) == 0, name
        assert int(k.get("sgpr_spill_count", 0)) == 0, name
        assert int(k.get("private_segment_fixed_size", 0)) == 0, name
        assert int(k.get("group_segment_fixed_size", 0)) <= LDS_MAX, name
    assert set(seen) == set(WANT)
    # the walkers keep their four columns in registers; the scan needs a few words per wave
    assert int(seen["k_rle_count"]["group_segment_fixed_size"]) == 0
    assert int(seen["k_rle_pack"]["group_segment_fixed_size"]) == 0
    assert 0 < int(seen["k_rle_scan"]["group_segment_fixed_size"]) <= 256
