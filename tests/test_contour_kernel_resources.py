"""Register/scratch/LDS budget of the contour kernels (ipp_contour.hip
k_contour_*): read from the amdhsa metadata of their ISA alone
(tests/kernel_isa.py, CPU only); a resource check only."""
from tests.kernel_isa import LDS_MAX, isa, needs_hipcc

pytestmark = needs_hipcc

WANT = ("k_contour_emit", "k_contour_link", "k_contour_jump", "k_contour_select", "k_contour_header",
        "k_contour_pack")


def test_contour_kernels_no_spills_no_private_segment():
    _, _, ks = isa("ipp_contour")
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
