"""Register/scratch/LDS budget of the oriented-box kernel (ipp_obb.hip
k_obb_*): read from the amdhsa metadata of its ISA alone (tests/kernel_isa.py,
CPU only); a resource check only."""
from tests.kernel_isa import LDS_MAX, isa, needs_hipcc

pytestmark = needs_hipcc

WANT = ("k_obb_rings",)


def test_obb_kernels_no_spills_no_private_segment():
    from image_processor_pipeline_amd import _native as N
    _, _, ks = isa("ipp_obb")
    seen = {}
    for k in ks:
        name = k.get("name") or ""
        if "k_obb_" not in name:
            continue
        seen[[w for w in WANT if w in name][0]] = k
        assert int(k.get("vgpr_spill_count", 0)) == 0, name
        assert int(k.get("sgpr_spill_count", 0)) == 0, name
        assert int(k.get("private_segment_fixed_size", 0)) == 0, name
        assert int(k.get("group_segment_fixed_size", 0)) <= LDS_MAX, name
    assert set(seen) == set(WANT)
    # the row window (least and greatest x: 8 B per row), the two chains (4 B per point) and a few words of state
    lds = int(seen["k_obb_rings"]["group_segment_fixed_size"])
    want = 8 * N.IPP_OBB_LDS_ROWS + 8 * N.IPP_OBB_LDS_HULL
    assert want <= lds <= want + 512
