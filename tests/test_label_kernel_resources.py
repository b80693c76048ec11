"""Register/scratch budget of the label kernels (ipp_label.hip): no VGPR
spills and no scratch in ipp_pipe_overlay_bbox's and ipp_alpha_bbox_min's
kernels.  Reads the amdhsa metadata of the file's ISA (tests/kernel_isa.py,
CPU only), as tests/test_kernel_resources.py does for the pipe."""
from tests.kernel_isa import isa, kernel_res, needs_hipcc

KERNELS = ("k_pipe_overlay_bbox", "k_alpha_bbox_min")


@needs_hipcc
def test_label_kernels_no_spills_no_scratch():
    _, text, ks = isa("ipp_label")
    seen = set()
    for k in ks:
        name = k.get("name") or ""
        hit = [h for h in KERNELS if h in name]
        if not hit:
            continue
        seen.add(hit[0])
        assert int(k.get("vgpr_spill_count", 0)) == 0, name
        assert int(k.get("sgpr_spill_count", 0)) == 0, name
        assert int(k.get("private_segment_fixed_size", 0)) == 0, name
        assert "scratch_" not in kernel_res.body(text, name), name
    assert seen == set(KERNELS)
    # the box kernel runs its taps on the matrix cores
    assert "v_mfma_i32_16x16x64_i8" in kernel_res.body(text, next(
        k["name"] for k in ks if "k_pipe_overlay_bbox" in (k.get("name") or "")))
