"""Register/scratch/LDS budget of the scene kernels: the in-place V kernel
(ipp_pipe_vblend.hip k_pipe_vblend_over) and ipp_pipe_scene_boxes' kernels
(ipp_label.hip).  Reads the amdhsa metadata of their ISA (tests/kernel_isa.py,
CPU only); a resource check only."""
from tests.kernel_isa import clean, isa, needs_hipcc

pytestmark = needs_hipcc


def test_inplace_v_kernel_matches_its_sibling():
    _, text, ks = isa("ipp_pipe_vblend")
    over = {k["name"]: k for k in ks if "k_pipe_vblend_over" in (k.get("name") or "")}
    sib = {k["name"]: k for k in ks if "k_pipe_vblend_mfma" in (k.get("name") or "")}
    assert len(over) == 2 and len(sib) == 2                    # MAGIC and the reciprocal form of each
    for name, k in over.items():
        clean(k, text)
        twin = next(s for n, s in sib.items() if ("ILb1E" in n) == ("ILb1E" in name))     # same MAGIC flag
        # the same static LDS (both take their rows as dynamic LDS sized by the
        # host from one formula) and the same occupancy class (≤ 160 registers
        # per lane: 3 waves per SIMD)
        assert int(k["group_segment_fixed_size"]) == int(twin["group_segment_fixed_size"]), name
        regs = int(k["vgpr_count"]) + int(k.get("agpr_count", 0))
        assert regs <= 160, (name, regs)


def test_scene_label_kernels_no_spills_no_scratch():
    _, text, ks = isa("ipp_label")
    want = ("k_scene_init", "k_scene_alpha", "k_scene_visible", "k_scene_finish")
    seen = set()
    for k in ks:
        hit = [w for w in want if w in (k.get("name") or "")]
        if hit:
            seen.add(hit[0])
            clean(k, text)
    assert seen == set(want)
