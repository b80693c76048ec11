"""Register/scratch/LDS budget of ipp_pipe_scene_amodal's kernels (ipp_label.hip
k_amodal_init, k_amodal_count, k_amodal_map, k_amodal_finish): read from the
amdhsa metadata of their ISA (tests/kernel_isa.py, CPU only); a resource check
only."""
from tests.kernel_isa import clean, isa, needs_hipcc

pytestmark = needs_hipcc


def test_amodal_kernels_no_spills_no_scratch():
    _, text, ks = isa("ipp_label")
    want = ("k_amodal_init", "k_amodal_count", "k_amodal_map", "k_amodal_finish")
    seen = {}
    for k in ks:
        hit = [w for w in want if w in (k.get("name") or "")]
        if hit:
            seen[hit[0]] = k
            clean(k, text)
    assert set(seen) == set(want)
    # k_amodal_count derives from k_scene_visible and k_amodal_map from k_scene_map: no LDS, and few enough
    # vector registers for their 8 waves per SIMD (<= 64 per lane) — the count keeps two counters per later
    # layer and two boxes per lane, the map two 16-B vectors
    for name in ("k_amodal_count", "k_amodal_map"):
        m = seen[name]
        assert int(m["group_segment_fixed_size"]) == 0, name
        assert int(m["vgpr_count"]) + int(m.get("agpr_count", 0)) <= 64, name
