"""Register/scratch/LDS budget of ipp_pipe_scene_cull's kernels (ipp_label.hip
k_cull_count, k_cull_clear), and the numbers of the pipe and scene kernels that
were there before them, which adding the cull must not move: read from the
amdhsa metadata of their ISA (tests/kernel_isa.py, CPU only); a resource check
only."""
import re

from tests.kernel_isa import clean, isa, needs_hipcc

pytestmark = needs_hipcc


def _numbers(k):
    return (int(k["vgpr_count"]), int(k.get("agpr_count", 0)), int(k["sgpr_count"]),
            int(k["group_segment_fixed_size"]))


def test_cull_kernels_no_spills_no_scratch():
    _, text, ks = isa("ipp_label")
    want = ("k_cull_count", "k_cull_clear")
    seen = {}
    for k in ks:
        hit = [w for w in want if w in (k.get("name") or "")]
        if hit:
            seen[hit[0]] = k
            clean(k, text)
    assert set(seen) == set(want)
    for k in seen.values():
        # no LDS, no AGPRs, and few enough registers for 8 waves per SIMD (<= 64 per lane): the count walk is
        # k_scene_visible's (byte loads hidden by occupancy), the clear a stream of 16-B stores
        assert int(k["group_segment_fixed_size"]) == 0 and int(k.get("agpr_count", 0)) == 0
        assert int(k["vgpr_count"]) <= 64


# (vgpr, agpr, sgpr, static LDS) of the kernels of ipp_label.hip as they were before the cull was added to the file
LABEL_BEFORE = {
    "k_pipe_overlay_bbox": (52, 12, 44, 0),
    "k_scene_init": (12, 0, 14, 0),
    "k_scene_finish": (4, 0, 11, 0),
    "k_scene_alpha": (76, 12, 38, 0),
    "k_scene_visible": (20, 0, 60, 0),
    "k_scene_table": (8, 0, 14, 0),
    "k_scene_map": (16, 0, 79, 0),
}


# the file's other nine kernels, as they were before the scene kernels came to share their device helpers
LABEL_BEFORE_SHARING = {
    "k_label_bbox_init": (6, 0, 11, 0),
    "k_label_bbox_finish": (4, 0, 11, 0),
    "k_alpha_bbox_min": (16, 0, 26, 0),
    "k_cull_count": (16, 0, 64, 0),
    "k_cull_clear": (11, 0, 20, 0),
    "k_amodal_init": (7, 0, 22, 0),
    "k_amodal_finish": (6, 0, 11, 0),
    "k_amodal_count": (52, 0, 104, 0),
    "k_amodal_map": (20, 0, 79, 0),
}


def test_the_label_files_other_kernels_are_unchanged():
    _, text, ks = isa("ipp_label")
    want_all = {**LABEL_BEFORE, **LABEL_BEFORE_SHARING}
    seen = {}
    for k in ks:
        for short, want in want_all.items():
            if re.search(r"\d+" + short + "E", k.get("name") or ""):
                seen[short] = _numbers(k)
                if short in LABEL_BEFORE_SHARING:
                    clean(k, text)      # no private segment either
    assert seen == want_all


# the V kernels (ipp_pipe_vblend.hip), by template argument MAGIC
VBLEND_BEFORE = {
    ("k_pipe_vblend_over", 1): (138, 0, 66, 0), ("k_pipe_vblend_over", 0): (138, 0, 68, 0),
    ("k_pipe_vblend_mfma", 1): (138, 0, 82, 0), ("k_pipe_vblend_mfma", 0): (136, 0, 86, 0),
}


def test_the_v_kernels_are_unchanged():
    _, _, ks = isa("ipp_pipe_vblend")
    seen = {}
    for k in ks:
        m = re.search(r"(k_pipe_vblend_over|k_pipe_vblend_mfma)ILb([01])E", k.get("name") or "")
        if m:
            seen[(m.group(1), int(m.group(2)))] = _numbers(k)
    assert seen == VBLEND_BEFORE


# the H kernel (ipp_pipe.hip k_pipe_hpass2<NR, ZONES, CN>): VGPRs of the zone forms by (NR, CN); the forms
# without zones take 128; 106 SGPRs all; static LDS 37328 bytes, 38400 with 16 ranges
HPASS_ZONES_VGPR = {(1, 4): 135, (1, 3): 135, (2, 4): 133, (2, 3): 135, (3, 4): 133, (3, 3): 133,
                    (4, 4): 135, (4, 3): 133, (6, 4): 137, (6, 3): 135, (16, 4): 143, (16, 3): 143}


def test_the_h_kernels_are_unchanged():
    _, _, ks = isa("ipp_pipe")
    n = 0
    for k in ks:
        m = re.search(r"k_pipe_hpass2ILi(\d+)ELb([01])ELi([34])EEE", k.get("name") or "")
        if not m:
            continue
        nr, zones, cn = int(m.group(1)), int(m.group(2)), int(m.group(3))
        want = (HPASS_ZONES_VGPR[(nr, cn)] if zones else 128, 0, 106, 38400 if nr == 16 else 37328)
        assert _numbers(k) == want, k["name"]
        n += 1
    assert n == 2 * len(HPASS_ZONES_VGPR)
