"""Register/scratch budget of the hot kernels: no VGPR
spills and no scratch in the pipe, CCL and gather kernels, and the H pass
within the 128 VGPRs that give four blocks per CU (the measured occupancy
lever: 3 blocks per CU made it 14 % slower).  Reads the amdhsa metadata of
the device code hipcc emits (tests/kernel_isa.py: `make` writes
build/obj/ipp_pipe.s; the others are compiled there, CPU only)."""
import pytest

from tests.kernel_isa import isa, kernel_res, needs_hipcc

# every instantiation of the two pipe files: 24 k_pipe_hpass2 (6 range counts,
# zones, 3 or 4 channels), 4 k_pipe_vblend_* (two kernels, MAGIC or not)
PIPE_KERNELS = {"ipp_pipe": 24, "ipp_pipe_vblend": 4}


@needs_hipcc
@pytest.mark.parametrize("name,hot", [("ipp_pipe", ("k_pipe_",)), ("ipp_ccl", ("k_ccl_",)),
                                      ("ipp_gather", ("k_rotate_flip_nearest", "k_copy_rows")),
                                      ("ipp_pipe_vblend", ("k_pipe_",))])
def test_no_spills_no_scratch(name, hot):
    _, text, ks = isa(name)
    checked = 0
    for k in ks:
        if not any(h in k.get("name", "") for h in hot):
            continue
        checked += 1
        assert int(k.get("vgpr_spill_count", 0)) == 0, k["name"]
        # no scratch: none reserved, or (the backend can keep a frame for SGPR
        # spill slots that all went to VGPR lanes) none ever accessed
        if int(k.get("private_segment_fixed_size", 0)):
            assert "scratch_" not in kernel_res.body(text, k["name"]), k["name"]
    if name in PIPE_KERNELS:
        assert checked == PIPE_KERNELS[name]
    else:
        assert checked > 0


@needs_hipcc
def test_hpass_fits_four_blocks_per_cu():
    for k in isa("ipp_pipe")[2]:
        n = k.get("name", "")
        if "k_pipe_hpass2" in n:
            regs = int(k["vgpr_count"]) + int(k.get("agpr_count", 0))
            lds = int(k["group_segment_fixed_size"])
            # 4 waves per SIMD: ≤ 128 registers per lane (the zone forms: 3
            # waves, ≤ 168); 4 blocks per CU: ≤ 40 KB of LDS
            zoned = "Lb1E" in n
            assert regs <= (168 if zoned else 128), n
            assert lds <= 40 * 1024, n
