"""Register/scratch/LDS budget of the JPEG decode kernels
(ipp_jpeg_decode.hip k_jpegd_*): read from the amdhsa metadata of its ISA
alone (tests/kernel_isa.py, CPU only); a resource check only."""
from tests.kernel_isa import clean, isa, needs_hipcc

pytestmark = needs_hipcc

WANT = ("k_jpegd_segs", "k_jpegd_zero", "k_jpegd_huff", "k_jpegd_write", "k_jpegd_dc", "k_jpegd_idct")


def test_jpeg_decode_kernels_no_spills_no_scratch():
    _, text, ks = isa("ipp_jpeg_decode")
    seen = {}
    for k in ks:
        name = k.get("name") or ""
        hit = [w for w in WANT if w in name]
        if not hit:
            continue
        seen[hit[0]] = k
        clean(k, text)
    assert set(seen) == set(WANT)
    # six Huffman tables (17 limits, 17 offsets, a 256-entry 16-bit lookahead, 256 symbols) and a flag or the
    # scan's four partial sums: no stream byte and no state is staged in LDS
    tables = 6 * (17 * 4 + 17 * 4 + 256 * 2 + 256)
    assert int(seen["k_jpegd_huff"]["group_segment_fixed_size"]) <= tables + 16
    assert int(seen["k_jpegd_write"]["group_segment_fixed_size"]) <= tables + 16 + 4     # and the lanes' largest fault
    assert int(seen["k_jpegd_zero"]["group_segment_fixed_size"]) == 0
    # the two chroma planes of a 128 x 128 tile, a byte a sample
    assert int(seen["k_jpegd_idct"]["group_segment_fixed_size"]) <= 2 * 128 * 128
    # 32 KiB of LDS allows five workgroups (20 waves) a CU, five a SIMD: 96 registers would be needed to fill them,
    # and a block's 64 samples with a row of chroma do not fit that; two waves a SIMD (up to 256) is the occupancy
    # chosen, and the kernel stands at 194: the ceiling leaves a few registers, not a third more
    assert int(seen["k_jpegd_idct"]["vgpr_count"]) <= 200
    # the entropy lanes wait on dependent loads: eight waves a SIMD hide them
    assert int(seen["k_jpegd_huff"]["vgpr_count"]) <= 64
    assert int(seen["k_jpegd_write"]["vgpr_count"]) <= 64
