"""Register/scratch/LDS budget of the JPEG kernels (ipp_jpeg.hip k_jpeg_*):
read from the amdhsa metadata of its ISA alone (tests/kernel_isa.py, CPU
only); a resource check only."""
from tests.kernel_isa import clean, isa, needs_hipcc

pytestmark = needs_hipcc

WANT = ("k_jpeg_dct", "k_jpeg_scan", "k_jpeg_zero", "k_jpeg_write", "k_jpeg_ffcount", "k_jpeg_ffscan",
        "k_jpeg_stuff", "k_jpeg_pack")


def test_jpeg_kernels_no_spills_no_scratch():
    _, text, ks = isa("ipp_jpeg")
    seen = {}
    for k in ks:
        name = k.get("name") or ""
        hit = [w for w in WANT if w in name]
        if not hit:
            continue
        seen[hit[0]] = k
        clean(k, text)
    assert set(seen) == set(WANT)
    # a block's 64 samples live in registers: the transform keeps no LDS but the Huffman tables
    assert int(seen["k_jpeg_dct"]["group_segment_fixed_size"]) <= 2 * 256 * 4 + 2 * 16 * 4
    assert int(seen["k_jpeg_write"]["group_segment_fixed_size"]) <= 2 * 256 * 4 + 2 * 16 * 4
    assert int(seen["k_jpeg_zero"]["group_segment_fixed_size"]) == 0
    assert int(seen["k_jpeg_pack"]["group_segment_fixed_size"]) == 0
    # three waves per SIMD at least for the transform
    assert int(seen["k_jpeg_dct"]["vgpr_count"]) <= 168   # three waves per SIMD
