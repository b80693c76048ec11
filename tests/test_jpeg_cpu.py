"""CPU: the restatement of the baseline JPEG rule (tests/jpeg_refs.py, the rule
of include/ipp.h: ipp_jpeg_encode) against the installed Pillow, byte for byte;
the host-built header and tables of image_processor_pipeline_amd/jpeg.py
against Pillow's own files; JpegEncoder's refusals that need no device."""
import io

import numpy as np
import pytest
from PIL import Image

from image_processor_pipeline_amd import jpeg as JP
from tests import jpeg_refs as J
from tests.conftest import GOLDEN, unpack


def pillow_bytes(a, quality, subsampling):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=J.pillow_subsampling(subsampling))
    return b.getvalue()


def golden_composite():
    g = np.load(GOLDEN / "overlays_ref.npz", allow_pickle=False)
    return unpack(g["comp_flat"], g["comp_shapes"])[2][3:80, 20:131].copy()   # 77 x 111, across the pasted overlay


@pytest.mark.parametrize("subsampling", J.SAMPLINGS)
def test_every_size_1_to_34_equals_pillow(subsampling):
    """Widths and heights 1..8, 9..16 and 17..24 (mod 16) take different edge
    paths in 4:2:0 (dummy blocks right, below, both; replication alone)."""
    rng = np.random.default_rng(11)
    total = J.Counters()
    for h in range(1, 35):
        for w in range(1, 35):
            a = rng.integers(0, 256, (h, w, 3), np.uint8)
            got, c = J.encode(a, 75, subsampling)
            assert got == pillow_bytes(a, 75, subsampling), (w, h)
            has_dummy = subsampling == "4:2:0" and (1 <= w % 16 <= 8 or 1 <= h % 16 <= 8)
            assert (c.dummy > 0) == has_dummy, (w, h)
            total.dummy += c.dummy
            total.stuffed += c.stuffed
            total.no_eob += c.no_eob
    assert total.stuffed > 0 and total.no_eob > 0
    assert (total.dummy > 0) == (subsampling == "4:2:0")


def test_default_save_is_quality_75_420():
    a = J.mixed(40, 56)
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG")
    assert b.getvalue() == J.encode(a, 75, "4:2:0")[0]


@pytest.mark.parametrize("subsampling", J.SAMPLINGS)
def test_qualities_and_contents_equal_pillow(subsampling):
    images = {name: make(75, 100) for name, make in J.CONTENTS.items()}
    images["golden"] = golden_composite()
    hit = J.Counters()
    for q in J.QUALITIES:
        for name, a in images.items():
            got, c = J.encode(a, q, subsampling)
            assert got == pillow_bytes(a, q, subsampling), (name, q)
            for f in ("zrl", "no_eob", "stuffed", "dummy", "max_dc_cat", "max_ac_cat"):
                setattr(hit, f, max(getattr(hit, f), getattr(c, f)))
    # the inputs really take every path (on the reference alone)
    assert hit.zrl > 0 and hit.no_eob > 0 and hit.stuffed > 0
    assert (hit.dummy > 0) == (subsampling == "4:2:0")
    assert hit.max_dc_cat >= 8 and hit.max_ac_cat >= 8


def test_mixed_image_takes_every_path_at_once():
    _, c = J.encode(J.mixed(75, 100), 75, "4:2:0")
    assert min(c.zrl, c.no_eob, c.stuffed, c.dummy) > 0


@pytest.mark.parametrize("quality", range(1, 101))
def test_header_and_tables_equal_pillows_file(quality):
    a = J.ramps(20, 37)
    for subsampling in J.SAMPLINGS:
        ref = pillow_bytes(a, quality, subsampling)
        hd = JP.jpeg_header(37, 20, quality, subsampling)
        assert ref[:len(hd)] == hd
        assert hd == J.header(37, 20, quality, subsampling)
    # Image.quantization is de-zigzagged by Pillow (row-major, as jpeg_tables); the file's DQT is in zigzag order
    tabs = Image.open(io.BytesIO(ref)).quantization
    for i, t in enumerate(JP.jpeg_tables(quality)):
        assert t.dtype == np.uint16 and t.shape == (64,)
        assert list(t) == list(tabs[i]), i
        assert bytes(int(v) for v in t[np.array(J.ZIGZAG)]) in hd
        assert list(t) == list(J.quant_tables(quality)[i])


def test_reciprocal_division_is_exact():
    """The kernels' (a · (floor(2^26 / d) + 1)) >> 26 equals a // d for every
    divisor d = 8q and every operand a = |coef| + d / 2 < 2^15; and the
    transform's coefficients stay far below that on the harshest inputs."""
    a = np.arange(1 << 15, dtype=np.uint64)
    for q in range(1, 256):
        d = 8 * q
        m = np.uint64((1 << 26) // d + 1)
        assert m < (1 << 24)
        assert np.array_equal((a * m) >> np.uint64(26), a // np.uint64(d)), q
    worst = 0
    for img in (J.noise(64, 64, 1), J.primaries(64, 64), np.where(J.noise(64, 64, 2) > 127, 255, 0).astype(np.uint8)):
        for p in J.component_planes(img, "4:4:4"):
            worst = max(worst, int(np.abs(J.fdct_islow(p.reshape(8, 8, 8, 8).swapaxes(1, 2) - 128)).max()))
    assert 0 < worst + 1020 < (1 << 15)


def test_capacity_bound_holds():
    for subsampling in J.SAMPLINGS:
        a = J.noise(33, 47, 5)
        body, _ = J.entropy(a, 100, subsampling)
        assert len(body) <= JP.jpeg_capacity_bound(47, 33, subsampling)


@pytest.mark.parametrize("kw, word", [
    (dict(quality=0), "quality"), (dict(quality=101), "quality"), (dict(quality=7.5), "quality"),
    (dict(subsampling="4:2:2"), "4:2:2"), (dict(subsampling="L"), "out of scope"), (dict(subsampling=2), "out of scope"),
    (dict(capacity=0), "capacity"), (dict(n=0), "n must"), (dict(hw=(0, 5)), "size"), (dict(hw=(5, 16385)), "size"),
])
def test_encoder_refusals_without_a_device(kw, word):
    args = dict(device="cuda", n=1, hw=(8, 8))
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        JP.JpegEncoder(**args)
    with pytest.raises(ValueError, match="ROCm device"):
        JP.JpegEncoder("cpu", 1, (8, 8))


def test_header_refusals():
    with pytest.raises(ValueError, match="4:2:2"):
        JP.jpeg_header(8, 8, 75, "4:2:2")
    with pytest.raises(ValueError, match="quality"):
        JP.jpeg_tables(0)
    from image_processor_pipeline_amd import fused
    assert fused.JpegEncoder is JP.JpegEncoder
