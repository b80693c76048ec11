"""CPU: the restatement of the decoding rule (tests/jpeg_decode_refs.py, what
include/ipp.h states under ipp_jpeg_decode) against the installed Pillow, and
jpeg.parse_jpeg on the files Pillow writes.  No GPU."""
import io

import numpy as np
import pytest
from PIL import Image

from image_processor_pipeline_amd import jpeg as JP
from tests import jpeg_decode_refs as R
from tests import jpeg_refs as J

SHAPES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (33, 17), (24, 40), (48, 32), (100, 75), (2, 15), (3, 5),
          (4, 17), (5, 3), (6, 2), (16, 1), (35, 18)]   # (w, h): the GPU sweep's; its 256 x 192 files are below


def save(a, mode="RGB", **kw):
    b = io.BytesIO()
    Image.fromarray(a).convert(mode).save(b, "JPEG", **kw)
    return b.getvalue()


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def agree(data):
    got = R.decode(data, JP.parse_jpeg(data))
    return np.array_equal(got, pillow(data))


@pytest.mark.parametrize("subsampling", (2, 0))
def test_restatement_equals_pillow_over_shapes(subsampling):
    for w, h in SHAPES:
        for make in (J.mixed, J.noise, J.primaries):
            assert agree(save(make(h, w), quality=75, subsampling=subsampling)), (w, h, make.__name__)


@pytest.mark.parametrize("subsampling", (2, 0))
def test_restatement_equals_pillow_over_qualities_and_contents(subsampling):
    for q in J.QUALITIES:
        for name, make in J.CONTENTS.items():
            assert agree(save(make(40, 52), quality=q, subsampling=subsampling)), (q, name)


def test_restatement_equals_pillow_on_the_large_files():
    """The GPU sweep's 256 x 192 files: three contents at quality 75 and both
    samplings are too slow for the plain-Python entropy decoder, so one
    content of the shape sweep and the three files of the synchronisation test
    stand for them (the per-sample arithmetic does not depend on the size)."""
    for a, kw in ((J.mixed(192, 256), dict(quality=75)), (J.noise(192, 256, 2), dict(quality=95)),
                  (J.constant(192, 256), dict(quality=75)), (J.primaries(192, 256), dict(quality=75)),
                  (J.mixed(75, 100), dict(quality=100, subsampling=0))):
        assert agree(save(a, **kw)), kw


def test_restatement_equals_pillow_with_own_tables_and_restarts():
    for kw in (dict(optimize=True), dict(restart_marker_rows=1), dict(restart_marker_blocks=1),
               dict(optimize=True, subsampling=0, restart_marker_blocks=1)):
        for make in (J.mixed, J.constant):
            assert agree(save(make(75, 100), quality=90, **kw)), kw


def test_parse_jpeg_fields():
    a = J.mixed(33, 47)
    f = JP.parse_jpeg(save(a))
    assert (f.w, f.h, f.subsampling, f.restart_interval) == (47, 33, "4:2:0", 0)
    assert f.qt == (0, 1, 1) and f.dc == (0, 1, 1) and f.ac == (0, 1, 1)
    lum, chrom = J.quant_tables(75)
    assert np.array_equal(f.qtables[0], lum) and np.array_equal(f.qtables[1], chrom)
    assert f.htables[(0, 0)] == (bytes(J.DC_LUMA[0]), bytes(J.DC_LUMA[1]))
    assert f.htables[(1, 1)] == (bytes(J.AC_CHROMA[0]), bytes(J.AC_CHROMA[1]))
    data = save(a)
    assert data[f.span[1]:] == b"\xff\xd9" and data[f.span[0] - 3:f.span[0]] == bytes((0, 63, 0))
    assert data[f.span[0]:f.span[1]] == J.entropy(a, 75, "4:2:0")[0]
    assert JP.parse_jpeg(save(a, subsampling=0)).subsampling == "4:4:4"
    opt = JP.parse_jpeg(save(a, optimize=True))
    assert opt.htables[(1, 0)] != f.htables[(1, 0)] and sum(opt.htables[(1, 0)][0]) == len(opt.htables[(1, 0)][1])
    assert JP.parse_jpeg(save(a, restart_marker_rows=1)).restart_interval == 3        # ⌈47 / 16⌉ MCUs a row
    assert JP.parse_jpeg(save(a, restart_marker_blocks=1)).restart_interval == 1
    # APPn and COM segments are skipped
    withcom = data[:2] + b"\xff\xfe\x00\x05abc" + b"\xff\xe1\x00\x04xy" + data[2:]
    g = JP.parse_jpeg(withcom)
    assert (g.w, g.h, g.span) == (47, 33, (f.span[0] + 13, f.span[1] + 13))


@pytest.mark.parametrize("kw,mode,word", [(dict(progressive=True), "RGB", "progressive"),
                                          (dict(subsampling=1), "RGB", "4:2:2"), (dict(), "L", "greyscale"),
                                          (dict(), "CMYK", "CMYK")])
def test_parse_jpeg_refuses_by_name(kw, mode, word):
    with pytest.raises(ValueError, match=word):
        JP.parse_jpeg(save(J.mixed(16, 24), mode, **kw))


def test_parse_jpeg_refuses_bad_headers():
    data = save(J.mixed(16, 24))
    f = JP.parse_jpeg(data)
    for cut in (1, 3, 30, f.span[0] - 5):
        with pytest.raises(ValueError, match="truncated header|not a JPEG"):
            JP.parse_jpeg(data[:cut])
    sof = data.index(b"\xff\xc0")
    with pytest.raises(ValueError, match="12-bit"):
        JP.parse_jpeg(data[:sof + 4] + bytes((12,)) + data[sof + 5:])
    big = (20000).to_bytes(2, "big")
    with pytest.raises(ValueError, match="IPP_JPEG_MAX_SIDE"):
        JP.parse_jpeg(data[:sof + 5] + big + data[sof + 7:])
    dqt = data.index(b"\xff\xdb")
    with pytest.raises(ValueError, match="16-bit"):
        JP.parse_jpeg(data[:dqt + 4] + bytes((0x10,)) + data[dqt + 5:])
    with pytest.raises(ValueError, match="more than one scan"):
        JP.parse_jpeg(data[:-2] + data[f.span[0] - 14:])
