"""GPU: the device JPEG encoder (ipp_jpeg_encode, ipp_jpeg_pack, JpegEncoder,
the overlays plugin's device_jpeg option) against the installed Pillow, byte
for byte.  tests/jpeg_refs.py supplies the coverage counters: per case the
dummy blocks its geometry must have, and over each sweep that stuffing, ZRL
and blocks without EOB occur in the reference streams (a 1x1 image cannot show
them alone)."""
import io
import random

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_refs as J
from tests.conftest import GOLDEN, unpack

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (33, 17), (24, 40), (48, 32), (100, 75), (256, 192)]   # (w, h)
CANARY = 0xA5


@pytest.fixture(scope="module")
def env():
    import torch
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import jpeg as JP
    assert torch.cuda.is_available()
    return torch, N, JP, N.load(), torch.device("cuda:0")


def pillow_bytes(a, quality, subsampling):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=J.pillow_subsampling(subsampling))
    return b.getvalue()


def three(h, w):
    return [J.mixed(h, w), J.noise(h, w, 7), J.primaries(h, w)]


@pytest.mark.parametrize("subsampling", J.SAMPLINGS)
def test_shapes_equal_pillow(env, subsampling):
    torch, N, JP, lib, dev = env
    seen = J.Counters()
    for w, h in SHAPES:
        imgs = three(h, w)
        for n in (1, 3):
            enc = JP.JpegEncoder(dev, 3, (h, w), 75, subsampling)
            got = enc.encode(torch.from_numpy(np.stack(imgs[:n])).to(dev))
            assert len(got) == n
            for i in range(n):
                assert got[i] == pillow_bytes(imgs[i], 75, subsampling), (w, h, n, i)
        for a in imgs:
            c = J.encode(a, 75, subsampling)[1]
            assert (c.dummy > 0) == (subsampling == "4:2:0" and (1 <= w % 16 <= 8 or 1 <= h % 16 <= 8)), (w, h)
            seen.zrl += c.zrl
            seen.no_eob += c.no_eob
            seen.stuffed += c.stuffed
            seen.dummy += c.dummy
    assert seen.zrl > 0 and seen.no_eob > 0 and seen.stuffed > 0
    assert (seen.dummy > 0) == (subsampling == "4:2:0")


@pytest.mark.parametrize("subsampling", J.SAMPLINGS)
def test_qualities_and_contents_equal_pillow(env, subsampling):
    torch, N, JP, lib, dev = env
    g = np.load(GOLDEN / "overlays_ref.npz", allow_pickle=False)
    gold = unpack(g["comp_flat"], g["comp_shapes"])[2][3:78, 20:120].copy()    # 75 x 100 of a golden composite
    imgs = [make(75, 100) for make in J.CONTENTS.values()] + [gold]
    dev_imgs = torch.from_numpy(np.stack(imgs)).to(dev)
    hit = J.Counters()
    for q in J.QUALITIES:
        # noise at quality 100 is longer than the raw image: the default capacity refuses it (tested below)
        cap = JP.jpeg_capacity_bound(100, 75, subsampling) if q == 100 else None
        got = JP.JpegEncoder(dev, len(imgs), (75, 100), q, subsampling, capacity=cap).encode(dev_imgs)
        for i, a in enumerate(imgs):
            assert got[i] == pillow_bytes(a, q, subsampling), (q, i)
            c = J.encode(a, q, subsampling)[1]
            for f in ("zrl", "no_eob", "stuffed", "dummy", "max_dc_cat", "max_ac_cat"):
                setattr(hit, f, max(getattr(hit, f), getattr(c, f)))
    assert hit.zrl > 0 and hit.no_eob > 0 and hit.stuffed > 0 and hit.max_dc_cat >= 8 and hit.max_ac_cat >= 8
    assert (hit.dummy > 0) == (subsampling == "4:2:0")


def _raw_call(env, imgs, quality, subsampling, capacity):
    """ipp_jpeg_encode on canary-filled slots and scratch with guard bands:
    (hdr, slots as (n, pitch), slot guard, scratch guard)."""
    torch, N, JP, lib, dev = env
    n, h, w = len(imgs), imgs[0].shape[0], imgs[0].shape[1]
    sampling = JP.SAMPLINGS[subsampling]
    pitch = (capacity + 15) // 16 * 16
    nb = lib.ipp_jpeg_scratch_bytes(n, w, h, sampling, capacity)
    assert nb > 0 and nb % 256 == 0
    scratch = torch.full((nb + 256,), CANARY, dtype=torch.uint8, device=dev)
    slots = torch.full((n * pitch + 256,), CANARY, dtype=torch.uint8, device=dev)
    hdr = torch.full((n * N.IPP_JPEG_HDR,), -7, dtype=torch.int32, device=dev)
    qtab = np.ascontiguousarray(np.concatenate(JP.jpeg_tables(quality)), np.uint16)
    d = torch.from_numpy(np.stack(imgs)).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    N.check(lib.ipp_jpeg_encode(d.data_ptr(), n, w, h, sampling, N.np_ptr(qtab), scratch.data_ptr(), slots.data_ptr(),
                                capacity, hdr.data_ptr(), st), "ipp_jpeg_encode")
    torch.cuda.synchronize()
    s = slots.cpu().numpy()
    return (hdr.cpu().numpy().reshape(n, 2), s[:n * pitch].reshape(n, pitch), s[n * pitch:],
            scratch.cpu().numpy()[nb:])


@pytest.mark.parametrize("subsampling", J.SAMPLINGS)
def test_capacity_refusal_and_extents(env, subsampling):
    torch, N, JP, lib, dev = env
    h, w = 32, 48
    imgs = [J.ramps(h, w), J.noise(h, w, 9), J.constant(h, w)]
    want = [J.entropy(a, 100, subsampling)[0] for a in imgs]
    assert J.entropy(imgs[1], 100, subsampling)[1].stuffed > 0
    capacity = (max(len(want[0]), len(want[2])) + len(want[1])) // 2
    assert max(len(want[0]), len(want[2])) < capacity < len(want[1])
    hdr, slots, slot_guard, scratch_guard = _raw_call(env, imgs, 100, subsampling, capacity)
    assert (slot_guard == CANARY).all() and (scratch_guard == CANARY).all()
    for i in (0, 2):
        assert tuple(hdr[i]) == (len(want[i]), 0)
        assert slots[i, :len(want[i])].tobytes() == want[i]
        assert (slots[i, len(want[i]):] == CANARY).all()
    assert hdr[1, 1] == N.IPP_JPEG_OVERFLOW and hdr[1, 0] > capacity
    assert (slots[1] == CANARY).all()                      # no byte of the refused image
    enc = JP.JpegEncoder(dev, 3, (h, w), 100, subsampling, capacity=capacity)
    d = torch.from_numpy(np.stack(imgs)).to(dev)
    with pytest.raises(ValueError, match=r"image 1: .*capacity") as e:
        enc.encode(d)
    assert "image 0" not in str(e.value) and "image 2" not in str(e.value)
    with pytest.raises(ValueError, match=r"b\.jpg"):
        enc.encode(d, names=["a.jpg", "b.jpg", "c.jpg"])
    # a stream that fits unstuffed but not stuffed is refused after the second scan, as cleanly
    body, c = J.entropy(imgs[1], 100, subsampling)
    tight = len(body) - 1
    assert tight >= len(body) - c.stuffed
    hdr, slots, slot_guard, _ = _raw_call(env, imgs[1:2], 100, subsampling, tight)
    assert tuple(hdr[0]) == (len(body), N.IPP_JPEG_OVERFLOW) and (slots == CANARY).all() and (slot_guard == CANARY).all()
    hdr, slots, _, _ = _raw_call(env, imgs[1:2], 100, subsampling, len(body))
    assert tuple(hdr[0]) == (len(body), 0) and slots[0, :len(body)].tobytes() == body


def test_pack_writes_only_the_streams(env):
    torch, N, JP, lib, dev = env
    h, w = 33, 17
    imgs = three(h, w)
    enc = JP.JpegEncoder(dev, 3, (h, w), 75, "4:2:0")
    hdr = enc.encode_device(torch.from_numpy(np.stack(imgs)).to(dev))
    sizes = hdr[:, 0].astype(np.int64)
    offsets = np.array([5, 5 + sizes[0] + 3, 5 + sizes[0] + 3 + sizes[1] + 16], np.int64)   # unaligned on purpose
    total = int(offsets[2] + sizes[2] + 9)
    out = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    N.check(lib.ipp_jpeg_pack(enc.slots.data_ptr(), enc.capacity, enc.hdr.data_ptr(), 3,
                              torch.from_numpy(offsets).to(dev).data_ptr(), out.data_ptr(), st), "ipp_jpeg_pack")
    host = out.cpu().numpy()
    mask = np.ones(total, bool)
    for i, a in enumerate(imgs):
        o, s = int(offsets[i]), int(sizes[i])
        assert host[o:o + s].tobytes() == J.entropy(a, 75, "4:2:0")[0], i
        mask[o:o + s] = False
    assert (host[mask] == CANARY).all()


def test_abi_refusals(env):
    torch, N, JP, lib, dev = env
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    p = buf.data_ptr()
    q = np.ascontiguousarray(np.concatenate(JP.jpeg_tables(75)), np.uint16)
    ok = dict(inp=p, n=1, w=8, h=8, s=0, q=N.np_ptr(q), scratch=p + 4096, slots=p + 32768, cap=1024, hdr=p + 60000)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ipp_jpeg_encode(a["inp"], a["n"], a["w"], a["h"], a["s"], a["q"], a["scratch"], a["slots"], a["cap"],
                                   a["hdr"], None)
    bad_q = q.copy()
    bad_q[5] = 0
    for kw in (dict(inp=None), dict(q=None), dict(scratch=None), dict(slots=None), dict(hdr=None), dict(n=-1),
               dict(n=65536), dict(w=0), dict(h=16385), dict(s=2), dict(cap=0), dict(cap=1 << 31),
               dict(scratch=p + 4100), dict(slots=p + 32772), dict(hdr=p + 60001), dict(q=N.np_ptr(bad_q))):
        assert call(**kw) == N.IPP_E_ARG, kw
    assert call(n=0) == N.IPP_OK
    assert lib.ipp_jpeg_scratch_bytes(1, 0, 8, 0, 64) == N.IPP_E_ARG
    assert lib.ipp_jpeg_scratch_bytes(0, 8, 8, 0, 64) >= 0
    assert lib.ipp_jpeg_pack(None, 64, p, 1, p, p, None) == N.IPP_E_ARG
    assert lib.ipp_jpeg_pack(p, 64, p, 1, p + 4, p, None) == N.IPP_E_ARG
    assert lib.ipp_jpeg_pack(p, 64, p, 0, p, p, None) == N.IPP_OK
    enc = JP.JpegEncoder(dev, 2, (8, 8))
    for bad, word in ((torch.zeros((1, 8, 8, 3), dtype=torch.float32, device=dev), "uint8"),
                      (torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=dev), "RGBA"),
                      (torch.zeros((1, 8, 8), dtype=torch.uint8, device=dev), "greyscale"),
                      (torch.zeros((1, 8, 9, 3), dtype=torch.uint8, device=dev), "size"),
                      (torch.zeros((3, 8, 8, 3), dtype=torch.uint8, device=dev), "at most"),
                      (torch.zeros((1, 8, 8, 3), dtype=torch.uint8), "images are on cpu")):
        with pytest.raises(ValueError, match=word):
            enc.encode(bad)
    assert enc.encode(torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=dev)) == []


def test_save_writes_pillows_files(env, tmp_path):
    torch, N, JP, lib, dev = env
    imgs = three(75, 100)
    paths = [tmp_path / f"{i}.jpg" for i in range(3)]
    JP.JpegEncoder(dev, 3, (75, 100), 90).save(torch.from_numpy(np.stack(imgs)).to(dev), paths, threads=2)
    for p, a in zip(paths, imgs):
        assert p.read_bytes() == pillow_bytes(a, 90, "4:2:0")


def test_plugin_device_jpeg_writes_identical_files(env, tmp_path):
    """.jpg backgrounds of odd sizes (100 x 150 and 120 x 160: dummy blocks and
    both replications) from the overlays fixture; a .png background takes the
    host path either way."""
    from image_processor_pipeline_amd.transforms import overlays
    g = np.load(GOLDEN / "overlays_ref.npz", allow_pickle=False)
    ovs = unpack(g["ov_flat"], g["ov_shapes"])
    bgs = unpack(g["bg_flat"], g["bg_shapes"])
    pairs = []
    for k, (ov, bg) in enumerate(zip(ovs, bgs)):
        po, pb = tmp_path / f"ov{k}.png", tmp_path / f"bg{k}{'.png' if k == 1 else '.jpg'}"
        Image.fromarray(ov, "RGBA").save(po)
        Image.fromarray(bg[:, :-1] if k == 2 else bg, "RGB").save(pb, **({} if k == 1 else dict(quality=95)))
        pairs.append((po, pb))

    def run(name, batch, **opts):
        di, dl = tmp_path / f"{name}_img", tmp_path / f"{name}_lbl"
        di.mkdir()
        dl.mkdir()
        random.seed(5)
        if batch:
            res = overlays.paste_overlay_onto_background.batch(pairs, [di, dl], **opts)
        else:
            res = [overlays.paste_overlay_onto_background(po, pb, [di, dl], **opts) for po, pb in pairs]
        assert all(r is not None and len(r) == 2 for r in res), res
        return [(r[0].name, r[0].read_bytes(), r[1].read_text()) for r in res]

    host = run("host", True)
    assert run("dev", True, device_jpeg=True) == host
    assert run("dev_file", False, device_jpeg=True) == host
    assert run("host_file", False, device_jpeg=False) == host
    assert [n.rsplit(".", 1)[1] for n, _, _ in host] == ["jpg", "png", "jpg"]
    assert Image.open(tmp_path / "bg2.jpg").size == (149, 100)
