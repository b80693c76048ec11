"""Baseline JPEG files of RGB composites, encoded on the device: byte for byte
the file ``Image.fromarray(a).save(path, quality=q)`` writes (Pillow 12.2.0,
libjpeg-turbo 3.1; include/ipp.h states the rule under ipp_jpeg_encode).

The header (SOI, APP0 JFIF, DQT, SOF0, DHT, SOS) and the EOI are built here in
plain Python — no imaging library is called — and the entropy-coded data come
from the kernels: ``ipp_jpeg_encode`` leaves each image's bytes in a slot and a
header (bytes, status); the headers are copied back, ``ipp_jpeg_pack`` compacts
the streams, and one more copy brings back exactly the files' bytes.

Out of scope, refused by name: "4:2:2" and other samplings, greyscale and RGBA
inputs, optimised Huffman tables, progressive files, restart markers, EXIF /
ICC / dpi / comments, images of different sizes in one call.

The other way, ``parse_jpeg`` walks a file's markers (plain Python too) and
``JpegDecoder`` decodes baseline files on the device to the pixels
``Image.open(f).convert("RGB")`` gives (ipp.h: ipp_jpeg_decode); progressive,
greyscale, CMYK, "4:2:2", 12-bit and multi-scan files are refused by name.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N

# Annex K.1 / K.2 (row-major) and K.3 ((BITS, HUFFVAL) per table)
_LUMA_Q = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
           14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_CHROMA_Q = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
             47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
           7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
           39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
_DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
_AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435"
    "363738393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798"
    "999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4"
    "f5f6f7f8f9fa"))
_AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a"
    "35363738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a9293949596"
    "9798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4"
    "f5f6f7f8f9fa"))

SAMPLINGS = {"4:2:0": N.IPP_JPEG_420, "4:4:4": N.IPP_JPEG_444}
_EOI = b"\xff\xd9"


def _check_quality(quality) -> int:
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be an integer in 1..100, got {quality!r}")
    return int(quality)


def _check_sampling(subsampling) -> int:
    if subsampling not in SAMPLINGS:
        raise ValueError(f"subsampling {subsampling!r} is out of scope: the device encoder writes \"4:2:0\" (Pillow's "
                         f"default for RGB) and \"4:4:4\" only (\"4:2:2\", greyscale and RGBA are not supported)")
    return SAMPLINGS[subsampling]


def jpeg_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """(luma, chroma) quantisation tables of jpeg_set_quality(quality,
    force_baseline): 64 uint16 each, row-major (not zigzag)."""
    q = _check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.array([min(max((t * s + 50) // 100, 1), 255) for t in tab], np.uint16)
                 for tab in (_LUMA_Q, _CHROMA_Q))


def _segment(marker: int, body: bytes) -> bytes:
    return bytes((0xFF, marker)) + (len(body) + 2).to_bytes(2, "big") + body


def jpeg_header(w: int, h: int, quality: int, subsampling: str = "4:2:0") -> bytes:
    """Everything before the entropy-coded data: SOI, APP0 (JFIF 1.01, aspect
    1:1 without unit, no thumbnail), one DQT per table (zigzag), SOF0 (8 bit,
    three components, luma 2x2 or 1x1), one DHT per table in the order DC0,
    AC0, DC1, AC1, and the SOS of the single scan."""
    sampling = _check_sampling(subsampling)
    if not (1 <= int(w) <= N.IPP_JPEG_MAX_SIDE and 1 <= int(h) <= N.IPP_JPEG_MAX_SIDE):
        raise ValueError(f"image size {w}x{h} outside 1..{N.IPP_JPEG_MAX_SIDE}")
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes((1, 1, 0, 0, 1, 0, 1, 0, 0)))
    for i, t in enumerate(jpeg_tables(quality)):
        out += _segment(0xDB, bytes((i,)) + bytes(int(t[z]) for z in _ZIGZAG))
    luma = 0x22 if sampling == N.IPP_JPEG_420 else 0x11
    out += _segment(0xC0, bytes((8,)) + int(h).to_bytes(2, "big") + int(w).to_bytes(2, "big") +
                    bytes((3, 1, luma, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for tc_th, (bits, vals) in ((0x00, _DC_LUMA), (0x10, _AC_LUMA), (0x01, _DC_CHROMA), (0x11, _AC_CHROMA)):
        out += _segment(0xC4, bytes((tc_th,)) + bytes(bits) + bytes(vals))
    return out + _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def _mcu_grid(w: int, h: int, sampling: int) -> Tuple[int, int, int]:
    """(MCU columns, MCU rows, MCU side in px)."""
    side = 16 if sampling == N.IPP_JPEG_420 else 8
    return (w + side - 1) // side, (h + side - 1) // side, side


def jpeg_capacity_bound(w: int, h: int, subsampling: str = "4:2:0") -> int:
    """A slot size no stream of this shape can exceed: per block a DC code of
    at most 11 + 11 bits and 63 AC codes of at most 16 + 10, every byte
    stuffed, plus the padded last byte."""
    sampling = _check_sampling(subsampling)
    mx, my, _ = _mcu_grid(w, h, sampling)
    blocks = mx * my * (6 if sampling == N.IPP_JPEG_420 else 3)
    return 2 * ((blocks * (22 + 63 * 26) + 7) // 8)


class JpegEncoder:
    """Encodes batches of up to ``n`` RGB images of one size ``hw = (h, w)`` on
    ``device``.  Owns the scratch and the per-image slots of ``capacity``
    bytes (default: the raw size 3·w·h of the image padded to whole MCUs — a
    1x1 image's data are longer than its 3 bytes).  An image whose entropy
    data exceed ``capacity`` is refused by name with ValueError, never
    truncated; ``jpeg_capacity_bound`` gives a capacity that cannot be
    exceeded (noise at quality 100 does exceed the default)."""

    def __init__(self, device, n: int, hw: Tuple[int, int], quality: int = 75, subsampling: str = "4:2:0",
                 capacity: Optional[int] = None):
        self.quality = _check_quality(quality)
        self.subsampling = subsampling
        self.sampling = _check_sampling(subsampling)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= 65535:
            raise ValueError(f"n must be in 1..65535, got {n!r}")
        h, w = (int(v) for v in hw)
        if not (1 <= w <= N.IPP_JPEG_MAX_SIDE and 1 <= h <= N.IPP_JPEG_MAX_SIDE):
            raise ValueError(f"image size {w}x{h} outside 1..{N.IPP_JPEG_MAX_SIDE}")
        mx, my, side = _mcu_grid(w, h, self.sampling)
        if capacity is None:
            capacity = 3 * mx * side * my * side
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or \
                not 1 <= int(capacity) <= N.IPP_JPEG_MAX_CAPACITY:
            raise ValueError(f"capacity must be in 1..{N.IPP_JPEG_MAX_CAPACITY}, got {capacity!r}")
        self.n, self.h, self.w, self.capacity = int(n), h, w, int(capacity)
        self.pitch = (self.capacity + 15) // 16 * 16
        self.header = jpeg_header(w, h, self.quality, subsampling)
        self.qtab = np.ascontiguousarray(np.concatenate(jpeg_tables(self.quality)), np.uint16)
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"JpegEncoder runs on a ROCm device, got {self.device}")
        self.lib = N.load()
        nb = self.lib.ipp_jpeg_scratch_bytes(self.n, w, h, self.sampling, self.capacity)
        if nb < 0:
            raise N.NativeError(f"ipp_jpeg_scratch_bytes failed with code {nb}")
        self.scratch = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=self.device)
        self.slots = torch.empty(self.n * self.pitch, dtype=torch.uint8, device=self.device)
        self.hdr = torch.empty(self.n * N.IPP_JPEG_HDR, dtype=torch.int32, device=self.device)

    def _check_images(self, images):
        import torch
        if not isinstance(images, torch.Tensor):
            raise ValueError("images must be a torch.Tensor on the encoder's device")
        if images.dtype != torch.uint8:
            raise ValueError(f"images must be uint8, got {images.dtype}")
        if images.ndim != 4 or images.shape[3] != 3:
            what = "greyscale" if images.ndim == 3 or (images.ndim == 4 and images.shape[3] == 1) else \
                "RGBA" if images.ndim == 4 and images.shape[3] == 4 else "this shape"
            raise ValueError(f"images must be (n, h, w, 3) RGB, got {tuple(images.shape)}: {what} is out of scope")
        if tuple(images.shape[1:3]) != (self.h, self.w):
            raise ValueError(f"images are {images.shape[1]}x{images.shape[2]} (h x w), the encoder was made for "
                             f"{self.h}x{self.w}: every image of a call has the encoder's size")
        if not 0 <= images.shape[0] <= self.n:
            raise ValueError(f"{images.shape[0]} images, the encoder was made for at most {self.n}")
        if images.device != self.device and not (images.device.type == "cuda" and self.device.index is None):
            raise ValueError(f"images are on {images.device}, the encoder on {self.device}")
        if not images.is_contiguous():
            raise ValueError("images must be contiguous")

    def encode_device(self, images) -> np.ndarray:
        """The launches of ipp_jpeg_encode and the copy back of the headers:
        (n, 2) int32 {bytes, status}.  The data stay in the slots."""
        import torch
        self._check_images(images)
        n = int(images.shape[0])
        if n == 0:
            return np.zeros((0, N.IPP_JPEG_HDR), np.int32)
        st = torch.cuda.current_stream(self.device).cuda_stream
        N.check(self.lib.ipp_jpeg_encode(images.data_ptr(), n, self.w, self.h, self.sampling, N.np_ptr(self.qtab),
                                         self.scratch.data_ptr(), self.slots.data_ptr(), self.capacity,
                                         self.hdr.data_ptr(), st), "ipp_jpeg_encode")
        return self.hdr[:N.IPP_JPEG_HDR * n].cpu().numpy().reshape(n, N.IPP_JPEG_HDR)      # synchronises

    def encode(self, images, names: Optional[Sequence[str]] = None) -> List[bytes]:
        """Complete files, one per image.  One copy back of the headers, then
        one of the packed streams.  ValueError names (``names[i]``, else the
        index) every image whose data exceed the capacity; nothing of such an
        image is produced."""
        import torch
        hdr = self.encode_device(images)
        n = hdr.shape[0]
        bad = [i for i in range(n) if hdr[i, 1] != 0]
        if bad:
            label = lambda i: str(names[i]) if names is not None else f"image {i}"
            raise ValueError("; ".join(
                f"{label(i)}: the JPEG data need at least {int(hdr[i, 0])} bytes, over the capacity of {self.capacity}"
                for i in bad) + " (nothing was written for them; raise capacity, see jpeg_capacity_bound)")
        if n == 0:
            return []
        sizes = hdr[:, 0].astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)]).astype(np.int64)   # 16-B aligned: vector stores
        packed = torch.empty(max(int(offsets[-1]), 16), dtype=torch.uint8, device=self.device)
        d_off = torch.from_numpy(offsets[:-1].copy()).to(self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        N.check(self.lib.ipp_jpeg_pack(self.slots.data_ptr(), self.capacity, self.hdr.data_ptr(), n, d_off.data_ptr(),
                                       packed.data_ptr(), st), "ipp_jpeg_pack")
        host = packed.cpu().numpy()
        self.bytes_back = int(hdr.nbytes + host.nbytes)
        return [self.header + host[o:o + s].tobytes() + _EOI for o, s in zip(offsets[:-1], sizes)]

    def save(self, images, paths: Sequence, threads: int = 8) -> List:
        """encode(), then the files written on host threads; returns the paths."""
        paths = list(paths)
        if len(paths) != int(images.shape[0]):
            raise ValueError(f"{len(paths)} paths for {int(images.shape[0])} images")
        files = self.encode(images, names=[str(p) for p in paths])

        def write(job):
            with open(job[0], "wb") as f:
                f.write(job[1])
        with ThreadPoolExecutor(max_workers=max(1, int(threads))) as pool:
            list(pool.map(write, zip(paths, files)))
        return paths


def encode_grouped(images: Sequence, quality: int = 75, subsampling: str = "4:2:0") -> List[bytes]:
    """Files of device images (h, w, 3) of any sizes: one JpegEncoder call per
    distinct size (the plugins' chunks); a group that does not fit the default
    capacity is encoded again with a capacity nothing can exceed."""
    import torch
    out: List[Optional[bytes]] = [None] * len(images)
    groups = {}
    for i, im in enumerate(images):
        groups.setdefault(tuple(im.shape), []).append(i)
    for shape, idx in groups.items():
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError(f"images must be (h, w, 3) RGB, got {shape}")
        batch = torch.stack([images[i] for i in idx]).contiguous()
        try:
            files = JpegEncoder(batch.device, len(idx), shape[:2], quality, subsampling).encode(batch)
        except ValueError:   # over the default capacity (noise at a high quality): the bound cannot be exceeded
            files = JpegEncoder(batch.device, len(idx), shape[:2], quality, subsampling,
                                capacity=jpeg_capacity_bound(shape[1], shape[0], subsampling)).encode(batch)
        for i, data in zip(idx, files):
            out[i] = data
    return out


# ---- decoding ----------------------------------------------------------------
@dataclass
class JpegInfo:
    """What parse_jpeg finds in a baseline file."""
    w: int
    h: int
    subsampling: str                      # "4:2:0" or "4:4:4"
    qt: Tuple[int, int, int]              # per component (Y, Cb, Cr): quantisation table id (SOF0)
    dc: Tuple[int, int, int]              # DC Huffman table id (SOS)
    ac: Tuple[int, int, int]              # AC Huffman table id (SOS)
    qtables: Dict[int, np.ndarray]        # id -> 64 uint16, natural (row-major) order
    htables: Dict[Tuple[int, int], Tuple[bytes, bytes]]   # (class 0 DC / 1 AC, id) -> (BITS, HUFFVAL)
    restart_interval: int                 # MCUs, 0 for none
    span: Tuple[int, int]                 # [start, end) of the entropy-coded data in the file


_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)",
              0xC5: "differential sequential (SOF5)", 0xC6: "differential progressive (SOF6)",
              0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)",
              0xCA: "progressive arithmetic coding (SOF10)", 0xCB: "lossless arithmetic coding (SOF11)",
              0xCD: "differential arithmetic coding (SOF13)", 0xCE: "differential progressive arithmetic coding (SOF14)",
              0xCF: "differential lossless arithmetic coding (SOF15)"}


def parse_jpeg(data: bytes) -> JpegInfo:
    """Walks the markers of a JPEG file; plain Python, no imaging library.
    ValueError names what is out of scope for the device decoder: anything but
    a baseline (SOF0) 8-bit YCbCr file sampled "4:2:0" or "4:4:4" with one
    interleaved scan — or what is wrong with the header."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file (no SOI marker)" if n >= 2 else "truncated header: the file ends before SOI")
    qtables: Dict[int, np.ndarray] = {}
    htables: Dict[Tuple[int, int], Tuple[bytes, bytes]] = {}
    restart, sof, adobe = 0, None, None
    at = 2
    while True:
        if at + 4 > n:
            raise ValueError("truncated header: the file ends before the scan (SOS)")
        if data[at] != 0xFF:
            raise ValueError(f"malformed header: no marker at byte {at}")
        m = data[at + 1]
        if m == 0xFF:               # fill byte
            at += 1
            continue
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            at += 2
            continue
        if m == 0xD9:
            raise ValueError("truncated header: EOI before any scan")
        ln = int.from_bytes(data[at + 2:at + 4], "big")
        if ln < 2 or at + 2 + ln > n:
            raise ValueError(f"truncated header: segment 0xFF{m:02X} runs past the end of the file")
        body = data[at + 4:at + 2 + ln]
        at += 2 + ln
        if m == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq != 0:
                    raise ValueError("16-bit quantisation tables are out of scope (baseline tables are 8-bit)")
                if tq > 3 or k + 65 > len(body):
                    raise ValueError("malformed header: bad DQT segment")
                t = np.zeros(64, np.uint16)
                for z in range(64):
                    t[_ZIGZAG[z]] = body[k + 1 + z]
                qtables[tq] = t
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(body):
                tc, th = body[k] >> 4, body[k] & 15
                if tc > 1 or th > 3 or k + 17 > len(body):
                    raise ValueError("malformed header: bad DHT segment")
                bits = body[k + 1:k + 17]
                nv = sum(bits)
                if nv > 256 or k + 17 + nv > len(body):
                    raise ValueError("malformed header: bad DHT segment")
                code = 0
                for ln_ in range(16):
                    code = (code + bits[ln_]) << 1
                    if code > (2 << ln_ << 1):
                        raise ValueError("malformed header: a DHT table that is no prefix code")
                htables[(tc, th)] = (bytes(bits), bytes(body[k + 17:k + 17 + nv]))
                k += 17 + nv
        elif m == 0xC0:
            if sof is not None:
                raise ValueError("more than one frame header (SOF0) is out of scope")
            sof = body
        elif m in _SOF_NAMES:
            raise ValueError(f"{_SOF_NAMES[m]} files are out of scope: the device decodes baseline (SOF0) only")
        elif m == 0xCC:
            raise ValueError("arithmetic coding (DAC) is out of scope")
        elif m == 0xDD:
            if len(body) != 2:
                raise ValueError("malformed header: bad DRI segment")
            restart = int.from_bytes(body, "big")
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDA:
            sos = body
            break
        # APPn, COM and anything else with a length: skipped
    if sof is None:
        raise ValueError("malformed header: a scan (SOS) before any frame header (SOF0)")
    if len(sof) < 6:
        raise ValueError("truncated header: short SOF0 segment")
    if sof[0] != 8:
        raise ValueError(f"{sof[0]}-bit precision is out of scope: the device decodes 8-bit files (12-bit is refused)")
    h, w, nc = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    if nc == 1:
        raise ValueError("greyscale files are out of scope: the device decodes three-component YCbCr")
    if nc == 4:
        raise ValueError("CMYK / four-component files are out of scope: the device decodes three-component YCbCr")
    if nc != 3 or len(sof) < 6 + 3 * nc:
        raise ValueError(f"{nc}-component files are out of scope: the device decodes three-component YCbCr")
    if adobe is not None and adobe != 1:
        raise ValueError(f"an Adobe APP14 colour transform of {adobe} (RGB- or CMYK-coded data) is out of scope")
    comps = [(sof[6 + 3 * i], sof[7 + 3 * i] >> 4, sof[7 + 3 * i] & 15, sof[8 + 3 * i]) for i in range(3)]
    if adobe is None and [c[0] for c in comps] == [ord("R"), ord("G"), ord("B")]:
        raise ValueError("RGB-coded JPEG (component ids R, G, B) is out of scope")
    samp = tuple((c[1], c[2]) for c in comps)
    if samp == ((2, 2), (1, 1), (1, 1)):
        subsampling = "4:2:0"
    elif samp == ((1, 1), (1, 1), (1, 1)):
        subsampling = "4:4:4"
    else:
        name = {((2, 1), (1, 1), (1, 1)): '"4:2:2"', ((1, 2), (1, 1), (1, 1)): '"4:4:0"',
                ((4, 1), (1, 1), (1, 1)): '"4:1:1"'}.get(samp, "this")
        raise ValueError(f"{name} sampling {samp} is out of scope: the device decodes \"4:2:0\" and \"4:4:4\"")
    if not (1 <= w <= N.IPP_JPEG_MAX_SIDE and 1 <= h <= N.IPP_JPEG_MAX_SIDE):
        raise ValueError(f"image size {w}x{h} outside 1..{N.IPP_JPEG_MAX_SIDE} (IPP_JPEG_MAX_SIDE)")
    if len(sos) < 1 or sos[0] != 3 or len(sos) < 10:
        raise ValueError("more than one scan (a scan that does not hold all three components) is out of scope")
    sel = {sos[1 + 2 * i]: (sos[2 + 2 * i] >> 4, sos[2 + 2 * i] & 15) for i in range(3)}
    if [sos[1 + 2 * i] for i in range(3)] != [c[0] for c in comps]:
        raise ValueError("a scan whose components are not the frame's, in order, is out of scope")
    if (sos[7], sos[8], sos[9]) != (0, 63, 0):
        raise ValueError("progressive scan parameters (spectral selection / approximation) are out of scope")
    qt = tuple(c[3] for c in comps)
    dc = tuple(sel[c[0]][0] for c in comps)
    ac = tuple(sel[c[0]][1] for c in comps)
    for i in range(3):
        if qt[i] not in qtables or (0, dc[i]) not in htables or (1, ac[i]) not in htables:
            raise ValueError("malformed header: a component names a table the file does not define")
    # the span ends at the first marker that is neither stuffing nor RSTn (the EOI), or with the file
    end = at
    while True:
        k = data.find(b"\xff", end)
        if k < 0 or k + 1 >= n:
            end = n
            break
        nx = data[k + 1]
        if nx == 0 or 0xD0 <= nx <= 0xD7:
            end = k + 2
            continue
        if nx == 0xFF:
            end = k + 1
            continue
        end = k
        if nx != 0xD9:
            raise ValueError("more than one scan (a marker other than EOI after the first scan) is out of scope")
        break
    if end - at > N.IPP_JPEGD_MAX_SPAN:
        raise ValueError(f"entropy-coded data over {N.IPP_JPEGD_MAX_SPAN} bytes are out of scope")
    return JpegInfo(w, h, subsampling, qt, dc, ac, qtables, htables, restart, (at, end))


class JpegDecoder:
    """Decodes baseline JPEG files on ``device`` to the RGB pixels
    ``np.asarray(Image.open(f).convert("RGB"))`` gives (ipp.h states the rule
    under ipp_jpeg_decode).  One pinned staging buffer and one copy up of the
    files' entropy-coded spans, descriptors and tables; the kernels; one copy
    back of the status words.  ``last_stats`` keeps them, (n, 4) int32
    {status, rounds, subsequences, marker status}: the rounds the slowest
    restart interval of each file took to synchronise and the most
    subsequences one of its intervals has."""

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"JpegDecoder runs on a ROCm device, got {self.device}")
        self.lib = N.load()
        self.last_stats = np.zeros((0, N.IPP_JPEGD_STAT), np.int32)
        self._stage = None        # pinned staging buffer, kept and grown: pinning is a slow, synchronising call
        self._scratch = None      # device scratch, kept and grown

    def _grown(self, buf, nbytes: int, **kw):
        import torch
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(16, nbytes + nbytes // 4), dtype=torch.uint8, **kw)
            if "device" not in kw:
                buf = buf.pin_memory()
        return buf

    def decode_some(self, datas: Sequence[bytes], parsed: Optional[Sequence] = None
                    ) -> Tuple[List, List[Optional[str]]]:
        """(images, reasons): per file its (h, w, 3) uint8 tensor on the device
        and None, or None and why it was refused — by parse_jpeg (out of
        scope) or by the device (a malformed stream; nothing of it was
        written).  The accepted files cost one call whatever the others are;
        the caller sends the refused ones another way.  The tensors are views
        of one allocation per call.  ``parsed[i]``: what parse_jpeg returned
        or raised for file i, where the caller has called it already (on its
        own threads, say)."""
        import torch
        n_all = len(datas)
        images: List = [None] * n_all
        reasons: List[Optional[str]] = [None] * n_all
        infos, idx = [], []
        for i, data in enumerate(datas):
            try:
                f = parsed[i] if parsed is not None else parse_jpeg(data)
                if isinstance(f, Exception):
                    raise f
                infos.append(f)
                idx.append(i)
            except ValueError as e:
                reasons[i] = str(e)
        n = len(idx)
        self.last_stats = np.zeros((n_all, N.IPP_JPEGD_STAT), np.int32)
        if n == 0:
            return images, reasons
        descs = np.zeros(n, N.JPEGD_DESC)
        qtabs, htabs, qid, hid = [], [], {}, {}

        def intern(store, ids, key, make):
            if key not in ids:
                ids[key] = len(store)
                store.append(make())
            return ids[key]

        def htab(spec):
            t = np.zeros(16 + 256, np.uint8)
            t[:16] = np.frombuffer(spec[0], np.uint8)
            t[16:16 + len(spec[1])] = np.frombuffer(spec[1], np.uint8)
            return t
        up16 = lambda v: (v + 15) // 16 * 16
        span_at = out_at = 0
        for k, f in enumerate(infos):
            d = descs[k]
            d["span_off"], d["span_len"] = span_at, f.span[1] - f.span[0]
            span_at += up16(int(d["span_len"]))
            d["w"], d["h"], d["sampling"], d["restart"] = f.w, f.h, SAMPLINGS[f.subsampling], f.restart_interval
            d["out_off"], d["out_pitch"] = out_at, 3 * f.w
            out_at += up16(3 * f.w * f.h)
            for c in range(3):
                d["qt"][c] = intern(qtabs, qid, f.qtables[f.qt[c]].tobytes(), lambda: f.qtables[f.qt[c]])
                d["dc"][c] = intern(htabs, hid, (0,) + f.htables[(0, f.dc[c])], lambda: htab(f.htables[(0, f.dc[c])]))
                d["ac"][c] = intern(htabs, hid, (1,) + f.htables[(1, f.ac[c])], lambda: htab(f.htables[(1, f.ac[c])]))
        nb = self.lib.ipp_jpeg_decode_scratch_bytes(descs.ctypes.data, n)
        if nb < 0:
            raise N.NativeError(f"ipp_jpeg_decode_scratch_bytes failed with code {nb}")
        # the staging buffer: spans, descriptors, quantisation tables, Huffman tables
        data_bytes = max(span_at, 16)
        o_desc = up16(data_bytes)
        o_q = up16(o_desc + descs.nbytes)
        o_h = up16(o_q + 128 * len(qtabs))
        total = up16(o_h + (16 + 256) * len(htabs))
        self._stage = self._grown(self._stage, total)
        host = self._stage.numpy()
        for d, i, f in zip(descs, idx, infos):
            host[int(d["span_off"]):int(d["span_off"]) + int(d["span_len"])] = np.frombuffer(
                datas[i], np.uint8, int(d["span_len"]), f.span[0])
        host[o_desc:o_desc + descs.nbytes] = descs.view(np.uint8).reshape(-1)
        host[o_q:o_q + 128 * len(qtabs)] = np.stack(qtabs).astype(np.uint16).view(np.uint8).reshape(-1)
        host[o_h:o_h + 272 * len(htabs)] = np.stack(htabs).reshape(-1)
        dev = self._stage[:total].to(self.device, non_blocking=True)
        self._scratch = self._grown(self._scratch, int(nb), device=self.device)
        out = torch.empty(max(out_at, 16), dtype=torch.uint8, device=self.device)
        stat = torch.empty(n * N.IPP_JPEGD_STAT, dtype=torch.int32, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        p = dev.data_ptr()
        N.check(self.lib.ipp_jpeg_decode(p, data_bytes, host.ctypes.data + o_desc, p + o_desc, n, p + o_q, len(qtabs),
                                         p + o_h, len(htabs), self._scratch.data_ptr(), int(nb), out.data_ptr(), out_at,
                                         stat.data_ptr(), st), "ipp_jpeg_decode")
        stats = stat.cpu().numpy().reshape(n, N.IPP_JPEGD_STAT)      # synchronises: the staging buffer is free again
        for k, (i, d, f) in enumerate(zip(idx, descs, infos)):
            self.last_stats[i] = stats[k]
            if stats[k, 0] != 0:
                reasons[i] = f"malformed JPEG data ({N.IPP_JPEGD_STATUS.get(int(stats[k, 0]), 'unknown')})"
            else:
                images[i] = out[int(d["out_off"]):int(d["out_off"]) + 3 * f.w * f.h].view(f.h, f.w, 3)
        return images, reasons

    def decode(self, datas: Sequence[bytes], names: Optional[Sequence[str]] = None) -> List:
        """One (h, w, 3) uint8 tensor on the device per file; sizes, samplings
        and tables may differ.  ValueError names (``names[i]``, else the
        index) every file parse_jpeg refuses or whose stream the device found
        malformed: nothing is returned for them (decode_some returns the
        others)."""
        images, reasons = self.decode_some(datas)
        bad = [i for i, r in enumerate(reasons) if r is not None]
        if bad:
            label = lambda i: str(names[i]) if names is not None else f"image {i}"
            raise ValueError("; ".join(f"{label(i)}: {reasons[i]}" for i in bad) + " (nothing was decoded for them)")
        return images

    def decode_batch(self, datas: Sequence[bytes]):
        """(n, h, w, 3) where every file has the same size."""
        import torch
        imgs = self.decode(datas)
        if len({tuple(im.shape) for im in imgs}) > 1:
            raise ValueError("decode_batch needs files of one size; use decode for mixed sizes")
        return torch.stack(imgs) if imgs else torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=self.device)
