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
ICC / dpi / comments, images of different sizes in one call, decoding.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple

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
