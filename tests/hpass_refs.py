"""Direct harness of the pipe's H launch (csrc/ipp_pipe.hip: ipp_pipe_hpass,
ipp_pipe_hpass_bgcopy, ipp_pipe_hpass_bgcopy_trim) without a planner and
without a V launch, CPU side: no torch, no GPU.

  reference    a plain int64 restatement of what the H launch computes for one
               item, written from the documents: the virtual cut-out M
               (include/ipp.h, ipp_gather_desc: affine_fixed in int32
               wrap-around, crop window, bbox origin, flip; the header of
               csrc/ipp_pipe.hip: an input alpha is dropped, kept pixels are
               (R, G, B, 255), excluded ones (0, 0, 0, 0), the fill pixel raw 0
               takes the same test) and Pillow's horizontal 8bpc pass
               clip8((2^21 + Σ M·k) >> 22) over the plain taps of
               geometry.resample_taps.  It never reads the MFMA tiles and
               reuses nothing of the kernel;
  tap tiles    built tile by tile by the host builder ipp_plan_mfma_tile
               (h_axis: compact 1, shift 0, phase 0, as the planner gives H axes);
  descriptors  written by hand (Launch): the fields the H launch reads;
  T            packed and unpacked by vblend_refs.pack_t / unpack_t, the one
               statement of the T layout in the tests.

The path predicates below (chunks, body_form, band_valid, case_tags) RESTATE
hp2_chunk's prefix rule, hpass_block's choice of the fast or the CLAMP body
and the meaning of "valid column"; they must move with the kernel.  They read
the descriptors and the tile headers only, never a kernel's output.  Every
row of the tables names the paths it is there for (`why`, and CLAIMS as
tags); tests/test_hpass_refs_cpu.py asserts that the claims are true and
tests/test_gpu_hpass_direct.py runs the tables.
"""
from collections import namedtuple

import numpy as np

from image_processor_pipeline_amd import _native as N
from image_processor_pipeline_amd.geometry import REFERENCE_HSV_RANGES, mfma_tiles, resample_taps, rotation_plan
from oracle import ops
from tests import hsv_refs as HR
from tests.vblend_refs import pack_t, unpack_t

BAND = 16                     # HR: M rows per H block
RING = 512                    # the LDS window ring, M columns
TRIM_MAX_TILES = 64           # items of more tiles are not trimmed


def i32(v):
    """Wrap to int32 (the 32-bit wrap-around arithmetic of affine_fixed)."""
    return ((np.asarray(v, np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


# --------------------------------------------------------------------------- HSV sets

Hsv = namedtuple("Hsv", "ranges zones")      # ranges: (hmin, smin, vmin, hmax, smax, vmax) ints; zones: (t, b, l, r) or None

_ODD = [(2 * k + 1, 1, 1, 2 * k + 1, 254, 254) for k in range(16)]      # narrow ranges that hold single hues, never black
BLACK = (0, 0, 0, 180, 255, 150)                                        # the reference's first range: holds (0, 0, 0)
REF4 = [tuple(int(round(v)) for v in f) for f in REFERENCE_HSV_RANGES]


def hsv_set(n, black=True, zones=False):
    """n ranges: the dark range BLACK first (or, black kept, a bright one)
    and n - 1 narrow ones; with zones every range gets margins, the first
    one's leave most of the image inside."""
    first = BLACK if black else (0, 0, 200, 180, 255, 255)
    ranges = ([first] + REF4[1:] + _ODD)[:n] if n >= 4 else ([first] + _ODD)[:n]
    zs = None
    if zones:
        zs = [(1, 2, 3, 1)] + [((3 * k) % 5, k % 4, (5 * k) % 7, (2 * k) % 3) for k in range(1, n)]
    return Hsv(ranges, zs)


def hsv_params(hs):
    """ipp_hsv_params of an Hsv, written by hand (the bounds are integers in
    range already: cv::inRange's preparation leaves them as they are)."""
    p = np.zeros((), N.HSV_PARAMS)
    p["n_ranges"], p["bgr"] = len(hs.ranges), 0
    for k, f in enumerate(hs.ranges):
        assert ops.inrange_bounds(f[:3], f[3:]) == ([min(v, 255) for v in f[:3]], [min(v, 255) for v in f[3:]]), f
        p["r"][k]["lo"], p["r"][k]["hi"] = [min(v, 255) for v in f[:3]], [min(v, 255) for v in f[3:]]
        p["r"][k]["zone"] = hs.zones[k] if hs.zones else (0, 0, 0, 0)
    return p


def nr_form(n_ranges):
    """The NR of the template form the dispatcher takes for n_ranges."""
    return n_ranges if n_ranges <= 4 else 6 if n_ranges <= 6 else 16


def has_zones(hs):
    return bool(hs.zones) and any(any(z) for z in hs.zones)


def black_excluded(hs):
    """Is the fill pixel (raw 0: h = s = v = 0) excluded where no zone applies?"""
    return bool(HR.excluded(np.zeros((1, 3), np.int64), hs.ranges)[0])


def trims(hs, ntiles):
    """May an H block of this launch trim (hpass_block: no zones, black excluded, ≤ 64 tiles)?"""
    return not has_zones(hs) and black_excluded(hs) and ntiles <= TRIM_MAX_TILES


# --------------------------------------------------------------------------- M, the virtual cut-out

def sample_xy(g, x, y):
    """(xin, yin) of M pixels (x, y) (int64 arrays), as ipp.h states it: the
    output pixel (x, y) is canvas pixel (off_x + fx, off_y + fy), fx =
    out_w - 1 - x under flip bit 0, fy likewise under bit 1, and canvas pixel
    (X, Y) reads (a2 + Y·a1 + X·a0) >> 16, (a5 + Y·a4 + X·a3) >> 16 in int32."""
    fl = int(g["flip"])
    fx = int(g["out_w"]) - 1 - x if fl & 1 else x
    fy = int(g["out_h"]) - 1 - y if fl & 2 else y
    X, Y = int(g["off_x"]) + fx, int(g["off_y"]) + fy
    a = [int(g["a%d" % k]) for k in range(6)]
    return i32(a[2] + Y * a[1] + X * a[0]) >> 16, i32(a[5] + Y * a[4] + X * a[3]) >> 16


def valid_xy(g, x, y):
    xin, yin = sample_xy(g, x, y)
    return (xin >= 0) & (xin < int(g["in_w"])) & (yin >= 0) & (yin < int(g["in_h"])), xin, yin


def zone_box(zone, out_w, out_h):
    """[r0, r1) × [c0, c1) of a range's zone: rows[t : H - b], cols[l : W - r], NumPy slice semantics."""
    t, b, l, r = zone
    r0, r1, _ = slice(t, out_h - b).indices(out_h)
    c0, c1, _ = slice(l, out_w - r).indices(out_w)
    return r0, max(r0, r1), c0, max(c0, c1)


def cutout(g, hs, src, y0, nrows, ncols):
    """M rows [y0, y0 + nrows) × columns [0, ncols), uint8 [nrows, ncols, 4],
    from the flat source buffer `src`; and the mask of the pixels sampled
    inside the crop window."""
    x = np.arange(ncols, dtype=np.int64)[None, :]
    y = (y0 + np.arange(nrows, dtype=np.int64))[:, None]
    ok, xin, yin = valid_xy(g, x, y)
    cn = int(g["src_cn"])
    addr = int(g["src_off"]) + (int(g["in_y0"]) + yin) * int(g["src_pitch"]) + (int(g["in_x0"]) + xin) * cn
    addr = np.where(ok, addr, 0)
    rgb = np.stack([src[addr + c] for c in range(3)], -1)          # a 4th channel is dropped
    rgb[~ok] = 0                                                   # transparent black; HSV sees (0, 0, 0)
    hsv = HR.hsv_of_rgb(rgb).reshape(-1, 3)
    ex = np.zeros(ok.shape, bool)
    for k, f in enumerate(hs.ranges):
        hit = HR.excluded(hsv, [f]).reshape(ok.shape)
        if hs.zones:
            r0, r1, c0, c1 = zone_box(hs.zones[k], int(g["out_w"]), int(g["out_h"]))
            hit = hit & (y >= r0) & (y < r1) & (x >= c0) & (x < c1)
        ex |= hit
    M = np.concatenate([rgb, np.full(ok.shape + (1,), 255, np.uint8)], -1)
    M[ex] = 0
    return M, ok


def cutout_scalar(g, hs, src, x, y):
    """One M pixel, written as straight-line scalar Python: the second
    restatement the rows out of the oracle's reach are held to."""
    w, h = int(g["out_w"]), int(g["out_h"])
    X = int(g["off_x"]) + (w - 1 - x if int(g["flip"]) & 1 else x)
    Y = int(g["off_y"]) + (h - 1 - y if int(g["flip"]) & 2 else y)

    def wrap(v):
        v &= 0xFFFFFFFF
        return v - (1 << 32) if v & 0x80000000 else v
    xin = wrap(int(g["a2"]) + Y * int(g["a1"]) + X * int(g["a0"])) >> 16
    yin = wrap(int(g["a5"]) + Y * int(g["a4"]) + X * int(g["a3"])) >> 16
    px = (0, 0, 0)
    if 0 <= xin < int(g["in_w"]) and 0 <= yin < int(g["in_h"]):
        o = int(g["src_off"]) + (int(g["in_y0"]) + yin) * int(g["src_pitch"]) + (int(g["in_x0"]) + xin) * int(g["src_cn"])
        px = tuple(int(v) for v in src[o:o + 3])
    hh, ss, vv = (int(v) for v in HR.hsv_of_rgb(np.array(px, np.uint8)))
    for k, f in enumerate(hs.ranges):
        inside = f[0] <= hh <= f[3] and f[1] <= ss <= f[4] and f[2] <= vv <= f[5]
        if hs.zones:
            r0, r1, c0, c1 = zone_box(hs.zones[k], w, h)
            inside = inside and r0 <= y < r1 and c0 <= x < c1
        if inside:
            return (0, 0, 0, 0)
    return px + (255,)


# --------------------------------------------------------------------------- the H pass

def plain_taps(in_len, out_len):
    """(bounds [out, 2] (xmin, count), taps [out, ksize]) int64 of Pillow's LANCZOS axis."""
    ks, buf = resample_taps("lanczos", in_len, out_len)
    return buf[:2 * out_len].reshape(out_len, 2).astype(np.int64), buf[2 * out_len:].reshape(out_len, ks).astype(np.int64)


def h_sums(M, in_len, out_len):
    """(2^21 + Σ_j M[r][xmin + j][c]·k_j) >> 22 before clip8, int64 [rows, out_len, 4]."""
    assert M.shape[1] == in_len
    bounds, kk = plain_taps(in_len, out_len)
    src = M.astype(np.int64)
    out = np.empty((M.shape[0], out_len, 4), np.int64)
    for xo in range(out_len):
        xmin, cnt = bounds[xo]
        out[:, xo] = ((1 << 21) + np.einsum("rkc,k->rc", src[:, xmin:xmin + cnt], kk[xo, :cnt])) >> 22
    return out


def hpass_ref(M, in_len, out_len):
    """T rows as pixels, uint8 [rows, out_len, 4]: clip8 of h_sums; an axis
    that keeps its length is the identity (Pillow skips the pass)."""
    if in_len == out_len:
        return M.copy()
    return np.clip(h_sums(M, in_len, out_len), 0, 255).astype(np.uint8)


def h_axis(in_len, out_len):
    """The H axis built by the host tile builder, as the planner configures H
    axes (compact 1, shift 0, phase 0, identity where the length is kept):
    (coefficient words int32, hdr [T, 4], nkb)."""
    lib = N.load()
    ident = int(in_len == out_len)
    ks = 1 if ident else lib.ipp_plan_lanczos_ksize(0.0, float(in_len), out_len)
    nkb = lib.ipp_plan_mfma_nk_bound(in_len, out_len, ks)
    T = (out_len + 15) >> 4
    a = np.zeros(1, N.TAP_AXIS)
    a["in_size"], a["out_size"], a["identity"], a["nkb"], a["compact"], a["n_tiles"] = in_len, out_len, ident, nkb, 1, T
    hdr, bias, blocks = mfma_tiles(a)
    for t, h4 in enumerate(hdr):
        assert h4[2] == t * nkb * 192
    words = np.concatenate([hdr.reshape(-1), bias.reshape(-1), blocks.reshape(-1).view(np.int32)])
    return words, hdr.astype(np.int64), nkb


# --------------------------------------------------------------------------- path predicates

def chunks(hdr, s_lo, s_hi):
    """hp2_chunk's walk over the tiles [s_lo, s_hi): per chunk the longest
    prefix of ≤ 4 tiles with max window end - W0 ≤ RING.  A list of dicts:
    s0, s1, W0, W1, c0 (first M column not yet in the ring), overlap (c0 =
    filled > W0), ring_stop (the extent e - W0 that stopped the prefix, or 0)."""
    out, filled, s0 = [], int(hdr[s_lo, 0]), s_lo
    while s0 < s_hi:
        W0 = int(hdr[s0, 0])
        W1, s1, stop = W0 + 64 * int(hdr[s0, 1]), s0 + 1, 0
        for k in range(1, 4):
            if s0 + k >= s_hi:
                break
            e = max(W1, int(hdr[s0 + k, 0]) + 64 * int(hdr[s0 + k, 1]))
            if e - W0 > RING:
                stop = e - W0
                break
            W1, s1 = e, s0 + k + 1
        out.append(dict(s0=s0, s1=s1, W0=W0, W1=W1, c0=max(filled, W0), overlap=filled > W0, ring_stop=stop))
        filled, s0 = max(filled, W1), s1
    return out


def body_form(g):
    """'fast' or 'clamp': hpass_block's need <= nrec && yr_range_ok; and
    whether a pixel of the window needs the clamp (its dword crosses the
    records' end), and yr_range_ok itself."""
    cn, pitch = int(g["src_cn"]), int(g["src_pitch"])
    nrec = (int(g["src_h"]) - int(g["in_y0"])) * pitch - int(g["in_x0"]) * cn
    need = (int(g["in_h"]) - 1) * pitch + int(g["in_w"]) * cn + (1 if cn == 3 else 0)
    yr = int(g["in_h"]) * pitch >= need and 32768 * pitch + need <= 1 << 32
    return dict(fast=need <= nrec and yr, clamps=need > nrec, yr=yr, need=need, nrec=nrec)


def band_valid(g, line0, band, ncols):
    """(first, last) M column in [0, ncols) of the band's 16 rows (rows past the
    item's lines included, as the block takes them) that samples inside the
    crop window, exactly; None when there is none."""
    ok, _, _ = valid_xy(g, np.arange(ncols, dtype=np.int64)[None, :],
                        (line0 + BAND * band + np.arange(BAND, dtype=np.int64))[:, None])
    cols = np.flatnonzero(ok.any(axis=0))
    return (int(cols[0]), int(cols[-1])) if len(cols) else None


# --------------------------------------------------------------------------- the case tables

Case = namedtuple("Case", "name src pad crop angle A canvas bbox flip out_len line0 lines prepared t_pad content why")


def row(name, why, src, out_len, angle=0.0, crop=None, A=None, canvas=None, bbox=None, flip=0, line0=0, lines=None,
        prepared=0, pad=0, t_pad=0, content="noise"):
    return Case(name, src, pad, crop, angle, A, canvas, bbox, flip, out_len, line0, lines, prepared, t_pad, content, why)


Table = namedtuple("Table", "name cn hsv rows")

FIX = 65536


def geometry(c):
    """(crop x0, y0, w, h; A; off_x, off_y, out_w, out_h) of a case."""
    sw, sh = c.src
    x0, y0, w, h = c.crop or (0, 0, sw, sh)
    assert 0 <= x0 and x0 + w <= sw and 0 <= y0 and y0 + h <= sh and w > 0 and h > 0
    if c.A is not None:
        A, (nw, nh) = c.A, c.canvas
    else:
        plan = rotation_plan(w, h, c.angle)
        A, nw, nh = plan.A, plan.nw, plan.nh
    return (x0, y0, w, h), tuple(int(v) for v in A), (c.bbox or (0, 0, nw, nh)), (nw, nh)


_pal = []


def _palette():
    if not _pal:
        _pal.append(HR.palette())
    return _pal[0]


def content(c, cn, w, h):
    """The pixels of the case's crop window, uint8 [h, w, cn] (seeded by the
    case alone, not by the garbage around it)."""
    rng = np.random.default_rng([len(c.name), w, h, c.out_len])
    px = rng.integers(0, 256, (h, w, cn), np.uint8)
    if c.content == "bright":          # blues (hue 90..120, v ≥ 200) that every range of the tables keeps; three distinct bytes each
        px[..., 0] = px[..., 0] % 90
        px[..., 1] = 100 + px[..., 1] % 50
        px[..., 2] = 200 + px[..., 2] % 56
    elif c.content == "stripes":       # hard 0 / 255 column stripes, two output pixels (2 × the downscale's period) each
        period = 2 * max(1, round(w / c.out_len))
        on = (np.arange(w) // period) % 2 == 1
        px[..., :3] = np.where(on, 255, 0)[None, :, None]
        px[h // 2:, :, 1] = np.where(on, 0, 255)[None, :]        # lower half: green in counter-phase (still bright or black)
    elif c.content == "palette":       # a sweep of the complete HSV palette
        pal = _palette()
        idx = (np.arange(w * h) * 613 + 7 * len(c.name)) % len(pal)
        px[..., :3] = pal[idx].reshape(h, w, 3)
    elif c.content == "clamp":         # bright, and the last two pixels hand-made: four distinct bytes around the clamp
        px[..., 0], px[..., 1], px[..., 2] = 40, 120, 220
        px[h - 1, w - 2, :3] = (77, 130, 230)
        px[h - 1, w - 1, :3] = (19, 163, 251)
    else:
        assert c.content == "noise", c.content
    return px


class Launch:
    """The buffers of one H launch over a table's rows: the source (seeded
    garbage everywhere, the crop windows' pixels on top), the tap words, the
    descriptors, the T geometry and the three byte classes of T."""

    def __init__(self, table, garbage=7, names=None):
        self.table = table
        self.cases = [c for c in table.rows if names is None or c.name in names]
        self.hsv, self.cn = table.hsv, table.cn
        n = len(self.cases)
        self.descs = np.zeros(n, N.PIPE_DESC)
        lib = N.load()
        # --- the source
        offs, total = [], 64
        for c in self.cases:
            sw, sh = c.src
            offs.append(total)
            total += sh * (sw * self.cn + c.pad) + 3 + 5 * (len(offs) % 4)      # gaps of odd sizes: no alignment
        self.src = np.random.default_rng([garbage, n]).integers(0, 256, total + 64, np.uint8)
        self.window = np.zeros(len(self.src), bool)            # the bytes of the crop windows: everything else is garbage
        coefs, self.hdrs, self.nkbs, axes, coef_off, t_off = [], [], [], {}, 0, 48
        self.t_items = []
        for i, c in enumerate(self.cases):
            (x0, y0, w, h), A, (off_x, off_y, out_w, out_h), _ = geometry(c)
            sw, sh = c.src
            pitch = sw * self.cn + c.pad
            img = np.lib.stride_tricks.as_strided(self.src[offs[i]:], (sh, pitch), (pitch, 1))
            img[y0:y0 + h, x0 * self.cn:(x0 + w) * self.cn] = content(c, self.cn, w, h).reshape(h, -1)
            np.lib.stride_tricks.as_strided(self.window[offs[i]:], (sh, pitch), (pitch, 1))[y0:y0 + h, x0 * self.cn:(x0 + w) * self.cn] = True
            d = self.descs[i]
            g = d["g"]
            g["src_off"], g["src_pitch"], g["src_cn"], g["src_w"], g["src_h"] = offs[i], pitch, self.cn, sw, sh
            g["in_x0"], g["in_y0"], g["in_w"], g["in_h"] = x0, y0, w, h
            for k in range(6):
                g["a%d" % k] = A[k]
            g["out_w"], g["out_h"], g["off_x"], g["off_y"], g["flip"] = out_w, out_h, off_x, off_y, c.flip
            # --- taps
            in_len = out_w
            key = (in_len, c.out_len)
            if key not in axes:
                words, hdr, nkb = h_axis(*key)
                axes[key] = (coef_off, hdr, nkb)
                coefs.append(words)
                coef_off += len(words)
                assert len(words) % 4 == 0
            c_off, hdr, nkb = axes[key]
            self.hdrs.append(hdr)
            self.nkbs.append(nkb)
            # --- T
            lines = out_h - c.line0 if c.lines is None else c.lines
            assert lines >= 1 and c.line0 >= 0
            t_pitch = 16 * (c.out_len + c.t_pad)
            groups = 4 * ((lines + 15) // 16)
            alloc = groups + 1 + i % 3                  # row groups past the written ones: poison class
            hd = d["h"]
            hd["dst_off"], hd["dst_pitch"], hd["in_len"], hd["out_len"] = t_off, t_pitch, in_len, c.out_len
            hd["lines"], hd["line0"], hd["coef_off"] = lines, c.line0, c_off
            hd["ksize"] = 1 if in_len == c.out_len else lib.ipp_plan_lanczos_ksize(0.0, float(in_len), c.out_len)
            self.t_items.append((t_off, t_pitch, groups, alloc, lines))
            t_off += alloc * t_pitch + 16 * (1 + i % 3)       # a gap between the items' T
        self.coefs = np.concatenate(coefs)
        self.t_bytes = t_off + 32
        for i, c in enumerate(self.cases):
            if c.prepared:
                N.check(lib.ipp_gather_prepare(N.np_ptr(self.descs[i:i + 1]), 1), "ipp_gather_prepare")
                assert int(self.descs[i]["g"]["prepared"]) == 1
        self.max_rows = max(t[4] for t in self.t_items)
        self.max_out_w = max(c.out_len for c in self.cases)
        self.params = hsv_params(self.hsv)

    # --- T classes
    def classes(self):
        """(specified, unspecified) bool masks over the T buffer; every other byte is the poison class."""
        spec, unspec = np.zeros(self.t_bytes, bool), np.zeros(self.t_bytes, bool)
        for (off, pitch, groups, _, lines), c in zip(self.t_items, self.cases):
            rows = 4 * np.arange(groups)[:, None] + np.arange(4)[None, :]                   # [g][r]
            for mask, sel in ((spec, rows < lines), (unspec, rows >= lines)):
                v = mask[off: off + groups * pitch].reshape(groups, pitch)[:, :16 * c.out_len].reshape(groups, c.out_len, 4, 4)
                v[...] = sel[:, None, None, :]
        return spec, unspec

    def item_view(self, buf, i):
        """[groups, out_len, 16] view of item i's written groups in a T buffer."""
        off, pitch, groups, _, _ = self.t_items[i]
        n = self.cases[i].out_len
        return buf[off: off + groups * pitch].reshape(groups, pitch)[:, :16 * n].reshape(groups, n, 16)

    def item_pixels(self, buf, i):
        off, pitch, groups, _, lines = self.t_items[i]
        return unpack_t(buf[off:], lines, self.cases[i].out_len, pitch)

    # --- reference
    def M(self, i, ncols=None):
        d = self.descs[i]
        return cutout(d["g"], self.hsv, self.src, int(d["h"]["line0"]), int(d["h"]["lines"]),
                      int(d["h"]["in_len"]) if ncols is None else ncols)[0]

    def reference(self, i):
        """T rows of item i as pixels [lines, out_len, 4]."""
        h = self.descs[i]["h"]
        return hpass_ref(self.M(i), int(h["in_len"]), int(h["out_len"]))

    def expected(self, poison, refs, only=None):
        """The T buffer after a launch on T pre-filled with `poison`: the
        references in the specified bytes, the poison everywhere else (the
        unspecified class is for the caller to mask out)."""
        exp = np.full(self.t_bytes, poison, np.uint8)
        for i, (off, pitch, groups, alloc, lines) in enumerate(self.t_items):
            if only is not None and i not in only:
                continue
            exp[off: off + groups * pitch] = pack_t(refs[i], pitch, 4 * groups, poison)
        return exp

    # --- a background for the entry points with copy blocks
    def with_background(self):
        """Hand-written paste descriptors on small composites (two shapes: a
        dense 16-B aligned one that all its items share, and an odd one);
        returns (bg bytes, dst bytes)."""
        shapes = ((48, 40), (37, 23))
        bg_off, dst_off = [0, 48 * 40 * 3 + 16], 0
        for i, c in enumerate(self.cases):
            bw, bh = shapes[i % 2]
            p = self.descs[i]["p"]
            p["bg_off"], p["dst_off"], p["bg_w"], p["bg_h"] = bg_off[i % 2], dst_off, bw, bh
            p["bg_pitch"] = p["dst_pitch"] = 3 * bw
            p["ov_w"], p["ov_h"] = min(c.out_len, 20), min(int(self.descs[i]["h"]["lines"]), 9)
            p["ov_pitch"], p["x"], p["y"] = 4 * int(p["ov_w"]), 1 + i % 5, 2 + i % 7
            assert int(p["x"]) + int(p["ov_w"]) <= bw and int(p["y"]) + int(p["ov_h"]) <= bh
            dst_off += (3 * bw * bh + 15) // 16 * 16
        return bg_off[1] + 37 * 23 * 3 + 16, dst_off + 16

    def blocks_per_item(self):
        return (self.max_rows + BAND - 1) // BAND

    # --- claims
    def tags(self, i):
        return case_tags(self, i)


def sums_range(L, i):
    """(min[4], max[4]) of item i's H sums >> 22 before clip8."""
    h = L.descs[i]["h"]
    s = h_sums(L.M(i), int(h["in_len"]), int(h["out_len"]))
    return s.min(axis=(0, 1)).tolist(), s.max(axis=(0, 1)).tolist()


def mixed_windows(L, i):
    """How many (row, output) tap windows of item i hold both kept and excluded in-source pixels."""
    h = L.descs[i]["h"]
    in_len, out_len = int(h["in_len"]), int(h["out_len"])
    a = L.M(i)[..., 3] == 255
    bounds, _ = plain_taps(in_len, out_len)
    return sum(int((a[:, x0:x0 + n].any(axis=1) & ~a[:, x0:x0 + n].all(axis=1)).sum()) for x0, n in bounds)


def case_tags(L, i):
    """Every property of row i the tables speak of, from its descriptor and
    its tile headers (and, for the value rows, from the reference)."""
    c, d, hdr = L.cases[i], L.descs[i], L.hdrs[i]
    g, h = d["g"], d["h"]
    in_len, out_len, lines, line0 = (int(h[k]) for k in ("in_len", "out_len", "lines", "line0"))
    nt = (out_len + 15) >> 4
    assert len(hdr) == nt
    tags = {"out%d" % out_len, "lines%d" % lines, "cn%d" % L.cn, "flip%d" % int(g["flip"]), "prepared%d" % c.prepared}
    if line0 > 0:
        tags.add("line0")
    nbands = (lines + 15) // 16
    if nbands + 2 <= L.blocks_per_item():
        tags.add("early_return")
    for t in range(nt):
        tags.add("nk%d" % hdr[t, 1])
        tags.add("compact" if hdr[t, 3] else "dense")
    if int(hdr[:, 1].max()) == 8 and nt > 0 and 64 * 8 == RING:
        tags.add("ring512")
    if in_len < out_len and in_len <= 3:
        tags.add("up_in%d" % in_len)
    if nt > TRIM_MAX_TILES:
        tags.add("gt64tiles")
    if c.t_pad:
        tags.add("t_pad")
    # --- the gather
    a = [int(g["a%d" % k]) for k in range(6)]
    exact = {(FIX, 0, 0, FIX): "rot0", (0, -FIX, FIX, 0): "rot90", (-FIX, 0, 0, -FIX): "rot180", (0, FIX, -FIX, 0): "rot270"}
    kind = exact.get((a[0], a[1], a[3], a[4]))
    tags.add(kind if kind else "oblique" if a[0] and a[1] and a[3] and a[4] else "hand_map")
    if a[0] == 0:
        tags.add("b0_zero")                    # b0 = ± a0: the bb == 0.0f branch of clip on the x axis
    sw, sh = c.src
    if int(g["in_x0"]) > 0 and int(g["in_y0"]) > 0 and int(g["in_x0"]) + int(g["in_w"]) < sw and int(g["in_y0"]) + int(g["in_h"]) < sh:
        tags.add("crop_inside")
    if c.pad:
        tags.add("pitch_pad")
    wend = int((hdr[:, 0] + 64 * hdr[:, 1]).max())
    valid = [band_valid(g, line0, b, max(wend, in_len)) for b in range(nbands)]
    if all(v is None for v in valid):
        tags.add("all_dead")
    for v in valid:
        if v is not None:
            for which, col in (("first", v[0]), ("last", v[1])):
                where = {0: "on", 15: "before", 1: "after"}.get(col % 16)
                if where and 0 < col < in_len - 1:
                    tags.add("%s_%s" % (which, where))
    # every band's valid columns meet the first and the last tile's window: a conservative interval sweeps all tiles
    full = all(v is not None and v[0] < hdr[0, 0] + 64 * hdr[0, 1] and v[1] >= hdr[-1, 0] for v in valid)
    if full or not trims(L.hsv, nt):
        tags.add("full_sweep")
        cks = chunks(hdr, 0, nt)
        for k in cks:
            size = k["s1"] - k["s0"]
            tags.add("chunk4" if size == 4 else "chunk%dr" % size if k["ring_stop"] else "chunk%dt" % size)
            if k["overlap"]:
                tags.add("overlap")
            if 0 < k["ring_stop"] <= RING + 64:
                tags.add("ring_tight")
        if wend > 2 * RING:
            tags.add("wrap2")
    # --- the source form
    f = body_form(g)
    if f["fast"]:
        tags.add("fast")
    else:
        tags.add("clamp_body")
        if f["need"] <= f["nrec"] and not f["yr"]:
            tags.add("yr_false")
        if f["clamps"]:
            # the window's last pixel is the source's last, and M samples it
            ok, xin, yin = valid_xy(g, np.arange(in_len, dtype=np.int64)[None, :], (line0 + np.arange(lines, dtype=np.int64))[:, None])
            if (ok & (xin == int(g["in_w"]) - 1) & (yin == int(g["in_h"]) - 1)).any():
                tags.add("clamp_last")
    # --- HSV
    tags.add("nr%d" % nr_form(len(L.hsv.ranges)))
    tags.add("n_ranges%d" % len(L.hsv.ranges))
    tags.add("zones" if has_zones(L.hsv) else "no_zones")
    tags.add("black_out" if black_excluded(L.hsv) else "black_kept")
    if has_zones(L.hsv) and nr_form(len(L.hsv.ranges)) > 8:
        tags.add("zones_lds")
    if trims(L.hsv, nt) and not full:
        tags.add("may_trim")
    # --- values
    if c.content == "stripes":
        lo, hi = sums_range(L, i)
        if min(lo[:3]) < 0 and max(hi[:3]) > 255:
            tags.add("saturates")
    if c.content == "palette" and mixed_windows(L, i) > lines * out_len // 2:
        tags.add("palette_mix")
    if not black_excluded(L.hsv) and not has_zones(L.hsv):
        M = L.M(i)
        okm = valid_xy(g, np.arange(in_len, dtype=np.int64)[None, :], (line0 + np.arange(lines, dtype=np.int64))[:, None])[0]
        if (~okm).any() and (M[~okm] == (0, 0, 0, 255)).all():
            tags.add("fill_opaque")
    return tags


# --------------------------------------------------------------------------- the tables

HALF = FIX // 2
# name, why, source (w, h), out_len; the rest by keyword.  in_len (= M's width) and the lines come from the
# geometry: the rotated canvas, or the bbox where one is given.
GEOMETRY_ROWS = [
    # --- tile geometry
    row("o1_l1", "out_len 1, lines 1: one T group, three of its four rows unspecified", (9, 1), 1),
    row("o15_l15", "out_len 15, lines 15: one ragged tile, one ragged band", (40, 15), 15, t_pad=2),
    row("o16_l16", "out_len 16, lines 16: exactly one tile, one band, nothing unspecified", (20, 16), 16),
    row("o17_l17", "out_len 17, lines 17: a second tile of one column, a second band of one row", (40, 17), 17, t_pad=1),
    row("o33_l33", "out_len 33, lines 33: three tiles, three bands (the launch's max_rows); nK 1 and 2, compact", (100, 33), 33),
    row("o1025", "out_len 64·16 + 1: 65 tiles, no fill trim; chunks of 4 tiles all along", (300, 5), 1025),
    row("line0", "line0 = 9 > 0: T row r is M row 9 + r; 17 lines of 40", (30, 40), 20, angle=180.0, line0=9, lines=17),
    # --- K steps
    row("nk3", "nK 3, compact and dense tiles in one item", (420, 6), 48),
    row("nk5", "nK 5, dense (more than 64 nonzero groups)", (260, 5), 16),
    row("nk8", "nK 8: a window of exactly 512 columns, the ring limit; every chunk one tile, stopped by the ring; overlap",
        (900, 4), 40),
    row("up_in1", "upscale of in_len 1", (1, 3), 5),
    row("up_in2", "upscale of in_len 2", (2, 4), 7),
    row("up_in3", "upscale of in_len 3, two tiles", (3, 5), 17),
    # --- chunks
    row("ck3", "chunks of 3 tiles: the 4th would span 576 = RING + 64 columns; c0 = filled > W0 in the next chunk", (560, 5), 64),
    row("ck2", "chunks of 2 tiles: the 3rd would span 560 columns", (500, 5), 33),
    row("wrap", "M 1200 columns wide (a hand-made map: every source column twice): the ring wraps twice; chunks of 3 and 4",
        (600, 6), 150, A=(HALF, 0, HALF // 2, 0, FIX, HALF), canvas=(1200, 6), content="bright"),
]

GATHER_ROWS = [
    # --- exact maps, flips
    row("rot90", "exact 90°: a0 = 0, the bb == 0 branch of the valid-column clip; mirror x", (37, 29), 24, angle=90.0, flip=1),
    row("rot180", "exact 180°; mirror y", (37, 29), 30, angle=180.0, flip=2),
    row("rot270", "exact 270°: a0 = 0 again, a3 < 0", (37, 29), 24, angle=270.0),
    row("obl_a", "oblique 17°: fill corners trimmed by the valid-column interval", (37, 29), 40, angle=17.0),
    row("obl_b", "oblique 296.5°, both mirrors", (37, 29), 36, angle=296.5, flip=3),
    row("crop_in", "a crop window strictly inside a larger source with a padded pitch, 30°: the fast body; garbage all around",
        (50, 40), 33, angle=30.0, crop=(7, 5, 30, 22), pad=5),
    row("prep0", "prepared = 0: the block computes the sampler", (33, 21), 28, angle=41.0, flip=1, crop=(2, 1, 29, 19), pad=3),
    row("prep1", "prepared = 1 on the same item: the sampler of ipp_gather_prepare; equal T", (33, 21), 28, angle=41.0, flip=1,
        crop=(2, 1, 29, 19), pad=3, prepared=1),
    row("dead", "a band wholly outside the source (the bbox lies beside the canvas): no valid column, every step dead",
        (20, 10), 24, bbox=(500, 0, 20, 10)),
    # --- the valid interval's ± 2 slack: the first / last valid column of the band on, one before, one after a step edge
    row("edge_on", "33°: the band's first valid column 16, its last 48: both on a 16-column step edge", (46, 25), 80,
        angle=33.0, bbox=(0, 0, 54, 16), content="bright"),
    row("edge_before", "33°: first valid column 15, last 47: both one before a step edge", (46, 25), 80,
        angle=33.0, bbox=(1, 0, 53, 16), content="bright"),
    row("edge_after", "20°: first valid column 1, last 49: both one after a step edge", (57, 25), 80,
        angle=20.0, bbox=(10, 0, 53, 16), content="bright"),
    # --- source forms
    row("clamp", "CN 3, dense pitch, the crop reaches the source's last pixel: the CLAMP body loads it one byte early",
        (6, 4), 16, content="clamp"),
    row("yr_false", "a full-width crop of a dense 3-channel source: in_h·pitch = need - 1, the row test stays (CLAMP body)",
        (12, 10), 20, crop=(0, 2, 12, 5)),
    # --- values
    row("stripes", "hard 0 / 255 column stripes two output pixels wide (at one the axis is at its Nyquist rate and cannot "
        "overshoot): the sums leave [0, 255] both ways", (64, 6), 16,
        content="stripes"),
    row("palette", "a sweep of the HSV palette: kept and excluded pixels alternate inside single tap windows", (60, 12), 25,
        angle=7.0, content="palette"),
]

FORM_ROWS = [
    row("f_pal", "palette colours through this template form, oblique", (33, 21), 24, angle=11.0, content="palette"),
    row("f_dn", "noise through this template form: nK 2, compact", (100, 18), 33),
]

KEPT_ROWS = [
    row("k_obl", "black kept: the fill is (0, 0, 0, 255), T's alpha outside the source is 255, nothing trims", (37, 29), 40,
        angle=17.0, content="bright"),
    row("k_dead", "black kept, band outside the source: every T pixel (0, 0, 0, 255)", (20, 10), 24, bbox=(500, 0, 20, 10)),
    row("k_dn", "black kept, nK 3", (420, 6), 48),
]

CN4_ROWS = [
    row("c4_obl", "CN 4: the source's alpha is dropped; oblique", (37, 29), 40, angle=17.0),
    row("c4_full", "CN 4, dense pitch, full crop: no clamp is ever needed (the fast body)", (6, 4), 16, content="clamp"),
    row("c4_crop", "CN 4, crop inside a padded source, 90°", (50, 40), 33, angle=90.0, crop=(7, 5, 30, 22), pad=6),
    row("c4_nk3", "CN 4, nK 3", (420, 6), 48),
]

REF_HSV = Hsv(REF4, None)
KEPT_HSV = Hsv([(0, 0, 1, 180, 255, 60)], None)
GEOMETRY = Table("geometry", 3, REF_HSV, GEOMETRY_ROWS)
GATHER = Table("gather", 3, REF_HSV, GATHER_ROWS)
KEPT = Table("black_kept", 3, KEPT_HSV, KEPT_ROWS)
CN4 = Table("cn4", 4, hsv_set(1), CN4_ROWS)
Z5 = Table("zones5", 3, hsv_set(5, zones=True), GATHER_ROWS[3:8])
Z7 = Table("zones7", 3, hsv_set(7, zones=True), GATHER_ROWS[3:8])
N7 = Table("ranges7", 3, hsv_set(7), GATHER_ROWS[3:8])
FORMS = [Table("form_n%d_z%d_c%d" % (n, z, cn), cn, hsv_set(n, zones=bool(z)), FORM_ROWS)
         for n in (1, 2, 3, 4, 5, 7) for z in (0, 1) for cn in (3, 4)]
TABLES = [GEOMETRY, GATHER, KEPT, CN4, Z5, Z7, N7]
ALONE = ("o33_l33", "nk8", "wrap")             # rows of GEOMETRY also launched alone, with descs advanced

# What each row is there for, as tags case_tags computes from the row's descriptor and tile headers.
CLAIMS = {
    "o1_l1": "out1 lines1 early_return",
    "o15_l15": "out15 lines15 t_pad",
    "o16_l16": "out16 lines16",
    "o17_l17": "out17 lines17",
    "o33_l33": "out33 lines33 nk1 nk2 compact dense",
    "o1025": "out1025 gt64tiles chunk4 full_sweep",
    "line0": "line0 rot180",
    "nk3": "nk3 compact dense",
    "nk5": "nk5 dense",
    "nk8": "nk8 ring512 chunk1r overlap full_sweep",
    "up_in1": "up_in1", "up_in2": "up_in2", "up_in3": "up_in3",
    "ck3": "chunk3r ring_tight overlap full_sweep",
    "ck2": "chunk2r ring_tight full_sweep",
    "wrap": "wrap2 chunk3r chunk4 hand_map full_sweep",
    "rot90": "rot90 b0_zero flip1",
    "rot180": "rot180 flip2",
    "rot270": "rot270 b0_zero",
    "obl_a": "oblique flip0",
    "obl_b": "oblique flip3",
    "crop_in": "crop_inside pitch_pad fast",
    "prep0": "prepared0", "prep1": "prepared1",
    "dead": "all_dead",
    "edge_on": "first_on last_on oblique",
    "edge_before": "first_before last_before oblique",
    "edge_after": "first_after last_after oblique",
    "clamp": "clamp_last clamp_body cn3",
    "yr_false": "yr_false clamp_body",
    "stripes": "saturates",
    "palette": "palette_mix",
    "f_pal": "oblique", "f_dn": "nk2 compact",
    "k_obl": "black_kept fill_opaque full_sweep",
    "k_dead": "black_kept all_dead fill_opaque",
    "k_dn": "black_kept nk3",
    "c4_obl": "cn4 oblique", "c4_full": "cn4 fast", "c4_crop": "cn4 crop_inside pitch_pad rot90", "c4_nk3": "cn4 nk3",
}
# what every row of a table must show (the launch's HSV form), and claims a row makes in one table only
TABLE_CLAIMS = {
    "geometry": "cn3 n_ranges4 nr4 no_zones black_out", "gather": "cn3 n_ranges4 nr4 no_zones black_out",
    "black_kept": "cn3 n_ranges1 nr1 no_zones black_kept full_sweep", "cn4": "cn4 n_ranges1 nr1 no_zones black_out",
    "zones5": "n_ranges5 nr6 zones full_sweep", "zones7": "n_ranges7 nr16 zones zones_lds full_sweep",
    "ranges7": "n_ranges7 nr16 no_zones black_out",
}
TABLE_ROW_CLAIMS = {("gather", "obl_a"): "may_trim", ("ranges7", "obl_a"): "may_trim", ("geometry", "o16_l16"): "rot0"}
# what the tables together must meet
REQUIRED = ("out1 out15 out16 out17 out33 out1025 lines1 lines15 lines16 lines17 lines33 line0 early_return "
            "nk1 nk2 nk3 nk5 nk8 ring512 dense compact up_in1 up_in2 up_in3 "
            "chunk1r chunk2r chunk3r chunk4 wrap2 overlap ring_tight "
            "rot0 rot90 rot180 rot270 b0_zero oblique flip0 flip1 flip2 flip3 crop_inside pitch_pad prepared0 prepared1 "
            "all_dead first_on first_before first_after last_on last_before last_after "
            "cn3 cn4 clamp_last yr_false fast "
            "n_ranges1 n_ranges4 n_ranges5 n_ranges7 nr6 nr16 zones no_zones zones_lds black_out black_kept may_trim "
            "fill_opaque gt64tiles saturates palette_mix t_pad").split()
