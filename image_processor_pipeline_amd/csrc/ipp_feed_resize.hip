// Training batches at the network's input size (ipp.h: ipp_scene_feed_resize,
// ipp_scene_feed_index_map_sampled, ipp_scene_feed_resize_lds; the traffic
// model and the LDS budget are in DESIGN.md §3).
//
//   k_feed_resize<T>   composites (S, bg_h, bg_w, 3) uint8 -> planar (S, 3,
//                      out_h, out_w) of T (2- or 4-byte opaque words): Pillow's
//                      two-pass Image.resize in integers, then a 3×256 table.
//                      One workgroup per (scene, tile of tw × th outputs).  In
//                      LDS: the table, the tile's bounds and taps (clamped to
//                      the staged span), the source span (span_y rows of span_x
//                      pixels, fetched in aligned dwords), and the H pass's
//                      uint8 intermediate as three planes.  The H pass takes
//                      one (source row, output column) per thread and all three
//                      channels, the V pass one (output row, channel, column)
//                      per thread: a wave stores 64 consecutive elements of one
//                      plane row.
//   k_feed_index_map_sampled   the index map of k_feed_index_map at the output
//                      size: a NEAREST gather through two coordinate tables,
//                      16 output bytes per thread in one 16-B store.
//   k_letterbox_images<T>   k_feed_resize into a rectangle of a larger canvas
//                      (ipp.h: ipp_scene_feed_letterbox): the same workgroup
//                      and LDS carve per tile of the canvas; the tile's part
//                      inside the rectangle goes through the same two passes,
//                      the rest is the table's pad word in aligned 16-B stores.
//   k_letterbox_index_map   k_feed_index_map_sampled into the same rectangle,
//                      0 around it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ipp.h"
#include "ipp_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = 32;          // the largest output tile; both halve until the extents fit
constexpr int kGroupsPerThread = 4;              // k_feed_index_map_sampled: 16-B groups a thread takes, a block apart
constexpr int kTileGroups = kThreads * kGroupsPerThread;

// The launch's geometry and the LDS carve (byte offsets, multiples of 16).
// Everything follows from (bg, out, ksize, elem_size): no table is read.
struct Geo {
    int32_t bg_w, bg_h, out_w, out_h, ksize_x, ksize_y;
    int32_t tw, th, ltw;         // tile (powers of two), log2 tw
    int32_t span_x, span_y;      // most source columns / rows a tile's windows cover
    int32_t row_dwords;          // dwords of a staged source row: 3·span_x bytes behind up to 3 bytes of lead
    int32_t t_pitch;             // bytes of an intermediate row: tw rounded up to 4
    uint32_t off_bx, off_by, off_kx, off_ky, off_src, off_t, total;
    uint32_t tiles_x, tiles_y;
};

inline uint32_t up16(uint32_t v) { return (v + 15u) & ~15u; }

// Source positions a run of `n` consecutive outputs can touch: the windows of
// Resample.c precompute_coeffs start at int(center - support + 0.5) and end at
// int(center + support + 0.5) with 2·support <= ksize - 1, so from the first
// window's start to the last one's end there are fewer than (n - 1)·in/out +
// ksize + 1 positions; never more than the axis has.
inline int32_t span_of(int32_t n, int32_t in_size, int32_t out_size, int32_t ksize) {
    const int64_t s = ((int64_t)(n - 1) * in_size + out_size - 1) / out_size + ksize + 1;
    return (int32_t)(s < in_size ? s : in_size);
}

inline void carve(Geo& g, int32_t tw, int32_t th, int32_t elem_size) {
    g.tw = tw, g.th = th;
    g.ltw = 0;
    while ((1 << g.ltw) < tw) ++g.ltw;
    g.span_x = span_of(tw, g.bg_w, g.out_w, g.ksize_x);
    g.span_y = span_of(th, g.bg_h, g.out_h, g.ksize_y);
    g.row_dwords = (3 * g.span_x + 3 + 3) / 4;
    g.t_pitch = (tw + 3) & ~3;
    uint32_t at = up16(3u * 256u * (uint32_t)elem_size);
    g.off_bx = at, at += up16(8u * (uint32_t)tw);
    g.off_by = at, at += up16(8u * (uint32_t)th);
    g.off_kx = at, at += up16(4u * (uint32_t)tw * (uint32_t)g.ksize_x);
    g.off_ky = at, at += up16(4u * (uint32_t)th * (uint32_t)g.ksize_y);
    g.off_src = at, at += up16(4u * (uint32_t)g.row_dwords * (uint32_t)g.span_y);
    g.off_t = at, at += up16(3u * (uint32_t)g.t_pitch * (uint32_t)g.span_y);
    g.total = at;
}

// The largest tile whose extents fit the budget: from 64 × 32, halve the side
// whose halving leaves fewer bytes (the height on a tie) until they do.  False
// when even 1 × 1 does not fit (no ksize up to IPP_FEED_RESIZE_MAX_KSIZE gets
// there: tests/test_feed_resize_cpu.py sweeps them).
bool plan_tile(Geo& g, int32_t elem_size) {
    int32_t tw = kTileW, th = kTileH;
    for (;;) {
        carve(g, tw, th, elem_size);
        if (g.total <= (uint32_t)IPP_FEED_RESIZE_LDS_BYTES) break;
        if (tw == 1 && th == 1) return false;
        Geo a = g, b = g;
        if (th > 1) carve(a, tw, th / 2, elem_size);
        if (tw > 1) carve(b, tw / 2, th, elem_size);
        if (tw == 1 || (th > 1 && a.total <= b.total))
            th /= 2;
        else
            tw /= 2;
    }
    g.tiles_x = (uint32_t)((g.out_w + g.tw - 1) / g.tw);
    g.tiles_y = (uint32_t)((g.out_h + g.th - 1) / g.th);
    return true;
}

bool geometry(Geo& g, int32_t bg_w, int32_t bg_h, int32_t out_w, int32_t out_h, int32_t ksize_x, int32_t ksize_y,
              int32_t elem_size) {
    if (bg_w < 1 || bg_h < 1 || out_w < 1 || out_h < 1) return false;
    if (elem_size != 2 && elem_size != 4) return false;
    if (ksize_x < 1 || ksize_x > IPP_FEED_RESIZE_MAX_KSIZE || ksize_y < 1 || ksize_y > IPP_FEED_RESIZE_MAX_KSIZE) return false;
    if ((int64_t)bg_w * bg_h >= (1ll << 28) || (int64_t)out_w * out_h >= (1ll << 28)) return false;
    g.bg_w = bg_w, g.bg_h = bg_h, g.out_w = out_w, g.out_h = out_h, g.ksize_x = ksize_x, g.ksize_y = ksize_y;
    return plan_tile(g, elem_size);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Why no byte outside the n_scenes·bg_h·bg_w·3 of `in` is read and none outside
// the n_scenes·3·out_h·out_w elements of `out` written, whatever the tables
// hold: the staged span starts at (x0, y0) clamped into the image and has nx <=
// bg_w - x0 columns and ny <= bg_h - y0 rows, so its bytes lie inside scene s <
// n_scenes; they are fetched in aligned dwords, and a dword that is not wholly
// inside [in, in_end) is assembled from those of its bytes that are.  Every
// window is clamped to the staged span when its bounds are copied to LDS (start
// in 0..nx, count in 0..min(ksize, nx - start); rows alike), and the taps of
// output i are read at i·ksize + k < tile·ksize words of LDS that were copied
// from words (xo0 + i)·ksize + k < out·ksize of the tap table.  Stores go to
// (dy0 + j, dx0 + i) of plane 0..2 of scene s: (yo0 + j < out_h, xo0 + i <
// out_w) in k_feed_resize, inside the rectangle in k_letterbox_images.
//
// resize_block is one workgroup's work on the run of nw × nh outputs from (xo0,
// yo0) of the resized image (nw <= g.tw, nh <= g.th: the extents of the carve
// hold for any such run, wherever it starts); they are stored from (dx0, dy0)
// of the dst_w-wide planes of Q elements of scene s.  k_feed_resize takes the
// tile itself there, k_letterbox_images the tile's part inside the rectangle.
template <typename T>
__device__ __forceinline__ void resize_block(uint8_t* smem, const uint8_t* __restrict__ in, T* __restrict__ out,
                                             const T* __restrict__ lut, const int32_t* __restrict__ taps_x,
                                             const int32_t* __restrict__ taps_y, int n_scenes, int bgr, const Geo& g,
                                             FastDiv row_dw, uint32_t s, int xo0, int yo0, int nw, int nh, int64_t Q,
                                             int dst_w, int dx0, int dy0) {
    T* const s_lut = reinterpret_cast<T*>(smem);
    int32_t* const s_bx = reinterpret_cast<int32_t*>(smem + g.off_bx);
    int32_t* const s_by = reinterpret_cast<int32_t*>(smem + g.off_by);
    int32_t* const s_kx = reinterpret_cast<int32_t*>(smem + g.off_kx);
    int32_t* const s_ky = reinterpret_cast<int32_t*>(smem + g.off_ky);
    uint8_t* const s_src = smem + g.off_src;
    uint8_t* const s_t = smem + g.off_t;

    const int tid = (int)threadIdx.x;
    const int x0 = clampi(taps_x[2 * xo0], 0, g.bg_w - 1), y0 = clampi(taps_y[2 * yo0], 0, g.bg_h - 1);
    const int nx = min(g.span_x, g.bg_w - x0), ny = min(g.span_y, g.bg_h - y0);

#pragma unroll
    for (int c = 0; c < 3; ++c) s_lut[256 * c + tid] = lut[256 * c + tid];
    for (int i = tid; i < nw; i += kThreads) {
        const int rel = clampi(taps_x[2 * (xo0 + i)] - x0, 0, nx);
        s_bx[2 * i] = rel;
        s_bx[2 * i + 1] = clampi(taps_x[2 * (xo0 + i) + 1], 0, min(g.ksize_x, nx - rel));
    }
    for (int j = tid; j < nh; j += kThreads) {
        const int rel = clampi(taps_y[2 * (yo0 + j)] - y0, 0, ny);
        s_by[2 * j] = rel;
        s_by[2 * j + 1] = clampi(taps_y[2 * (yo0 + j) + 1], 0, min(g.ksize_y, ny - rel));
    }
    {
        const int32_t* kx = taps_x + 2 * (int64_t)g.out_w + (int64_t)xo0 * g.ksize_x;
        for (int i = tid; i < nw * g.ksize_x; i += kThreads) s_kx[i] = kx[i];
        const int32_t* ky = taps_y + 2 * (int64_t)g.out_h + (int64_t)yo0 * g.ksize_y;
        for (int j = tid; j < nh * g.ksize_y; j += kThreads) s_ky[j] = ky[j];
    }

    // The source span: row r's bytes start at p_r = scene + 3·((y0 + r)·bg_w +
    // x0); the dwords from p_r rounded down to 4 go to the row's LDS dwords,
    // so pixel x0 + i sits `lead` = p_r & 3 bytes into the LDS row.
    const int64_t P = (int64_t)g.bg_w * g.bg_h;
    const uint8_t* const scene = in + (int64_t)s * 3 * P;
    const uintptr_t in_lo = reinterpret_cast<uintptr_t>(in), in_hi = in_lo + (uintptr_t)((int64_t)n_scenes * 3 * P);
    const uintptr_t span0 = reinterpret_cast<uintptr_t>(scene) + 3u * (uintptr_t)((int64_t)y0 * g.bg_w + x0);
    const uint32_t row_step = 3u * (uint32_t)g.bg_w;
    for (uint32_t idx = (uint32_t)tid; idx < (uint32_t)(ny * g.row_dwords); idx += kThreads) {
        const uint32_t r = fdiv(idx, row_dw), d = idx - r * row_dw.d;
        const uintptr_t p = span0 + (uintptr_t)r * row_step;
        const uint32_t lead = (uint32_t)p & 3u;
        if (4u * d >= lead + 3u * (uint32_t)nx) continue;
        const uintptr_t q = p - lead + 4u * d;
        uint32_t w;
        if (q >= in_lo && q + 4u <= in_hi) {
            w = *reinterpret_cast<const uint32_t*>(q);
        } else {
            w = 0u;
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b)
                if (q + b >= in_lo && q + b < in_hi) w |= (uint32_t)*reinterpret_cast<const uint8_t*>(q + b) << (8u * b);
        }
        reinterpret_cast<uint32_t*>(s_src)[idx] = w;
    }
    __syncthreads();

    // H pass: t[c][r][i] = clip8((2^21 + Σ_k src[r][rel_i + k][c] · kx[i][k]) >> 22), rounded and clipped to uint8.
    const int plane_t = g.span_y * g.t_pitch;
    for (int idx = tid; idx < (ny << g.ltw); idx += kThreads) {
        const int r = idx >> g.ltw, i = idx & (g.tw - 1);
        if (i >= nw) continue;
        const uint32_t lead = (uint32_t)(span0 + (uintptr_t)r * row_step) & 3u;
        const int rel = s_bx[2 * i], cnt = s_bx[2 * i + 1];
        const int32_t* k = s_kx + i * g.ksize_x;
        const uint8_t* sp = s_src + 4 * r * g.row_dwords + lead + 3 * rel;
        int32_t a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int kk = 0; kk < cnt; ++kk) {
            const int32_t tap = k[kk];
            a0 += (int32_t)sp[3 * kk] * tap;
            a1 += (int32_t)sp[3 * kk + 1] * tap;
            a2 += (int32_t)sp[3 * kk + 2] * tap;
        }
        uint8_t* t = s_t + r * g.t_pitch + i;
        t[0] = (uint8_t)clip8(a0);
        t[plane_t] = (uint8_t)clip8(a1);
        t[2 * plane_t] = (uint8_t)clip8(a2);
    }
    __syncthreads();

    // V pass over t, then the table: input channel c feeds plane pl = c (2 - c with bgr) through table row pl.
    T* const dst = out + (int64_t)s * 3 * Q;
    for (int idx = tid; idx < ((3 * nh) << g.ltw); idx += kThreads) {
        const int jc = idx >> g.ltw, i = idx & (g.tw - 1);
        if (i >= nw) continue;
        const int j = jc / 3, c = jc - 3 * j;
        const int rel = s_by[2 * j], cnt = s_by[2 * j + 1];
        const int32_t* k = s_ky + j * g.ksize_y;
        const uint8_t* tp = s_t + c * plane_t + rel * g.t_pitch + i;
        int32_t a = 1 << 21;
        for (int kk = 0; kk < cnt; ++kk) a += (int32_t)tp[kk * g.t_pitch] * k[kk];
        const int pl = bgr ? 2 - c : c;
        dst[(int64_t)pl * Q + (int64_t)(dy0 + j) * dst_w + (dx0 + i)] = s_lut[256 * pl + (int)clip8(a)];
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_feed_resize(const uint8_t* __restrict__ in, T* __restrict__ out,
                                                          const T* __restrict__ lut,
                                                          const int32_t* __restrict__ taps_x,
                                                          const int32_t* __restrict__ taps_y, int n_scenes, int bgr,
                                                          Geo g, FastDiv tiles_x, FastDiv tiles_xy, FastDiv row_dw) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t s = fdiv(blockIdx.x, tiles_xy), rest = blockIdx.x - s * tiles_xy.d;
    const uint32_t ty = fdiv(rest, tiles_x), tx = rest - ty * tiles_x.d;
    const int xo0 = (int)tx * g.tw, yo0 = (int)ty * g.th;
    const int nw = min(g.tw, g.out_w - xo0), nh = min(g.th, g.out_h - yo0);
    resize_block<T>(smem, in, out, lut, taps_x, taps_y, n_scenes, bgr, g, row_dw, s, xo0, yo0, nw, nh,
                    (int64_t)g.out_w * g.out_h, g.out_w, xo0, yo0);
}

// The table of scene s as in k_feed_index_map (ipp_feed.hip), one entry per thread.
__device__ __forceinline__ void scene_index_table(uint8_t* s_idx, const int32_t* __restrict__ slot, uint32_t s,
                                                  int per_scene, uint32_t tid) {
    uint32_t keepmask = 0u;
    for (int k = 0; k < per_scene; ++k) keepmask |= (slot[(int64_t)s * per_scene + k] >= 0 ? 1u : 0u) << k;
    const uint32_t v = tid & keepmask;
    s_idx[tid] = v == 0u ? 0u : (uint8_t)(1 + __popc(keepmask & ((1u << (31 - __clz((int)v))) - 1u)));
    __syncthreads();
}

// A group is 16 bytes of an output row; its bytes at columns >= out_w are 0.
// Coordinates are clamped into the map, so a wrong table cannot read outside
// the n_scenes·bg_h·pitch bytes; only the n_scenes·out_h·out_pitch bytes of out
// are written.
__global__ __launch_bounds__(kThreads) void k_feed_index_map_sampled(
    const uint8_t* __restrict__ map, int pitch, int bg_w, int bg_h, const int32_t* __restrict__ slot, int per_scene,
    const int32_t* __restrict__ xtab, const int32_t* __restrict__ ytab, int out_w, uint32_t groups_per_scene,
    FastDiv tiles, FastDiv row_groups, uint8_t* __restrict__ out) {
    __shared__ uint8_t s_idx[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t s = fdiv(blockIdx.x, tiles), tile = blockIdx.x - s * tiles.d;
    scene_index_table(s_idx, slot, s, per_scene, tid);
    const uint8_t* const src = map + (int64_t)s * bg_h * pitch;
    uint8_t* const dst = out + (int64_t)s * groups_per_scene * 16;
#pragma unroll
    for (int u = 0; u < kGroupsPerThread; ++u) {
        const uint32_t gi = tile * (uint32_t)kTileGroups + tid + (uint32_t)(u * kThreads);
        if (gi >= groups_per_scene) continue;
        const uint32_t y = fdiv(gi, row_groups);
        const int col0 = (int)(gi - y * row_groups.d) * 16;
        const uint8_t* row = src + (int64_t)clampi(ytab[y], 0, bg_h - 1) * pitch;
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i] = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int x = col0 + 4 * i + b;
                if (x < out_w) w[i] |= (uint32_t)s_idx[row[clampi(xtab[x], 0, bg_w - 1)]] << (8 * b);
            }
        }
        *reinterpret_cast<uint4*>(dst + 16 * (int64_t)gi) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// The canvas of a letterboxed batch around the rectangle of g.out_w × g.out_h
// resized pixels at (left, top).
struct Canvas {
    int32_t w, h, left, top, pad;
};

// Elements [p, p + n) of one plane row set to v by 32 lanes: lane l takes the
// l-th 16-B aligned chunk that meets the run (a run of a tile has at most
// 64·4 / 16 + 1 = 17), in one 16-B store where the chunk lies inside the run
// and element by element where it is cut by the run's first or last byte.
template <typename T>
__device__ __forceinline__ void fill_run(T* p, int n, T v, int l) {
    if (n <= 0) return;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(p), a1 = a0 + (uintptr_t)n * sizeof(T);
    const uintptr_t c = (a0 & ~(uintptr_t)15) + 16u * (uintptr_t)l;
    if (c >= a1) return;
    if (c >= a0 && c + 16u <= a1) {
        const uint32_t w = sizeof(T) == 2 ? (uint32_t)v * 0x10001u : (uint32_t)v;
        *reinterpret_cast<uint4*>(c) = make_uint4(w, w, w, w);
    } else {
        const uintptr_t hi = c + 16u < a1 ? c + 16u : a1;
        for (uintptr_t q = c > a0 ? c : a0; q < hi; q += sizeof(T)) *reinterpret_cast<T*>(q) = v;
    }
}

// One workgroup per (scene, tile of g.tw × g.th canvas elements).  The tile's
// part inside the rectangle is a run of at most g.tw × g.th resized outputs and
// goes through resize_block; a tile wholly in the pad skips it: it reads
// nothing of `in`, of the taps or of the table but its three pad words, and
// stages nothing.  The rest of the tile — per row the columns before and
// behind the rectangle, or all of them — is filled by fill_run, 32 lanes per
// row, so that every element of the canvas is written by exactly one of the
// two parts and stores stay inside rows y < cv.h, columns x < cv.w of scene s.
template <typename T>
__global__ __launch_bounds__(kThreads) void k_letterbox_images(const uint8_t* __restrict__ in, T* __restrict__ out,
                                                               const T* __restrict__ lut,
                                                               const int32_t* __restrict__ taps_x,
                                                               const int32_t* __restrict__ taps_y, int n_scenes,
                                                               int bgr, Geo g, Canvas cv, FastDiv tiles_x,
                                                               FastDiv tiles_xy, FastDiv row_dw) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t s = fdiv(blockIdx.x, tiles_xy), rest = blockIdx.x - s * tiles_xy.d;
    const uint32_t ty = fdiv(rest, tiles_x), tx = rest - ty * tiles_x.d;
    const int cx0 = (int)tx * g.tw, cy0 = (int)ty * g.th;
    const int cx1 = cx0 + min(g.tw, cv.w - cx0), cy1 = cy0 + min(g.th, cv.h - cy0);
    const int ix0 = max(cx0, cv.left), ix1 = min(cx1, cv.left + g.out_w);
    const int iy0 = max(cy0, cv.top), iy1 = min(cy1, cv.top + g.out_h);
    const bool meets = ix0 < ix1 && iy0 < iy1;
    const int64_t Q = (int64_t)cv.w * cv.h;
    if (meets)
        resize_block<T>(smem, in, out, lut, taps_x, taps_y, n_scenes, bgr, g, row_dw, s, ix0 - cv.left, iy0 - cv.top,
                        ix1 - ix0, iy1 - iy0, Q, cv.w, ix0, iy0);
    const int l = (int)threadIdx.x & 31;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        const T v = lut[256 * pl + cv.pad];
        T* const plane = out + ((int64_t)s * 3 + pl) * Q;
        for (int y = cy0 + ((int)threadIdx.x >> 5); y < cy1; y += kThreads / 32) {
            const bool inside = meets && y >= iy0 && y < iy1;
            T* const row = plane + (int64_t)y * cv.w;
            fill_run<T>(row + cx0, (inside ? ix0 : cx1) - cx0, v, l);
            if (inside) fill_run<T>(row + ix1, cx1 - ix1, v, l);
        }
    }
}

// k_feed_index_map_sampled inside the rectangle of new_w × new_h samples at
// (left, top) of the output rows, 0 around it: a group that lies in the pad
// reads neither the tables nor the map.  left + new_w <= out_w <= out_pitch, so
// the pitch columns are pad too.
__global__ __launch_bounds__(kThreads) void k_letterbox_index_map(
    const uint8_t* __restrict__ map, int pitch, int bg_w, int bg_h, const int32_t* __restrict__ slot, int per_scene,
    const int32_t* __restrict__ xtab, const int32_t* __restrict__ ytab, int new_w, int new_h, int left, int top,
    uint32_t groups_per_scene, FastDiv tiles, FastDiv row_groups, uint8_t* __restrict__ out) {
    __shared__ uint8_t s_idx[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t s = fdiv(blockIdx.x, tiles), tile = blockIdx.x - s * tiles.d;
    scene_index_table(s_idx, slot, s, per_scene, tid);
    const uint8_t* const src = map + (int64_t)s * bg_h * pitch;
    uint8_t* const dst = out + (int64_t)s * groups_per_scene * 16;
#pragma unroll
    for (int u = 0; u < kGroupsPerThread; ++u) {
        const uint32_t gi = tile * (uint32_t)kTileGroups + tid + (uint32_t)(u * kThreads);
        if (gi >= groups_per_scene) continue;
        const uint32_t y = fdiv(gi, row_groups);
        const int col0 = (int)(gi - y * row_groups.d) * 16 - left, yy = (int)y - top;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if ((unsigned)yy < (unsigned)new_h && col0 + 15 >= 0 && col0 < new_w) {
            const uint8_t* row = src + (int64_t)clampi(ytab[yy], 0, bg_h - 1) * pitch;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int x = col0 + 4 * i + b;
                    if ((unsigned)x < (unsigned)new_w) w[i] |= (uint32_t)s_idx[row[clampi(xtab[x], 0, bg_w - 1)]] << (8 * b);
                }
            }
        }
        *reinterpret_cast<uint4*>(dst + 16 * (int64_t)gi) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

template <typename T>
void launch_letterbox(const uint8_t* in, void* out, const void* lut, const int32_t* taps_x, const int32_t* taps_y,
                      int n_scenes, int bgr, const Geo& g, const Canvas& cv, uint32_t tiles_x, uint32_t tiles_y,
                      hipStream_t s) {
    const uint32_t per_scene = tiles_x * tiles_y;
    hipLaunchKernelGGL(k_letterbox_images<T>, dim3((uint32_t)n_scenes * per_scene), dim3(kThreads), g.total, s, in,
                       static_cast<T*>(out), static_cast<const T*>(lut), taps_x, taps_y, n_scenes, bgr, g, cv,
                       fast_div(tiles_x), fast_div(per_scene), fast_div((uint32_t)g.row_dwords));
}

// The rectangle of new_w × new_h at (left, top) lies inside out_w × out_h.
inline bool rect_inside(int32_t new_w, int32_t new_h, int32_t left, int32_t top, int32_t out_w, int32_t out_h) {
    return new_w >= 1 && new_h >= 1 && left >= 0 && top >= 0 && out_w >= 1 && out_h >= 1 &&
           (int64_t)left + new_w <= out_w && (int64_t)top + new_h <= out_h;
}

template <typename T>
void launch_resize(const uint8_t* in, void* out, const void* lut, const int32_t* taps_x, const int32_t* taps_y,
                   int n_scenes, int bgr, const Geo& g, hipStream_t s) {
    const uint32_t per_scene = g.tiles_x * g.tiles_y;
    hipLaunchKernelGGL(k_feed_resize<T>, dim3((uint32_t)n_scenes * per_scene), dim3(kThreads), g.total, s, in,
                       static_cast<T*>(out), static_cast<const T*>(lut), taps_x, taps_y, n_scenes, bgr, g,
                       fast_div(g.tiles_x), fast_div(per_scene), fast_div((uint32_t)g.row_dwords));
}

}  // namespace

extern "C" int64_t ipp_scene_feed_resize_lds(int32_t bg_w, int32_t bg_h, int32_t out_w, int32_t out_h, int32_t ksize_x,
                                             int32_t ksize_y, int32_t elem_size, int32_t* tile) {
    Geo g;
    if (!geometry(g, bg_w, bg_h, out_w, out_h, ksize_x, ksize_y, elem_size)) return IPP_E_ARG;
    if (tile) tile[0] = g.tw, tile[1] = g.th;
    return (int64_t)g.total;
}

extern "C" int ipp_scene_feed_resize(const uint8_t* in, void* out, const void* lut, const int32_t* taps_x,
                                     const int32_t* taps_y, int32_t n_scenes, int32_t bg_w, int32_t bg_h, int32_t out_w,
                                     int32_t out_h, int32_t ksize_x, int32_t ksize_y, int32_t elem_size, int32_t bgr,
                                     void* stream) {
    if (!in || !out || !lut || !taps_x || !taps_y || n_scenes < 1) return IPP_E_ARG;
    if (bgr != 0 && bgr != 1) return IPP_E_ARG;
    Geo g;
    if (!geometry(g, bg_w, bg_h, out_w, out_h, ksize_x, ksize_y, elem_size)) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(lut)) & (uintptr_t)(elem_size - 1)) != 0) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(taps_x) | reinterpret_cast<uintptr_t>(taps_y)) & 3u) != 0) return IPP_E_ARG;
    if ((int64_t)g.tiles_x * g.tiles_y * n_scenes >= INT32_MAX) return IPP_E_ARG;
    if (elem_size == 2)
        launch_resize<uint16_t>(in, out, lut, taps_x, taps_y, n_scenes, bgr, g, (hipStream_t)stream);
    else
        launch_resize<uint32_t>(in, out, lut, taps_x, taps_y, n_scenes, bgr, g, (hipStream_t)stream);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

extern "C" int ipp_scene_feed_index_map_sampled(const uint8_t* map, int64_t map_pitch, int32_t bg_w, int32_t bg_h,
                                                const int32_t* slot, int32_t n_scenes, int32_t per_scene,
                                                const int32_t* xtab, const int32_t* ytab, int32_t out_w, int32_t out_h,
                                                uint8_t* out, int64_t out_pitch, void* stream) {
    if (!map || !slot || !xtab || !ytab || !out || n_scenes < 1 || bg_w < 1 || bg_h < 1 || out_w < 1 || out_h < 1)
        return IPP_E_ARG;
    if (per_scene < 1 || per_scene > IPP_SCENE_MAP_MAX_LAYERS) return IPP_E_ARG;
    if (map_pitch < bg_w || map_pitch > INT32_MAX) return IPP_E_ARG;
    if (out_pitch < out_w || (out_pitch & 15) != 0 || out_pitch > INT32_MAX) return IPP_E_ARG;
    if ((reinterpret_cast<uintptr_t>(out) & 15u) != 0 ||
        ((reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(xtab) | reinterpret_cast<uintptr_t>(ytab)) & 3u) != 0)
        return IPP_E_ARG;
    if ((int64_t)bg_h * map_pitch >= (1ll << 32)) return IPP_E_ARG;
    const int64_t groups = (int64_t)out_h * (out_pitch / 16);
    if (groups >= (1ll << 28)) return IPP_E_ARG;  // offsets inside a scene fit 32 bits
    const int64_t tiles = (groups + kTileGroups - 1) / kTileGroups;
    if (tiles * n_scenes >= INT32_MAX) return IPP_E_ARG;
    hipLaunchKernelGGL(k_feed_index_map_sampled, dim3((uint32_t)(n_scenes * tiles)), dim3(kThreads), 0,
                       (hipStream_t)stream, map, (int)map_pitch, bg_w, bg_h, slot, per_scene, xtab, ytab, out_w,
                       (uint32_t)groups, fast_div((uint32_t)tiles), fast_div((uint32_t)(out_pitch / 16)), out);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

extern "C" int ipp_scene_feed_letterbox(const uint8_t* in, void* out, const void* lut, const int32_t* taps_x,
                                        const int32_t* taps_y, int32_t n_scenes, int32_t bg_w, int32_t bg_h,
                                        int32_t new_w, int32_t new_h, int32_t left, int32_t top, int32_t out_w,
                                        int32_t out_h, int32_t ksize_x, int32_t ksize_y, int32_t pad, int32_t elem_size,
                                        int32_t bgr, void* stream) {
    if (!in || !out || !lut || !taps_x || !taps_y || n_scenes < 1) return IPP_E_ARG;
    if ((bgr != 0 && bgr != 1) || pad < 0 || pad > 255) return IPP_E_ARG;
    if (!rect_inside(new_w, new_h, left, top, out_w, out_h) || (int64_t)out_w * out_h >= (1ll << 28)) return IPP_E_ARG;
    Geo g;  // of the rectangle: ipp_scene_feed_resize_lds(bg_w, bg_h, new_w, new_h, ...) states this tile and these bytes
    if (!geometry(g, bg_w, bg_h, new_w, new_h, ksize_x, ksize_y, elem_size)) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(lut)) & (uintptr_t)(elem_size - 1)) != 0) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(taps_x) | reinterpret_cast<uintptr_t>(taps_y)) & 3u) != 0) return IPP_E_ARG;
    const uint32_t tiles_x = (uint32_t)((out_w + g.tw - 1) / g.tw), tiles_y = (uint32_t)((out_h + g.th - 1) / g.th);
    if ((int64_t)tiles_x * tiles_y * n_scenes >= INT32_MAX) return IPP_E_ARG;
    const Canvas cv = {out_w, out_h, left, top, pad};
    if (elem_size == 2)
        launch_letterbox<uint16_t>(in, out, lut, taps_x, taps_y, n_scenes, bgr, g, cv, tiles_x, tiles_y, (hipStream_t)stream);
    else
        launch_letterbox<uint32_t>(in, out, lut, taps_x, taps_y, n_scenes, bgr, g, cv, tiles_x, tiles_y, (hipStream_t)stream);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

extern "C" int ipp_scene_feed_index_map_letterbox(const uint8_t* map, int64_t map_pitch, int32_t bg_w, int32_t bg_h,
                                                  const int32_t* slot, int32_t n_scenes, int32_t per_scene,
                                                  const int32_t* xtab, const int32_t* ytab, int32_t new_w,
                                                  int32_t new_h, int32_t left, int32_t top, int32_t out_w,
                                                  int32_t out_h, uint8_t* out, int64_t out_pitch, void* stream) {
    if (!map || !slot || !xtab || !ytab || !out || n_scenes < 1 || bg_w < 1 || bg_h < 1) return IPP_E_ARG;
    if (!rect_inside(new_w, new_h, left, top, out_w, out_h)) return IPP_E_ARG;
    if (per_scene < 1 || per_scene > IPP_SCENE_MAP_MAX_LAYERS) return IPP_E_ARG;
    if (map_pitch < bg_w || map_pitch > INT32_MAX) return IPP_E_ARG;
    if (out_pitch < out_w || (out_pitch & 15) != 0 || out_pitch > INT32_MAX) return IPP_E_ARG;
    if ((reinterpret_cast<uintptr_t>(out) & 15u) != 0 ||
        ((reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(xtab) | reinterpret_cast<uintptr_t>(ytab)) & 3u) != 0)
        return IPP_E_ARG;
    if ((int64_t)bg_h * map_pitch >= (1ll << 32)) return IPP_E_ARG;
    const int64_t groups = (int64_t)out_h * (out_pitch / 16);
    if (groups >= (1ll << 28)) return IPP_E_ARG;  // offsets inside a scene fit 32 bits
    const int64_t tiles = (groups + kTileGroups - 1) / kTileGroups;
    if (tiles * n_scenes >= INT32_MAX) return IPP_E_ARG;
    hipLaunchKernelGGL(k_letterbox_index_map, dim3((uint32_t)(n_scenes * tiles)), dim3(kThreads), 0,
                       (hipStream_t)stream, map, (int)map_pitch, bg_w, bg_h, slot, per_scene, xtab, ytab, new_w, new_h,
                       left, top, (uint32_t)groups, fast_div((uint32_t)tiles), fast_div((uint32_t)(out_pitch / 16)), out);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}
