// ipp_label.hip — boxes for the YOLO labels of pasted overlays
// (overlays.py:141-149 writes one label per composite).
//
//   ipp_pipe_overlay_bbox: the tight box of each item's resized overlay in the
//   fused pipe.  The resized overlay is never materialised there: its alpha
//   exists only as T (the H pass's scratch) combined with the V-axis tap
//   tiles.  The kernel is the V pass of ipp_pipe_vblend.hip's k_pipe_vblend_mfma
//   restricted to channel 3: it reads dword 3 of each 16-B T group and the
//   band's tap tile, and writes nothing but the boxes.
//
//   ipp_alpha_bbox_min: the same box on a materialised 2/4-channel image
//   (the plugin path), ipp_alpha_bbox with a threshold.
//
//   ipp_pipe_scene_boxes: scenes of K overlays per composite — per overlay
//   the box of the pixels no later layer covers, its present and its visible
//   pixel counts (the same channel-3 V pass, stored as alpha planes, then a
//   pass that compares the planes by composite coordinate).
//
//   ipp_pipe_scene_map: the same rule's per-pixel answer — one visibility map
//   per composite, bit k = layer k visible (instance masks), from the same
//   planes; optionally the boxes with it.
//
//   ipp_pipe_scene_cull: the rule once more, top down and with a verdict —
//   an overlay that the kept later layers leave too little of is culled: its T
//   is overwritten with 0x80, the T of a transparent overlay, so the V launches
//   paste nothing of it and every later reader of tmp sees it absent.
//
//   ipp_pipe_scene_amodal: what the rule hides — per overlay the box and the
//   map of its present pixels, covered or not (the amodal ground truth), and
//   per pair of layers how many pixels the later one covers and hides, from the
//   same planes; optionally the visible boxes and map with them.
//
// All follow ipp_alpha_bbox's convention (ipp_gather.hip): the boxes are
// pre-set to (INT_MAX, INT_MAX, -1, -1), every wave that saw a visible pixel
// issues four device-scope atomics, and a finish kernel turns an untouched row
// into (-1, -1, -1, -1).
#include <climits>

#include "ipp_device.h"
#include "ipp_pipe_layout.h"

namespace {

using namespace pipe_layout;

__global__ void k_label_bbox_init(int32_t* bbox, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        bbox[4 * i + 0] = INT32_MAX;
        bbox[4 * i + 1] = INT32_MAX;
        bbox[4 * i + 2] = -1;
        bbox[4 * i + 3] = -1;
    }
}

__global__ void k_label_bbox_finish(int32_t* bbox, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && bbox[4 * i + 2] < 0) bbox[4 * i + 0] = bbox[4 * i + 1] = -1;
}

// Wave-wide min/max of the lanes' boxes, then four atomics from lane 0.
__device__ __forceinline__ void bbox_commit(int32_t* __restrict__ row, int xmin, int ymin, int xmax, int ymax) {
    for (int off = 32; off > 0; off >>= 1) {
        xmin = min(xmin, __shfl_xor(xmin, off));
        ymin = min(ymin, __shfl_xor(ymin, off));
        xmax = max(xmax, __shfl_xor(xmax, off));
        ymax = max(ymax, __shfl_xor(ymax, off));
    }
    if ((threadIdx.x & 63) == 0 && xmax >= 0) {
        atomicMin(&row[0], xmin);
        atomicMin(&row[1], ymin);
        atomicMax(&row[2], xmax + 1);
        atomicMax(&row[3], ymax + 1);
    }
}

// Block = one V tap tile (one 16-row composite band the overlay touches) of
// one item; its four waves stride over the 16-column tiles.
//
// The band, tap tile and T group addressing is ipp_pipe_layout.h's, as in
// ipp_pipe_vblend.hip's vblend_block (tests/test_gpu_labels.py compares the boxes
// with the resized overlay's alpha).
//   A = the tile's taps, one byte plane per MFMA (lane l: row l&15, T rows
//       16(l>>4)..+15 of the K step);
//   B = 64 T rows × 16 overlay columns of alpha: dword 3 (byte offset 12) of
//       the lane's four 16-B T groups;
//   D lane l = column l&15, rows 4(l>>4)..+3.
// One accumulator per tap byte plane over a runtime K loop (every nK the
// planner emits; T is read once), the row bias in plane 0's initial value,
// then the Horner step over the planes (planes3) — vblend_block's generic
// form for channel 3 alone: 3 MFMAs per K step.
//
// overlay_alpha_band is that block: it hands every pixel of the band (overlay
// column x, overlay row o, alpha a) to `sink`, each pixel from exactly one
// lane.  k_pipe_overlay_bbox folds them into a box; k_scene_alpha
// (ipp_pipe_scene_boxes) stores them as a plane.
template <typename Sink>
__device__ __forceinline__ void overlay_alpha_band(const uint8_t* __restrict__ tmp, const int32_t* __restrict__ coefs,
                                                   const ipp_pipe_desc* __restrict__ descs, int im, int ty,
                                                   const uint16_t* __restrict__ trim, Sink sink) {
    const ipp_paste_desc p = descs[im].p;
    int vb0, vb1;
    paste_bands(p, vb0, vb1);
    const int y0 = vb0 + ty * kBandRows;
    if (y0 >= vb1 || y0 >= p.bg_h) return;  // block-uniform
    const int nrows = min(kBandRows, p.bg_h - y0);
    const int oy_lo = max(0, y0 - p.y), oy_hi = min(p.ov_h, y0 + nrows - p.y);
    if (oy_lo >= oy_hi) return;  // block-uniform
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    const ipp_resample_desc v = descs[im].v;
    const int phase = tap_phase(p.y);
    const int t = band_tap_tile(y0, p.y, phase);
    const TapTiles tt = tap_tiles(coefs, v.coef_off, tap_ntiles(v.out_len, phase));
    int4 th = tt.hdr[t];
    th.x = __builtin_amdgcn_readfirstlane(th.x);  // first T row of the tile's window
    th.y = __builtin_amdgcn_readfirstlane(th.y);  // K steps
    th.z = __builtin_amdgcn_readfirstlane(th.z);  // first tap block
    const int ctiles = (p.ov_w + 15) >> 4;
    const int64_t gstride = t_pitch_vecs(v.src_pitch);
    const int x_l = lane & 15;
    int32_t rb[4];  // the row biases
#pragma unroll
    for (int r = 0; r < 4; ++r) rb[r] = tt.bias[kBiasWords * t + 4 * (lane >> 4) + r];
    const int gbase = t_row_group(th.x + 16 * (lane >> 4));
    const int hbands = trim_bands(descs[im].h.lines);  // H bands of the item with a trim entry
    // The alpha dword of T group (row group gbase, column 0); the loop below
    // walks t_group's address from it by whole groups and group rows.
    const uint8_t* abase = tmp + v.src_off + gbase * gstride * kTGroupBytes + kTAlphaByte;

    for (int ct = wave; ct < ctiles; ct += 4) {
        const int x = 16 * ct + x_l;
        const int xs = min(x, p.ov_w - 1);
        const uint8_t* aq = abase + (int64_t)xs * kTGroupBytes;
        i32x4 acc[3];
        acc[0] = i32x4{rb[0], rb[1], rb[2], rb[3]};
        acc[1] = i32x4{0, 0, 0, 0};
        acc[2] = i32x4{0, 0, 0, 0};
#pragma unroll 1
        for (int ks = 0; ks < th.y; ++ks) {
            // the lane's four groups are one H band: constant (0x80, not
            // stored) where the item's trim entries say so (ipp_pipe_layout.h)
            uint32_t e = kTrimNone;
            if (trim) {
                const int hb = trim_v_band(th.x, ks, lane);
                e = hb < hbands ? (uint32_t)trim[hb] : kTrimAll;
            }
            i32x4 bq = i32x4{(int32_t)0x80808080u, (int32_t)0x80808080u, (int32_t)0x80808080u, (int32_t)0x80808080u};
            if (!trim_const(e, ct)) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    bq[j] = *reinterpret_cast<const int32_t*>(aq + (kKStepGroups * ks + j) * gstride * kTGroupBytes);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const i32x4 a = __builtin_bit_cast(i32x4, tt.blk[th.z + tap_dense_block(ks, q, lane)]);
                acc[q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bq, acc[q], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // plain code reads the accumulators (planes3)
            const int32_t s = planes3(acc[0][r], acc[1][r], acc[2][r]);
            const int32_t a = min(max(s >> 22, 0), 255);  // Resample.c clip8
            const int o = y0 + 4 * (lane >> 4) + r - p.y;  // overlay row 16 t - phase + tile row
            if (x < p.ov_w && o >= oy_lo && o < oy_hi) sink(x, o, a);
        }
    }
}

__global__ void __launch_bounds__(256)
k_pipe_overlay_bbox(const uint8_t* __restrict__ tmp, const int32_t* __restrict__ coefs,
                    const ipp_pipe_desc* __restrict__ descs, FastDiv tiles_y, int alpha_min,
                    int32_t* __restrict__ bbox, const uint16_t* __restrict__ trim, int trim_stride) {
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int im = (int)fdiv(b, tiles_y);
    const int ty = (int)(b - (uint32_t)im * tiles_y.d);
    int xmin = INT32_MAX, ymin = INT32_MAX, xmax = -1, ymax = -1;
    // (trim: the H launch's trim table, trim_stride entries per item, or null)
    const uint16_t* trow = trim ? trim + (int64_t)im * trim_stride : nullptr;
    overlay_alpha_band(tmp, coefs, descs, im, ty, trow, [&](int x, int o, int a) {
        if (a >= alpha_min) {
            xmin = min(xmin, x);
            xmax = max(xmax, x);
            ymin = min(ymin, o);
            ymax = max(ymax, o);
        }
    });
    bbox_commit(bbox + 4 * (int64_t)im, xmin, ymin, xmax, ymax);
}

// ipp_alpha_bbox's tiling (ipp_gather.hip k_alpha_bbox): 64×16 pixels per
// block, 4 pixels of one row per thread.
constexpr int BT_W = 64, BT_H = 16, BT_PX = 4;

__global__ void __launch_bounds__(256)
k_alpha_bbox_min(const uint8_t* __restrict__ img, const ipp_image_desc* __restrict__ descs, int tiles_x,
                 int tiles_y, int alpha_min, int32_t* __restrict__ bbox) {
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int per_img = tiles_x * tiles_y;
    const int im = b / per_img;
    const int t = b - im * per_img;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const ipp_image_desc d = descs[im];
    const int y = ty * BT_H + (int)(threadIdx.x >> 4);
    const int x0 = tx * BT_W + (int)(threadIdx.x & 15) * BT_PX;
    int xmin = INT32_MAX, ymin = INT32_MAX, xmax = -1, ymax = -1;
    // images without an alpha band (cn other than 2 or 4) have no visible pixel
    if (y < d.h && (d.cn == 2 || d.cn == 4)) {
        const uint8_t* row = img + d.off + (int64_t)y * d.pitch;
        for (int k = 0; k < BT_PX; ++k) {
            const int x = x0 + k;
            if (x < d.w && (int)row[(int64_t)x * d.cn + d.cn - 1] >= alpha_min) {
                xmin = min(xmin, x);
                xmax = max(xmax, x);
                ymin = min(ymin, y);
                ymax = max(ymax, y);
            }
        }
    }
    bbox_commit(bbox + 4 * (int64_t)im, xmin, ymin, xmax, ymax);
}

// ---------------------------------------------------------------------------
// ipp_pipe_scene_boxes: occlusion-aware labels of scenes (K overlays pasted in
// layer order onto one composite).
//
// Scratch: the table slot → descriptor (int32[n_scenes·K], slot = scene·K +
// layer, -1 = no descriptor), then one alpha plane per descriptor, max_ov_h
// rows of scene_pitch(max_ov_w) bytes.  Three launches in stream order:
//   k_scene_init   rows (INT_MAX, INT_MAX, -1, -1, 0, 0) and the slot table;
//   k_scene_alpha  overlay_alpha_band, every alpha byte stored to its plane;
//   k_scene_visible  one block per (descriptor, 16-row strip of its overlay):
//     a pixel is present when its alpha >= alpha_min and visible when no later
//     layer of its scene whose rectangle holds the pixel has alpha >= cover_min
//     there (read from that layer's plane by composite coordinate); wave-wide
//     box and counts, six atomics from lane 0;
// then k_scene_finish turns an untouched box into (-1, -1, -1, -1).
// A descriptor larger than (max_ov_w, max_ov_h) has no plane: it is skipped
// and never read as a later layer, so every plane access stays in bounds.
// ---------------------------------------------------------------------------
__host__ __device__ constexpr int64_t scene_pitch(int max_ov_w) { return ((int64_t)max_ov_w + 15) & ~(int64_t)15; }
__host__ __device__ constexpr int64_t scene_table_bytes(int64_t slots) { return (4 * slots + 255) & ~(int64_t)255; }

__global__ void k_scene_init(int32_t* __restrict__ out, int32_t* __restrict__ table,
                             const int32_t* __restrict__ scene_layer, int n, int n_scenes, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[6 * i + 0] = INT32_MAX;
    out[6 * i + 1] = INT32_MAX;
    out[6 * i + 2] = -1;
    out[6 * i + 3] = -1;
    out[6 * i + 4] = 0;
    out[6 * i + 5] = 0;
    const int s = scene_layer[2 * i], k = scene_layer[2 * i + 1];
    if ((unsigned)s < (unsigned)n_scenes && (unsigned)k < (unsigned)K) table[(int64_t)s * K + k] = i;
}

__global__ void k_scene_finish(int32_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && out[6 * i + 2] < 0) out[6 * i + 0] = out[6 * i + 1] = -1;
}

__global__ void __launch_bounds__(256)
k_scene_alpha(const uint8_t* __restrict__ tmp, const int32_t* __restrict__ coefs,
              const ipp_pipe_desc* __restrict__ descs, FastDiv tiles_y, int max_ov_w, int max_ov_h,
              uint8_t* __restrict__ planes) {
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int im = (int)fdiv(b, tiles_y);
    const int ty = (int)(b - (uint32_t)im * tiles_y.d);
    if (descs[im].p.ov_w > max_ov_w || descs[im].p.ov_h > max_ov_h) return;  // no plane (block-uniform)
    const int64_t pitch = scene_pitch(max_ov_w);
    uint8_t* plane = planes + (int64_t)im * max_ov_h * pitch;
    // (no trim table: a scene's T is written in full)
    overlay_alpha_band(tmp, coefs, descs, im, ty, nullptr,
                       [&](int x, int o, int a) { plane[(int64_t)o * pitch + x] = (uint8_t)a; });
}

constexpr int SVR = 16;  // overlay rows per k_scene_visible block

__global__ void __launch_bounds__(256)
k_scene_visible(const ipp_pipe_desc* __restrict__ descs, const int32_t* __restrict__ scene_layer,
                const int32_t* __restrict__ table, const uint8_t* __restrict__ planes, FastDiv strips, int n,
                int n_scenes, int K, int max_ov_w, int max_ov_h, int alpha_min, int cover_min,
                int32_t* __restrict__ out) {
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int im = (int)fdiv(b, strips);
    const int v0 = (int)(b - (uint32_t)im * strips.d) * SVR;
    const ipp_paste_desc p = descs[im].p;
    if (v0 >= p.ov_h || p.ov_w > max_ov_w || p.ov_h > max_ov_h) return;  // block-uniform
    const int64_t pitch = scene_pitch(max_ov_w), psize = (int64_t)max_ov_h * pitch;
    const uint8_t* plane = planes + (int64_t)im * psize;
    const int scene = scene_layer[2 * im], layer = scene_layer[2 * im + 1];
    const bool mapped = (unsigned)scene < (unsigned)n_scenes && (unsigned)layer < (unsigned)K;
    const int v = v0 + (int)(threadIdx.x >> 4);
    int xmin = INT32_MAX, ymin = INT32_MAX, xmax = -1, ymax = -1, area = 0, vis = 0;
    // 4 pixels of one row per thread and step (one aligned dword of the plane:
    // its pitch is a multiple of 16, bytes past ov_w are masked below)
    for (int u0 = 4 * (int)(threadIdx.x & 15); u0 < p.ov_w; u0 += 64) {
        uint32_t a4 = 0u;
        if (v < p.ov_h) a4 = *reinterpret_cast<const uint32_t*>(plane + (int64_t)v * pitch + u0);
        uint32_t present = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            present |= (uint32_t)(v < p.ov_h && u0 + k < p.ov_w && (int)((a4 >> (8 * k)) & 255u) >= alpha_min) << k;
        uint32_t hidden = 0u;
        // later layers of the scene (the loop is block-uniform)
        for (int j = mapped ? layer + 1 : K; j < K; ++j) {
            const int dj = table[(int64_t)scene * K + j];
            if ((unsigned)dj >= (unsigned)n) continue;
            const ipp_paste_desc q = descs[dj].p;
            if (q.ov_w > max_ov_w || q.ov_h > max_ov_h) continue;  // no plane
            const int cy = p.y + v - q.y;                          // the row in layer j's overlay
            if ((unsigned)cy >= (unsigned)q.ov_h) continue;
            const uint8_t* qrow = planes + (int64_t)dj * psize + (int64_t)cy * pitch;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int cx = p.x + u0 + k - q.x;
                if (((present >> k) & 1u) && (unsigned)cx < (unsigned)q.ov_w && (int)qrow[cx] >= cover_min)
                    hidden |= 1u << k;
            }
        }
        const uint32_t visible = present & ~hidden;
        area += __builtin_popcount(present);
        vis += __builtin_popcount(visible);
        if (visible) {
            xmin = min(xmin, p.x + u0 + (int)__builtin_ctz(visible));
            xmax = max(xmax, p.x + u0 + 31 - (int)__builtin_clz(visible));
            ymin = min(ymin, p.y + v);
            ymax = max(ymax, p.y + v);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        area += __shfl_xor(area, off);
        vis += __shfl_xor(vis, off);
    }
    int32_t* row = out + 6 * (int64_t)im;
    bbox_commit(row, xmin, ymin, xmax, ymax);
    if ((threadIdx.x & 63) == 0) {
        if (area) atomicAdd(&row[4], area);
        if (vis) atomicAdd(&row[5], vis);
    }
}

// ---------------------------------------------------------------------------
// ipp_pipe_scene_map: the visibility rule's per-pixel answer (instance masks).
// Byte (Y, X) of scene s's map holds bit k iff layer k is mapped, has a plane,
// its rectangle clipped to the background holds (X, Y), A_k >= alpha_min there
// and no later layer with a plane has A_j >= cover_min there.
//
// Composite-centric: a block is MT_H rows × MT_W columns of one scene's map,
// a thread MT_PX consecutive pixels of one row, stored as one aligned 16-B
// vector (the map and its pitch are 16-B aligned, so a vector never crosses
// the pitch).  Every byte of every slot has exactly one writer, so there are
// no atomics and the caller clears nothing.  The scene's slot entries and
// rectangles are block-uniform (scalar loads); the layers are walked from the
// top down with a per-pixel `covered` bit, and a layer whose clipped rectangle
// misses the wave's rows or the block's columns is not touched: a block no
// layer meets stores zeros and reads no plane.  Plane bytes are read by
// composite coordinate with byte loads (cx = X - x_k is unaligned), each
// guarded by the clipped rectangle: 0 <= cy < ov_h <= max_ov_h and 0 <= cx <
// ov_w <= max_ov_w, so every access lies in the plane of a descriptor in
// [0, n), and the rows it reads are the ones k_scene_alpha wrote (the
// overlay's rows inside the background).
// ---------------------------------------------------------------------------
constexpr int MT_W = 256, MT_H = 16, MT_PX = 16;
constexpr int kSceneMapMaxLayers = IPP_SCENE_MAP_MAX_LAYERS;
static_assert(kSceneMapMaxLayers == 8, "one bit per layer in a map byte");
static_assert(MT_PX == 16 && MT_W == 16 * MT_PX && MT_H * (MT_W / MT_PX) == 256, "k_scene_map's thread map");

// The slot table alone, for a map without boxes (k_scene_init fills it beside the rows).
__global__ void k_scene_table(int32_t* __restrict__ table, const int32_t* __restrict__ scene_layer, int n,
                              int n_scenes, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = scene_layer[2 * i], k = scene_layer[2 * i + 1];
    if ((unsigned)s < (unsigned)n_scenes && (unsigned)k < (unsigned)K) table[(int64_t)s * K + k] = i;
}

__global__ void __launch_bounds__(256)
k_scene_map(const ipp_pipe_desc* __restrict__ descs, const int32_t* __restrict__ table,
            const uint8_t* __restrict__ planes, FastDiv tiles, FastDiv tiles_x, int n, int K, int bg_w, int bg_h,
            int max_ov_w, int max_ov_h, int alpha_min, int cover_min, uint8_t* __restrict__ map,
            int64_t map_pitch) {
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int scene = (int)fdiv(b, tiles);
    const uint32_t t = b - (uint32_t)scene * tiles.d;
    const int ty = (int)fdiv(t, tiles_x), tx = (int)(t - (uint32_t)ty * tiles_x.d);
    const int bx0 = tx * MT_W;                                                  // the block's columns
    const int wy0 = ty * MT_H + 4 * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // the wave's 4 rows
    const int Y = ty * MT_H + (int)(threadIdx.x >> 4);
    const int X0 = bx0 + MT_PX * (int)(threadIdx.x & 15);
    const int64_t pitch = scene_pitch(max_ov_w), psize = (int64_t)max_ov_h * pitch;

    // Phase 1 (block-uniform): each layer's descriptor and paste position; d[k]
    // stays -1 unless the layer's clipped rectangle meets the wave's pixels.
    int d[kSceneMapMaxLayers], px[kSceneMapMaxLayers], py[kSceneMapMaxLayers], pw[kSceneMapMaxLayers],
        ph[kSceneMapMaxLayers];
#pragma unroll
    for (int k = 0; k < kSceneMapMaxLayers; ++k) {
        d[k] = -1;
        px[k] = py[k] = pw[k] = ph[k] = 0;
        if (k >= K) continue;
        const int dk = table[(int64_t)scene * K + k];
        if ((unsigned)dk >= (unsigned)n) continue;  // no descriptor in this slot
        const ipp_paste_desc p = descs[dk].p;
        if (p.ov_w <= 0 || p.ov_h <= 0 || p.ov_w > max_ov_w || p.ov_h > max_ov_h) continue;  // no plane
        // the rectangle clipped to the background (64-bit: x + ov_w of a foreign descriptor must not wrap)
        const int64_t rx0 = max((int64_t)p.x, (int64_t)0), rx1 = min((int64_t)p.x + p.ov_w, (int64_t)bg_w);
        const int64_t ry0 = max((int64_t)p.y, (int64_t)0), ry1 = min((int64_t)p.y + p.ov_h, (int64_t)bg_h);
        if (rx0 >= (int64_t)bx0 + MT_W || rx1 <= bx0 || ry0 >= (int64_t)wy0 + 4 || ry1 <= wy0) continue;
        d[k] = dk;
        px[k] = p.x, py[k] = p.y, pw[k] = p.ov_w, ph[k] = p.ov_h;
    }

    if (Y >= bg_h || X0 >= map_pitch) return;  // (no barrier below)
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    uint32_t covered = 0u;  // bit i: a later layer covers pixel X0 + i
    // Phase 2: top down.
#pragma unroll
    for (int k = kSceneMapMaxLayers - 1; k >= 0; --k) {
        if (d[k] < 0) continue;  // wave-uniform
        const int cy = Y - py[k];
        if ((unsigned)cy >= (unsigned)ph[k]) continue;
        const uint8_t* row = planes + (int64_t)d[k] * psize + (int64_t)cy * pitch;
        const int cx0 = X0 - px[k];  // (X0 < map_pitch and |x| of a met rectangle are far below 2^31)
        const int xlim = min(pw[k], bg_w - px[k]);  // columns of the overlay inside the background
#pragma unroll
        for (int i = 0; i < MT_PX; ++i) {
            const int cx = cx0 + i;
            if (cx >= 0 && cx < xlim) {
                const int a = row[cx];
                if (!((covered >> i) & 1u) && a >= alpha_min) w[i >> 2] |= (1u << k) << (8 * (i & 3));
                if (a >= cover_min) covered |= 1u << i;
            }
        }
    }
    store16<0>(map + ((int64_t)scene * bg_h + Y) * map_pitch + X0, 16, true, w);
}

// The launches of ipp_pipe_scene_boxes and ipp_pipe_scene_map after their
// argument checks: the slot table, the alpha planes, then the boxes (`rows`)
// and / or the map, whichever is given.
int scene_launches(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs, const int32_t* scene_layer,
                   int n_images, int n_scenes, int per_scene, int bg_w, int bg_h, int max_ov_w, int max_ov_h,
                   int alpha_min, int cover_min, uint8_t* scratch, int32_t* rows, uint8_t* map, int64_t map_pitch,
                   hipStream_t s) {
    const int tyb = paste_max_bands(max_ov_h), strips = (max_ov_h + SVR - 1) / SVR;
    const int64_t slots = (int64_t)n_scenes * per_scene;
    if ((int64_t)tyb * n_images >= INT32_MAX || (int64_t)strips * n_images >= INT32_MAX || slots >= INT32_MAX)
        return IPP_E_ARG;
    int mtx = 0, mty = 0;
    if (map) {
        mtx = (int)((map_pitch + MT_W - 1) / MT_W), mty = (bg_h + MT_H - 1) / MT_H;
        if ((int64_t)mtx * mty * n_scenes >= INT32_MAX) return IPP_E_ARG;
    }
    int32_t* table = reinterpret_cast<int32_t*>(scratch);
    uint8_t* planes = scratch + scene_table_bytes(slots);
    if (slots > 0 && hipMemsetAsync(table, 0xFF, 4 * (size_t)slots, s) != hipSuccess) return IPP_E_LAUNCH;
    if (n_images > 0) {
        const int ib = (n_images + 255) / 256;
        if (rows)
            hipLaunchKernelGGL(k_scene_init, dim3(ib), dim3(256), 0, s, rows, table, scene_layer, n_images, n_scenes,
                               per_scene);
        else
            hipLaunchKernelGGL(k_scene_table, dim3(ib), dim3(256), 0, s, table, scene_layer, n_images, n_scenes,
                               per_scene);
        hipLaunchKernelGGL(k_scene_alpha, dim3((uint32_t)(tyb * n_images)), dim3(256), 0, s, tmp, coefs, descs,
                           fast_div((uint32_t)tyb), max_ov_w, max_ov_h, planes);
        if (rows) {
            hipLaunchKernelGGL(k_scene_visible, dim3((uint32_t)(strips * n_images)), dim3(256), 0, s, descs,
                               scene_layer, table, planes, fast_div((uint32_t)strips), n_images, n_scenes, per_scene,
                               max_ov_w, max_ov_h, alpha_min, cover_min, rows);
            hipLaunchKernelGGL(k_scene_finish, dim3(ib), dim3(256), 0, s, rows, n_images);
        }
    }
    if (map && n_scenes > 0)
        hipLaunchKernelGGL(k_scene_map, dim3((uint32_t)(mtx * mty * n_scenes)), dim3(256), 0, s, descs, table, planes,
                           fast_div((uint32_t)(mtx * mty)), fast_div((uint32_t)mtx), n_images, per_scene, bg_w, bg_h,
                           max_ov_w, max_ov_h, alpha_min, cover_min, map, map_pitch);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

// ---------------------------------------------------------------------------
// ipp_pipe_scene_cull: cull the overlays the later layers leave too little of,
// between the H launches and the first V launch (include/ipp.h states the rule).
//
// Same scratch, slot table and alpha planes as the boxes (k_scene_table,
// k_scene_alpha).  `cull` (int32[n][4] = keep, area, visible, 0) is zeroed and
// serves as the counters.  Then one k_cull_count launch per layer, K-1 down to
// 0: k_scene_visible's walk without the box, for the descriptors of that layer
// alone (the unmapped ones ride with the first launch: alone in their scene,
// they wait for nobody), whose later-layer loop skips the layers that are
// culled.  Whether layer j > k is culled is cull_keep of its two counters,
// which the earlier launches of the stream have finished; the counters are
// sums of integer atomicAdds, so no result depends on the atomics' order.
// k_cull_clear evaluates the same predicate for every descriptor, writes the
// verdict, and stores 0x80 over the T of the culled ones.
//
// T of a descriptor, as the H launch writes it (ipp_pipe.hip: one block per 16
// T rows, a lane per group): group rows [0, 4·⌈h.lines/16⌉) of h.out_len
// 16-B groups each, at tmp + h.dst_off + g·h.dst_pitch + 16·x.  t_groups()
// sizes the item's T for at least these rows (its first term), so the clear
// stays inside the descriptor's own T.  The rows a V tile's window reads past
// them are the ones no H launch writes either: every tap there is 0.
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ bool cull_keep(int area, int vis, int min_q, int min_pixels) {
    return vis >= (min_pixels > 1 ? min_pixels : 1) && (int64_t)65536 * vis >= (int64_t)min_q * area;
}

__global__ void __launch_bounds__(256)
k_cull_count(const ipp_pipe_desc* __restrict__ descs, const int32_t* __restrict__ scene_layer,
             const int32_t* __restrict__ table, const uint8_t* __restrict__ planes, FastDiv strips, int n,
             int n_scenes, int K, int cur, int max_ov_w, int max_ov_h, int alpha_min, int cover_min, int min_q,
             int min_pixels, int32_t* cull) {
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int im = (int)fdiv(b, strips);
    const int v0 = (int)(b - (uint32_t)im * strips.d) * SVR;
    const int scene = scene_layer[2 * im], layer = scene_layer[2 * im + 1];
    const bool mapped = (unsigned)scene < (unsigned)n_scenes && (unsigned)layer < (unsigned)K;
    if ((mapped ? layer : K - 1) != cur) return;  // another launch's descriptor (block-uniform)
    const ipp_paste_desc p = descs[im].p;
    if (v0 >= p.ov_h || p.ov_w > max_ov_w || p.ov_h > max_ov_h) return;  // block-uniform
    const int64_t pitch = scene_pitch(max_ov_w), psize = (int64_t)max_ov_h * pitch;
    const uint8_t* plane = planes + (int64_t)im * psize;
    const int v = v0 + (int)(threadIdx.x >> 4);
    int area = 0, vis = 0;
    // 4 pixels of one row per thread and step, as in k_scene_visible
    for (int u0 = 4 * (int)(threadIdx.x & 15); u0 < p.ov_w; u0 += 64) {
        uint32_t a4 = 0u;
        if (v < p.ov_h) a4 = *reinterpret_cast<const uint32_t*>(plane + (int64_t)v * pitch + u0);
        uint32_t present = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            present |= (uint32_t)(v < p.ov_h && u0 + k < p.ov_w && (int)((a4 >> (8 * k)) & 255u) >= alpha_min) << k;
        uint32_t hidden = 0u;
        // the kept later layers of the scene (the loop is block-uniform)
        for (int j = mapped ? layer + 1 : K; j < K; ++j) {
            const int dj = table[(int64_t)scene * K + j];
            if ((unsigned)dj >= (unsigned)n) continue;
            const ipp_paste_desc q = descs[dj].p;
            if (q.ov_w > max_ov_w || q.ov_h > max_ov_h) continue;  // no plane
            // layer j's counters are final: its launch came earlier in the stream
            if (!cull_keep(cull[4 * (int64_t)dj + 1], cull[4 * (int64_t)dj + 2], min_q, min_pixels)) continue;
            const int cy = p.y + v - q.y;  // the row in layer j's overlay
            if ((unsigned)cy >= (unsigned)q.ov_h) continue;
            const uint8_t* qrow = planes + (int64_t)dj * psize + (int64_t)cy * pitch;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int cx = p.x + u0 + k - q.x;
                if (((present >> k) & 1u) && (unsigned)cx < (unsigned)q.ov_w && (int)qrow[cx] >= cover_min)
                    hidden |= 1u << k;
            }
        }
        area += __builtin_popcount(present);
        vis += __builtin_popcount(present & ~hidden);
    }
    for (int off = 32; off > 0; off >>= 1) {
        area += __shfl_xor(area, off);
        vis += __shfl_xor(vis, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (area) atomicAdd(&cull[4 * (int64_t)im + 1], area);
        if (vis) atomicAdd(&cull[4 * (int64_t)im + 2], vis);
    }
}

constexpr int kCullClearBlocks = 16;  // blocks per descriptor of k_cull_clear, striding over its T groups

__global__ void __launch_bounds__(256)
k_cull_clear(uint8_t* __restrict__ tmp, const ipp_pipe_desc* __restrict__ descs, int max_ov_w, int max_ov_h,
             int min_q, int min_pixels, int32_t* __restrict__ cull) {
    const int im = (int)(blockIdx.x / kCullClearBlocks), part = (int)(blockIdx.x % kCullClearBlocks);
    const ipp_paste_desc p = descs[im].p;
    int32_t* row = cull + 4 * (int64_t)im;
    // a descriptor without a plane was never counted: it is kept as it is
    const bool keep = p.ov_w > max_ov_w || p.ov_h > max_ov_h || cull_keep(row[1], row[2], min_q, min_pixels);
    if (part == 0 && threadIdx.x == 0) {
        row[0] = keep ? 1 : 0;
        row[3] = 0;
    }
    if (keep) return;  // block-uniform
    const ipp_resample_desc h = descs[im].h;
    const int G = ((h.lines + 15) >> 4) << kTGroupRowsLog2;  // the H launch's group rows, h.out_len groups each
    const uint32_t w[4] = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
    // a wave per group row, its lanes over the row's groups
    for (int g = 4 * part + (int)(threadIdx.x >> 6); g < G; g += 4 * kCullClearBlocks) {
        uint8_t* trow = tmp + h.dst_off + (int64_t)g * h.dst_pitch;
        for (int x = (int)(threadIdx.x & 63); x < h.out_len; x += 64)
            store16<0>(trow + (int64_t)kTGroupBytes * x, kTGroupBytes, true, w);
    }
}

int cull_launches(uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs, const int32_t* scene_layer,
                  int n_images, int n_scenes, int per_scene, int max_ov_w, int max_ov_h, int alpha_min, int cover_min,
                  int min_q, int min_pixels, uint8_t* scratch, int32_t* cull, hipStream_t s) {
    const int tyb = paste_max_bands(max_ov_h), strips = (max_ov_h + SVR - 1) / SVR;
    const int64_t slots = (int64_t)n_scenes * per_scene;
    if ((int64_t)tyb * n_images >= INT32_MAX || (int64_t)strips * n_images >= INT32_MAX || slots >= INT32_MAX ||
        (int64_t)kCullClearBlocks * n_images >= INT32_MAX)
        return IPP_E_ARG;
    int32_t* table = reinterpret_cast<int32_t*>(scratch);
    uint8_t* planes = scratch + scene_table_bytes(slots);
    if (slots > 0 && hipMemsetAsync(table, 0xFF, 4 * (size_t)slots, s) != hipSuccess) return IPP_E_LAUNCH;
    if (hipMemsetAsync(cull, 0, 16 * (size_t)n_images, s) != hipSuccess) return IPP_E_LAUNCH;
    hipLaunchKernelGGL(k_scene_table, dim3((n_images + 255) / 256), dim3(256), 0, s, table, scene_layer, n_images,
                       n_scenes, per_scene);
    hipLaunchKernelGGL(k_scene_alpha, dim3((uint32_t)(tyb * n_images)), dim3(256), 0, s, tmp, coefs, descs,
                       fast_div((uint32_t)tyb), max_ov_w, max_ov_h, planes);
    for (int k = per_scene - 1; k >= 0; --k)
        hipLaunchKernelGGL(k_cull_count, dim3((uint32_t)(strips * n_images)), dim3(256), 0, s, descs, scene_layer, table,
                           planes, fast_div((uint32_t)strips), n_images, n_scenes, per_scene, k, max_ov_w, max_ov_h,
                           alpha_min, cover_min, min_q, min_pixels, cull);
    hipLaunchKernelGGL(k_cull_clear, dim3((uint32_t)(kCullClearBlocks * n_images)), dim3(256), 0, s, tmp, descs,
                       max_ov_w, max_ov_h, min_q, min_pixels, cull);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

// ---------------------------------------------------------------------------
// ipp_pipe_scene_amodal: the full extent of every overlay behind its occluders
// (include/ipp.h states the rule): the presence map, the amodal rows and the
// pairwise occlusion counts, with the visible rows and map of
// ipp_pipe_scene_map from the same alpha planes.
//
// Same scratch, slot table and alpha planes as the boxes.  In stream order:
//   memsets         the slot table (0xFF) and occ (0);
//   k_amodal_init   arows and rows (INT_MAX, INT_MAX, -1, -1, 0, 0), the table;
//   k_scene_alpha   once, whatever is asked for;
//   k_amodal_count  k_scene_visible's blocks and pixel groups (one block per
//     descriptor and 16-row strip, 4 pixels of a row per thread and step), the
//     later layers walked from the top down with the per-pixel `hidden` mask:
//     of layer j, COVERS += popcount(present & cover_j) and HIDES +=
//     popcount(present & cover_j & ~hidden) before hidden |= cover_j.  Each
//     count is summed over the wave and added by lane 0 (integer atomicAdd:
//     no result depends on the atomics' order); the present box and, when
//     `rows` is given, the visible box go through bbox_commit;
//   k_amodal_finish untouched boxes become (-1, -1, -1, -1);
//   k_amodal_map    k_scene_map's sweep storing the presence and / or the
//     visibility map: one 16-B vector per thread and map, one writer per byte.
// Phase 1 of k_amodal_count is block-uniform: a later layer is kept only when
// it is in [0, n), has a plane and its rectangle meets the strip's rows and the
// overlay's columns (64-bit, a foreign descriptor must not wrap), so inside
// the loop 0 <= cy < ov_h <= max_ov_h and 0 <= cx < ov_w <= max_ov_w are the
// only loads: every access lies in the plane of a descriptor in [0, n).
// ---------------------------------------------------------------------------
__global__ void k_amodal_init(int32_t* __restrict__ arows, int32_t* __restrict__ rows, int32_t* __restrict__ table,
                              const int32_t* __restrict__ scene_layer, int n, int n_scenes, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int w = 0; w < 6; ++w) {
        const int32_t v = w < 2 ? INT32_MAX : w < 4 ? -1 : 0;
        arows[6 * i + w] = v;
        if (rows) rows[6 * i + w] = v;
    }
    const int s = scene_layer[2 * i], k = scene_layer[2 * i + 1];
    if ((unsigned)s < (unsigned)n_scenes && (unsigned)k < (unsigned)K) table[(int64_t)s * K + k] = i;
}

__global__ void k_amodal_finish(int32_t* __restrict__ arows, int32_t* __restrict__ rows, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (arows[6 * i + 2] < 0) arows[6 * i + 0] = arows[6 * i + 1] = -1;
    if (rows && rows[6 * i + 2] < 0) rows[6 * i + 0] = rows[6 * i + 1] = -1;
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void __launch_bounds__(256)
k_amodal_count(const ipp_pipe_desc* __restrict__ descs, const int32_t* __restrict__ scene_layer,
               const int32_t* __restrict__ table, const uint8_t* __restrict__ planes, FastDiv strips, int n,
               int n_scenes, int K, int max_ov_w, int max_ov_h, int alpha_min, int cover_min,
               int32_t* __restrict__ arows, int32_t* __restrict__ occ, int32_t* __restrict__ rows) {
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int im = (int)fdiv(b, strips);
    const int v0 = (int)(b - (uint32_t)im * strips.d) * SVR;
    const ipp_paste_desc p = descs[im].p;
    if (v0 >= p.ov_h || p.ov_w > max_ov_w || p.ov_h > max_ov_h) return;  // block-uniform
    const int64_t pitch = scene_pitch(max_ov_w), psize = (int64_t)max_ov_h * pitch;
    const uint8_t* plane = planes + (int64_t)im * psize;
    const int scene = scene_layer[2 * im], layer = scene_layer[2 * im + 1];
    const bool mapped = (unsigned)scene < (unsigned)n_scenes && (unsigned)layer < (unsigned)K;

    // Phase 1 (block-uniform): the later layers that can cover a pixel of this strip.
    int d[kSceneMapMaxLayers], qx[kSceneMapMaxLayers], qy[kSceneMapMaxLayers], qw[kSceneMapMaxLayers],
        qh[kSceneMapMaxLayers];
#pragma unroll
    for (int j = 0; j < kSceneMapMaxLayers; ++j) {
        d[j] = -1;
        qx[j] = qy[j] = qw[j] = qh[j] = 0;
        if (!mapped || j <= layer || j >= K) continue;
        const int dj = table[(int64_t)scene * K + j];
        if ((unsigned)dj >= (unsigned)n) continue;  // no descriptor in this slot
        const ipp_paste_desc q = descs[dj].p;
        if (q.ov_w <= 0 || q.ov_h <= 0 || q.ov_w > max_ov_w || q.ov_h > max_ov_h) continue;  // no plane
        const int64_t cy0 = (int64_t)p.y + v0 - q.y, cx0 = (int64_t)p.x - q.x;  // of the strip's first pixel
        if (cy0 + SVR <= 0 || cy0 >= q.ov_h || cx0 + p.ov_w <= 0 || cx0 >= q.ov_w) continue;
        d[j] = dj;
        qx[j] = q.x, qy[j] = q.y, qw[j] = q.ov_w, qh[j] = q.ov_h;
    }

    const int v = v0 + (int)(threadIdx.x >> 4);
    int axmin = INT32_MAX, aymin = INT32_MAX, axmax = -1, aymax = -1;  // the present box
    int xmin = INT32_MAX, ymin = INT32_MAX, xmax = -1, ymax = -1;      // the visible box
    int area = 0, vis = 0;
    int cov[kSceneMapMaxLayers], hid[kSceneMapMaxLayers];
#pragma unroll
    for (int j = 0; j < kSceneMapMaxLayers; ++j) cov[j] = hid[j] = 0;
    // 4 pixels of one row per thread and step, as in k_scene_visible
    for (int u0 = 4 * (int)(threadIdx.x & 15); u0 < p.ov_w; u0 += 64) {
        uint32_t a4 = 0u;
        if (v < p.ov_h) a4 = *reinterpret_cast<const uint32_t*>(plane + (int64_t)v * pitch + u0);
        uint32_t present = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            present |= (uint32_t)(v < p.ov_h && u0 + k < p.ov_w && (int)((a4 >> (8 * k)) & 255u) >= alpha_min) << k;
        uint32_t hidden = 0u;
        // Phase 2: the later layers, top down (layer 0 is nobody's later layer)
#pragma unroll
        for (int j = kSceneMapMaxLayers - 1; j > 0; --j) {
            if (d[j] < 0) continue;  // block-uniform
            const int cy = p.y + v - qy[j];  // the row in layer j's overlay
            uint32_t c = 0u;
            if ((unsigned)cy < (unsigned)qh[j]) {
                const uint8_t* qrow = planes + (int64_t)d[j] * psize + (int64_t)cy * pitch;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int cx = p.x + u0 + k - qx[j];
                    if (((present >> k) & 1u) && (unsigned)cx < (unsigned)qw[j] && (int)qrow[cx] >= cover_min)
                        c |= 1u << k;
                }
            }
            cov[j] += __builtin_popcount(c);
            hid[j] += __builtin_popcount(c & ~hidden);
            hidden |= c;
        }
        const uint32_t visible = present & ~hidden;
        area += __builtin_popcount(present);
        vis += __builtin_popcount(visible);
        if (present) {
            axmin = min(axmin, p.x + u0 + (int)__builtin_ctz(present));
            axmax = max(axmax, p.x + u0 + 31 - (int)__builtin_clz(present));
            aymin = min(aymin, p.y + v);
            aymax = max(aymax, p.y + v);
        }
        if (visible) {
            xmin = min(xmin, p.x + u0 + (int)__builtin_ctz(visible));
            xmax = max(xmax, p.x + u0 + 31 - (int)__builtin_clz(visible));
            ymin = min(ymin, p.y + v);
            ymax = max(ymax, p.y + v);
        }
    }
    area = wave_sum(area);
    vis = wave_sum(vis);
    const bool lane0 = (threadIdx.x & 63) == 0;
    int32_t* arow = arows + 6 * (int64_t)im;
    bbox_commit(arow, axmin, aymin, axmax, aymax);
    if (lane0) {
        if (area) atomicAdd(&arow[4], area);
        if (vis) atomicAdd(&arow[5], vis);
    }
    if (rows) {  // (uniform) what k_scene_visible writes
        int32_t* row = rows + 6 * (int64_t)im;
        bbox_commit(row, xmin, ymin, xmax, ymax);
        if (lane0) {
            if (area) atomicAdd(&row[4], area);
            if (vis) atomicAdd(&row[5], vis);
        }
    }
    if (!mapped) return;  // block-uniform: alone in its scene, in no slot of occ
    int32_t* oc0 = occ + (((int64_t)scene * 2) * K + layer) * K;  // occ[scene][0][layer][.]
    int32_t* oc1 = oc0 + (int64_t)K * K;                          // occ[scene][1][layer][.]
    if (lane0) {
        if (area) atomicAdd(&oc0[layer], area);
        if (vis) atomicAdd(&oc1[layer], vis);
    }
#pragma unroll
    for (int j = 1; j < kSceneMapMaxLayers; ++j) {
        if (d[j] < 0) continue;  // block-uniform
        const int c = wave_sum(cov[j]), h = wave_sum(hid[j]);
        if (lane0) {
            if (c) atomicAdd(&oc0[j], c);
            if (h) atomicAdd(&oc1[j], h);
        }
    }
}

// k_scene_map with two outputs: `amap` takes bit k wherever layer k is present,
// `vmap` where it is also under no covering later layer (k_scene_map's byte).
// Either may be null (uniform).  The thread map, the guards of every plane
// access and the single writer per byte are k_scene_map's.
__global__ void __launch_bounds__(256)
k_amodal_map(const ipp_pipe_desc* __restrict__ descs, const int32_t* __restrict__ table,
             const uint8_t* __restrict__ planes, FastDiv tiles, FastDiv tiles_x, int n, int K, int bg_w, int bg_h,
             int max_ov_w, int max_ov_h, int alpha_min, int cover_min, uint8_t* __restrict__ amap,
             uint8_t* __restrict__ vmap, int64_t map_pitch) {
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int scene = (int)fdiv(b, tiles);
    const uint32_t t = b - (uint32_t)scene * tiles.d;
    const int ty = (int)fdiv(t, tiles_x), tx = (int)(t - (uint32_t)ty * tiles_x.d);
    const int bx0 = tx * MT_W;                                                  // the block's columns
    const int wy0 = ty * MT_H + 4 * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // the wave's 4 rows
    const int Y = ty * MT_H + (int)(threadIdx.x >> 4);
    const int X0 = bx0 + MT_PX * (int)(threadIdx.x & 15);
    const int64_t pitch = scene_pitch(max_ov_w), psize = (int64_t)max_ov_h * pitch;

    // Phase 1 (block-uniform), as in k_scene_map.
    int d[kSceneMapMaxLayers], px[kSceneMapMaxLayers], py[kSceneMapMaxLayers], pw[kSceneMapMaxLayers],
        ph[kSceneMapMaxLayers];
#pragma unroll
    for (int k = 0; k < kSceneMapMaxLayers; ++k) {
        d[k] = -1;
        px[k] = py[k] = pw[k] = ph[k] = 0;
        if (k >= K) continue;
        const int dk = table[(int64_t)scene * K + k];
        if ((unsigned)dk >= (unsigned)n) continue;  // no descriptor in this slot
        const ipp_paste_desc p = descs[dk].p;
        if (p.ov_w <= 0 || p.ov_h <= 0 || p.ov_w > max_ov_w || p.ov_h > max_ov_h) continue;  // no plane
        const int64_t rx0 = max((int64_t)p.x, (int64_t)0), rx1 = min((int64_t)p.x + p.ov_w, (int64_t)bg_w);
        const int64_t ry0 = max((int64_t)p.y, (int64_t)0), ry1 = min((int64_t)p.y + p.ov_h, (int64_t)bg_h);
        if (rx0 >= (int64_t)bx0 + MT_W || rx1 <= bx0 || ry0 >= (int64_t)wy0 + 4 || ry1 <= wy0) continue;
        d[k] = dk;
        px[k] = p.x, py[k] = p.y, pw[k] = p.ov_w, ph[k] = p.ov_h;
    }

    if (Y >= bg_h || X0 >= map_pitch) return;  // (no barrier below)
    uint32_t wa[4] = {0u, 0u, 0u, 0u}, wv[4] = {0u, 0u, 0u, 0u};
    uint32_t covered = 0u;  // bit i: a later layer covers pixel X0 + i
    // Phase 2: top down.
#pragma unroll
    for (int k = kSceneMapMaxLayers - 1; k >= 0; --k) {
        if (d[k] < 0) continue;  // wave-uniform
        const int cy = Y - py[k];
        if ((unsigned)cy >= (unsigned)ph[k]) continue;
        const uint8_t* row = planes + (int64_t)d[k] * psize + (int64_t)cy * pitch;
        const int cx0 = X0 - px[k];
        const int xlim = min(pw[k], bg_w - px[k]);  // columns of the overlay inside the background
#pragma unroll
        for (int i = 0; i < MT_PX; ++i) {
            const int cx = cx0 + i;
            if (cx >= 0 && cx < xlim) {
                const int a = row[cx];
                const uint32_t bit = (a >= alpha_min ? 1u << k : 0u) << (8 * (i & 3));
                wa[i >> 2] |= bit;
                if (!((covered >> i) & 1u)) wv[i >> 2] |= bit;
                if (a >= cover_min) covered |= 1u << i;
            }
        }
    }
    const int64_t at = ((int64_t)scene * bg_h + Y) * map_pitch + X0;
    if (amap) store16<0>(amap + at, 16, true, wa);
    if (vmap) store16<0>(vmap + at, 16, true, wv);
}

int amodal_launches(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs, const int32_t* scene_layer,
                    int n_images, int n_scenes, int per_scene, int bg_w, int bg_h, int max_ov_w, int max_ov_h,
                    int alpha_min, int cover_min, uint8_t* scratch, int32_t* arows, int32_t* occ, uint8_t* amap,
                    int32_t* rows, uint8_t* vmap, int64_t map_pitch, hipStream_t s) {
    const int tyb = paste_max_bands(max_ov_h), strips = (max_ov_h + SVR - 1) / SVR;
    const int64_t slots = (int64_t)n_scenes * per_scene;
    const int mtx = (int)((map_pitch + MT_W - 1) / MT_W), mty = (bg_h + MT_H - 1) / MT_H;
    if ((int64_t)tyb * n_images >= INT32_MAX || (int64_t)strips * n_images >= INT32_MAX || slots >= INT32_MAX ||
        (int64_t)mtx * mty * n_scenes >= INT32_MAX)
        return IPP_E_ARG;
    int32_t* table = reinterpret_cast<int32_t*>(scratch);
    uint8_t* planes = scratch + scene_table_bytes(slots);
    if (slots > 0 && hipMemsetAsync(table, 0xFF, 4 * (size_t)slots, s) != hipSuccess) return IPP_E_LAUNCH;
    if (slots > 0 && hipMemsetAsync(occ, 0, 8 * (size_t)slots * per_scene, s) != hipSuccess) return IPP_E_LAUNCH;
    if (n_images > 0) {
        const int ib = (n_images + 255) / 256;
        hipLaunchKernelGGL(k_amodal_init, dim3(ib), dim3(256), 0, s, arows, rows, table, scene_layer, n_images,
                           n_scenes, per_scene);
        hipLaunchKernelGGL(k_scene_alpha, dim3((uint32_t)(tyb * n_images)), dim3(256), 0, s, tmp, coefs, descs,
                           fast_div((uint32_t)tyb), max_ov_w, max_ov_h, planes);
        hipLaunchKernelGGL(k_amodal_count, dim3((uint32_t)(strips * n_images)), dim3(256), 0, s, descs, scene_layer,
                           table, planes, fast_div((uint32_t)strips), n_images, n_scenes, per_scene, max_ov_w,
                           max_ov_h, alpha_min, cover_min, arows, occ, rows);
        hipLaunchKernelGGL(k_amodal_finish, dim3(ib), dim3(256), 0, s, arows, rows, n_images);
    }
    if ((amap || vmap) && n_scenes > 0)
        hipLaunchKernelGGL(k_amodal_map, dim3((uint32_t)(mtx * mty * n_scenes)), dim3(256), 0, s, descs, table,
                           planes, fast_div((uint32_t)(mtx * mty)), fast_div((uint32_t)mtx), n_images, per_scene, bg_w,
                           bg_h, max_ov_w, max_ov_h, alpha_min, cover_min, amap, vmap, map_pitch);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

}  // namespace

extern "C" int ipp_pipe_scene_amodal(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                                     const int32_t* scene_layer, int32_t n_images, int32_t n_scenes,
                                     int32_t per_scene, int32_t bg_w, int32_t bg_h, int32_t max_ov_w,
                                     int32_t max_ov_h, int32_t alpha_min, int32_t cover_min, int32_t tap_format,
                                     uint8_t* scratch, int32_t* arows, int32_t* occ, uint8_t* amap, int32_t* rows,
                                     uint8_t* vmap, int64_t map_pitch, void* stream) {
    if (alpha_min < 1 || alpha_min > 255 || cover_min < 1 || cover_min > 255 || tap_format != IPP_TAPS_MFMA)
        return IPP_E_ARG;
    if (!tmp || !coefs || !descs || !scene_layer || !scratch || !arows || !occ || n_images < 0 || n_scenes < 0 ||
        per_scene < 1 || per_scene > IPP_SCENE_MAP_MAX_LAYERS || max_ov_w <= 0 || max_ov_h <= 0)
        return IPP_E_ARG;
    if (bg_w <= 0 || bg_h <= 0 || map_pitch < bg_w || (map_pitch & 15) != 0 || map_pitch > INT32_MAX)
        return IPP_E_ARG;
    // the planes are read by dwords, the maps are stored by 16-B vectors
    if (((reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(amap) |
          reinterpret_cast<uintptr_t>(vmap)) & 15u) != 0)
        return IPP_E_ARG;
    return amodal_launches(tmp, coefs, descs, scene_layer, n_images, n_scenes, per_scene, bg_w, bg_h, max_ov_w,
                           max_ov_h, alpha_min, cover_min, scratch, arows, occ, amap, rows, vmap, map_pitch,
                           (hipStream_t)stream);
}

extern "C" int ipp_pipe_overlay_bbox_trim(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                                          int32_t n_images, int32_t max_ov_w, int32_t max_ov_h, int32_t alpha_min,
                                          int32_t tap_format, int32_t* bbox, const uint16_t* trim, int32_t max_rows,
                                          void* stream) {
    if (alpha_min < 1 || alpha_min > 255 || tap_format != IPP_TAPS_MFMA) return IPP_E_ARG;
    if (!tmp || !coefs || !descs || !bbox || n_images < 0 || max_ov_w <= 0 || max_ov_h <= 0) return IPP_E_ARG;
    if (trim && max_rows <= 0) return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    const int tyb = paste_max_bands(max_ov_h);
    const int64_t nb = (int64_t)tyb * n_images;
    if (nb >= INT32_MAX) return IPP_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int ib = (n_images + 255) / 256;
    hipLaunchKernelGGL(k_label_bbox_init, dim3(ib), dim3(256), 0, s, bbox, n_images);
    hipLaunchKernelGGL(k_pipe_overlay_bbox, dim3((uint32_t)nb), dim3(256), 0, s, tmp, coefs, descs,
                       fast_div((uint32_t)tyb), alpha_min, bbox, trim, trim ? trim_bands(max_rows) : 0);
    hipLaunchKernelGGL(k_label_bbox_finish, dim3(ib), dim3(256), 0, s, bbox, n_images);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

extern "C" int ipp_pipe_overlay_bbox(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                                     int32_t n_images, int32_t max_ov_w, int32_t max_ov_h, int32_t alpha_min,
                                     int32_t tap_format, int32_t* bbox, void* stream) {
    return ipp_pipe_overlay_bbox_trim(tmp, coefs, descs, n_images, max_ov_w, max_ov_h, alpha_min, tap_format, bbox,
                                      nullptr, 0, stream);
}

extern "C" int ipp_alpha_bbox_min(const uint8_t* img, const ipp_image_desc* descs, int32_t n_images,
                                  int32_t max_w, int32_t max_h, int32_t alpha_min, int32_t* bbox, void* stream) {
    if (alpha_min < 1 || alpha_min > 255) return IPP_E_ARG;
    if (!img || !descs || !bbox || n_images < 0 || max_w <= 0 || max_h <= 0) return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    const int tx = (max_w + BT_W - 1) / BT_W, ty = (max_h + BT_H - 1) / BT_H;
    const int64_t blocks = (int64_t)tx * ty * n_images;
    if (blocks >= (int64_t)INT32_MAX) return IPP_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int ib = (n_images + 255) / 256;
    hipLaunchKernelGGL(k_label_bbox_init, dim3(ib), dim3(256), 0, s, bbox, n_images);
    hipLaunchKernelGGL(k_alpha_bbox_min, dim3((uint32_t)blocks), dim3(256), 0, s, img, descs, tx, ty, alpha_min,
                       bbox);
    hipLaunchKernelGGL(k_label_bbox_finish, dim3(ib), dim3(256), 0, s, bbox, n_images);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

extern "C" int64_t ipp_pipe_scene_scratch_bytes(int32_t n_images, int32_t n_scenes, int32_t per_scene,
                                                int32_t max_ov_w, int32_t max_ov_h) {
    if (n_images < 0 || n_scenes < 0 || per_scene < 1 || max_ov_w <= 0 || max_ov_h <= 0) return IPP_E_ARG;
    return scene_table_bytes((int64_t)n_scenes * per_scene) + (int64_t)n_images * max_ov_h * scene_pitch(max_ov_w);
}

extern "C" int ipp_pipe_scene_boxes(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                                    const int32_t* scene_layer, int32_t n_images, int32_t n_scenes,
                                    int32_t per_scene, int32_t max_ov_w, int32_t max_ov_h, int32_t alpha_min,
                                    int32_t cover_min, int32_t tap_format, uint8_t* scratch, int32_t* out,
                                    void* stream) {
    if (alpha_min < 1 || alpha_min > 255 || cover_min < 1 || cover_min > 255 || tap_format != IPP_TAPS_MFMA)
        return IPP_E_ARG;
    if (!tmp || !coefs || !descs || !scene_layer || !scratch || !out || n_images < 0 || n_scenes < 0 ||
        per_scene < 1 || max_ov_w <= 0 || max_ov_h <= 0)
        return IPP_E_ARG;
    if ((reinterpret_cast<uintptr_t>(scratch) & 15u) != 0) return IPP_E_ARG;  // the planes are read by dwords
    if (n_images == 0) return IPP_OK;
    return scene_launches(tmp, coefs, descs, scene_layer, n_images, n_scenes, per_scene, 0, 0, max_ov_w, max_ov_h,
                          alpha_min, cover_min, scratch, out, nullptr, 0, (hipStream_t)stream);
}

extern "C" int ipp_pipe_scene_map(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                                  const int32_t* scene_layer, int32_t n_images, int32_t n_scenes, int32_t per_scene,
                                  int32_t bg_w, int32_t bg_h, int32_t max_ov_w, int32_t max_ov_h, int32_t alpha_min,
                                  int32_t cover_min, int32_t tap_format, uint8_t* scratch, int32_t* rows,
                                  uint8_t* map, int64_t map_pitch, void* stream) {
    if (alpha_min < 1 || alpha_min > 255 || cover_min < 1 || cover_min > 255 || tap_format != IPP_TAPS_MFMA)
        return IPP_E_ARG;
    if (!tmp || !coefs || !descs || !scene_layer || !scratch || !map || n_images < 0 || n_scenes < 0 ||
        per_scene < 1 || per_scene > IPP_SCENE_MAP_MAX_LAYERS || max_ov_w <= 0 || max_ov_h <= 0)
        return IPP_E_ARG;
    if (bg_w <= 0 || bg_h <= 0 || map_pitch < bg_w || (map_pitch & 15) != 0 || map_pitch > INT32_MAX)
        return IPP_E_ARG;
    // the planes are read by dwords, the map is stored by 16-B vectors
    if (((reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(map)) & 15u) != 0) return IPP_E_ARG;
    return scene_launches(tmp, coefs, descs, scene_layer, n_images, n_scenes, per_scene, bg_w, bg_h, max_ov_w,
                          max_ov_h, alpha_min, cover_min, scratch, rows, map, map_pitch, (hipStream_t)stream);
}

extern "C" int ipp_pipe_scene_cull(uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                                   const int32_t* scene_layer, int32_t n_images, int32_t n_scenes, int32_t per_scene,
                                   int32_t max_ov_w, int32_t max_ov_h, int32_t alpha_min, int32_t cover_min,
                                   int32_t min_q, int32_t min_pixels, int32_t tap_format, uint8_t* scratch,
                                   int32_t* cull, void* stream) {
    if (alpha_min < 1 || alpha_min > 255 || cover_min < 1 || cover_min > 255 || tap_format != IPP_TAPS_MFMA)
        return IPP_E_ARG;
    if (min_q < 0 || min_q > 65536 || min_pixels < 0) return IPP_E_ARG;
    if (!tmp || !coefs || !descs || !scene_layer || !scratch || !cull || n_images < 0 || n_scenes < 0 ||
        per_scene < 1 || max_ov_w <= 0 || max_ov_h <= 0)
        return IPP_E_ARG;
    // the planes are read by dwords, T is cleared by 16-B vectors
    if (((reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(tmp)) & 15u) != 0) return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    return cull_launches(tmp, coefs, descs, scene_layer, n_images, n_scenes, per_scene, max_ov_w, max_ov_h, alpha_min,
                         cover_min, min_q, min_pixels, scratch, cull, (hipStream_t)stream);
}
