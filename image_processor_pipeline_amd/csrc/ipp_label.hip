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
// The four scene entries share one statement of the visibility rule and of its
// bounds, and one set of device helpers (the strip step present4 / cover4 /
// hidden4, MaskBox and commit_row6, the map sweep map_tile / layer_rects /
// map_sweep, the row and slot-table helpers) and host helpers (ScenePrep,
// scene_args_ok); the kernels are callers of those.
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
// Scenes (K overlays pasted in layer order onto one composite): what the four
// scene entries share.
//
// Scratch: the table slot → descriptor (int32[n_scenes·K], slot = scene·K +
// layer, -1 = no descriptor), then one alpha plane per descriptor, max_ov_h
// rows of scene_pitch(max_ov_w) bytes, which k_scene_alpha fills from
// overlay_alpha_band (the overlay's rows inside the background).
//
// THE RULE.  A pixel of an overlay is PRESENT when its alpha >= alpha_min.  A
// later layer of its scene COVERS it when that layer's rectangle holds the
// pixel and its alpha there (read from its plane by composite coordinate) is
// >= cover_min.  A present pixel no later layer covers is VISIBLE.  present4
// and cover4 are the rule on the overlay's side (4 pixels of a strip row),
// map_sweep on the composite's (16 pixels of a map row).
//
// THE BOUNDS.  A later layer is read only when its slot entry lies in [0, n)
// and it has a plane (not ScenePlanes::lacks: not larger than (max_ov_w,
// max_ov_h); a larger descriptor is skipped and never read), and then only at
// 0 <= cy < ov_h <= max_ov_h and 0 <= cx < ov_w <= max_ov_w: every access lies
// in the plane of a descriptor in [0, n).
//
// Rows are (x0, y0, x1, y1, area, visible): reset to (INT_MAX, INT_MAX, -1, -1,
// 0, 0), committed per wave (commit_row6), an untouched box finished to -1s.
// ---------------------------------------------------------------------------
__host__ __device__ constexpr int64_t scene_pitch(int max_ov_w) { return ((int64_t)max_ov_w + 15) & ~(int64_t)15; }
__host__ __device__ constexpr int64_t scene_table_bytes(int64_t slots) { return (4 * slots + 255) & ~(int64_t)255; }

struct ScenePlanes {
    const uint8_t* base;
    int64_t pitch, psize;
    int max_w, max_h;
    __device__ __forceinline__ bool lacks(const ipp_paste_desc p) const { return p.ov_w > max_w || p.ov_h > max_h; }
    __device__ __forceinline__ const uint8_t* row(int d, int r) const {
        return base + (int64_t)d * psize + (int64_t)r * pitch;
    }
};

__device__ __forceinline__ ScenePlanes scene_planes(const uint8_t* planes, int max_ov_w, int max_ov_h) {
    const int64_t pitch = scene_pitch(max_ov_w);
    return {planes, pitch, (int64_t)max_ov_h * pitch, max_ov_w, max_ov_h};
}

// (scene, layer) of descriptor i; unmapped = alone in its scene, in no slot.
struct SceneSlot {
    int scene, layer;
    bool mapped;
};

__device__ __forceinline__ SceneSlot scene_slot(const int32_t* __restrict__ scene_layer, int i, int n_scenes, int K) {
    const int s = scene_layer[2 * i], k = scene_layer[2 * i + 1];
    return {s, k, (unsigned)s < (unsigned)n_scenes && (unsigned)k < (unsigned)K};
}

__device__ __forceinline__ void slot_table_set(int32_t* __restrict__ table, const int32_t* __restrict__ scene_layer,
                                               int i, int n_scenes, int K) {
    const SceneSlot at = scene_slot(scene_layer, i, n_scenes, K);
    if (at.mapped) table[(int64_t)at.scene * K + at.layer] = i;
}

__device__ __forceinline__ void row6_reset(int32_t* row) {
    row[0] = INT32_MAX;
    row[1] = INT32_MAX;
    row[2] = -1;
    row[3] = -1;
    row[4] = 0;
    row[5] = 0;
}

__device__ __forceinline__ void row6_finish(int32_t* row) {
    if (row[2] < 0) row[0] = row[1] = -1;
}

__global__ void k_scene_init(int32_t* __restrict__ out, int32_t* __restrict__ table,
                             const int32_t* __restrict__ scene_layer, int n, int n_scenes, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    row6_reset(out + 6 * i);
    slot_table_set(table, scene_layer, i, n_scenes, K);
}

// The slot table alone, for a launch without rows.
__global__ void k_scene_table(int32_t* __restrict__ table, const int32_t* __restrict__ scene_layer, int n,
                              int n_scenes, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) slot_table_set(table, scene_layer, i, n_scenes, K);
}

__global__ void k_scene_finish(int32_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) row6_finish(out + 6 * i);
}

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
    row6_finish(arows + 6 * i);
    if (rows) row6_finish(rows + 6 * i);
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

// ---------------------------------------------------------------------------
// The strip walk (k_scene_visible, k_cull_count, k_amodal_count): one block per
// (descriptor, SVR-row strip of its overlay), a thread per row and 4 pixels of
// it per step, u0 = 4·(lane & 15) + 64·step — one aligned dword of the plane
// (its pitch is a multiple of 16; bytes past ov_w are masked).
// ---------------------------------------------------------------------------
constexpr int SVR = 16;  // overlay rows per block

// The present mask of pixels (u0 .. u0+3, v) of overlay p, whose plane row v is `prow`.
__device__ __forceinline__ uint32_t present4(const uint8_t* __restrict__ prow, int v, int u0, const ipp_paste_desc p,
                                             int alpha_min) {
    uint32_t a4 = 0u;
    if (v < p.ov_h) a4 = *reinterpret_cast<const uint32_t*>(prow + u0);
    uint32_t present = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        present |= (uint32_t)(v < p.ov_h && u0 + k < p.ov_w && (int)((a4 >> (8 * k)) & 255u) >= alpha_min) << k;
    return present;
}

// Which of the 4 present pixels a layer covers: `qrow` is the row of its plane
// that holds them, cx0 the first one's column there, ov_w its width.
__device__ __forceinline__ uint32_t cover4(const uint8_t* __restrict__ qrow, int cx0, int ov_w, uint32_t present,
                                           int cover_min, uint32_t c = 0u) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int cx = cx0 + k;
        if (((present >> k) & 1u) && (unsigned)cx < (unsigned)ov_w && (int)qrow[cx] >= cover_min) c |= 1u << k;
    }
    return c;
}

// What the later layers of p's scene hide of its 4 present pixels (u0.., v):
// the runtime walk over the slots layer+1 .. K-1 (any K; block-uniform), which
// skips a layer without a descriptor, without a plane, or not `taken(dj)`.
// (Unlike layer_rects and k_amodal_count's tables, this walk does not test
// ov_w <= 0 / ov_h <= 0 of a later layer: the planner emits no such descriptor,
// and the test moves k_scene_visible's and k_cull_count's pinned VGPR counts
// (20 -> 19, 16 -> 15).  A hand-made descriptor with a negative size is the
// caller's error here, as it was before the walk was shared.)
template <typename Taken>
__device__ __forceinline__ uint32_t hidden4(const ipp_pipe_desc* __restrict__ descs, const int32_t* __restrict__ table,
                                            const ScenePlanes pl, int n, int K, const SceneSlot at,
                                            const ipp_paste_desc p, int v, int u0, uint32_t present, int cover_min,
                                            Taken taken) {
    uint32_t hidden = 0u;
    for (int j = at.mapped ? at.layer + 1 : K; j < K; ++j) {
        const int dj = table[(int64_t)at.scene * K + j];
        if ((unsigned)dj >= (unsigned)n) continue;
        const ipp_paste_desc q = descs[dj].p;
        if (pl.lacks(q) || !taken(dj)) continue;
        const int cy = p.y + v - q.y;  // the row in layer j's overlay
        if ((unsigned)cy >= (unsigned)q.ov_h) continue;
        hidden = cover4(pl.row(dj, cy), p.x + u0 - q.x, q.ov_w, present, cover_min, hidden);
    }
    return hidden;
}

// The box of the set bits of 4-pixel masks, bit k = pixel (x0 + k, y).
struct MaskBox {
    int xmin = INT32_MAX, ymin = INT32_MAX, xmax = -1, ymax = -1;
    __device__ __forceinline__ void add(uint32_t mask, int x0, int y) {
        if (!mask) return;
        xmin = min(xmin, x0 + (int)__builtin_ctz(mask));
        xmax = max(xmax, x0 + 31 - (int)__builtin_clz(mask));
        ymin = min(ymin, y);
        ymax = max(ymax, y);
    }
};

__device__ __forceinline__ int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Two counts at once, their shuffles interleaved.
__device__ __forceinline__ void wave_sum(int& a, int& b) {
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
    }
}

// Lane 0 adds the wave's two sums (integer atomicAdd: no result depends on the atomics' order).
__device__ __forceinline__ void lane0_add2(int32_t* a, int va, int32_t* b, int vb) {
    if ((threadIdx.x & 63) == 0) {
        if (va) atomicAdd(a, va);
        if (vb) atomicAdd(b, vb);
    }
}

// The wave's box and its (wave-summed) counts into a row: six atomics from lane 0.
__device__ __forceinline__ void commit_row6(int32_t* __restrict__ row, const MaskBox box, int area, int vis) {
    bbox_commit(row, box.xmin, box.ymin, box.xmax, box.ymax);
    lane0_add2(&row[4], area, &row[5], vis);
}

// ipp_pipe_scene_boxes: per overlay the box of its visible pixels, its present
// and its visible pixel counts.
__global__ void __launch_bounds__(256)
k_scene_visible(const ipp_pipe_desc* __restrict__ descs, const int32_t* __restrict__ scene_layer,
                const int32_t* __restrict__ table, const uint8_t* __restrict__ planes, FastDiv strips, int n,
                int n_scenes, int K, int max_ov_w, int max_ov_h, int alpha_min, int cover_min,
                int32_t* __restrict__ out) {
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int im = (int)fdiv(b, strips);
    const int v0 = (int)(b - (uint32_t)im * strips.d) * SVR;
    const ipp_paste_desc p = descs[im].p;
    const ScenePlanes pl = scene_planes(planes, max_ov_w, max_ov_h);
    if (v0 >= p.ov_h || pl.lacks(p)) return;  // block-uniform
    const SceneSlot at = scene_slot(scene_layer, im, n_scenes, K);
    const int v = v0 + (int)(threadIdx.x >> 4);
    MaskBox box;
    int area = 0, vis = 0;
    for (int u0 = 4 * (int)(threadIdx.x & 15); u0 < p.ov_w; u0 += 64) {
        const uint32_t present = present4(pl.row(im, v), v, u0, p, alpha_min);
        const uint32_t visible = present & ~hidden4(descs, table, pl, n, K, at, p, v, u0, present, cover_min,
                                                    [](int) { return true; });
        area += __builtin_popcount(present);
        vis += __builtin_popcount(visible);
        box.add(visible, p.x + u0, p.y + v);
    }
    wave_sum(area, vis);
    commit_row6(out + 6 * (int64_t)im, box, area, vis);
}

// ---------------------------------------------------------------------------
// The map sweep (k_scene_map, k_amodal_map): the rule's per-pixel answer.
// Byte (Y, X) of scene s's visibility map holds bit k iff layer k is mapped,
// has a plane, its rectangle clipped to the background holds (X, Y), it is
// present there and no later layer with a plane covers it; the presence map
// holds bit k whether covered or not.
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
// guarded by the clipped rectangle (THE BOUNDS above), and the rows it reads
// are the ones k_scene_alpha wrote.
// ---------------------------------------------------------------------------
constexpr int MT_W = 256, MT_H = 16, MT_PX = 16;
constexpr int kSceneMapMaxLayers = IPP_SCENE_MAP_MAX_LAYERS;
static_assert(kSceneMapMaxLayers == 8, "one bit per layer in a map byte");
static_assert(MT_PX == 16 && MT_W == 16 * MT_PX && MT_H * (MT_W / MT_PX) == 256, "the map kernels' thread map");

struct MapTile {
    int scene;
    int bx0, wy0;  // the block's first column, the wave's first of 4 rows
    int X0, Y;     // the thread's first pixel
};

__device__ __forceinline__ MapTile map_tile(FastDiv tiles, FastDiv tiles_x) {
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int scene = (int)fdiv(b, tiles);
    const uint32_t t = b - (uint32_t)scene * tiles.d;
    const int ty = (int)fdiv(t, tiles_x), tx = (int)(t - (uint32_t)ty * tiles_x.d);
    const int bx0 = tx * MT_W;
    return {scene, bx0, ty * MT_H + 4 * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)),
            bx0 + MT_PX * (int)(threadIdx.x & 15), ty * MT_H + (int)(threadIdx.x >> 4)};
}

// Per layer of the scene the descriptor and its paste rectangle; d[k] stays -1
// unless the layer's clipped rectangle meets the wave's pixels.
struct LayerRects {
    int d[kSceneMapMaxLayers], x[kSceneMapMaxLayers], y[kSceneMapMaxLayers], w[kSceneMapMaxLayers],
        h[kSceneMapMaxLayers];
};

// Phase 1 (block-uniform).
__device__ __forceinline__ LayerRects layer_rects(const ipp_pipe_desc* __restrict__ descs,
                                            const int32_t* __restrict__ table, const ScenePlanes pl,
                                            const MapTile t, int n, int K, int bg_w, int bg_h) {
    LayerRects r;
#pragma unroll
    for (int k = 0; k < kSceneMapMaxLayers; ++k) {
        r.d[k] = -1;
        r.x[k] = r.y[k] = r.w[k] = r.h[k] = 0;
        if (k >= K) continue;
        const int dk = table[(int64_t)t.scene * K + k];
        if ((unsigned)dk >= (unsigned)n) continue;  // no descriptor in this slot
        const ipp_paste_desc p = descs[dk].p;
        if (p.ov_w <= 0 || p.ov_h <= 0 || pl.lacks(p)) continue;  // no plane
        // the rectangle clipped to the background (64-bit: x + ov_w of a foreign descriptor must not wrap)
        const int64_t rx0 = max((int64_t)p.x, (int64_t)0), rx1 = min((int64_t)p.x + p.ov_w, (int64_t)bg_w);
        const int64_t ry0 = max((int64_t)p.y, (int64_t)0), ry1 = min((int64_t)p.y + p.ov_h, (int64_t)bg_h);
        if (rx0 >= (int64_t)t.bx0 + MT_W || rx1 <= t.bx0 || ry0 >= (int64_t)t.wy0 + 4 || ry1 <= t.wy0) continue;
        r.d[k] = dk;
        r.x[k] = p.x, r.y[k] = p.y, r.w[k] = p.ov_w, r.h[k] = p.ov_h;
    }
    return r;
}

// Phase 2: top down; the visibility words always, with PRESENCE the presence
// words too, handed to `store`.  The two forms of the bit are the two kernels'
// own (one select against one combined test): either way bit k of pixel i is
// set iff a >= alpha_min, in wv only while no later layer has covered it.
template <bool PRESENCE, typename Store>
__device__ __forceinline__ void map_sweep(const LayerRects& r, const ScenePlanes pl, const MapTile t, int bg_w,
                                          int alpha_min, int cover_min, Store store) {
    uint32_t wa[4] = {0u, 0u, 0u, 0u}, wv[4] = {0u, 0u, 0u, 0u};
    uint32_t covered = 0u;  // bit i: a later layer covers pixel X0 + i
#pragma unroll
    for (int k = kSceneMapMaxLayers - 1; k >= 0; --k) {
        if (r.d[k] < 0) continue;  // wave-uniform
        const int cy = t.Y - r.y[k];
        if ((unsigned)cy >= (unsigned)r.h[k]) continue;
        const uint8_t* row = pl.row(r.d[k], cy);
        const int cx0 = t.X0 - r.x[k];  // (X0 < map_pitch and |x| of a met rectangle are far below 2^31)
        const int xlim = min(r.w[k], bg_w - r.x[k]);  // columns of the overlay inside the background
#pragma unroll
        for (int i = 0; i < MT_PX; ++i) {
            const int cx = cx0 + i;
            if (cx >= 0 && cx < xlim) {
                const int a = row[cx];
                if constexpr (PRESENCE) {
                    const uint32_t bit = (a >= alpha_min ? 1u << k : 0u) << (8 * (i & 3));
                    wa[i >> 2] |= bit;
                    if (!((covered >> i) & 1u)) wv[i >> 2] |= bit;
                } else {
                    if (!((covered >> i) & 1u) && a >= alpha_min) wv[i >> 2] |= (1u << k) << (8 * (i & 3));
                }
                if (a >= cover_min) covered |= 1u << i;
            }
        }
    }
    store(wa, wv);
}

// ipp_pipe_scene_map: one visibility map per composite (instance masks).
__global__ void __launch_bounds__(256)
k_scene_map(const ipp_pipe_desc* __restrict__ descs, const int32_t* __restrict__ table,
            const uint8_t* __restrict__ planes, FastDiv tiles, FastDiv tiles_x, int n, int K, int bg_w, int bg_h,
            int max_ov_w, int max_ov_h, int alpha_min, int cover_min, uint8_t* __restrict__ map,
            int64_t map_pitch) {
    const MapTile t = map_tile(tiles, tiles_x);
    const ScenePlanes pl = scene_planes(planes, max_ov_w, max_ov_h);
    const LayerRects r = layer_rects(descs, table, pl, t, n, K, bg_w, bg_h);
    if (t.Y >= bg_h || t.X0 >= map_pitch) return;  // (no barrier below)
    map_sweep<false>(r, pl, t, bg_w, alpha_min, cover_min, [&](const uint32_t*, const uint32_t* wv) {
        store16<0>(map + ((int64_t)t.scene * bg_h + t.Y) * map_pitch + t.X0, 16, true, wv);
    });
}

// What the launches of a scene entry share after its argument checks: the grid
// sizes and their limits, the split of the scratch into slot table and planes,
// the table's memset, the alpha launch.
struct ScenePrep {
    int tyb, strips, ib;  // bands and strips per descriptor, blocks of a thread per descriptor
    int mtx = 0, mty = 0;  // map tiles
    int64_t slots;
    int32_t* table;
    uint8_t* planes;

    // IPP_OK with the table memset issued, or the code to return.  map_pitch > 0: the launch has a map.
    int begin(int n_images, int n_scenes, int per_scene, int max_ov_h, uint8_t* scratch, int bg_h, int64_t map_pitch,
              hipStream_t s) {
        tyb = paste_max_bands(max_ov_h), strips = (max_ov_h + SVR - 1) / SVR, ib = (n_images + 255) / 256;
        slots = (int64_t)n_scenes * per_scene;
        if ((int64_t)tyb * n_images >= INT32_MAX || (int64_t)strips * n_images >= INT32_MAX || slots >= INT32_MAX)
            return IPP_E_ARG;
        if (map_pitch > 0) {
            mtx = (int)((map_pitch + MT_W - 1) / MT_W), mty = (bg_h + MT_H - 1) / MT_H;
            if ((int64_t)mtx * mty * n_scenes >= INT32_MAX) return IPP_E_ARG;
        }
        table = reinterpret_cast<int32_t*>(scratch);
        planes = scratch + scene_table_bytes(slots);
        if (slots > 0 && hipMemsetAsync(table, 0xFF, 4 * (size_t)slots, s) != hipSuccess) return IPP_E_LAUNCH;
        return IPP_OK;
    }

    void alpha(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs, int n_images, int max_ov_w,
               int max_ov_h, hipStream_t s) const {
        hipLaunchKernelGGL(k_scene_alpha, dim3((uint32_t)(tyb * n_images)), dim3(256), 0, s, tmp, coefs, descs,
                           fast_div((uint32_t)tyb), max_ov_w, max_ov_h, planes);
    }
};

// The launches of ipp_pipe_scene_boxes and ipp_pipe_scene_map: k_scene_init
// (with rows) or k_scene_table, k_scene_alpha, then the boxes (`rows`:
// k_scene_visible, k_scene_finish) and / or the map, whichever is given.
int scene_launches(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs, const int32_t* scene_layer,
                   int n_images, int n_scenes, int per_scene, int bg_w, int bg_h, int max_ov_w, int max_ov_h,
                   int alpha_min, int cover_min, uint8_t* scratch, int32_t* rows, uint8_t* map, int64_t map_pitch,
                   hipStream_t s) {
    ScenePrep sp;
    if (const int rc = sp.begin(n_images, n_scenes, per_scene, max_ov_h, scratch, bg_h, map ? map_pitch : 0, s))
        return rc;
    if (n_images > 0) {
        if (rows)
            hipLaunchKernelGGL(k_scene_init, dim3(sp.ib), dim3(256), 0, s, rows, sp.table, scene_layer, n_images,
                               n_scenes, per_scene);
        else
            hipLaunchKernelGGL(k_scene_table, dim3(sp.ib), dim3(256), 0, s, sp.table, scene_layer, n_images, n_scenes,
                               per_scene);
        sp.alpha(tmp, coefs, descs, n_images, max_ov_w, max_ov_h, s);
        if (rows) {
            hipLaunchKernelGGL(k_scene_visible, dim3((uint32_t)(sp.strips * n_images)), dim3(256), 0, s, descs,
                               scene_layer, sp.table, sp.planes, fast_div((uint32_t)sp.strips), n_images, n_scenes,
                               per_scene, max_ov_w, max_ov_h, alpha_min, cover_min, rows);
            hipLaunchKernelGGL(k_scene_finish, dim3(sp.ib), dim3(256), 0, s, rows, n_images);
        }
    }
    if (map && n_scenes > 0)
        hipLaunchKernelGGL(k_scene_map, dim3((uint32_t)(sp.mtx * sp.mty * n_scenes)), dim3(256), 0, s, descs, sp.table,
                           sp.planes, fast_div((uint32_t)(sp.mtx * sp.mty)), fast_div((uint32_t)sp.mtx), n_images,
                           per_scene, bg_w, bg_h, max_ov_w, max_ov_h, alpha_min, cover_min, map, map_pitch);
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
    const SceneSlot at = scene_slot(scene_layer, im, n_scenes, K);
    if ((at.mapped ? at.layer : K - 1) != cur) return;  // another launch's descriptor (block-uniform)
    const ipp_paste_desc p = descs[im].p;
    const ScenePlanes pl = scene_planes(planes, max_ov_w, max_ov_h);
    if (v0 >= p.ov_h || pl.lacks(p)) return;  // block-uniform
    const int v = v0 + (int)(threadIdx.x >> 4);
    int area = 0, vis = 0;
    for (int u0 = 4 * (int)(threadIdx.x & 15); u0 < p.ov_w; u0 += 64) {
        const uint32_t present = present4(pl.row(im, v), v, u0, p, alpha_min);
        // the kept later layers: layer j's counters are final, its launch came earlier in the stream
        const uint32_t hidden = hidden4(descs, table, pl, n, K, at, p, v, u0, present, cover_min, [&](int dj) {
            return cull_keep(cull[4 * (int64_t)dj + 1], cull[4 * (int64_t)dj + 2], min_q, min_pixels);
        });
        area += __builtin_popcount(present);
        vis += __builtin_popcount(present & ~hidden);
    }
    wave_sum(area, vis);
    lane0_add2(&cull[4 * (int64_t)im + 1], area, &cull[4 * (int64_t)im + 2], vis);
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
    if ((int64_t)kCullClearBlocks * n_images >= INT32_MAX) return IPP_E_ARG;
    ScenePrep sp;
    if (const int rc = sp.begin(n_images, n_scenes, per_scene, max_ov_h, scratch, 0, 0, s)) return rc;
    if (hipMemsetAsync(cull, 0, 16 * (size_t)n_images, s) != hipSuccess) return IPP_E_LAUNCH;
    hipLaunchKernelGGL(k_scene_table, dim3(sp.ib), dim3(256), 0, s, sp.table, scene_layer, n_images, n_scenes,
                       per_scene);
    sp.alpha(tmp, coefs, descs, n_images, max_ov_w, max_ov_h, s);
    for (int k = per_scene - 1; k >= 0; --k)
        hipLaunchKernelGGL(k_cull_count, dim3((uint32_t)(sp.strips * n_images)), dim3(256), 0, s, descs, scene_layer,
                           sp.table, sp.planes, fast_div((uint32_t)sp.strips), n_images, n_scenes, per_scene, k,
                           max_ov_w, max_ov_h, alpha_min, cover_min, min_q, min_pixels, cull);
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
//   k_amodal_init   arows and rows reset, the table;
//   k_scene_alpha   once, whatever is asked for;
//   k_amodal_count  the strip walk with per-layer counters: of later layer j,
//     top down, COVERS += popcount(present & cover_j) and HIDES +=
//     popcount(present & cover_j & ~hidden) before hidden |= cover_j; the
//     present box and, when `rows` is given, the visible box (what
//     k_scene_visible writes);
//   k_amodal_finish untouched boxes become (-1, -1, -1, -1);
//   k_amodal_map    the map sweep storing the presence and / or the visibility
//     map.
// Scenes have at most 8 layers here, so k_amodal_count keeps the later layers
// in unrolled block-uniform tables instead of hidden4's runtime walk: phase 1
// keeps layer j only when it is in [0, n), has a plane and its rectangle meets
// the strip's rows and the overlay's columns (64-bit, a foreign descriptor must
// not wrap), so inside the loop cover4's loads are the only ones (THE BOUNDS).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_amodal_count(const ipp_pipe_desc* __restrict__ descs, const int32_t* __restrict__ scene_layer,
               const int32_t* __restrict__ table, const uint8_t* __restrict__ planes, FastDiv strips, int n,
               int n_scenes, int K, int max_ov_w, int max_ov_h, int alpha_min, int cover_min,
               int32_t* __restrict__ arows, int32_t* __restrict__ occ, int32_t* __restrict__ rows) {
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int im = (int)fdiv(b, strips);
    const int v0 = (int)(b - (uint32_t)im * strips.d) * SVR;
    const ipp_paste_desc p = descs[im].p;
    const ScenePlanes pl = scene_planes(planes, max_ov_w, max_ov_h);
    if (v0 >= p.ov_h || pl.lacks(p)) return;  // block-uniform
    const SceneSlot at = scene_slot(scene_layer, im, n_scenes, K);
    const int scene = at.scene, layer = at.layer;
    const bool mapped = at.mapped;

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
        if (q.ov_w <= 0 || q.ov_h <= 0 || pl.lacks(q)) continue;  // no plane
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
    for (int u0 = 4 * (int)(threadIdx.x & 15); u0 < p.ov_w; u0 += 64) {
        const uint32_t present = present4(pl.row(im, v), v, u0, p, alpha_min);
        uint32_t hidden = 0u;
        // Phase 2: the later layers, top down (layer 0 is nobody's later layer)
#pragma unroll
        for (int j = kSceneMapMaxLayers - 1; j > 0; --j) {
            if (d[j] < 0) continue;  // block-uniform
            const int cy = p.y + v - qy[j];  // the row in layer j's overlay
            uint32_t c = 0u;
            if ((unsigned)cy < (unsigned)qh[j])
                c = cover4(pl.row(d[j], cy), p.x + u0 - qx[j], qw[j], present,
                           cover_min);
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
    int32_t* arow = arows + 6 * (int64_t)im;
    bbox_commit(arow, axmin, aymin, axmax, aymax);
    lane0_add2(&arow[4], area, &arow[5], vis);
    if (rows) {  // (uniform) what k_scene_visible writes
        int32_t* row = rows + 6 * (int64_t)im;
        bbox_commit(row, xmin, ymin, xmax, ymax);
        lane0_add2(&row[4], area, &row[5], vis);
    }
    if (!mapped) return;  // block-uniform: alone in its scene, in no slot of occ
    int32_t* oc0 = occ + (((int64_t)scene * 2) * K + layer) * K;  // occ[scene][0][layer][.]
    int32_t* oc1 = oc0 + (int64_t)K * K;                          // occ[scene][1][layer][.]
    lane0_add2(&oc0[layer], area, &oc1[layer], vis);
#pragma unroll
    for (int j = 1; j < kSceneMapMaxLayers; ++j) {
        if (d[j] < 0) continue;  // block-uniform
        lane0_add2(&oc0[j], wave_sum(cov[j]), &oc1[j], wave_sum(hid[j]));
    }
}

// The presence map in `amap`, the visibility map (k_scene_map's) in `vmap`; either may be null (uniform).
__global__ void __launch_bounds__(256)
k_amodal_map(const ipp_pipe_desc* __restrict__ descs, const int32_t* __restrict__ table,
             const uint8_t* __restrict__ planes, FastDiv tiles, FastDiv tiles_x, int n, int K, int bg_w, int bg_h,
             int max_ov_w, int max_ov_h, int alpha_min, int cover_min, uint8_t* __restrict__ amap,
             uint8_t* __restrict__ vmap, int64_t map_pitch) {
    const MapTile t = map_tile(tiles, tiles_x);
    const ScenePlanes pl = scene_planes(planes, max_ov_w, max_ov_h);
    const LayerRects r = layer_rects(descs, table, pl, t, n, K, bg_w, bg_h);
    if (t.Y >= bg_h || t.X0 >= map_pitch) return;  // (no barrier below)
    map_sweep<true>(r, pl, t, bg_w, alpha_min, cover_min, [&](const uint32_t* wa, const uint32_t* wv) {
        const int64_t at = ((int64_t)t.scene * bg_h + t.Y) * map_pitch + t.X0;
        if (amap) store16<0>(amap + at, 16, true, wa);
        if (vmap) store16<0>(vmap + at, 16, true, wv);
    });
}

int amodal_launches(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs, const int32_t* scene_layer,
                    int n_images, int n_scenes, int per_scene, int bg_w, int bg_h, int max_ov_w, int max_ov_h,
                    int alpha_min, int cover_min, uint8_t* scratch, int32_t* arows, int32_t* occ, uint8_t* amap,
                    int32_t* rows, uint8_t* vmap, int64_t map_pitch, hipStream_t s) {
    ScenePrep sp;
    if (const int rc = sp.begin(n_images, n_scenes, per_scene, max_ov_h, scratch, bg_h, map_pitch, s)) return rc;
    if (sp.slots > 0 && hipMemsetAsync(occ, 0, 8 * (size_t)sp.slots * per_scene, s) != hipSuccess)
        return IPP_E_LAUNCH;
    if (n_images > 0) {
        hipLaunchKernelGGL(k_amodal_init, dim3(sp.ib), dim3(256), 0, s, arows, rows, sp.table, scene_layer, n_images,
                           n_scenes, per_scene);
        sp.alpha(tmp, coefs, descs, n_images, max_ov_w, max_ov_h, s);
        hipLaunchKernelGGL(k_amodal_count, dim3((uint32_t)(sp.strips * n_images)), dim3(256), 0, s, descs, scene_layer,
                           sp.table, sp.planes, fast_div((uint32_t)sp.strips), n_images, n_scenes, per_scene, max_ov_w,
                           max_ov_h, alpha_min, cover_min, arows, occ, rows);
        hipLaunchKernelGGL(k_amodal_finish, dim3(sp.ib), dim3(256), 0, s, arows, rows, n_images);
    }
    if ((amap || vmap) && n_scenes > 0)
        hipLaunchKernelGGL(k_amodal_map, dim3((uint32_t)(sp.mtx * sp.mty * n_scenes)), dim3(256), 0, s, descs, sp.table,
                           sp.planes, fast_div((uint32_t)(sp.mtx * sp.mty)), fast_div((uint32_t)sp.mtx), n_images,
                           per_scene, bg_w, bg_h, max_ov_w, max_ov_h, alpha_min, cover_min, amap, vmap, map_pitch);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

// The checks common to the four scene entries.
bool scene_args_ok(const void* tmp, const void* coefs, const void* descs, const void* scene_layer, const void* scratch,
                   int n_images, int n_scenes, int per_scene, int max_ov_w, int max_ov_h, int alpha_min, int cover_min,
                   int tap_format) {
    return alpha_min >= 1 && alpha_min <= 255 && cover_min >= 1 && cover_min <= 255 && tap_format == IPP_TAPS_MFMA &&
           tmp && coefs && descs && scene_layer && scratch && n_images >= 0 && n_scenes >= 0 && per_scene >= 1 &&
           max_ov_w > 0 && max_ov_h > 0;
}

// Those of the two entries with maps: one bit per layer, the background, the maps' pitch.
bool scene_map_args_ok(int per_scene, int bg_w, int bg_h, int64_t map_pitch) {
    return per_scene <= IPP_SCENE_MAP_MAX_LAYERS && bg_w > 0 && bg_h > 0 && map_pitch >= bg_w &&
           (map_pitch & 15) == 0 && map_pitch <= INT32_MAX;
}

// The planes are read by dwords, the maps and T are written by 16-B vectors.
bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c);
    return (bits & 15u) == 0;
}

}  // namespace

extern "C" int ipp_pipe_scene_amodal(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                                     const int32_t* scene_layer, int32_t n_images, int32_t n_scenes,
                                     int32_t per_scene, int32_t bg_w, int32_t bg_h, int32_t max_ov_w,
                                     int32_t max_ov_h, int32_t alpha_min, int32_t cover_min, int32_t tap_format,
                                     uint8_t* scratch, int32_t* arows, int32_t* occ, uint8_t* amap, int32_t* rows,
                                     uint8_t* vmap, int64_t map_pitch, void* stream) {
    if (!scene_args_ok(tmp, coefs, descs, scene_layer, scratch, n_images, n_scenes, per_scene, max_ov_w, max_ov_h,
                       alpha_min, cover_min, tap_format) ||
        !scene_map_args_ok(per_scene, bg_w, bg_h, map_pitch) || !arows || !occ || !aligned16(scratch, amap, vmap))
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
    if (!scene_args_ok(tmp, coefs, descs, scene_layer, scratch, n_images, n_scenes, per_scene, max_ov_w, max_ov_h,
                       alpha_min, cover_min, tap_format) ||
        !out || !aligned16(scratch))
        return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    return scene_launches(tmp, coefs, descs, scene_layer, n_images, n_scenes, per_scene, 0, 0, max_ov_w, max_ov_h,
                          alpha_min, cover_min, scratch, out, nullptr, 0, (hipStream_t)stream);
}

extern "C" int ipp_pipe_scene_map(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                                  const int32_t* scene_layer, int32_t n_images, int32_t n_scenes, int32_t per_scene,
                                  int32_t bg_w, int32_t bg_h, int32_t max_ov_w, int32_t max_ov_h, int32_t alpha_min,
                                  int32_t cover_min, int32_t tap_format, uint8_t* scratch, int32_t* rows,
                                  uint8_t* map, int64_t map_pitch, void* stream) {
    if (!scene_args_ok(tmp, coefs, descs, scene_layer, scratch, n_images, n_scenes, per_scene, max_ov_w, max_ov_h,
                       alpha_min, cover_min, tap_format) ||
        !scene_map_args_ok(per_scene, bg_w, bg_h, map_pitch) || !map || !aligned16(scratch, map))
        return IPP_E_ARG;
    return scene_launches(tmp, coefs, descs, scene_layer, n_images, n_scenes, per_scene, bg_w, bg_h, max_ov_w,
                          max_ov_h, alpha_min, cover_min, scratch, rows, map, map_pitch, (hipStream_t)stream);
}

extern "C" int ipp_pipe_scene_cull(uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                                   const int32_t* scene_layer, int32_t n_images, int32_t n_scenes, int32_t per_scene,
                                   int32_t max_ov_w, int32_t max_ov_h, int32_t alpha_min, int32_t cover_min,
                                   int32_t min_q, int32_t min_pixels, int32_t tap_format, uint8_t* scratch,
                                   int32_t* cull, void* stream) {
    if (!scene_args_ok(tmp, coefs, descs, scene_layer, scratch, n_images, n_scenes, per_scene, max_ov_w, max_ov_h,
                       alpha_min, cover_min, tap_format) ||
        min_q < 0 || min_q > 65536 || min_pixels < 0 || !cull || !aligned16(scratch, tmp))
        return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    return cull_launches(tmp, coefs, descs, scene_layer, n_images, n_scenes, per_scene, max_ov_w, max_ov_h, alpha_min,
                         cover_min, min_q, min_pixels, scratch, cull, (hipStream_t)stream);
}
