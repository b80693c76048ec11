// Training batches left on the device (ipp.h: ipp_scene_feed_images,
// ipp_scene_feed_targets, ipp_scene_feed_index_map; the traffic model is in
// DESIGN.md §3).
//
//   k_feed_images<T>   composites (S, bg_h, bg_w, 3) uint8 -> planar (S, 3,
//                      bg_h, bg_w) of T (2- or 4-byte opaque words) through a
//                      3×256 table kept in LDS.  A scene is a flat stream of P
//                      = bg_w·bg_h pixels on both sides.  Its first `head`
//                      pixels (0..15, chosen so that the byte behind them is
//                      16-B aligned) and the `tail` (< 16) after its last full
//                      run go one pixel per thread; between them a lane takes
//                      a run of 16 pixels: three aligned 16-B loads, 48 table
//                      reads, and per plane 16·sizeof(T) bytes in 16-B stores
//                      (unaligned ones where the plane is not 16-B aligned
//                      behind the head: with an odd P the three planes of a
//                      scene cannot all be).
//   k_feed_targets     one workgroup: inverts the descriptor permutation into
//                      `slot`, then scans the S·K overlays in scene, layer
//                      order in chunks of 1024 with a carried prefix and
//                      stores the kept rows compacted.
//   k_letterbox_targets   the same scan with the rows moved and scaled into a
//                      letterbox rectangle (targets_scan<true>).
//   k_feed_index_map   visibility map -> per-pixel row index within the
//                      scene's run of targets, through a 256-entry table per
//                      scene in LDS; 16-B loads and stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ipp.h"
#include "ipp_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRunPixels = 16;                   // pixels of a lane's run: 48 input bytes
constexpr int kRunsPerThread = 4;                // runs a thread takes, a block apart
constexpr int kTileRuns = kThreads * kRunsPerThread;
constexpr int kScanThreads = 1024;               // k_feed_targets: one workgroup, one chunk per sweep
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kGroupsPerThread = 4;              // k_feed_index_map: 16-B groups a thread takes, a block apart
constexpr int kTileGroups = kThreads * kGroupsPerThread;

// Byte j (0..47) of the three dwordx4 of a run.
__device__ __forceinline__ uint32_t run_byte(const uint4 (&v)[3], int j) {
    const uint4& q = v[j >> 4];
    const int d = (j >> 2) & 3;
    const uint32_t w = d == 0 ? q.x : d == 1 ? q.y : d == 2 ? q.z : q.w;
    return (w >> (8 * (j & 3))) & 0xFFu;
}

// 16 bytes stored at an address that is only known to be a multiple of the
// element size (2 or 4).  gfx950 runs the HSA queues in unaligned-access mode
// (ipp_device.h: ld_u32_unaligned), so this is one global_store_dwordx4 either
// way; the typedef keeps the compiler from assuming more than holds.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(2), may_alias)) u32x4_elem_aligned;

// The 16 elements of one plane of a run, as dwords, in 16-B stores.
template <int WORDS>
__device__ __forceinline__ void store_plane(uint8_t* p, const uint32_t (&w)[WORDS]) {
#pragma unroll
    for (int i = 0; i < WORDS; i += 4) {
        const u32x4 v = {w[i], w[i + 1], w[i + 2], w[i + 3]};
        *reinterpret_cast<u32x4_elem_aligned*>(p + 4 * i) = v;
    }
}

// Why no byte outside the S·P·3 input bytes is read and none outside the
// S·3·P output elements written: a thread touches scene s < n_scenes only.  A
// run r is taken iff r < runs = (P - head) / 16, and reads the 48 bytes from
// 3·head + 48·r of the scene's slot, which end at 3·(head + 16·(r + 1)) <=
// 3·P; it writes elements head + 16·r .. head + 16·r + 15 < P of each of the
// scene's three planes.  The head and tail threads read the three bytes of one
// pixel p < P each and write element p of the three planes.  The 16-B loads
// are aligned by the choice of the head; the 16-B stores are aligned whenever
// the plane is behind the head (always, when 3·P·sizeof(T) and `out` are
// multiples of 16 and `in` is 16-B aligned: then head = 0 too), and are
// unaligned stores of exactly the same 16 bytes otherwise.
template <typename T>
__global__ __launch_bounds__(kThreads) void k_feed_images(const uint8_t* __restrict__ in, T* __restrict__ out,
                                                          const T* __restrict__ lut, uint32_t P, int bgr,
                                                          FastDiv tiles) {
    constexpr int kWords = kRunPixels * (int)sizeof(T) / 4;  // dwords of one plane of a run
    __shared__ T s_lut[3 * 256];
    const uint32_t tid = threadIdx.x;
    const uint32_t s = fdiv(blockIdx.x, tiles), tile = blockIdx.x - s * tiles.d;
#pragma unroll
    for (int c = 0; c < 3; ++c) s_lut[256 * c + tid] = lut[256 * c + tid];

    const uint8_t* src = in + (int64_t)s * 3 * P;
    T* dst = out + (int64_t)s * 3 * P;
    // head: 3·head ≡ -src (mod 16); 3·11 = 33 ≡ 1, so head ≡ -11·src
    uint32_t head = (uint32_t)((16u - ((uint32_t)reinterpret_cast<uintptr_t>(src) & 15u)) * 11u) & 15u;
    if (head > P) head = P;
    const uint32_t runs = (P - head) / kRunPixels, tail0 = head + runs * kRunPixels;
    // input channel k feeds plane pl[k] through table row pl[k]
    const int pl0 = bgr ? 2 : 0, pl2 = bgr ? 0 : 2;
    T* const plane[3] = {dst + (int64_t)pl0 * P + head, dst + (int64_t)P + head, dst + (int64_t)pl2 * P + head};
    const T* const row[3] = {s_lut + 256 * pl0, s_lut + 256, s_lut + 256 * pl2};
    __syncthreads();

    if (tile == 0u) {  // the head and the tail: fewer than 32 pixels, one per thread
        const uint32_t n_edge = head + (P - tail0);
        if (tid < n_edge) {
            const uint32_t p = tid < head ? tid : tail0 + (tid - head);
            const uint8_t* px = src + 3 * (int64_t)p;
#pragma unroll
            for (int k = 0; k < 3; ++k) plane[k][(int64_t)p - head] = row[k][px[k]];
        }
    }

    const uint32_t r0 = tile * (uint32_t)kTileRuns + tid;
    const uint8_t* body = src + 3 * head;
    uint4 v[kRunsPerThread][3];
#pragma unroll
    for (int u = 0; u < kRunsPerThread; ++u) {
        const uint32_t r = r0 + (uint32_t)(u * kThreads);
        if (r < runs) {
            const uint4* q = reinterpret_cast<const uint4*>(body + 48 * (int64_t)r);
            v[u][0] = q[0], v[u][1] = q[1], v[u][2] = q[2];
        }
    }
#pragma unroll
    for (int u = 0; u < kRunsPerThread; ++u) {
        const uint32_t r = r0 + (uint32_t)(u * kThreads);
        if (r >= runs) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            uint32_t w[kWords];
            if (sizeof(T) == 2) {
#pragma unroll
                for (int i = 0; i < kWords; ++i)
                    w[i] = (uint32_t)row[k][run_byte(v[u], 6 * i + k)] | ((uint32_t)row[k][run_byte(v[u], 6 * i + 3 + k)] << 16);
            } else {
#pragma unroll
                for (int i = 0; i < kWords; ++i) w[i] = (uint32_t)row[k][run_byte(v[u], 3 * i + k)];
            }
            store_plane<kWords>(reinterpret_cast<uint8_t*>(plane[k] + (int64_t)r * kRunPixels), w);
        }
    }
}

// The number of set flags in the lanes below this one, and the wave's total.
__device__ __forceinline__ uint32_t wave_rank(bool flag, uint32_t& total) {
    const uint64_t m = __ballot(flag);
    total = (uint32_t)__popcll(m);
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));  // set flags below the lane
}

// The rectangle of a letterboxed batch (ipp.h: ipp_scene_feed_targets_letterbox).
struct Letterbox {
    int32_t new_w, new_h, left, top, out_w, out_h;
};

// `slot` doubles as the inverse of the descriptor permutation until the sweep
// replaces each word by its answer: word q = scene·per_scene + layer first
// holds the highest descriptor that scene_layer maps there (an integer max:
// the same whatever order the lanes arrive in), or -1.  The words are read
// back with agent-scope loads, which are served by the L2 the atomics ran in.
// targets_scan is the whole of both kernels; only ROW differs: with LB each of
// the four numbers is an exact int64 numerator over an exact int64 denominator
// (both below 2^49, exact in float64), ONE correctly rounded float64 division
// and ONE round-to-nearest conversion to float32.
template <bool LB>
__device__ __forceinline__ void targets_scan(const int32_t* __restrict__ rows, const int32_t* __restrict__ scene_layer,
                                             const int32_t* __restrict__ class_ids, int n, int n_scenes, int per_scene,
                                             int bg_w, int bg_h, int min_q, const Letterbox& lb,
                                             float* __restrict__ targets, int32_t* __restrict__ count, int32_t* slot) {
    __shared__ uint32_t s_wave[kScanWaves];
    const int tid = (int)threadIdx.x, wave = tid >> 6;
    const int total = n_scenes * per_scene;
    for (int q = tid; q < total; q += kScanThreads) __hip_atomic_store(&slot[q], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    for (int d = tid; d < n; d += kScanThreads) {
        const int s = scene_layer[2 * d], k = scene_layer[2 * d + 1];
        if ((unsigned)s < (unsigned)n_scenes && (unsigned)k < (unsigned)per_scene) atomicMax(&slot[s * per_scene + k], d);
    }
    __syncthreads();
    const float fw = (float)bg_w, fh = (float)bg_h, fw2 = (float)(2 * bg_w), fh2 = (float)(2 * bg_h);
    uint32_t base = 0u;  // kept overlays before this chunk
    for (int q0 = 0; q0 < total; q0 += kScanThreads) {
        const int q = q0 + tid;
        const int d = q < total ? __hip_atomic_load(&slot[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1;
        int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        bool keep = false;
        if (d >= 0) {
            const int32_t* r = rows + 6 * (int64_t)d;
            x0 = r[0], y0 = r[1], x1 = r[2], y1 = r[3];
            const int64_t area = r[4], vis = r[5];
            keep = vis > 0 && 65536ll * vis >= (int64_t)min_q * area;
        }
        uint32_t in_wave;
        const uint32_t below = wave_rank(keep, in_wave);
        if ((tid & 63) == 0) s_wave[wave] = in_wave;
        __syncthreads();
        uint32_t before = base, all = 0u;
#pragma unroll
        for (int k = 0; k < kScanWaves; ++k) {
            if (k < wave) before += s_wave[k];
            all += s_wave[k];
        }
        if (q < total) {
            const uint32_t pos = before + below;
            slot[q] = keep ? (int32_t)pos : -1;
            if (keep) {
                float* t = targets + 6 * (int64_t)pos;
                t[0] = (float)(q / per_scene);
                t[1] = (float)(class_ids ? class_ids[d] : 0);
                if (LB) {
                    const int64_t dx = (int64_t)bg_w * lb.out_w, dy = (int64_t)bg_h * lb.out_h;
                    const int64_t cx = (int64_t)(x0 + x1) * lb.new_w + 2 * (int64_t)lb.left * bg_w;
                    const int64_t cy = (int64_t)(y0 + y1) * lb.new_h + 2 * (int64_t)lb.top * bg_h;
                    t[2] = __double2float_rn(__ddiv_rn((double)cx, (double)(2 * dx)));
                    t[3] = __double2float_rn(__ddiv_rn((double)cy, (double)(2 * dy)));
                    t[4] = __double2float_rn(__ddiv_rn((double)((int64_t)(x1 - x0) * lb.new_w), (double)dx));
                    t[5] = __double2float_rn(__ddiv_rn((double)((int64_t)(y1 - y0) * lb.new_h), (double)dy));
                } else {
                    t[2] = __fdiv_rn((float)(x0 + x1), fw2);
                    t[3] = __fdiv_rn((float)(y0 + y1), fh2);
                    t[4] = __fdiv_rn((float)(x1 - x0), fw);
                    t[5] = __fdiv_rn((float)(y1 - y0), fh);
                }
            }
        }
        base += all;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    if (tid == 0) *count = (int32_t)base;
    for (int64_t e = 6 * (int64_t)base + tid; e < 6 * (int64_t)total; e += kScanThreads) targets[e] = -1.0f;
}

__global__ __launch_bounds__(kScanThreads) void k_feed_targets(const int32_t* __restrict__ rows,
                                                               const int32_t* __restrict__ scene_layer,
                                                               const int32_t* __restrict__ class_ids, int n,
                                                               int n_scenes, int per_scene, int bg_w, int bg_h,
                                                               int min_q, float* __restrict__ targets,
                                                               int32_t* __restrict__ count, int32_t* slot) {
    targets_scan<false>(rows, scene_layer, class_ids, n, n_scenes, per_scene, bg_w, bg_h, min_q, Letterbox{}, targets,
                        count, slot);
}

__global__ __launch_bounds__(kScanThreads) void k_letterbox_targets(const int32_t* __restrict__ rows,
                                                                    const int32_t* __restrict__ scene_layer,
                                                                    const int32_t* __restrict__ class_ids, int n,
                                                                    int n_scenes, int per_scene, int bg_w, int bg_h,
                                                                    int min_q, Letterbox lb,
                                                                    float* __restrict__ targets,
                                                                    int32_t* __restrict__ count, int32_t* slot) {
    targets_scan<true>(rows, scene_layer, class_ids, n, n_scenes, per_scene, bg_w, bg_h, min_q, lb, targets, count, slot);
}

// The table of scene s: entry v is 0 when v has no kept layer's bit, else 1 +
// the kept layers below its topmost kept bit.  A group is 16 bytes of a map
// row; those of columns >= bg_w become 0 whatever the map holds there.  Only
// the n_scenes·bg_h·pitch bytes of both maps are touched: group g <
// groups_per_scene = bg_h·pitch / 16 of scene s < n_scenes.
__global__ __launch_bounds__(kThreads) void k_feed_index_map(const uint8_t* __restrict__ map, int pitch, int bg_w,
                                                             uint32_t groups_per_scene, const int32_t* __restrict__ slot,
                                                             int per_scene, FastDiv tiles, FastDiv row_groups,
                                                             uint8_t* __restrict__ out) {
    __shared__ uint8_t s_idx[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t s = fdiv(blockIdx.x, tiles), tile = blockIdx.x - s * tiles.d;
    uint32_t keepmask = 0u;
    for (int k = 0; k < per_scene; ++k) keepmask |= (slot[(int64_t)s * per_scene + k] >= 0 ? 1u : 0u) << k;
    {
        const uint32_t v = tid & keepmask;
        s_idx[tid] = v == 0u ? 0u : (uint8_t)(1 + __popc(keepmask & ((1u << (31 - __clz((int)v))) - 1u)));
    }
    __syncthreads();
    const int64_t at = (int64_t)s * groups_per_scene * 16;
    const uint32_t g0 = tile * (uint32_t)kTileGroups + tid;
    uint4 v[kGroupsPerThread];
#pragma unroll
    for (int u = 0; u < kGroupsPerThread; ++u) {
        const uint32_t g = g0 + (uint32_t)(u * kThreads);
        if (g < groups_per_scene) v[u] = *reinterpret_cast<const uint4*>(map + at + 16 * (int64_t)g);
    }
#pragma unroll
    for (int u = 0; u < kGroupsPerThread; ++u) {
        const uint32_t g = g0 + (uint32_t)(u * kThreads);
        if (g >= groups_per_scene) continue;
        const int col0 = (int)(g - fdiv(g, row_groups) * row_groups.d) * 16;
        const int valid = bg_w - col0;  // bytes of the group that are columns of the background (may be <= 0)
        const uint32_t in[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i] = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t id = s_idx[(in[i] >> (8 * b)) & 0xFFu];
                w[i] |= (4 * i + b < valid ? id : 0u) << (8 * b);
            }
        }
        *reinterpret_cast<uint4*>(out + at + 16 * (int64_t)g) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

template <typename T>
void launch_images(const uint8_t* in, void* out, const void* lut, int n_scenes, uint32_t P, int bgr, uint32_t tiles,
                   hipStream_t s) {
    hipLaunchKernelGGL(k_feed_images<T>, dim3((uint32_t)n_scenes * tiles), dim3(kThreads), 0, s, in, static_cast<T*>(out),
                       static_cast<const T*>(lut), P, bgr, fast_div(tiles));
}

}  // namespace

extern "C" int ipp_scene_feed_images(const uint8_t* in, void* out, const void* lut, int32_t n_scenes, int32_t bg_w,
                                     int32_t bg_h, int32_t elem_size, int32_t bgr, void* stream) {
    if (!in || !out || !lut || n_scenes <= 0 || bg_w <= 0 || bg_h <= 0) return IPP_E_ARG;
    if ((elem_size != 2 && elem_size != 4) || (bgr != 0 && bgr != 1)) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(lut)) & (uintptr_t)(elem_size - 1)) != 0) return IPP_E_ARG;
    const int64_t P = (int64_t)bg_w * bg_h;
    if (P >= (1ll << 28)) return IPP_E_ARG;  // offsets inside a scene fit 32 bits
    const int64_t tiles = (P / kRunPixels + kTileRuns - 1) / kTileRuns > 0 ? (P / kRunPixels + kTileRuns - 1) / kTileRuns : 1;
    if (tiles * n_scenes >= INT32_MAX) return IPP_E_ARG;
    if (elem_size == 2)
        launch_images<uint16_t>(in, out, lut, n_scenes, (uint32_t)P, bgr, (uint32_t)tiles, (hipStream_t)stream);
    else
        launch_images<uint32_t>(in, out, lut, n_scenes, (uint32_t)P, bgr, (uint32_t)tiles, (hipStream_t)stream);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

// What both targets entries refuse.
static bool targets_args_ok(const int32_t* rows, const int32_t* scene_layer, const int32_t* class_ids, int32_t n_images,
                            int32_t n_scenes, int32_t per_scene, int32_t bg_w, int32_t bg_h, int32_t min_q,
                            const float* targets, const int32_t* count, const int32_t* slot) {
    if (!rows || !scene_layer || !targets || !count || !slot) return false;
    if (n_images < 0 || n_images > IPP_FEED_MAX_TARGETS || n_scenes < 1 || per_scene < 1) return false;
    if ((int64_t)n_scenes * per_scene > IPP_FEED_MAX_TARGETS) return false;
    if (bg_w < 1 || bg_h < 1 || bg_w > IPP_FEED_MAX_SIDE || bg_h > IPP_FEED_MAX_SIDE) return false;
    if (min_q < 0 || min_q > 65536) return false;
    return ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(scene_layer) |
             reinterpret_cast<uintptr_t>(class_ids) | reinterpret_cast<uintptr_t>(targets) |
             reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(slot)) & 3u) == 0;
}

extern "C" int ipp_scene_feed_targets(const int32_t* rows, const int32_t* scene_layer, const int32_t* class_ids,
                                      int32_t n_images, int32_t n_scenes, int32_t per_scene, int32_t bg_w, int32_t bg_h,
                                      int32_t min_q, float* targets, int32_t* count, int32_t* slot, void* stream) {
    if (!targets_args_ok(rows, scene_layer, class_ids, n_images, n_scenes, per_scene, bg_w, bg_h, min_q, targets, count, slot))
        return IPP_E_ARG;
    hipLaunchKernelGGL(k_feed_targets, dim3(1), dim3(kScanThreads), 0, (hipStream_t)stream, rows, scene_layer, class_ids,
                       n_images, n_scenes, per_scene, bg_w, bg_h, min_q, targets, count, slot);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

extern "C" int ipp_scene_feed_targets_letterbox(const int32_t* rows, const int32_t* scene_layer,
                                                const int32_t* class_ids, int32_t n_images, int32_t n_scenes,
                                                int32_t per_scene, int32_t bg_w, int32_t bg_h, int32_t min_q,
                                                int32_t new_w, int32_t new_h, int32_t left, int32_t top, int32_t out_w,
                                                int32_t out_h, float* targets, int32_t* count, int32_t* slot,
                                                void* stream) {
    if (!targets_args_ok(rows, scene_layer, class_ids, n_images, n_scenes, per_scene, bg_w, bg_h, min_q, targets, count, slot))
        return IPP_E_ARG;
    if (out_w < 1 || out_h < 1 || out_w > IPP_FEED_MAX_SIDE || out_h > IPP_FEED_MAX_SIDE) return IPP_E_ARG;
    if (new_w < 1 || new_h < 1 || left < 0 || top < 0 || (int64_t)left + new_w > out_w || (int64_t)top + new_h > out_h)
        return IPP_E_ARG;
    const Letterbox lb = {new_w, new_h, left, top, out_w, out_h};
    hipLaunchKernelGGL(k_letterbox_targets, dim3(1), dim3(kScanThreads), 0, (hipStream_t)stream, rows, scene_layer,
                       class_ids, n_images, n_scenes, per_scene, bg_w, bg_h, min_q, lb, targets, count, slot);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

extern "C" int ipp_scene_feed_index_map(const uint8_t* map, int64_t map_pitch, int32_t bg_w, int32_t bg_h,
                                        const int32_t* slot, int32_t n_scenes, int32_t per_scene, uint8_t* out,
                                        void* stream) {
    if (!map || !slot || !out || n_scenes < 1 || bg_w < 1 || bg_h < 1) return IPP_E_ARG;
    if (per_scene < 1 || per_scene > IPP_SCENE_MAP_MAX_LAYERS) return IPP_E_ARG;
    if (map_pitch < bg_w || (map_pitch & 15) != 0 || map_pitch > INT32_MAX) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(map) | reinterpret_cast<uintptr_t>(out)) & 15u) != 0 ||
        (reinterpret_cast<uintptr_t>(slot) & 3u) != 0)
        return IPP_E_ARG;
    const int64_t groups = (int64_t)bg_h * (map_pitch / 16);
    if (groups >= (1ll << 28)) return IPP_E_ARG;  // offsets inside a scene fit 32 bits
    const int64_t tiles = (groups + kTileGroups - 1) / kTileGroups;
    if (tiles * n_scenes >= INT32_MAX) return IPP_E_ARG;
    hipLaunchKernelGGL(k_feed_index_map, dim3((uint32_t)(n_scenes * tiles)), dim3(kThreads), 0, (hipStream_t)stream, map,
                       (int)map_pitch, bg_w, (uint32_t)groups, slot, per_scene, fast_div((uint32_t)tiles),
                       fast_div((uint32_t)(map_pitch / 16)), out);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}
