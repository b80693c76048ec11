// COCO run-length encoding of every overlay's visible pixels on the device,
// from the visibility maps of ipp_pipe_scene_map (ipp.h: ipp_scene_rle,
// ipp_scene_rle_pack; the definition — column-major order over the whole
// background, transitions, counts — is stated there and in DESIGN.md §3).
//
// A lane owns four adjacent columns of the background, the dword 4g .. 4g + 3
// of every map row, and a wave 256 adjacent columns: it walks the box's rows,
// so a row read is one coalesced run of up to 256 B of the map.  Of a dword
// only the bytes whose column lies in the box count; bit `layer` of each is
// the pixel.  A column's transitions are the changes of that bit down the
// column, against the rule's starting value (walk_columns), plus its closing
// transition; they are found by the same function in both passes.
//   k_rle_count  per column: its number of transitions and its last one, and
//                per lane the number of set pixels, into the scratch.
//   k_rle_scan   one workgroup per descriptor: the exclusive sum of the counts
//                (a column's first slot) and the running last transition (what
//                a column's first count is measured from), a scan through
//                shuffles and LDS over 256 columns at a time, in place; the sum
//                of the set pixels; the header.
//   k_rle_pack   walks the same columns again and stores t - prev at the
//                column's slot; the lane of the box's last column then stores
//                the closing count N - t_T.
// No kernel waits on another block and there is no atomic: every sum is taken
// in a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ipp.h"
#include "ipp_device.h"

namespace {

constexpr int kLaneCols = 4;                  // columns of a lane: one dword of a map row
constexpr int kGroupCols = 64 * kLaneCols;    // columns of a wave = of a block of the count and pack launches
constexpr int kScanThreads = 256;
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kRowsAhead = 4;                 // map rows loaded before the first is used
constexpr uint32_t kNone = 0xFFFFFFFFu;       // a column without a transition (kNone + 1 == 0 is the least of the max scan)

inline int64_t padded_cols(int bg_w) { return ((int64_t)bg_w + kLaneCols - 1) / kLaneCols * kLaneCols; }

// The three planes of the scratch, n_images rows each: cnt and last hold one
// uint32 per column (padded_cols per row), ones one per lane (a quarter).
struct Planes {
    uint32_t* cnt;   // transitions of the column; after the scan: its first slot
    uint32_t* last;  // its last transition or kNone; after the scan: the last transition before the column, or 0
    uint32_t* ones;  // set pixels of the lane's columns
};

inline Planes planes_of(uint8_t* scratch, int64_t n_images, int64_t wp) {
    uint32_t* p = reinterpret_cast<uint32_t*>(scratch);
    return Planes{p, p + n_images * wp, p + 2 * n_images * wp};
}

struct Box {
    int x0, y0, x1, y1, scene, layer;
    bool ok;
};

// A box outside the map is no box (rows come from ipp_pipe_scene_map; nothing is read outside the map for any others).
__device__ __forceinline__ Box load_box(const int32_t* __restrict__ rows, const int32_t* __restrict__ scene_layer,
                                        uint32_t i, int n_scenes, int per_scene, int bg_w, int bg_h) {
    Box b;
    b.x0 = rows[6 * (int64_t)i + 0], b.y0 = rows[6 * (int64_t)i + 1];
    b.x1 = rows[6 * (int64_t)i + 2], b.y1 = rows[6 * (int64_t)i + 3];
    b.scene = scene_layer[2 * (int64_t)i + 0], b.layer = scene_layer[2 * (int64_t)i + 1];
    b.ok = (unsigned)b.scene < (unsigned)n_scenes && (unsigned)b.layer < (unsigned)per_scene && b.x0 >= 0 &&
           b.y0 >= 0 && b.x0 < b.x1 && b.y0 < b.y1 && b.x1 <= bg_w && b.y1 <= bg_h;
    return b;
}

// True when the lane's columns X0 .. X0 + 3 meet the box.
__device__ __forceinline__ bool lane_in_box(const Box& b, int X0) { return X0 < b.x1 && X0 + kLaneCols > b.x0; }

// Every transition of the lane's four columns X0 .. X0 + 3 (X0 a multiple of 4,
// the lane meets the box): emit(c, position) for column X0 + c, in increasing
// position per column.  Returns the set pixels of the four columns.
//   start   M just before a column's first box row is 0 — the row above lies
//           outside the box, or the pixel before (X, 0) is the previous column's
//           last row, outside a box that does not span the full height — except
//           in a full-height box, where column X > x0 starts against pixel
//           (X - 1, bg_h - 1);
//   close   a column that ends set changes at X·bg_h + y1, the pixel below the
//           box or the next column's row 0: a transition unless that is N, or
//           the next column is in a full-height box and takes it as its start.
template <class Emit>
__device__ __forceinline__ uint32_t walk_columns(const uint8_t* __restrict__ base, int64_t pitch, int bg_w, int bg_h,
                                                 const Box& b, int X0, Emit&& emit) {
    const uint32_t N = (uint32_t)bg_w * (uint32_t)bg_h;
    const bool full = b.y0 == 0 && b.y1 == bg_h;
    uint32_t colmask = 0u, pm = 0u, ones = 0u;
#pragma unroll
    for (int c = 0; c < kLaneCols; ++c) {
        const int X = X0 + c;
        if (X < b.x0 || X >= b.x1) continue;
        colmask |= 1u << (8 * c);
        if (full && X > b.x0) pm |= ((uint32_t)(base[(int64_t)(bg_h - 1) * pitch + X - 1] >> b.layer) & 1u) << (8 * c);
    }
    const uint8_t* col = base + X0;  // 4-B aligned: map 16-B aligned, pitch a multiple of 16
    for (int y = b.y0; y < b.y1; y += kRowsAhead) {
        uint32_t w[kRowsAhead];
#pragma unroll
        for (int j = 0; j < kRowsAhead; ++j)
            w[j] = y + j < b.y1 ? *reinterpret_cast<const uint32_t*>(col + (int64_t)(y + j) * pitch) : 0u;
#pragma unroll
        for (int j = 0; j < kRowsAhead; ++j) {
            if (y + j >= b.y1) break;
            const uint32_t m = (w[j] >> b.layer) & 0x01010101u & colmask;
            const uint32_t ch = m ^ pm;
            pm = m;
            ones += (uint32_t)__popc(m);
            if (ch == 0u) continue;
#pragma unroll
            for (int c = 0; c < kLaneCols; ++c)
                if ((ch >> (8 * c)) & 1u) emit(c, (uint32_t)(X0 + c) * (uint32_t)bg_h + (uint32_t)(y + j));
        }
    }
#pragma unroll
    for (int c = 0; c < kLaneCols; ++c) {
        const int X = X0 + c;
        if (!((pm >> (8 * c)) & 1u) || (full && X + 1 < b.x1)) continue;  // (a set bit of pm is a column of the box)
        const uint32_t pos = (uint32_t)X * (uint32_t)bg_h + (uint32_t)b.y1;
        if (pos < N) emit(c, pos);
    }
    return ones;
}

// (descriptor, first column of the lane) of a thread of the count and pack launches.
__device__ __forceinline__ void lane_of_thread(FastDiv groups, uint32_t& i, int& X0) {
    i = fdiv(blockIdx.x, groups);
    X0 = (int)((blockIdx.x - i * groups.d) * (uint32_t)kGroupCols + threadIdx.x * (uint32_t)kLaneCols);
}

__global__ __launch_bounds__(64) void k_rle_count(const uint8_t* __restrict__ map, int64_t pitch, int bg_w, int bg_h,
                                                  const int32_t* __restrict__ rows,
                                                  const int32_t* __restrict__ scene_layer, int n_scenes,
                                                  int per_scene, FastDiv groups, int64_t wp, Planes pl) {
    uint32_t i;
    int X0;
    lane_of_thread(groups, i, X0);
    const Box b = load_box(rows, scene_layer, i, n_scenes, per_scene, bg_w, bg_h);
    if (!b.ok || !lane_in_box(b, X0)) return;
    uint32_t c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u, l0 = kNone, l1 = kNone, l2 = kNone, l3 = kNone;
    const uint32_t ones = walk_columns(map + (int64_t)b.scene * bg_h * pitch, pitch, bg_w, bg_h, b, X0,
                                       [&](int c, uint32_t pos) {
                                           if (c == 0) ++c0, l0 = pos;
                                           else if (c == 1) ++c1, l1 = pos;
                                           else if (c == 2) ++c2, l2 = pos;
                                           else ++c3, l3 = pos;
                                       });
    const int64_t at = (int64_t)i * wp + X0;  // a multiple of 4: one 16-B store per plane
    *reinterpret_cast<uint4*>(pl.cnt + at) = make_uint4(c0, c1, c2, c3);
    *reinterpret_cast<uint4*>(pl.last + at) = make_uint4(l0, l1, l2, l3);
    pl.ones[at / kLaneCols] = ones;
}

__global__ __launch_bounds__(kScanThreads) void k_rle_scan(const int32_t* __restrict__ rows,
                                                           const int32_t* __restrict__ scene_layer, int n_scenes,
                                                           int per_scene, int bg_w, int bg_h, int64_t wp, Planes pl,
                                                           int32_t* __restrict__ hdr) {
    __shared__ uint32_t s_sum[kScanWaves], s_max[kScanWaves], s_ones[kScanWaves];
    const uint32_t i = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    int32_t* h = hdr + (int64_t)IPP_RLE_HDR * i;
    const Box b = load_box(rows, scene_layer, i, n_scenes, per_scene, bg_w, bg_h);
    if (!b.ok) {  // block-uniform
        if (tid < (uint32_t)IPP_RLE_HDR) h[tid] = 0;
        return;
    }
    uint32_t* cnt = pl.cnt + (int64_t)i * wp;
    uint32_t* last = pl.last + (int64_t)i * wp;
    uint32_t base_cnt = 0u, base_last = 0u;  // of the columns before this chunk; last transitions as position + 1, 0 = none
    for (int xb = b.x0; xb < b.x1; xb += kScanThreads) {
        const int x = xb + (int)tid;
        const bool in = x < b.x1;
        const uint32_t c = in ? cnt[x] : 0u, l = in ? last[x] + 1u : 0u;
        uint32_t sc = c, sl = l;  // inclusive over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t tc = __shfl_up(sc, o), tl = __shfl_up(sl, o);
            if (lane >= (uint32_t)o) sc += tc, sl = max(sl, tl);
        }
        uint32_t el = __shfl_up(sl, 1);  // exclusive
        if (lane == 0u) el = 0u;
        if (lane == 63u) s_sum[wave] = sc, s_max[wave] = sl;
        __syncthreads();
        uint32_t pc = base_cnt, pm = base_last, tot = 0u, top = 0u;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)kScanWaves; ++k) {
            if (k < wave) pc += s_sum[k], pm = max(pm, s_max[k]);
            tot += s_sum[k], top = max(top, s_max[k]);
        }
        if (in) {
            const uint32_t before = max(pm, el);
            cnt[x] = pc + sc - c;
            last[x] = before == 0u ? 0u : before - 1u;
        }
        base_cnt += tot, base_last = max(base_last, top);
        __syncthreads();  // s_sum and s_max are rewritten by the next chunk
    }
    const uint32_t* ones = pl.ones + (int64_t)i * (wp / kLaneCols);
    uint32_t n1 = 0u;
    for (int g = b.x0 / kLaneCols + (int)tid; g < (b.x1 + kLaneCols - 1) / kLaneCols; g += kScanThreads) n1 += ones[g];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n1 += __shfl_xor(n1, o);
    if (lane == 0u) s_ones[wave] = n1;
    __syncthreads();
    if (tid == 0u) {
        uint32_t all = 0u;
#pragma unroll
        for (int k = 0; k < kScanWaves; ++k) all += s_ones[k];
        h[0] = (int32_t)(base_cnt + 1u);  // T transitions, T + 1 counts
        h[1] = (int32_t)all;
    }
}

__global__ __launch_bounds__(64) void k_rle_pack(const uint8_t* __restrict__ map, int64_t pitch, int bg_w, int bg_h,
                                                 const int32_t* __restrict__ rows,
                                                 const int32_t* __restrict__ scene_layer, int n_scenes, int per_scene,
                                                 FastDiv groups, int64_t wp, Planes pl,
                                                 const int32_t* __restrict__ hdr, const int64_t* __restrict__ offsets,
                                                 uint32_t* __restrict__ counts) {
    uint32_t i;
    int X0;
    lane_of_thread(groups, i, X0);
    const Box b = load_box(rows, scene_layer, i, n_scenes, per_scene, bg_w, bg_h);
    const int32_t nc = hdr[(int64_t)IPP_RLE_HDR * i];
    if (!b.ok || nc <= 0 || !lane_in_box(b, X0)) return;
    const uint32_t n = (uint32_t)nc;  // no slot at or past it is ever written
    const int64_t at = (int64_t)i * wp + X0;
    const uint4 off = *reinterpret_cast<const uint4*>(pl.cnt + at), pre = *reinterpret_cast<const uint4*>(pl.last + at);
    uint32_t i0 = off.x, i1 = off.y, i2 = off.z, i3 = off.w, p0 = pre.x, p1 = pre.y, p2 = pre.z, p3 = pre.w;
    uint32_t* out = counts + offsets[i];
    auto put = [&](uint32_t& slot, uint32_t& prev, uint32_t pos) {
        if (slot < n) out[slot] = pos - prev;
        prev = pos;
        ++slot;
    };
    walk_columns(map + (int64_t)b.scene * bg_h * pitch, pitch, bg_w, bg_h, b, X0, [&](int c, uint32_t pos) {
        if (c == 0) put(i0, p0, pos);
        else if (c == 1) put(i1, p1, pos);
        else if (c == 2) put(i2, p2, pos);
        else put(i3, p3, pos);
    });
    // the closing count, by the lane of the box's last column: its slot is now T and its prev t_T (0 without a transition)
    const int cl = b.x1 - 1 - X0;
    if (cl < 0 || cl >= kLaneCols) return;
    const uint32_t slot = cl == 0 ? i0 : cl == 1 ? i1 : cl == 2 ? i2 : i3;
    const uint32_t prev = cl == 0 ? p0 : cl == 1 ? p1 : cl == 2 ? p2 : p3;
    if (slot < n) out[slot] = (uint32_t)bg_w * (uint32_t)bg_h - prev;
}

// Blocks of the count and pack launches: ⌈bg_w / 256⌉ per descriptor; 0 = the grid would overflow.
int64_t lane_blocks(int n_images, int bg_w, int& groups) {
    groups = (bg_w + kGroupCols - 1) / kGroupCols;
    const int64_t nb = (int64_t)groups * n_images;
    return nb >= INT32_MAX ? 0 : nb;
}

// Everything both entries refuse; nb receives the blocks of the count / pack launch.
int check_args(const uint8_t* map, int64_t map_pitch, int32_t bg_w, int32_t bg_h, const int32_t* rows,
               const int32_t* scene_layer, int32_t n_images, int32_t n_scenes, int32_t per_scene,
               const uint8_t* scratch, const int32_t* hdr, int& groups, int64_t& nb) {
    if (!map || !rows || !scene_layer || !scratch || !hdr || n_images < 0 || n_scenes < 0) return IPP_E_ARG;
    if (per_scene < 1 || per_scene > IPP_SCENE_MAP_MAX_LAYERS) return IPP_E_ARG;
    if (bg_w <= 0 || bg_h <= 0 || (int64_t)bg_w * bg_h >= (1ll << 30)) return IPP_E_ARG;  // positions and counts fit 32 bits
    if (map_pitch < bg_w || (map_pitch & 15) != 0 || map_pitch > INT32_MAX) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(map)) & 15u) != 0) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(scene_layer) |
          reinterpret_cast<uintptr_t>(hdr)) & 3u) != 0)
        return IPP_E_ARG;
    nb = lane_blocks(n_images, bg_w, groups);
    if (n_images > 0 && nb == 0) return IPP_E_ARG;
    return IPP_OK;
}

}  // namespace

extern "C" int64_t ipp_scene_rle_scratch_bytes(int32_t n_images, int32_t bg_w) {
    if (n_images < 0 || bg_w <= 0) return IPP_E_ARG;
    return (9 * (int64_t)n_images * padded_cols(bg_w) + 255) / 256 * 256;
}

extern "C" int ipp_scene_rle(const uint8_t* map, int64_t map_pitch, int32_t bg_w, int32_t bg_h, const int32_t* rows,
                             const int32_t* scene_layer, int32_t n_images, int32_t n_scenes, int32_t per_scene,
                             uint8_t* scratch, int32_t* hdr, void* stream) {
    int groups = 0;
    int64_t nb = 0;
    const int rc = check_args(map, map_pitch, bg_w, bg_h, rows, scene_layer, n_images, n_scenes, per_scene, scratch,
                              hdr, groups, nb);
    if (rc != IPP_OK) return rc;
    if (n_images == 0) return IPP_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t wp = padded_cols(bg_w);
    const Planes pl = planes_of(scratch, n_images, wp);
    hipLaunchKernelGGL(k_rle_count, dim3((uint32_t)nb), dim3(64), 0, s, map, map_pitch, bg_w, bg_h, rows, scene_layer,
                       n_scenes, per_scene, fast_div((uint32_t)groups), wp, pl);
    hipLaunchKernelGGL(k_rle_scan, dim3((uint32_t)n_images), dim3(kScanThreads), 0, s, rows, scene_layer, n_scenes,
                       per_scene, bg_w, bg_h, wp, pl, hdr);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

extern "C" int ipp_scene_rle_pack(const uint8_t* map, int64_t map_pitch, int32_t bg_w, int32_t bg_h,
                                  const int32_t* rows, const int32_t* scene_layer, int32_t n_images, int32_t n_scenes,
                                  int32_t per_scene, const uint8_t* scratch, const int32_t* hdr,
                                  const int64_t* offsets, uint32_t* counts, void* stream) {
    int groups = 0;
    int64_t nb = 0;
    const int rc = check_args(map, map_pitch, bg_w, bg_h, rows, scene_layer, n_images, n_scenes, per_scene, scratch,
                              hdr, groups, nb);
    if (rc != IPP_OK) return rc;
    if (!offsets || !counts || (reinterpret_cast<uintptr_t>(offsets) & 7u) != 0 ||
        (reinterpret_cast<uintptr_t>(counts) & 3u) != 0)
        return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    const int64_t wp = padded_cols(bg_w);
    const Planes pl = planes_of(const_cast<uint8_t*>(scratch), n_images, wp);
    hipLaunchKernelGGL(k_rle_pack, dim3((uint32_t)nb), dim3(64), 0, (hipStream_t)stream, map, map_pitch, bg_w, bg_h,
                       rows, scene_layer, n_scenes, per_scene, fast_div((uint32_t)groups), wp, pl, hdr, offsets,
                       counts);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}
