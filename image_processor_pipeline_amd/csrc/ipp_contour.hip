// Scene polygons: the outer contour of every overlay's visible pixels, traced on
// the device from the visibility maps of ipp_pipe_scene_map (ipp.h:
// ipp_scene_contours, ipp_scene_contours_pack; the definition — boundary edges
// with the foreground on their right, successor by left / straight / right,
// signed area, start edge, chosen cycle — is stated there and in DESIGN.md §3).
//
// An EDGE is (pixel (X, Y) of the foreground, kind d): 0 = top (+x), 1 = right
// (+y), 2 = bottom (-x), 3 = left (-y).  Its KEY is ((Y·bg_w + X) << 2) | d
// (below 2^32: bg_w·bg_h < 2^30), so key order is (y, x, kind) order.
//   k_contour_emit    one wave per descriptor walks its box in raster order and
//                     writes one 32-B record per edge, in key order, into the
//                     descriptor's slots [0, n_edges): the key, the successor's
//                     KEY, the corner flag and the shoelace term.  It counts
//                     every edge and stores only those below max_edges.
//   k_contour_link    per edge: the successor's slot, by binary search of its key.
//   k_contour_jump    one launch per round, ⌈log2 max_edges⌉ rounds of pointer
//                     jumping between two record arrays (below).
//   k_contour_select  per cycle leader: area2, then the descriptor's counts and
//                     its 64-bit atomicMax key (area2, inverted start slot).
//   k_contour_header  per descriptor: the header.
//   k_contour_pack    per corner edge of the chosen cycle: its vertex.
// No kernel waits on another block; the only atomics are integer max and add,
// whose results do not depend on their order.
//
// Pointer jumping on CYCLES.  After r rounds record e describes the segment
// [e, jump) of 2^r edges: jump = next^(2^r)(e); lead = the least slot of a top
// edge in the segment (kNone if it has none); sum / cnt = shoelace terms and
// corners of the whole segment; to_sum / to_cnt = those of [e, first
// occurrence of lead) (the whole segment while lead is kNone).  Joining [e, j)
// and [j, ...): the second's lead wins iff it is smaller, and then to_* = the
// first's whole sums plus the second's to_*.  A segment that has wrapped round
// its cycle already holds the cycle's least top edge, so its (then meaningless)
// whole sums are never used again.  After R rounds, 2^R >= max_edges >= any
// cycle, every record holds its cycle's leader and its sums up to the leader.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ipp.h"
#include "ipp_device.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kCorner = 0x80000000u;  // in Rec::next: the edge's tail is a corner
constexpr int kEdgeThreads = 256;
constexpr int kMinEdges = 4, kMaxEdges = 1 << 22;

struct __attribute__((aligned(16))) Rec {
    uint32_t jump;    // slot of next^(2^r)
    uint32_t lead;    // least top-edge slot of the segment, or kNone
    uint32_t to_sum;  // shoelace terms of [e, lead) (mod 2^32)
    uint32_t to_cnt;  // corners of [e, lead)
    uint32_t sum;     // shoelace terms of the whole segment
    uint32_t cnt;     // corners of the whole segment
    uint32_t key;     // the edge
    uint32_t next;    // successor's slot | kCorner (k_contour_emit leaves the successor's KEY here, the flag in cnt)
};
static_assert(sizeof(Rec) == 32, "Rec is two 16-B vectors");

// Per descriptor, at the head of the scratch.
struct __attribute__((aligned(16))) Info {
    uint32_t n_edges;  // true count
    uint32_t n_outer, n_holes;
    uint32_t leader;   // chosen cycle's start slot (k_contour_header)
    unsigned long long best;  // (area2 << 32) | ~start slot of the best outer cycle so far; 0 = none
    uint32_t bg_w;     // the divisor of the keys' pixel index (the pack call is not given it)
    uint32_t pad_;
};
static_assert(sizeof(Info) == 32, "Info");

inline int64_t info_bytes(int64_t n) { return (n * (int64_t)sizeof(Info) + 255) / 256 * 256; }
inline int rounds_of(int max_edges) {
    int r = 0;
    while ((1 << r) < max_edges) ++r;
    return r;
}

__device__ __forceinline__ Rec load_rec(const Rec* p) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    return Rec{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}
__device__ __forceinline__ void store_rec(Rec* p, const Rec& r) {
    reinterpret_cast<uint4*>(p)[0] = make_uint4(r.jump, r.lead, r.to_sum, r.to_cnt);
    reinterpret_cast<uint4*>(p)[1] = make_uint4(r.sum, r.cnt, r.key, r.next);
}

// Shoelace term x_tail·y_head − x_head·y_tail of edge (X, Y, d), mod 2^32.
__device__ __forceinline__ uint32_t edge_term(uint32_t X, uint32_t Y, uint32_t d) {
    return d == 0 ? 0u - Y : d == 1 ? X + 1u : d == 2 ? Y + 1u : 0u - X;
}

// The edges a descriptor's later kernels sweep: none when it overflowed.
__device__ __forceinline__ uint32_t live_edges(const Info* info, uint32_t i, uint32_t max_edges) {
    const uint32_t n = info[i].n_edges;
    return n > max_edges ? 0u : n;
}

__global__ __launch_bounds__(64) void k_contour_emit(const uint8_t* __restrict__ map, int64_t map_pitch, int bg_w,
                                                     int bg_h, const int32_t* __restrict__ rows,
                                                     const int32_t* __restrict__ scene_layer, int n_scenes,
                                                     int per_scene, uint32_t max_edges, Info* __restrict__ info,
                                                     Rec* __restrict__ recs) {
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const int x0 = rows[6 * i + 0], y0 = rows[6 * i + 1], x1 = rows[6 * i + 2], y1 = rows[6 * i + 3];
    const int scene = scene_layer[2 * i + 0], layer = scene_layer[2 * i + 1];
    // a box outside the map is no box (rows come from ipp_pipe_scene_map; nothing is read outside the map for any others)
    const bool ok = (unsigned)scene < (unsigned)n_scenes && (unsigned)layer < (unsigned)per_scene && x0 >= 0 &&
                    y0 >= 0 && x0 < x1 && y0 < y1 && x1 <= bg_w && y1 <= bg_h;
    uint32_t count = 0;  // wave-uniform
    if (ok) {
        const uint8_t* base = map + (int64_t)scene * bg_h * map_pitch;
        Rec* out = recs + (int64_t)i * max_edges;
        const uint64_t below = (1ull << lane) - 1ull;
        const uint64_t inner = 0x7FFFFFFFFFFFFFFEull;  // lanes 0 and 63 are the halo columns
        for (int Y = y0; Y < y1; ++Y) {
            for (int wx = x0; wx < x1; wx += 62) {
                const int X = wx - 1 + (int)lane;
                const bool in = X >= x0 && X < x1;  // outside the box is background
                const uint8_t* p = base + (int64_t)Y * map_pitch + X;
                const bool fc = in && ((p[0] >> layer) & 1);
                const bool fu = in && Y > y0 && ((p[-map_pitch] >> layer) & 1);
                const bool fd = in && Y + 1 < y1 && ((p[map_pitch] >> layer) & 1);
                const uint64_t m = __ballot(fc), up = __ballot(fu), dn = __ballot(fd);
                if (m == 0) continue;
                // bit X of (w << 1) is pixel X-1, of (w >> 1) pixel X+1
                const uint64_t ml = m << 1, mr = m >> 1, ul = up << 1, ur = up >> 1, dl = dn << 1, dr = dn >> 1;
                const uint64_t T = m & ~up & inner, R = m & ~mr & inner, B = m & ~dn & inner, L = m & ~ml & inner;
                // the tail is a corner unless the predecessor runs straight on: the pixel behind is foreground
                // and the one behind it on the outer side is not
                const uint64_t cT = T & (ul | ~ml), cR = R & (ur | ~up), cB = B & (dr | ~mr), cL = L & (dl | ~dn);
                uint32_t slot = count + __popcll(T & below) + __popcll(R & below) + __popcll(B & below) +
                                __popcll(L & below);
                const uint32_t pix = (uint32_t)Y * (uint32_t)bg_w + (uint32_t)X;
                const uint32_t W = (uint32_t)bg_w;
#pragma unroll
                for (uint32_t d = 0; d < 4; ++d) {
                    const uint64_t E = d == 0 ? T : d == 1 ? R : d == 2 ? B : L;
                    if (!((E >> lane) & 1)) continue;
                    // A = the pixel ahead on the outer side (left turn), F = the pixel ahead (straight on)
                    const uint64_t Aw = d == 0 ? ur : d == 1 ? dr : d == 2 ? dl : ul;
                    const uint64_t Fw = d == 0 ? mr : d == 1 ? dn : d == 2 ? ml : up;
                    const uint32_t pA = d == 0 ? pix + 1 - W : d == 1 ? pix + 1 + W : d == 2 ? pix - 1 + W : pix - 1 - W;
                    const uint32_t pF = d == 0 ? pix + 1 : d == 1 ? pix + W : d == 2 ? pix - 1 : pix - W;
                    uint32_t succ;
                    if ((Aw >> lane) & 1) succ = (pA << 2) | ((d + 3u) & 3u);
                    else if ((Fw >> lane) & 1) succ = (pF << 2) | d;
                    else succ = (pix << 2) | ((d + 1u) & 3u);
                    const uint64_t Cw = d == 0 ? cT : d == 1 ? cR : d == 2 ? cB : cL;
                    const uint32_t c = (uint32_t)((Cw >> lane) & 1);
                    const uint32_t term = edge_term((uint32_t)X, (uint32_t)Y, d);
                    if (slot < max_edges) {
                        Rec r;
                        r.jump = slot;  // k_contour_link
                        r.lead = d == 0 ? slot : kNone;
                        r.to_sum = d == 0 ? 0u : term;
                        r.to_cnt = d == 0 ? 0u : c;
                        r.sum = term, r.cnt = c, r.key = (pix << 2) | d, r.next = succ;
                        store_rec(out + slot, r);
                    }
                    ++slot;
                }
                count += __popcll(T) + __popcll(R) + __popcll(B) + __popcll(L);
            }
        }
    }
    if (lane == 0) {
        Info f;
        f.n_edges = count, f.n_outer = f.n_holes = 0, f.leader = 0, f.best = 0ull, f.bg_w = (uint32_t)bg_w, f.pad_ = 0;
        info[i] = f;
    }
}

// (descriptor, slot) of a thread of the per-edge kernels; false past the descriptor's edges.
__device__ __forceinline__ bool edge_of_thread(const Info* info, FastDiv per_desc, uint32_t max_edges, uint32_t& i,
                                               uint32_t& e, uint32_t& n) {
    i = fdiv(blockIdx.x, per_desc);
    e = (blockIdx.x - i * per_desc.d) * kEdgeThreads + threadIdx.x;
    n = live_edges(info, i, max_edges);
    return e < n;
}

__global__ __launch_bounds__(kEdgeThreads) void k_contour_link(const Info* __restrict__ info, Rec* recs,
                                                               FastDiv per_desc, uint32_t max_edges) {
    uint32_t i, e, n;
    if (!edge_of_thread(info, per_desc, max_edges, i, e, n)) return;
    Rec* r = recs + (int64_t)i * max_edges;
    const uint32_t want = r[e].next, c = r[e].cnt;
    uint32_t lo = 0, hi = n;  // the first slot whose key >= want
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (r[mid].key < want) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= n || r[lo].key != want) lo = e;  // (every successor is a boundary edge; a self-loop stays in bounds)
    // this thread alone writes jump and next of record e; the others read keys only
    r[e].jump = lo;
    r[e].next = lo | (c ? kCorner : 0u);
}

__global__ __launch_bounds__(kEdgeThreads) void k_contour_jump(const Info* __restrict__ info,
                                                               const Rec* __restrict__ src, Rec* __restrict__ dst,
                                                               FastDiv per_desc, uint32_t max_edges) {
    uint32_t i, e, n;
    if (!edge_of_thread(info, per_desc, max_edges, i, e, n)) return;
    const Rec* s = src + (int64_t)i * max_edges;
    Rec a = load_rec(s + e);
    const Rec b = load_rec(s + a.jump);
    if (a.lead == kNone || b.lead < a.lead) {
        a.lead = b.lead;
        a.to_sum = a.sum + b.to_sum;
        a.to_cnt = a.cnt + b.to_cnt;
    }
    a.sum += b.sum;
    a.cnt += b.cnt;
    a.jump = b.jump;
    store_rec(dst + (int64_t)i * max_edges + e, a);
}

__global__ __launch_bounds__(kEdgeThreads) void k_contour_select(Info* __restrict__ info, const Rec* __restrict__ fin,
                                                                 FastDiv per_desc, uint32_t max_edges, int bg_w) {
    uint32_t i, e, n;
    if (!edge_of_thread(info, per_desc, max_edges, i, e, n)) return;
    const Rec* r = fin + (int64_t)i * max_edges;
    const Rec a = load_rec(r + e);
    if (a.lead != e) return;  // not a start edge
    const Rec b = load_rec(r + (a.next & ~kCorner));
    const uint32_t pix = a.key >> 2, Y = pix / (uint32_t)bg_w, X = pix - Y * (uint32_t)bg_w;
    const int32_t area2 = (int32_t)(b.to_sum + edge_term(X, Y, 0));
    if (area2 > 0) {
        atomicAdd(&info[i].n_outer, 1u);
        atomicMax(&info[i].best, ((unsigned long long)(uint32_t)area2 << 32) | (uint32_t)~e);
    } else if (area2 < 0) {
        atomicAdd(&info[i].n_holes, 1u);
    }
}

__global__ __launch_bounds__(256) void k_contour_header(Info* __restrict__ info, const Rec* __restrict__ fin,
                                                        int n_images, uint32_t max_edges, int bg_w,
                                                        int32_t* __restrict__ hdr) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint32_t)n_images) return;
    const Info f = info[i];
    int32_t h[IPP_CONTOUR_HDR] = {(int32_t)f.n_edges, 0, 0, 0, 0, 0, 0, 0};
    if (f.n_edges > max_edges) {
        h[7] = 1;
    } else if (f.best != 0ull) {
        const Rec* r = fin + (int64_t)i * max_edges;
        const uint32_t e = ~(uint32_t)f.best;
        const Rec a = load_rec(r + e);
        const Rec b = load_rec(r + (a.next & ~kCorner));
        const uint32_t pix = a.key >> 2, Y = pix / (uint32_t)bg_w, X = pix - Y * (uint32_t)bg_w;
        h[1] = (int32_t)f.n_outer, h[2] = (int32_t)f.n_holes, h[3] = (int32_t)(b.to_cnt + 1u);
        h[4] = (int32_t)(uint32_t)(f.best >> 32), h[5] = (int32_t)X, h[6] = (int32_t)Y;
        info[i].leader = e;
    }
#pragma unroll
    for (int j = 0; j < IPP_CONTOUR_HDR; ++j) hdr[(int64_t)IPP_CONTOUR_HDR * i + j] = h[j];
}

__global__ __launch_bounds__(kEdgeThreads) void k_contour_pack(const Info* __restrict__ info,
                                                               const Rec* __restrict__ fin,
                                                               const int32_t* __restrict__ hdr,
                                                               const int64_t* __restrict__ offsets, FastDiv per_desc,
                                                               uint32_t max_edges, int32_t* __restrict__ verts) {
    uint32_t i, e, n;
    if (!edge_of_thread(info, per_desc, max_edges, i, e, n)) return;
    const int32_t* h = hdr + (int64_t)IPP_CONTOUR_HDR * i;
    const uint32_t nv = (uint32_t)h[3];
    if (h[3] <= 0 || h[7] != 0) return;
    const Rec a = load_rec(fin + (int64_t)i * max_edges + e);
    const uint32_t leader = info[i].leader, W = info[i].bg_w;
    if (a.lead != leader || !(a.next & kCorner)) return;
    const uint32_t pos = e == leader ? 0u : nv - a.to_cnt;  // corners of [leader, e)
    if (pos >= nv) return;
    // the edge's tail
    const uint32_t d = a.key & 3u, pix = a.key >> 2, Y = pix / W, X = pix - Y * W;
    int32_t* v = verts + 2 * (offsets[i] + (int64_t)pos);
    v[0] = (int32_t)(X + (d == 1 || d == 2 ? 1u : 0u));
    v[1] = (int32_t)(Y + (d >= 2 ? 1u : 0u));
}

// Blocks of the per-edge kernels: ⌈max_edges / 256⌉ per descriptor; 0 = the grid would overflow.
int64_t edge_blocks(int n_images, int max_edges, int& per_desc) {
    per_desc = (max_edges + kEdgeThreads - 1) / kEdgeThreads;
    const int64_t nb = (int64_t)per_desc * n_images;
    return nb >= INT32_MAX ? 0 : nb;
}

}  // namespace

extern "C" int64_t ipp_scene_contours_scratch_bytes(int32_t n_images, int32_t max_edges) {
    if (n_images < 0 || max_edges < kMinEdges || max_edges > kMaxEdges) return IPP_E_ARG;
    return info_bytes(n_images) + 2 * (int64_t)n_images * max_edges * (int64_t)sizeof(Rec);
}

extern "C" int ipp_scene_contours(const uint8_t* map, int64_t map_pitch, int32_t bg_w, int32_t bg_h,
                                  const int32_t* rows, const int32_t* scene_layer, int32_t n_images,
                                  int32_t n_scenes, int32_t per_scene, int32_t max_edges, uint8_t* scratch,
                                  int32_t* hdr, void* stream) {
    if (!map || !rows || !scene_layer || !scratch || !hdr || n_images < 0 || n_scenes < 0) return IPP_E_ARG;
    if (per_scene < 1 || per_scene > IPP_SCENE_MAP_MAX_LAYERS) return IPP_E_ARG;
    if (bg_w <= 0 || bg_h <= 0 || (int64_t)bg_w * bg_h >= (1ll << 30)) return IPP_E_ARG;  // area2 and the keys fit 32 bits
    if (map_pitch < bg_w || (map_pitch & 15) != 0 || map_pitch > INT32_MAX) return IPP_E_ARG;
    if (max_edges < kMinEdges || max_edges > kMaxEdges) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(map)) & 15u) != 0) return IPP_E_ARG;
    int per_desc = 0;
    const int64_t nb = edge_blocks(n_images, max_edges, per_desc);
    if (n_images > 0 && nb == 0) return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    hipStream_t s = (hipStream_t)stream;
    Info* info = reinterpret_cast<Info*>(scratch);
    Rec* buf[2];
    buf[0] = reinterpret_cast<Rec*>(scratch + info_bytes(n_images));
    buf[1] = buf[0] + (int64_t)n_images * max_edges;
    const FastDiv pd = fast_div((uint32_t)per_desc);
    const uint32_t me = (uint32_t)max_edges;
    hipLaunchKernelGGL(k_contour_emit, dim3((uint32_t)n_images), dim3(64), 0, s, map, map_pitch, bg_w, bg_h, rows,
                       scene_layer, n_scenes, per_scene, me, info, buf[0]);
    hipLaunchKernelGGL(k_contour_link, dim3((uint32_t)nb), dim3(kEdgeThreads), 0, s, info, buf[0], pd, me);
    const int rounds = rounds_of(max_edges);
    for (int r = 0; r < rounds; ++r)  // a round boundary is a launch boundary: no block waits on another
        hipLaunchKernelGGL(k_contour_jump, dim3((uint32_t)nb), dim3(kEdgeThreads), 0, s, info, buf[r & 1],
                           buf[(r + 1) & 1], pd, me);
    const Rec* fin = buf[rounds & 1];
    hipLaunchKernelGGL(k_contour_select, dim3((uint32_t)nb), dim3(kEdgeThreads), 0, s, info, fin, pd, me, bg_w);
    hipLaunchKernelGGL(k_contour_header, dim3((uint32_t)((n_images + 255) / 256)), dim3(256), 0, s, info, fin,
                       n_images, me, bg_w, hdr);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

extern "C" int ipp_scene_contours_pack(const uint8_t* scratch, const int32_t* hdr, const int64_t* offsets,
                                       int32_t n_images, int32_t max_edges, int32_t* verts, void* stream) {
    if (!scratch || !hdr || !offsets || !verts || n_images < 0) return IPP_E_ARG;
    if (max_edges < kMinEdges || max_edges > kMaxEdges) return IPP_E_ARG;
    if ((reinterpret_cast<uintptr_t>(scratch) & 15u) != 0) return IPP_E_ARG;
    int per_desc = 0;
    const int64_t nb = edge_blocks(n_images, max_edges, per_desc);
    if (n_images > 0 && nb == 0) return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    const Info* info = reinterpret_cast<const Info*>(scratch);
    const Rec* buf0 = reinterpret_cast<const Rec*>(scratch + info_bytes(n_images));
    const Rec* fin = buf0 + (rounds_of(max_edges) & 1) * (int64_t)n_images * max_edges;
    hipLaunchKernelGGL(k_contour_pack, dim3((uint32_t)nb), dim3(kEdgeThreads), 0, (hipStream_t)stream, info, fin,
                       hdr, offsets, fast_div((uint32_t)per_desc), (uint32_t)max_edges, verts);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}
