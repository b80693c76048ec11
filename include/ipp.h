/*
 * ipp.h — C ABI of the MI355X-native image_processor_pipeline hot path.
 *
 * The reference (Tezahc/image_processor_pipeline) is pure Python: its pixel
 * arithmetic lives in Pillow's and OpenCV's C routines, called from the
 * transforms plugins.  Each entry point below replaces one of those library
 * calls (or a fused chain of them); the reference call site it stands in for
 * is cited on each declaration.  The Python host layer
 * (image_processor_pipeline_amd/) keeps the reference's plugin signatures and
 * binds these symbols with ctypes.
 *
 * Conventions
 *   - Images are HWC uint8 in caller-owned DEVICE memory; every pointer is a
 *     device pointer, every size is in bytes/pixels as named.
 *   - Batched calls take a DEVICE array of per-image descriptors, so one launch
 *     covers a ragged batch.  Nothing here allocates persistent memory: scratch
 *     is caller-provided.  All calls are asynchronous and stream-ordered on the
 *     given hipStream_t (passed as void*), reentrant, and graph-capturable.
 *   - Return value: 0 on success, a negative IPP_E* code otherwise (the Python
 *     wrappers map codes to the exceptions the reference raises).
 *   - Host-side planning helpers (ipp_plan_*) run on the CPU and fill
 *     descriptors / tap tables; they reproduce the library's host arithmetic
 *     bit-for-bit (double precision, same libm).
 */
#ifndef IPP_H
#define IPP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPP_OK 0
#define IPP_E_ARG (-1)      /* invalid argument (null pointer, bad size)      */
#define IPP_E_LAUNCH (-2)   /* HIP launch / runtime error                     */
#define IPP_E_RANGE (-3)    /* geometry outside the supported fixed-point range */

#define IPP_MAX_HSV_RANGES 16

/* ------------------------------------------------------------------------ */
/* K1+K2+K3+K4+K5: crop → RGBA → NEAREST rotate (expand) → bbox crop → flip  */
/* ------------------------------------------------------------------------ */
/* One image of the ragged batch.  The rotated canvas pixel (X, Y) reads
 *   xin = (a2 + Y*a1 + X*a0) >> 16,  yin = (a5 + Y*a4 + X*a3) >> 16
 * (int32 arithmetic, exactly Pillow Geometry.c affine_fixed) from the crop
 * window [in_x0, in_x0+in_w) × [in_y0, in_y0+in_h) of the source, or writes
 * (0,0,0,0) when (xin, yin) falls outside it.  Output pixel (x, y) is canvas
 * pixel (off_x + fx, off_y + fy) with fx = flip&1 ? out_w-1-x : x and
 * fy = flip&2 ? out_h-1-y : y.  Pillow's 0/90/180/270 fast paths are encoded
 * with exact integer coefficients by ipp_plan_rotate.                        */
typedef struct ipp_gather_desc {
    int64_t src_off;   /* byte offset of this image's source in src         */
    int64_t dst_off;   /* byte offset of this image's output in dst         */
    int32_t src_pitch; /* bytes per source row                              */
    int32_t src_cn;    /* source channels: 3 (RGB) or 4 (RGBA)              */
    int32_t src_w, src_h; /* full source dims (bounds the wide loads)       */
    int32_t in_x0, in_y0, in_w, in_h; /* crop window = image seen by rotate */
    int32_t a0, a1, a2, a3, a4, a5;   /* 16.16 inverse affine               */
    int32_t out_w, out_h;             /* output dims (after the bbox crop)  */
    int32_t off_x, off_y;             /* bbox origin inside the canvas      */
    int32_t flip;                     /* bit0: mirror x ('h'), bit1: mirror y ('v') */
    int32_t dst_pitch;                /* bytes per output row (≥ 4*out_w)   */
    /* The sampler of the fields above, filled by ipp_gather_prepare
     * (prepared = 1) so that every block of the gather kernels reads it
     * instead of recomputing it; with prepared = 0 the kernels compute it. */
    int64_t base_off;                 /* src_off + in_y0*src_pitch + in_x0*src_cn */
    uint32_t lim;                     /* last byte offset from base where a 4-byte load fits
                                         (0 when fewer than 4 bytes are left) */
    int32_t b[6];                     /* 16.16 map with the flip and bbox origin folded in:
                                         x_src = b2 + y*b1 + x*b0, y_src = b5 + y*b4 + x*b3 */
    int32_t prepared;
} ipp_gather_desc;

/* Fills the sampler fields of n host-side descriptors (same arithmetic as
 * the kernels' own, 32-bit wrap-around). */
int ipp_gather_prepare(ipp_gather_desc* descs, int32_t n);

/* rotations.py:55 convert('RGBA') + :96 rotate(angle, expand=True) + :99-101
 * getbbox()/crop(), recadrages.py:46 margin crop, symmetry.py:114-119 flip —
 * fused gather.  Writes RGBA.
 * A 3-channel pixel is read with one 4-byte load, clamped to the last dword
 * of the source (lim), and pixels outside the window read the window's
 * origin.  So for every 3-channel descriptor src must extend at least 4 bytes
 * from the window's origin, base_off + 4 <= size of src: a 1×1 window on the
 * source's last pixel (3 bytes left) needs one byte after the source.
 * device.rotate_flip_nearest launches from a longer copy in that case. */
int ipp_rotate_flip_nearest(const uint8_t* src, uint8_t* dst,
                            const ipp_gather_desc* descs, int32_t n_images,
                            int32_t max_out_w, int32_t max_out_h, void* stream);

/* Opt-in BILINEAR rotation: Pillow rotate(angle, expand=True,
 * resample=BILINEAR) of an RGB/RGBA source through RGBa (PIL/Image.py:2978-
 * 2983, Geometry.c affine_transform + bilinear_filter32RGB).  The
 * reference's rotations.py:96 is NEAREST; north_star asks for "rotations.py
 * (bilinear)" — process_rotations(..., resample="bilinear").  Output: the
 * full RGBA canvas (out_w × out_h = the expanded size) with the flip bits
 * folded into the write (bit0 mirror x, bit1 mirror y); the caller crops it
 * to its alpha bbox (ipp_alpha_bbox + ipp_copy_window).  m = Pillow's double
 * inverse matrix, and it may be any matrix: the call is
 * Image.transform((out_w, out_h), AFFINE, m, BILINEAR) of the window
 * [in_x0, in_x0+in_w) × [in_y0, in_y0+in_h), which is the whole image the
 * filter sees — neighbours are clamped to the window and a row below it is
 * never read, whatever surrounds it in src.
 * One launch takes n_images descriptors of any sizes under one max_out_w ×
 * max_out_h grid (each ≥ the largest out_w / out_h, both > 0).
 *   - Every output pixel is one aligned 4-byte store: dst must be 4-byte
 *     aligned, and dst_off and dst_pitch (≥ 4*out_w) multiples of 4.  No more
 *     is asked (not 16), and only the 4*out_w bytes of each row are written.
 *   - The source is read byte by byte: src, src_off and src_pitch
 *     (≥ in_w*src_cn) need no alignment, and no byte outside the window is
 *     read.
 *   - Empty items are allowed: out_w = 0 or out_h = 0 writes nothing, and
 *     in_w = 0 or in_h = 0 rejects every point, so the canvas is written as
 *     zeros and src is not read. */
typedef struct ipp_affine_desc {
    int64_t src_off, dst_off;         /* dst_off: multiple of 4              */
    int32_t src_pitch, src_cn;        /* cn 3 (α = 255) or 4 (RGBA)          */
    int32_t in_x0, in_y0, in_w, in_h; /* source window seen by rotate        */
    int32_t out_w, out_h, dst_pitch;  /* canvas; dst_pitch multiple of 4     */
    int32_t flip;
    double m[6];
} ipp_affine_desc;

int ipp_rotate_bilinear(const uint8_t* src, uint8_t* dst, const ipp_affine_desc* descs,
                        int32_t n_images, int32_t max_out_w, int32_t max_out_h, void* stream);

/* ------------------------------------------------------------------------ */
/* Plain 2-D window copy / flip (recadrages.py:46 slice, crop_square.py:196  */
/* slice, symmetry.py:114-119 cv2.flip codes 1/0/-1, pixels_isolés.py:81).   */
/* ------------------------------------------------------------------------ */
typedef struct ipp_copy_desc {
    int64_t src_off, dst_off;
    int32_t src_pitch, dst_pitch;
    int32_t x0, y0, w, h;   /* window in the source (pixels)               */
    int32_t cn;             /* bytes per pixel (1..4)                       */
    int32_t flip;           /* bit0 mirror x, bit1 mirror y                 */
} ipp_copy_desc;

int ipp_copy_window(const uint8_t* src, uint8_t* dst, const ipp_copy_desc* descs,
                    int32_t n_images, int32_t max_w, int32_t max_h, void* stream);

/* Crop-fit with the window taken from a DEVICE bbox array (x0, y0, x1, y1 per
 * image, as ipp_alpha_bbox / ipp_ccl_keep_largest write it) — the
 * pixels_isolés.py:74-81 `_crop_fit` slice without a host round trip.  The
 * descriptor's x0/y0/w/h are ignored; images whose bbox is empty (x0 < 0) are
 * not written.  max_w/max_h bound the windows (pixels); cn = bytes per pixel. */
int ipp_crop_to_bbox(const uint8_t* src, uint8_t* dst, const ipp_copy_desc* descs,
                     const int32_t* bbox, int32_t n_images, int32_t max_w, int32_t max_h,
                     int32_t cn, void* stream);

/* ------------------------------------------------------------------------ */
/* K6+K7: OpenCV BGR2HSV (8-bit) + inRange × R + zone AND + OR + NOT → alpha */
/* filtres_liste.py:84 imread(BGR) :90 cvtColor :97-123 inRange/zone/OR/NOT  */
/* :132-134 merge(b, g, r, alpha).                                           */
/* ------------------------------------------------------------------------ */
typedef struct ipp_hsv_range {
    int32_t lo[3], hi[3];   /* inRange bounds already prepared like cv::inRange
                               (cvRound'ed, saturated; empty → lo=1, hi=0)   */
    int32_t zone[4];        /* (top, bottom, left, right) margins; NumPy slice
                               semantics rows[top:H-bottom], cols[left:W-right] */
} ipp_hsv_range;

typedef struct ipp_hsv_params {
    int32_t n_ranges;
    int32_t bgr;            /* 1: input channel order is B,G,R (cv2); 0: R,G,B */
    ipp_hsv_range r[IPP_MAX_HSV_RANGES];
} ipp_hsv_params;

typedef struct ipp_image_desc {
    int64_t off;            /* byte offset in the buffer                    */
    int32_t w, h, pitch;    /* dims, bytes per row                          */
    int32_t cn;             /* channels                                     */
} ipp_image_desc;

/* src: 3- or 4-channel images (an input alpha is dropped, as cv2.imread
 * IMREAD_COLOR does); dst: 4-channel (same channel order + new alpha). */
int ipp_hsv_mask(const uint8_t* src, const ipp_image_desc* src_descs,
                 uint8_t* dst, const ipp_image_desc* dst_descs, int32_t n_images,
                 int32_t max_w, int32_t max_h, const ipp_hsv_params* params, void* stream);

/* ------------------------------------------------------------------------ */
/* K8: Pillow resize(LANCZOS) of RGBA — separable 8bpc passes                */
/* overlays.py:129 (PIL Image.resize → RGBa convert → ImagingResample H,V →  */
/* RGBA convert).  Taps are int32 (22-bit fixed point) from ipp_plan_lanczos. */
/* ------------------------------------------------------------------------ */
typedef struct ipp_resample_desc {
    int64_t src_off, dst_off;
    int32_t src_pitch, dst_pitch;
    int32_t in_len;         /* H pass: input width;  V pass: input height     */
    int32_t out_len;        /* H pass: output width; V pass: output height    */
    int32_t lines;          /* H pass: rows processed; V pass: columns        */
    int32_t line0;          /* H pass: first source row (ybox_first)          */
    int32_t ksize;          /* taps per output sample                         */
    int32_t pad_;
    int64_t coef_off;       /* int32 index of this image's bounds in coefs:
                               bounds[2*out_len] (xmin, count) then
                               taps[out_len*ksize]                            */
} ipp_resample_desc;

/* flags */
#define IPP_RS_PREMULTIPLY 1   /* apply rgbA2rgba on the input (H pass)      */
#define IPP_RS_UNPREMULTIPLY 2 /* apply rgba2rgbA on the output (V pass)     */

int ipp_lanczos_h(const uint8_t* src, uint8_t* dst, const int32_t* coefs,
                  const ipp_resample_desc* descs, int32_t n_images,
                  int32_t max_out, int32_t max_lines, int32_t flags, void* stream);
int ipp_lanczos_v(const uint8_t* src, uint8_t* dst, const int32_t* coefs,
                  const ipp_resample_desc* descs, int32_t n_images,
                  int32_t max_out, int32_t max_lines, int32_t flags, void* stream);

/* ------------------------------------------------------------------------ */
/* K9: background.copy() + paste(ov, (x, y), ov) onto RGB                     */
/* overlays.py:138-139 (Paste.c paste_mask_RGBA, BLEND = DIV255).             */
/* ------------------------------------------------------------------------ */
typedef struct ipp_paste_desc {
    int64_t bg_off, ov_off, dst_off;
    int32_t bg_w, bg_h, bg_pitch, dst_pitch;
    int32_t ov_w, ov_h, ov_pitch;
    int32_t x, y;           /* paste position (must fit inside the bg)        */
    int32_t pad_;
} ipp_paste_desc;

int ipp_paste_blend(const uint8_t* bg, const uint8_t* ov, uint8_t* dst,
                    const ipp_paste_desc* descs, int32_t n_images,
                    int32_t bg_w, int32_t bg_h, void* stream);

/* ------------------------------------------------------------------------ */
/* Fused 5-stage pipe (configs 3/4): crop → rotate → flip → HSV mask →        */
/* LANCZOS H pass, all computed on the fly from the source (the RGBA cut-out  */
/* is never materialised); then LANCZOS V pass → unpremultiply → paste onto   */
/* the background, fused with the background copy.                           */
/* ------------------------------------------------------------------------ */
typedef struct ipp_pipe_desc {
    ipp_gather_desc g;      /* stage 1-3 (dst fields unused)                  */
    ipp_resample_desc h;    /* H pass: src = the virtual cut-out, dst = tmp   */
    ipp_resample_desc v;    /* V pass: src = tmp                              */
    ipp_paste_desc p;       /* paste: ov = V-pass result (never stored)        */
} ipp_pipe_desc;

/* Tap format of the pipe kernels (the tiles of ipp_pipe_plan_taps).
 * The pipe kernels take IPP_TAPS_MFMA only; any other value returns
 * IPP_E_ARG. */
#define IPP_TAPS_MFMA 1   /* 16-output tiles, v_mfma_i32_16x16x64_i8          */

/* The batched 5-stage pipe as two launches (fused.PipeRunner.run, bench.py;
 * reference chain pipeline.py:526-541 → rotations.py:96, symmetry.py:114-119,
 * filtres_liste.py:84-134, overlays.py:129,138-139).  A composite's rows
 * outside the 16-row bands the overlay touches, [16⌊y/16⌋, 16⌈(y + ov_h)/16⌉),
 * are plain copies of the background (Paste.c leaves them untouched), and so
 * are, inside those bands, the 16-pixel groups outside the overlay's
 * [⌊x/16⌋, ⌈(x + ov_w)/16⌉) when the composite is dense and 16-B aligned with
 * a width that is a multiple of 16 (the "column split", one predicate in both
 * kernels):
 *   ipp_pipe_hpass_bgcopy: the LANCZOS H pass over the virtual cut-out (crop →
 *     rotate → flip → HSV α computed per pixel from the source, never stored)
 *     into the scratch `tmp`, plus the copy of those background bytes into
 *     `dst` by copy blocks that run beside the H-pass blocks: one block per
 *     row slab and group of IPP_PIPE_COPY_GROUP consecutive items, each
 *     background vector loaded once and stored to every item of the group on
 *     that background;
 *   ipp_pipe_vblend_bands: the V pass over the overlay bands, fused with the
 *     unpremultiply and the alpha blend; it writes the rest of each band: the
 *     overlay's 16-pixel groups under the column split, the whole band rows
 *     otherwise.
 * The two launches together write every composite byte exactly once: run
 * both, in this order, on the same dst (either alone leaves part of it
 * unwritten).
 * src_cn: channels of every source in the batch (3 or 4); hsv: HOST pointer;
 * tap_format: IPP_TAPS_MFMA (V axes planned with transposed = 2 + (p.y mod
 * 16), i.e. tap tiles aligned with 16-row background bands); max_ov_w /
 * max_ov_h bound the overlay sizes; ipp_pipe_vblend_bands takes overlays up
 * to IPP_PIPE_MAX_OV_W pixels wide (their 16 rows live in 64 KB of LDS;
 * fused.plan_pipe rejects wider ones before either launch runs).
 * Ring limit: the H pass keeps each 16-output tile's input window in a
 * 512-column LDS ring, so every H tile must satisfy 64·nK ≤ 512 (nK = its K
 * steps; ipp_plan_mfma_nk_bound(in, out, ksize) ≤ 8, i.e. LANCZOS downscales
 * of at most ≈ 23×; fused.plan_pipe refuses plans beyond it).  A violating
 * tile sets bit 0 of the sticky status read by ipp_pipe_status; its T columns
 * are then wrong.
 * What ipp_pipe_vblend_bands (and _bands_trim, ipp_pipe_vblend_over) reads of
 * an ipp_pipe_desc: v.src_off and v.src_pitch (the item's T in tmp, 16-B
 * aligned, pitch a multiple of 16 and ≥ 16·p.ov_w), v.out_len and v.coef_off
 * (its V tap tiles, phase p.y mod 16), h.lines (the item's T rows: loaded by
 * every launch, used with a trim table only, so the descriptor's h part must
 * be mapped) and all of p (ov_off and ov_pitch unused); nothing of g, nothing
 * else of h and v.  The bg_w / bg_h arguments bound the launch (max_ov_w ≤
 * bg_w, bands per item); each item's own p.bg_w / p.bg_h size its composite.
 * T is allocated for t_groups(rows, nkb) row groups per item
 * (csrc/ipp_pipe_layout.h): its rows past h.lines may hold anything (they
 * are read, but every tap there is zero), and so may the padding of its pitch
 * (never read).  tests/test_gpu_vblend_direct.py relies on exactly this.
 * What the H launch (ipp_pipe_hpass, ipp_pipe_hpass_bgcopy and _trim) reads of
 * an ipp_pipe_desc: of g, src_off, src_pitch, src_cn (= the src_cn argument),
 * src_h (with in_x0 / in_y0 it bounds the loads: src must hold src_h·src_pitch
 * bytes from src_off), the crop window in_x0, in_y0, in_w, in_h, the map a0..a5,
 * out_w, out_h, off_x, off_y and flip; with prepared = 1, base_off, lim and
 * b[6] stand in for src_off, the map, off_x, off_y and flip (the crop window
 * and src_h still bound the loads, out_w and out_h still size the HSV zones); of h,
 * dst_off and dst_pitch (the item's T in tmp, 16-B aligned, pitch a multiple of
 * 16 and ≥ 16·out_len), out_len, lines, line0 and coef_off (its H tap tiles:
 * phase 0, shift 0); with copy blocks all of p but ov_off and ov_pitch; nothing
 * of v, and of g neither src_w nor the dst fields, of h neither in_len nor
 * ksize.  The T bytes of an item fall in three classes:
 *   1. T rows [0, lines) × columns [0, out_len) are written and specified: row
 *      r, column x', channel c holds clip8((2^21 + Σ_j M[line0 + r][xmin + j][c]
 *      ·k_j) >> 22) ^ 0x80 at dst_off + (r / 4)·dst_pitch + 16·x' + 4·c + r % 4
 *      (with a trim table, the groups it marks constant are left unstored);
 *   2. rows [lines, 16·⌈lines / 16⌉) of the same columns are written (a block
 *      stores whole 16-B groups of its 16-row band) and may hold anything;
 *   3. no other byte of tmp is written: not the padding of the pitch past
 *      16·out_len, not the row groups from 4·⌈lines / 16⌉ on, nothing between
 *      two items' T and nothing of a descriptor outside the launch's range.
 * tests/test_gpu_hpass_direct.py relies on exactly this. */
int ipp_pipe_hpass_bgcopy(const uint8_t* src, uint8_t* tmp, const int32_t* coefs,
                          const ipp_pipe_desc* descs, int32_t n_images,
                          int32_t max_out_w, int32_t max_rows, int32_t src_cn,
                          const ipp_hsv_params* hsv, int32_t tap_format,
                          const uint8_t* bg, uint8_t* dst, void* stream);
int ipp_pipe_vblend_bands(const uint8_t* tmp, const uint8_t* bg, uint8_t* dst,
                          const int32_t* coefs, const ipp_pipe_desc* descs, int32_t n_images,
                          int32_t bg_w, int32_t bg_h, int32_t max_ov_w, int32_t max_ov_h,
                          int32_t tap_format, void* stream);

/* Reads and clears the sticky status of the pipe kernels (bit 0: ring limit
 * violated, see above).  Synchronises `stream`. */
int ipp_pipe_status(int32_t* status, void* stream);

/* After ipp_pipe_hpass_bgcopy on the same stream, before tmp is reused:
 * bbox[4*i..] = (x0, y0, x1, y1), half-open, in OVERLAY coordinates, of the
 * pixels of descriptor i's resized overlay whose alpha >= alpha_min (the alpha
 * Pillow's resize(LANCZOS) gives the RGBA overlay, i.e. the paste mask of
 * overlays.py:139); (-1,-1,-1,-1) when there is none.  1 <= alpha_min <= 255.
 * Reads tmp and coefs only. */
int ipp_pipe_overlay_bbox(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                          int32_t n_images, int32_t max_ov_w, int32_t max_ov_h,
                          int32_t alpha_min, int32_t tap_format, int32_t* bbox, void* stream);

/* The same three launches with the H launch's trim table.  Where the HSV
 * ranges exclude black and there are no zones, a 16-row band of an item's T
 * is the constant 0x80 in its leading and trailing 16-column tiles whose
 * input window holds only the rotation's fill (items of at most 64 tiles).
 * trim: device uint16[n_images][(max_rows + 15) / 16], written by the H
 * launch, one entry lo | hi << 8 per (descriptor, band): the band's other
 * tiles [lo, hi) (hi 255: no upper bound; a band that does not trim has lo 0
 * and hi = its tile count; bands past the item's rows have no entry).  With
 * a table the H launch does not store the constant 16-B groups and the V
 * launch and the box launch do not load them: tmp is then SPARSE, and only
 * these two entry points, given the same table and the same max_rows, may
 * read it (every other reader of tmp takes the T of ipp_pipe_hpass_bgcopy or
 * ipp_pipe_hpass, written in full).  A launch over a sub-range of the
 * descriptors takes trim advanced by the same number of rows as descs.
 * trim == NULL: exactly the entry points above (max_rows is ignored). */
int ipp_pipe_hpass_bgcopy_trim(const uint8_t* src, uint8_t* tmp, const int32_t* coefs,
                               const ipp_pipe_desc* descs, int32_t n_images,
                               int32_t max_out_w, int32_t max_rows, int32_t src_cn,
                               const ipp_hsv_params* hsv, int32_t tap_format,
                               const uint8_t* bg, uint8_t* dst, uint16_t* trim, void* stream);
int ipp_pipe_vblend_bands_trim(const uint8_t* tmp, const uint8_t* bg, uint8_t* dst,
                               const int32_t* coefs, const ipp_pipe_desc* descs, int32_t n_images,
                               int32_t bg_w, int32_t bg_h, int32_t max_ov_w, int32_t max_ov_h,
                               int32_t tap_format, const uint16_t* trim, int32_t max_rows,
                               void* stream);
int ipp_pipe_overlay_bbox_trim(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                               int32_t n_images, int32_t max_ov_w, int32_t max_ov_h,
                               int32_t alpha_min, int32_t tap_format, int32_t* bbox,
                               const uint16_t* trim, int32_t max_rows, void* stream);

/* ------------------------------------------------------------------------ */
/* Scenes: K overlays (layers 0 .. K-1, layer K-1 on top) pasted in layer     */
/* order onto one composite, each by paste(ov, (x, y), ov) onto the result of */
/* the layer before (fused.plan_scenes / SceneRunner).  An addition: the      */
/* reference pastes one overlay per composite.  Launch sequence for the       */
/* layer-major descriptors of a batch, all on one stream:                     */
/*   ipp_pipe_hpass_bgcopy  layer-0 descriptors (p.bg_off = the background,   */
/*                          p.dst_off = the scene's composite);               */
/*   ipp_pipe_hpass         every later layer's descriptors (one launch);     */
/*   ipp_pipe_vblend_bands  layer 0;                                          */
/*   ipp_pipe_vblend_over   once per layer 1 .. K-1, in layer order.          */
/* ------------------------------------------------------------------------ */
/* The H pass of ipp_pipe_hpass_bgcopy with no background copy: the same kernel
 * launched without copy blocks; it writes `tmp` only.  Same arguments (minus
 * bg and dst), checks and ring limit. */
int ipp_pipe_hpass(const uint8_t* src, uint8_t* tmp, const int32_t* coefs,
                   const ipp_pipe_desc* descs, int32_t n_images, int32_t max_out_w,
                   int32_t max_rows, int32_t src_cn, const ipp_hsv_params* hsv,
                   int32_t tap_format, void* stream);
/* The V pass, unpremultiply and alpha blend of ipp_pipe_vblend_bands IN PLACE
 * on `dst`: it reads the composite at p.dst_off / p.dst_pitch (p.bg_off and
 * p.bg_pitch are ignored), blends the overlay and writes the result back.  It
 * touches only the overlay's 16-pixel groups of its 16-row bands under the
 * column split (see above), the band rows otherwise; what it stores outside
 * the overlay's rectangle are the bytes it loaded there.  Every byte range is
 * loaded and stored by one thread, load first, so the result does not depend
 * on how the blocks are scheduled — PROVIDED no two descriptors of one launch
 * share a composite: two overlays of one scene must never be in the same
 * launch.  Launch it once per layer; stream order is the layer order.  Same
 * checks and IPP_PIPE_MAX_OV_W limit as ipp_pipe_vblend_bands; tmp, coefs and
 * descs must not overlap dst. */
int ipp_pipe_vblend_over(const uint8_t* tmp, uint8_t* dst, const int32_t* coefs,
                         const ipp_pipe_desc* descs, int32_t n_images, int32_t bg_w, int32_t bg_h,
                         int32_t max_ov_w, int32_t max_ov_h, int32_t tap_format, void* stream);
/* Occlusion-aware labels of scenes.  After the H launches of the batch on the
 * same stream, before tmp is reused (reads tmp and coefs, like
 * ipp_pipe_overlay_bbox).  scene_layer: device int32[n_images][2] = (scene,
 * layer) of each descriptor, 0 <= scene < n_scenes, 0 <= layer < per_scene (a
 * descriptor outside those ranges is labelled as if alone in its scene).
 * With A_k the alpha of layer k's resized overlay (its paste mask) at (x_k,
 * y_k): an overlay pixel is PRESENT iff its alpha >= alpha_min, and VISIBLE iff
 * it is present and every later layer j > k of the same scene whose rectangle
 * holds that composite pixel has A_j < cover_min there.
 * out[6*i..] = (x0, y0, x1, y1, area, visible) of descriptor i: the half-open
 * tight box of its visible pixels in COMPOSITE coordinates, (-1,-1,-1,-1) when
 * it has none; area = its present pixels, visible = its visible pixels.
 * 1 <= alpha_min, cover_min <= 255.  scratch: device, 16-B aligned,
 * ipp_pipe_scene_scratch_bytes(...) bytes = a slot table of n_scenes·per_scene
 * int32 (rounded up to 256 B) + n_images alpha planes of max_ov_h rows of
 * ⌈max_ov_w / 16⌉·16 bytes.  Descriptors larger than (max_ov_w, max_ov_h) are
 * left at (-1,-1,-1,-1, 0, 0) and hide nothing. */
int64_t ipp_pipe_scene_scratch_bytes(int32_t n_images, int32_t n_scenes, int32_t per_scene,
                                     int32_t max_ov_w, int32_t max_ov_h);
int ipp_pipe_scene_boxes(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                         const int32_t* scene_layer, int32_t n_images, int32_t n_scenes,
                         int32_t per_scene, int32_t max_ov_w, int32_t max_ov_h, int32_t alpha_min,
                         int32_t cover_min, int32_t tap_format, uint8_t* scratch, int32_t* out,
                         void* stream);
/* Instance masks of scenes: the per-pixel answer of the rule above.  The
 * VISIBILITY MAP of scene s is a uint8 image of bg_h rows of map_pitch bytes at
 * map + s * bg_h * map_pitch.  Bit k of byte (Y, X) is 1 iff layer k of scene
 * s is mapped by scene_layer and has a plane (ov_w <= max_ov_w and ov_h <=
 * max_ov_h, as for the boxes), (X, Y) lies in its rectangle clipped to the
 * bg_w x bg_h background, A_k >= alpha_min there, and every later layer j > k
 * of the scene that has a plane and whose rectangle holds (X, Y) has A_j <
 * cover_min there.  A byte may hold several bits (a faint upper layer is
 * visible and does not cover the one below); with alpha_min > cover_min a
 * pixel inside a rectangle may hold none.  Columns [bg_w, map_pitch) are 0, a
 * scene slot without a descriptor is all 0, and the launch writes EVERY byte
 * of all n_scenes slots (n_images == 0 included): the caller clears nothing.
 * Per descriptor, the number of its bits in its scene's map is `visible` of
 * ipp_pipe_scene_boxes and their bounding box is its (x0, y0, x1, y1).
 * rows: NULL, or device int32[n_images][6] that receives exactly what
 * ipp_pipe_scene_boxes writes to `out` (boxes and map from one alpha pass).
 * scratch: as for ipp_pipe_scene_boxes (ipp_pipe_scene_scratch_bytes).  map:
 * device, 16-B aligned; map_pitch >= bg_w, a multiple of 16, below 2^31.
 * 1 <= per_scene <= IPP_SCENE_MAP_MAX_LAYERS: more layers are refused
 * (IPP_E_ARG), not truncated.  Same place in the stream as the boxes: after
 * the H launches, before tmp is refilled. */
#define IPP_SCENE_MAP_MAX_LAYERS 8
int ipp_pipe_scene_map(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                       const int32_t* scene_layer, int32_t n_images, int32_t n_scenes, int32_t per_scene,
                       int32_t bg_w, int32_t bg_h, int32_t max_ov_w, int32_t max_ov_h,
                       int32_t alpha_min, int32_t cover_min, int32_t tap_format,
                       uint8_t* scratch, int32_t* rows /* may be NULL */,
                       uint8_t* map, int64_t map_pitch, void* stream);
/* Cull the overlays of scenes that the later layers leave too little of,
 * BEFORE anything is pasted: after every H launch of the batch and before the
 * first V launch, all on one stream.  A culled overlay's T (its part of tmp) is
 * overwritten with 0x80 in every byte — the T of a fully transparent overlay:
 * the V launches derive alpha 0 from it at every pixel and Paste.c's blend at
 * alpha 0 returns the background byte, DIV255(255·b + 128) = b — so the V
 * launches stay as they are (layer 0's must run anyway: it writes the band
 * bytes the H launch's copy left out), the composite is the one without the
 * overlay, and every later reader of tmp (ipp_pipe_scene_boxes,
 * ipp_pipe_scene_map and what is traced or encoded from the map) sees the
 * overlay as absent, until the next H launch rewrites its T.
 *
 * The rule, with A_k, PRESENT, scene_layer and the planes as for
 * ipp_pipe_scene_boxes; area_k = the present pixels of layer k.  The layers of
 * a scene are decided top down, k = per_scene-1, ..., 0:
 *   vis_k  = the present pixels of layer k where every KEPT later layer j > k
 *            of the scene that has a plane and whose rectangle holds the
 *            composite pixel has A_j < cover_min;
 *   keep_k = vis_k >= max(min_pixels, 1)  and  65536·vis_k >= min_q·area_k
 *            (int64), 0 <= min_q <= 65536, min_pixels >= 0.
 * keep_k depends only on the layers above k, and a culled layer hides nothing:
 * an overlay that only a culled overlay would hide is kept.  A descriptor
 * larger than (max_ov_w, max_ov_h) has no plane: it is kept, not cleared, hides
 * nothing, and its counts are 0.  A descriptor that scene_layer does not map
 * into n_scenes x per_scene is decided as if alone in its scene.  per_scene has
 * no upper limit here (one counting launch per layer).
 * cull: device int32[n_images][4] = {keep (0 or 1), area, visible, 0} of every
 * descriptor, area and visible as they were when it was decided; every word is
 * written.  The T that is cleared is what the H launch wrote of the
 * descriptor: the 16-B groups x < h.out_len of group rows g < 4·⌈h.lines/16⌉ at
 * tmp + h.dst_off + g·h.dst_pitch + 16·x, with 16-B vector stores (tmp 16-B
 * aligned); no other byte of tmp changes.  scratch: as for
 * ipp_pipe_scene_boxes.  IPP_E_ARG, before any launch: a NULL pointer, a
 * threshold outside its range, per_scene < 1, a tap_format other than
 * IPP_TAPS_MFMA, a grid of 2^31 blocks or more. */
int ipp_pipe_scene_cull(uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                        const int32_t* scene_layer, int32_t n_images, int32_t n_scenes, int32_t per_scene,
                        int32_t max_ov_w, int32_t max_ov_h, int32_t alpha_min, int32_t cover_min,
                        int32_t min_q, int32_t min_pixels, int32_t tap_format,
                        uint8_t* scratch, int32_t* cull, void* stream);
/* Amodal labels of scenes: the full extent of every overlay behind its
 * occluders, and who occludes whom.  A_k, PRESENT, VISIBLE, "has a plane"
 * (ov_w <= max_ov_w and ov_h <= max_ov_h), scene_layer and the scratch are
 * those of ipp_pipe_scene_boxes; the map layout is ipp_pipe_scene_map's.  Same
 * place in the stream as the boxes: after the H launches, before tmp is
 * refilled.  One call makes one alpha pass, whatever outputs are asked for.
 *
 * PRESENCE MAP (amap, may be NULL): n_scenes slots of bg_h rows of map_pitch
 * bytes.  Bit k of byte (Y, X) of slot s is 1 iff layer k of scene s is mapped
 * by scene_layer and has a plane, (X, Y) lies in its rectangle clipped to the
 * bg_w x bg_h background, and A_k >= alpha_min there.  Later layers play no
 * part.  Columns [bg_w, map_pitch) are 0, a slot without descriptors is all 0,
 * and EVERY byte of every slot is written (n_images == 0 included).
 *
 * AMODAL ROWS (arows, device int32[n_images][6], descriptor order): (x0, y0,
 * x1, y1, area, visible): the half-open tight box of the descriptor's PRESENT
 * pixels in composite coordinates, (-1,-1,-1,-1) when it has none; area and
 * visible are exactly those of ipp_pipe_scene_boxes.  A descriptor without a
 * plane gets (-1,-1,-1,-1, 0, 0).  area is the number of the descriptor's bits
 * in amap and the box is their bounding box.
 *
 * OCCLUSION MATRIX (occ, device int32[n_scenes][2][per_scene][per_scene]),
 * indexed by slot (scene, layer), every word written by the call:
 *   occ[s][0][k][j], COVERS, k < j: the number of composite pixels where layer
 *     k is PRESENT and layer j, which has a plane and whose rectangle holds the
 *     pixel, has A_j >= cover_min — whether or not other layers cover the
 *     pixel too.  occ[s][0][k][k] = area_k.  0 for j < k.
 *   occ[s][1][k][j], HIDES, k < j: the number of PRESENT pixels of layer k
 *     whose TOPMOST layer j' > k with A_j' >= cover_min (a plane, the rectangle
 *     holds the pixel) is j.  occ[s][1][k][k] = visible_k.  0 for j < k.
 * Each row of plane 1 partitions the present pixels: sum_{j >= k}
 * occ[s][1][k][j] = area_k; and occ[s][1][k][j] <= occ[s][0][k][j].  An empty
 * slot, a descriptor without a plane and a descriptor that scene_layer does not
 * map into n_scenes x per_scene contribute 0 everywhere; the last is labelled
 * in arows as if alone in its scene and hides nothing, as in the boxes.
 *
 * rows (may be NULL) and vmap (may be NULL) receive byte for byte what
 * ipp_pipe_scene_map writes to its `rows` and `map` with the same arguments;
 * amap and vmap share map_pitch.  With a NULL output the others are unchanged.
 * Every result is a sum, a minimum or a maximum of integers: none depends on
 * the order of the atomics.
 * 1 <= per_scene <= IPP_SCENE_MAP_MAX_LAYERS.  scratch: as for
 * ipp_pipe_scene_boxes (ipp_pipe_scene_scratch_bytes, the same table and
 * planes), 16-B aligned; amap and vmap 16-B aligned; map_pitch >= bg_w, a
 * multiple of 16, below 2^31 (checked even when both maps are NULL).
 * IPP_E_ARG, before any launch: a NULL tmp, coefs, descs, scene_layer, scratch,
 * arows or occ; a threshold outside 1..255; per_scene outside its range; a
 * pitch or an alignment as above; a tap_format other than IPP_TAPS_MFMA; a
 * grid of 2^31 blocks or more.  n_images == 0 still writes all of occ (zeros)
 * and all map slots. */
int ipp_pipe_scene_amodal(const uint8_t* tmp, const int32_t* coefs, const ipp_pipe_desc* descs,
                          const int32_t* scene_layer, int32_t n_images, int32_t n_scenes, int32_t per_scene,
                          int32_t bg_w, int32_t bg_h, int32_t max_ov_w, int32_t max_ov_h,
                          int32_t alpha_min, int32_t cover_min, int32_t tap_format, uint8_t* scratch,
                          int32_t* arows, int32_t* occ,
                          uint8_t* amap /* may be NULL */, int32_t* rows /* may be NULL */,
                          uint8_t* vmap /* may be NULL */, int64_t map_pitch, void* stream);

/* Polygons of scenes: the outer contour of each overlay's visible pixels,
 * traced on the device from the visibility maps.  map, map_pitch, rows (device
 * int32[n_images][6], descriptor order) and scene_layer are what
 * ipp_pipe_scene_map takes and writes; only the map and the rows are read (not
 * tmp), so this may run any time after the map launch on the same stream.
 *
 * For descriptor i = (scene s, layer k) the foreground F is the pixels of the
 * half-open box rows[i][0:4] whose byte in scene s's map has bit k set;
 * everything else is background.  Pixel (X, Y) is the unit square (X, Y) ..
 * (X+1, Y+1), y down.  A BOUNDARY EDGE is a unit lattice edge between a pixel
 * of F and one not in F, directed with F on its right: a foreground pixel's
 * top edge runs +x, its right edge +y, its bottom edge -x, its left edge -y.
 * The SUCCESSOR of an edge is the boundary edge leaving its head vertex, taken
 * in the order left turn (from +x: -y), straight on, right turn: foreground is
 * 8-connected and a contour crosses a saddle vertex to the diagonal pixel.
 * Every edge has one successor and one predecessor: the edges split into
 * directed cycles.  area2 of a cycle = sum over its edges of x_tail·y_head -
 * x_head·y_tail; cycles with area2 > 0 are OUTER contours (one per 8-connected
 * component, area2 / 2 = its pixels with its holes filled), those with area2 <
 * 0 HOLES (one per 4-connected background region enclosed by F).  A cycle's
 * START EDGE is its least top edge in (y, x) order (its tail is a corner).
 * The CHOSEN cycle is the outer cycle of largest area2, ties to the lesser
 * start edge.  The POLYGON is the chosen cycle's corner vertices — the tails
 * of the edges whose direction differs from their predecessor's — in
 * traversal order from the start edge's tail, not closed, a pinch vertex once
 * per pass: an even number >= 4 of lattice points in 0..bg_w x 0..bg_h.
 *
 * hdr (device int32[n_images][IPP_CONTOUR_HDR]) receives {n_edges, n_outer,
 * n_holes, n_vertices, area2, start_x, start_y, flags} per descriptor:
 * n_edges = all its boundary edges; n_vertices, area2, start_x, start_y = the
 * chosen cycle's.  A descriptor whose row is (-1,-1,-1,-1) (or whose box does
 * not lie in the map) or that scene_layer does not map into n_scenes x
 * per_scene gets all zeros.  Every word of every header is written.  A
 * descriptor with n_edges > max_edges is REFUSED, not truncated: flags bit 0
 * set, its true n_edges, every other word 0; it touches only its own scratch
 * slot.  The results do not depend on the order of any atomic.
 * scratch: device, 16-B aligned, ipp_scene_contours_scratch_bytes(n_images,
 * max_edges) bytes = 32 B per descriptor (rounded up to 256 B in all) + 2
 * arrays of n_images·max_edges edge records of 32 B (the ping-pong of the
 * list ranking: ⌈log2 max_edges⌉ launches, one per round).
 * IPP_E_ARG, before any launch: a NULL pointer; map or scratch not 16-B
 * aligned; per_scene outside 1..IPP_SCENE_MAP_MAX_LAYERS; map_pitch < bg_w or
 * not a multiple of 16; bg_w·bg_h >= 2^30 (area2 must fit int32); max_edges
 * outside 4..2^22; n_images·⌈max_edges / 256⌉ >= 2^31 - 1 (the grid).
 *
 * ipp_scene_contours_pack, after it on the same stream with the same scratch
 * and max_edges: writes descriptor i's polygon as n_vertices (x, y) int32
 * pairs at verts + 2·offsets[i] (offsets: device int64[n_images], computed by
 * the caller from the copied-back headers, e.g. the running sum of
 * n_vertices, so the packed buffer is exactly as large as the polygons).  It
 * writes nothing for a descriptor whose header has n_vertices == 0 or flags
 * != 0, and nothing else. */
#define IPP_CONTOUR_HDR 8
int64_t ipp_scene_contours_scratch_bytes(int32_t n_images, int32_t max_edges);
int ipp_scene_contours(const uint8_t* map, int64_t map_pitch, int32_t bg_w, int32_t bg_h,
                       const int32_t* rows, const int32_t* scene_layer, int32_t n_images,
                       int32_t n_scenes, int32_t per_scene, int32_t max_edges,
                       uint8_t* scratch, int32_t* hdr, void* stream);
int ipp_scene_contours_pack(const uint8_t* scratch, const int32_t* hdr, const int64_t* offsets,
                            int32_t n_images, int32_t max_edges, int32_t* verts, void* stream);

/* Simplification of the packed polygons on the device: line-distance
 * Douglas–Peucker, this project's own normative definition in exact integers.
 *
 * INPUT.  A ring P[0..n-1] of lattice points, not closed.  For traced polygons
 * this is the chosen cycle's corner vertices, P[0] being the start vertex.
 * Let P[n] = P[0].
 * TOLERANCE.  eps_q is an integer in quarter pixels, eps = eps_q / 4, with
 * 1 <= eps_q <= 4096.
 * OVERFLOW BOUNDS.  All arithmetic is exact integer.  Coordinates must lie in
 * 0..16384 on both axes: the entry takes bg_w and bg_h and returns IPP_E_ARG
 * when either exceeds 16384.  With those bounds |cross| <= 2^28, 16·cross² <=
 * 2^60 and eps_q²·len² <= 2^53, so 64-bit unsigned arithmetic suffices (a
 * measure fits 32 bits).  The coordinate range is the CALLER'S CONTRACT: bg_w
 * and bg_h are checked, the vertices (device data) are not.  Vertices outside
 * 0..16384 give an unspecified selection (the LDS path packs x and y into 16
 * bits each), but no access outside the rings, the scratch and counts.
 * ANCHORS.  A = 0.  B is the index in 1..n-1 with the largest squared
 * Euclidean distance from P[0], ties to the least index.  Both anchors are
 * kept.  The two chains are indices A..B and B..n.
 * SPLIT of a segment (a, b), b > a + 1.  For each interior j, cross_j =
 * (P[b]-P[a]) × (P[j]-P[a]) and len2 = |P[b]-P[a]|².  The measure m_j is
 * |cross_j| when len2 > 0; when len2 = 0 it is |P[j]-P[a]|² (a pinch vertex
 * visited twice).  The candidate is the j of largest m_j, ties to the least
 * j.  It is kept, and both halves (a, j) and (j, b) are split in turn, iff
 * 16·cross_j² > eps_q²·len2; when len2 = 0 the condition is 16·m_j > eps_q².
 * Otherwise every interior vertex of the segment is dropped.
 * AT LEAST A TRIANGLE.  If only A and B are kept after both chains, the vertex
 * of largest |cross| against (A, B) over the whole ring is also kept, ties to
 * the least index, provided that value is non-zero.  A traced polygon has
 * positive area, so it always ends with at least 3 vertices.
 * OUTPUT.  The kept vertices in ring order from P[0].  A ring with n < 3 is
 * returned whole.
 * EQUIVALENCE.  Each segment's split depends on that segment alone, so "split
 * every open segment once per round until none is open" gives exactly the
 * recursive result; the device works level by level.
 *
 * ipp_polygons_simplify: verts, offsets and hdr are exactly what
 * ipp_scene_contours_pack took and wrote (ring i = hdr[i].n_vertices pairs at
 * verts + 2·offsets[i]); it runs on the same stream after the pack.  The rings
 * must be disjoint and lie below total_vertices: offsets[i] + n_vertices <=
 * total_vertices (the scratch is indexed like verts).  counts (device
 * int32[n_images]) receives the kept vertices of every descriptor, 0 where the
 * header has n_vertices == 0 or flags != 0; every word of counts is written.
 * Each vertex's keep mark is left in the scratch: uint32 at scratch + 4·(
 * offsets[i] + j), 0 = dropped, else 1 + its position among the ring's kept.
 * One workgroup per ring; a ring of at most IPP_SIMPLIFY_LDS_VERTS vertices
 * keeps its state in LDS, a longer one (the tracer emits up to max_edges) runs
 * the same rounds on the scratch: never refused, never truncated.  The only
 * atomics are integer max: the results do not depend on their order.
 * scratch: device, 16-B aligned, ipp_polygons_simplify_scratch_bytes(n_images,
 * total_vertices) = 4·total_vertices rounded up to 256 B (the marks) + 16 B
 * per vertex (the long rings' slot, a and b arrays).
 * ipp_polygons_simplify_pack, after it on the same stream with the same
 * arguments: writes descriptor i's kept vertices, in order, as counts[i] int32
 * pairs at out + 2·out_offsets[i] (out_offsets: device int64[n_images], computed
 * by the caller from the copied-back counts, so the final buffer is exactly as
 * large as the simplified polygons), and nothing else.
 * IPP_E_ARG, before any launch: a NULL pointer; scratch not 16-B, offsets or
 * out_offsets not 8-B, another pointer not 4-B aligned; eps_q outside 1..4096;
 * bg_w or bg_h outside 1..16384; n_images or total_vertices negative;
 * n_images >= 2^24 (the grid: 256 threads per ring below 2^32 threads);
 * total_vertices > 2^40. */
#define IPP_SIMPLIFY_LDS_VERTS 2048
#define IPP_SIMPLIFY_THREADS 256 /* threads of a ring's workgroup: thread t owns vertices t, t + 256, ... */
int64_t ipp_polygons_simplify_scratch_bytes(int32_t n_images, int64_t total_vertices);
int ipp_polygons_simplify(const int32_t* verts, const int64_t* offsets, const int32_t* hdr, int32_t n_images,
                          int64_t total_vertices, int32_t bg_w, int32_t bg_h, int32_t eps_q, uint8_t* scratch,
                          int32_t* counts, void* stream);
int ipp_polygons_simplify_pack(const int32_t* verts, const int64_t* offsets, const int32_t* hdr,
                               const uint8_t* scratch, const int32_t* counts, const int64_t* out_offsets,
                               int32_t n_images, int32_t* out, void* stream);

/* Oriented boxes (YOLO-OBB) of the packed polygons on the device: the
 * minimum-area enclosing rectangle of each ring, this project's own normative
 * definition in exact integers.
 *
 * INPUT.  A ring P[0..n-1] of lattice points with both coordinates in
 * 0..16384; for traced polygons exactly what ipp_scene_contours_pack wrote.
 * The result depends on the POINT SET only, not on the order of the points:
 * pinch vertices, repeated points and self-crossing rings are legal input.
 * With cross(u, v) = ux·vy − uy·vx:
 * HULL.  H[0..m-1] are the vertices of the strictly convex hull (no hull
 * vertex lies on the segment between two others).  H[0] is the point least in
 * (y, x) order; the others follow so that cross(H[e+1]−H[e], H[e+2]−H[e+1]) >
 * 0, indices mod m.  With y down this leaves H[0] towards +x: clockwise on the
 * screen, the direction in which the tracer walks an outer contour.  m = 1
 * when all points coincide, m = 2 when they are collinear.
 * EDGE e (0 <= e < m, m >= 3).  a = H[e], d = H[(e+1) mod m] − a, nn = dx² +
 * dy².  For every point p: t = dx·(px−ax) + dy·(py−ay) and s = −dy·(px−ax) +
 * dx·(py−ay); every s is >= 0 (the interior is on the right).  lo = min t (<=
 * 0), hi = max t (>= nn), hgt = max s.  The rectangle on edge e has area
 * (hi−lo)·hgt / nn.
 * CHOICE.  The edge of least area, compared exactly: e1 beats e2 iff
 * (hi1−lo1)·hgt1·nn2 < (hi2−lo2)·hgt2·nn1; ties go to the lesser e.
 * OVERFLOW BOUNDS.  |t| <= 2^29, hi−lo <= 2^30, hgt <= 2^29, nn <= 2^29: every
 * record word fits int32, (hi−lo)·hgt <= 2^59 fits 64 bits, and the compared
 * products reach 2^88: the comparison is 128-bit (no division anywhere).
 * RECORD.  IPP_OBB_REC int32 words {ax, ay, dx, dy, lo, hi, hgt, m} of the
 * chosen edge.  m = 2: e = 0, lo = 0, hi = nn, hgt = 0.  m = 1: {ax, ay, 0, 0,
 * 0, 0, 0, 1}.
 * CORNERS (host, float64, part of the rule).  C(t, s) = (ax + (t·dx − s·dy) /
 * nn, ay + (t·dy + s·dx) / nn), evaluated in exactly that operation order, for
 * (lo, 0), (hi, 0), (hi, hgt), (lo, hgt) in this order.  They are NOT clipped
 * to the image: the rectangle of an object at the border may leave it.
 *
 * ipp_polygons_obb: verts, offsets, hdr and total_vertices are exactly what
 * ipp_polygons_simplify takes (ring i = hdr[i].n_vertices pairs at verts +
 * 2·offsets[i], the rings disjoint and below total_vertices); it runs on the
 * same stream after ipp_scene_contours_pack and is independent of the simplify
 * entries (it reads the unsimplified ring).  obb (device int32[n_images][
 * IPP_OBB_REC]) receives one record per descriptor, all eight words 0 where
 * the header has n_vertices == 0 or flags != 0; every word of every record is
 * written and nothing else is, but the ring's own slots of the scratch (below).
 * The coordinate range is the CALLER'S CONTRACT: bg_w and bg_h are checked,
 * the vertices (device data) are not.  Vertices outside 0..16384 give an
 * unspecified record (they are clamped on load), but no access outside the
 * rings, the scratch and the records.
 * One workgroup of IPP_OBB_THREADS threads per ring, any n_vertices (the
 * tracer emits up to max_edges = 2^22): never refused, never truncated.  It
 * reduces the ring to the least and greatest x of each lattice row, a window
 * of IPP_OBB_LDS_ROWS rows at a time in LDS (a ring spanning more rows sweeps
 * its vertices once per window), and extends the hull's right and left
 * monotone chains after each window.  The first IPP_OBB_LDS_HULL points of
 * each chain live in LDS, later ones in the scratch; the rectangle search runs
 * over the hull alone.  The only atomics are integer min and max: the result
 * does not depend on their order.
 * scratch: device, 16-B aligned, ipp_polygons_obb_scratch_bytes(n_images,
 * total_vertices) = 8·total_vertices rounded up to 256 B: uint32 slots
 * offsets[i] .. offsets[i] + n_vertices − 1 for ring i's right chain and the
 * same slots + total_vertices for its left chain.  A chain of at most
 * IPP_OBB_LDS_HULL points (so every ring of at most that many vertices)
 * touches none of them; what a longer chain leaves in its ring's slots is
 * unspecified.
 * IPP_E_ARG, before any launch: a NULL pointer; scratch not 16-B, offsets not
 * 8-B, another pointer not 4-B aligned; bg_w or bg_h outside 1..16384;
 * n_images or total_vertices negative; n_images >= 2^24 (the grid);
 * total_vertices > 2^40.  n_images == 0 is IPP_OK and launches nothing. */
#define IPP_OBB_REC 8
#define IPP_OBB_LDS_ROWS 2048 /* lattice rows of one window of the row reduction */
#define IPP_OBB_LDS_HULL 512  /* points of each monotone chain kept in LDS */
#define IPP_OBB_THREADS 256   /* threads of a ring's workgroup: thread t owns vertices and hull edges t, t + 256, ... */
int64_t ipp_polygons_obb_scratch_bytes(int32_t n_images, int64_t total_vertices);
int ipp_polygons_obb(const int32_t* verts, const int64_t* offsets, const int32_t* hdr, int32_t n_images,
                     int64_t total_vertices, int32_t bg_w, int32_t bg_h, uint8_t* scratch,
                     int32_t* obb /* [n_images][IPP_OBB_REC] */, void* stream);

/* COCO run-length encoding of scenes: the exact mask of each overlay's visible
 * pixels — every part, every hole — as the COCO API's uncompressed RLE of the
 * bg_h x bg_w mask, encoded on the device from the visibility maps.  map,
 * map_pitch, rows (device int32[n_images][6], descriptor order) and
 * scene_layer are what ipp_pipe_scene_map takes and writes; only the map and
 * the rows are read (not tmp), so these entries may run any time after the map
 * launch on the same stream.  This project's normative definition, in exact
 * integers:
 *
 * FOREGROUND.  For descriptor i = (scene s, layer k), F is what
 * ipp_scene_contours calls the foreground: the pixels of the half-open box
 * rows[i][0:4] whose byte in scene s's map has bit k set.
 * ORDER.  Pixels are ordered column-major over the whole background: pixel (X,
 * Y) has position p = X·bg_h + Y, and N = bg_w·bg_h.
 * TRANSITIONS.  With M(p) = 1 iff p is in F, and M(-1) = 0, the transitions
 * are the positions t_1 < ... < t_T in [0, N) with M(p) != M(p-1).
 * COUNTS.  t_1, t_2 - t_1, ..., t_T - t_(T-1), N - t_T: T + 1 counts that
 * alternate zeros-run, ones-run, starting with a zeros-run (the first count is
 * 0 when pixel (0, 0) is in F), and sum to N.  A box without a set bit gives
 * the single count N.  Runs continue across columns: the last row of column X
 * and the first of column X + 1 are neighbours.
 * CROSS-CHECKS.  The ones-runs (counts 1, 3, ...) sum to `visible` of
 * ipp_pipe_scene_boxes; the mask's bounding box is the row's box.
 *
 * ipp_scene_rle: hdr (device int32[n_images][IPP_RLE_HDR]) receives {n_counts,
 * n_ones} per descriptor: n_counts = T + 1, n_ones = the sum of the ones-runs.
 * A descriptor whose row is (-1,-1,-1,-1) (or whose box does not lie in the
 * map) or that scene_layer does not map into n_scenes x per_scene gets {0, 0}.
 * Every word of every header is written.
 * ipp_scene_rle_pack, after it on the same stream with the same arguments and
 * scratch: writes descriptor i's n_counts counts as uint32 at counts +
 * offsets[i] (offsets: device int64[n_images], computed by the caller from the
 * copied-back headers, e.g. the running sum of n_counts, so the packed buffer
 * is exactly as large as the encodings).  It writes nothing for a descriptor
 * whose header has n_counts == 0, and nothing else anywhere.
 * One lane per four adjacent columns (one dword of a map row), 256 columns per
 * 64-thread block, ⌈bg_w / 256⌉ blocks per descriptor; those outside the box
 * (known only on the device) exit at once.  The map is read inside the boxes
 * only, once per entry.  There is no atomic: nothing depends on any order.
 * scratch: device, 16-B aligned, ipp_scene_rle_scratch_bytes(n_images, bg_w) =
 * 9·n_images·(4·⌈bg_w / 4⌉) rounded up to 256 B: per descriptor and column a
 * uint32 transition count and a uint32 last transition (after the scan: the
 * column's first slot and the last transition before it), and per four columns
 * a uint32 number of set pixels.
 * IPP_E_ARG, before any launch: a NULL pointer; map or scratch not 16-B
 * aligned, offsets not 8-B, another pointer not 4-B aligned; per_scene outside
 * 1..IPP_SCENE_MAP_MAX_LAYERS; map_pitch < bg_w, not a multiple of 16 or >=
 * 2^31; bg_w or bg_h < 1; bg_w·bg_h >= 2^30 (positions and counts fit 32 bits
 * with room); n_images or n_scenes negative; n_images·⌈bg_w / 256⌉ >= 2^31 - 1
 * (the grid).  n_images == 0 is IPP_OK, launches and writes nothing. */
#define IPP_RLE_HDR 2
int64_t ipp_scene_rle_scratch_bytes(int32_t n_images, int32_t bg_w);
int ipp_scene_rle(const uint8_t* map, int64_t map_pitch, int32_t bg_w, int32_t bg_h,
                  const int32_t* rows, const int32_t* scene_layer, int32_t n_images,
                  int32_t n_scenes, int32_t per_scene, uint8_t* scratch, int32_t* hdr, void* stream);
int ipp_scene_rle_pack(const uint8_t* map, int64_t map_pitch, int32_t bg_w, int32_t bg_h,
                       const int32_t* rows, const int32_t* scene_layer, int32_t n_images,
                       int32_t n_scenes, int32_t per_scene, const uint8_t* scratch, const int32_t* hdr,
                       const int64_t* offsets, uint32_t* counts, void* stream);
/* Training batches left on the device: what a detector's loss takes, made from
 * the composites and the device rows of a box, map or amodal launch without a
 * copy back.  The three entries read no tmp: they may run any time after the
 * launches that wrote their inputs, on the same stream.
 *
 * ipp_scene_feed_images: in = the composites, n_scenes x bg_h x bg_w x 3
 * contiguous uint8 (what the V launches write); out = n_scenes x 3 x bg_h x
 * bg_w contiguous elements of elem_size bytes (2 or 4):
 *   out[s][c][y][x] = lut[c][ in[s][y][x][ch(c)] ],  ch(c) = c, or 2 - c with bgr = 1.
 * lut: device, 3 x 256 elements of elem_size bytes, copied as opaque words:
 * whatever float format and per-channel curve the caller tabulated comes out
 * bit for bit, and no float arithmetic runs on the device.  The table is kept
 * in LDS; a scene is a flat stream of bg_w·bg_h pixels on both sides, a lane
 * takes 16 pixels (three 16-B loads, 16-B stores per plane).  Nothing is
 * assumed of the alignment of `in` (any byte address) or of a scene's slot: up
 * to 15 pixels before the first 16-B boundary of a scene's bytes and fewer
 * than 16 after its last full run go one by one, and a plane that does not
 * start 16-B aligned behind them takes unaligned 16-B stores.  No byte
 * outside the n_scenes·bg_h·bg_w·3 of `in` is read, none outside `out` written.
 * IPP_E_ARG, before any launch: a NULL pointer; n_scenes, bg_w or bg_h < 1;
 * elem_size other than 2 or 4; bgr other than 0 or 1; out or lut not aligned
 * to elem_size; bg_w·bg_h >= 2^28; n_scenes·⌈bg_w·bg_h / 16384⌉ >= 2^31 - 1.
 *
 * ipp_scene_feed_targets: rows = device int32[n_images][6] (x0, y0, x1, y1,
 * area, visible) in descriptor order, exactly what ipp_pipe_scene_boxes,
 * ipp_pipe_scene_map or ipp_pipe_scene_amodal wrote; scene_layer as there;
 * class_ids = device int32[n_images] by descriptor, or NULL for class 0.  With
 * T = n_scenes·per_scene and overlay q = scene·per_scene + layer:
 *   DESCRIPTOR of q: the highest d < n_images with scene_layer[d] = (scene,
 *     layer) (plan_scenes maps every q exactly once); none: q is absent.
 *   KEPT: q has a descriptor, visible > 0 and 65536·visible >= min_q·area in
 *     int64 (ipp_pipe_scene_cull's fraction test), 0 <= min_q <= 65536.
 *   ORDER: the kept overlays in increasing q (scene, layer order), compacted:
 *     slot[q] = the number of kept overlays before q, or -1 when q is not kept;
 *     *count = the number of kept overlays.
 *   ROW slot[q] of targets (float32[T][6]) = (scene, class, cx, cy, w, h),
 *     cx = float(x0 + x1) / float(2·bg_w), w = float(x1 - x0) / float(bg_w), cy
 *     and h alike with y and bg_h: each ONE correctly rounded float32 division.
 *     bg_w, bg_h <= IPP_FEED_MAX_SIDE = 2^23 guarantees that both operands are
 *     integers of at most 2^24, which float32 holds exactly, for every box
 *     inside the background (0 <= x0 < x1 <= bg_w); larger sides are refused.
 *     scene and class are converted to float32 (exact below 2^24).
 *   Rows count .. T-1 are -1 in all six elements.  EVERY element of targets
 *   and slot and *count are written: `targets[:, 0] >= 0` masks the rows
 *   without reading count.
 * One workgroup of 1024 threads: it inverts the permutation into slot (an
 * integer max, the same in any order), then sweeps the T overlays in chunks of
 * 1024 with a carried prefix.  No float atomic, nothing depends on an order.
 * IPP_E_ARG, before any launch: a NULL pointer other than class_ids; a pointer
 * not 4-B aligned; n_images < 0; n_scenes or per_scene < 1; n_images or T >
 * IPP_FEED_MAX_TARGETS; bg_w or bg_h outside 1..IPP_FEED_MAX_SIDE; min_q
 * outside 0..65536.
 *
 * ipp_scene_feed_index_map: map = the visibility maps of ipp_pipe_scene_map
 * (n_scenes slots of bg_h rows of map_pitch bytes), slot = what
 * ipp_scene_feed_targets wrote for the same scenes.  out has the map's layout.
 * For byte v at (Y, X < bg_w) of scene s, with keepmask_s = the bits k with
 * slot[s·per_scene + k] >= 0 and v' = v & keepmask_s:
 *   out = 0 when v' == 0, else 1 + the number of bits of keepmask_s below the
 *   topmost set bit of v': 1 + the row, within the scene's run of targets, of
 *   the topmost kept layer visible there.
 * Columns [bg_w, map_pitch) of out are 0 whatever the map holds there; every
 * byte of all n_scenes slots is written.  A 256-entry table per scene in LDS;
 * 16-B loads and stores.
 * IPP_E_ARG, before any launch: a NULL pointer; map or out not 16-B, slot not
 * 4-B aligned; n_scenes, bg_w or bg_h < 1; per_scene outside
 * 1..IPP_SCENE_MAP_MAX_LAYERS; map_pitch < bg_w, not a multiple of 16 or >=
 * 2^31; bg_h·map_pitch >= 2^32; n_scenes·⌈bg_h·map_pitch / 16384⌉ >= 2^31 - 1. */
#define IPP_FEED_MAX_SIDE 8388608
#define IPP_FEED_MAX_TARGETS 1048576
int ipp_scene_feed_images(const uint8_t* in, void* out, const void* lut, int32_t n_scenes,
                          int32_t bg_w, int32_t bg_h, int32_t elem_size, int32_t bgr, void* stream);
int ipp_scene_feed_targets(const int32_t* rows, const int32_t* scene_layer,
                           const int32_t* class_ids /* may be NULL */, int32_t n_images,
                           int32_t n_scenes, int32_t per_scene, int32_t bg_w, int32_t bg_h,
                           int32_t min_q, float* targets, int32_t* count, int32_t* slot, void* stream);
int ipp_scene_feed_index_map(const uint8_t* map, int64_t map_pitch, int32_t bg_w, int32_t bg_h,
                             const int32_t* slot, int32_t n_scenes, int32_t per_scene, uint8_t* out,
                             void* stream);
/* The same batch at the network's input size: the composites resized on the
 * device exactly as Pillow's Image.resize((out_w, out_h), filter) resizes an
 * RGB image (Resample.c, 8 bits per channel), then the table.
 *
 * ipp_scene_feed_resize: in, lut, elem_size, bgr as for ipp_scene_feed_images;
 * out = n_scenes x 3 x out_h x out_w contiguous elements.  taps_x, taps_y:
 * device int32 tables of ipp_plan_resample for (bg_w -> out_w) and (bg_h ->
 * out_h) with ksize_x and ksize_y, or geometry.identity_taps (ksize 1) for an
 * axis whose sizes are equal (Pillow skips that pass; the identity taps
 * reproduce the input).  With (xmin, n) = the bounds of an output and k its taps:
 *   H FIRST:  t[y][xo][c] = clip8((2^21 + sum_k in[s][y][xmin + k][c] * kx[xo][k]) >> 22),
 *             stored as uint8: rounded and clipped BEFORE the vertical pass;
 *   THEN V:   r[yo][xo][c] = clip8((2^21 + sum_k t[ymin + k][xo][c] * ky[yo][k]) >> 22);
 *   THEN THE TABLE: out[s][c][yo][xo] = lut[c][ r[yo][xo][ch(c)] ], ch(c) = c, or
 *             2 - c with bgr = 1; the table's words are copied as opaque words.
 * clip8(v) = min(max(v, 0), 255) with an arithmetic shift; the sums are int32
 * as in Pillow.  No float arithmetic runs on the device.
 * One workgroup of 256 threads per (scene, tile of tw x th outputs).  The
 * table, the tile's bounds and taps, the source span of the tile's windows
 * (fetched in aligned dwords; a scene's slot and a row may start at any byte)
 * and the uint8 intermediate live in LDS; a wave stores 64 consecutive
 * elements of one plane row.  The LDS extents follow from (bg, out, ksize,
 * elem_size) alone: a run of n outputs touches fewer than (n - 1)·in/out +
 * ksize + 1 source positions.  The tile is 64 x 32, each side halved (the one
 * whose halving leaves fewer bytes, the height on a tie) until the extents fit
 * IPP_FEED_RESIZE_LDS_BYTES = 64 KiB, so that two workgroups share a CU's LDS.
 * ipp_scene_feed_resize_lds returns those bytes and the tile (tile[0] = tw,
 * tile[1] = th; tile may be NULL).  It is host code and needs no device: it
 * exists for planning (what a geometry will cost before any launch) and for
 * testing (the extents are dynamic LDS, which a kernel's metadata does not
 * show; tests/test_feed_resize_cpu.py sweeps them through it); no launch needs
 * a call to it.
 * IPP_FEED_RESIZE_MAX_KSIZE = 128 is the largest ksize of either axis: up to it
 * even the 1 x 1 tile of the most reducing filter fits the budget (a ksize_y x
 * ksize_x span at 129 x 392 B, 57 KiB in all).  LANCZOS reaches it at a 21x
 * reduction, BILINEAR at 63x.  A larger ksize is refused, never truncated.
 * Every window is clamped to its axis and to the staged span, so whatever the
 * tables hold no byte outside the n_scenes·bg_h·bg_w·3 of `in` is read and none
 * outside `out` written (tables that are not ipp_plan_resample's give pixels
 * this rule does not state).
 * IPP_E_ARG, before any launch: a NULL pointer; n_scenes, bg_w, bg_h, out_w or
 * out_h < 1; elem_size other than 2 or 4; bgr other than 0 or 1; out or lut not
 * aligned to elem_size, taps_x or taps_y not 4-B aligned; ksize_x or ksize_y
 * outside 1..IPP_FEED_RESIZE_MAX_KSIZE; bg_w·bg_h or out_w·out_h >= 2^28;
 * n_scenes·tiles >= 2^31 - 1 (the grid).  ipp_scene_feed_resize_lds returns
 * IPP_E_ARG for the same sizes.
 *
 * ipp_scene_feed_index_map_sampled: ipp_scene_feed_index_map at the output
 * size, as Pillow's NEAREST resize of the full-size index map (Geometry.c
 * ImagingScaleAffine): xtab = device int32[out_w] with xtab[x] = int(o), o
 * starting at 0.5·(bg_w / out_w) and advanced by REPEATED ADDITION of bg_w /
 * out_w in double; ytab alike (geometry.nearest_table).  With f the per-scene
 * rule of ipp_scene_feed_index_map:
 *   out[s][y][x] = f(map[s][ytab[y]][xtab[x]])   for x < out_w,
 * in n_scenes slots of out_h rows of out_pitch bytes; columns [out_w,
 * out_pitch) are 0 and every byte of all slots is written.  The map is read at
 * the sampled positions only (coordinates are clamped into it).
 * IPP_E_ARG, before any launch: a NULL pointer; out not 16-B, slot, xtab or
 * ytab not 4-B aligned; n_scenes, bg_w, bg_h, out_w or out_h < 1; per_scene
 * outside 1..IPP_SCENE_MAP_MAX_LAYERS; map_pitch < bg_w or >= 2^31; out_pitch <
 * out_w, not a multiple of 16 or >= 2^31; bg_h·map_pitch >= 2^32; out_h·
 * out_pitch >= 2^32; n_scenes·⌈out_h·out_pitch / 16384⌉ >= 2^31 - 1. */
#define IPP_FEED_RESIZE_MAX_KSIZE 128
#define IPP_FEED_RESIZE_LDS_BYTES 65536
int ipp_scene_feed_resize(const uint8_t* in, void* out, const void* lut, const int32_t* taps_x,
                          const int32_t* taps_y, int32_t n_scenes, int32_t bg_w, int32_t bg_h,
                          int32_t out_w, int32_t out_h, int32_t ksize_x, int32_t ksize_y,
                          int32_t elem_size, int32_t bgr, void* stream);
int64_t ipp_scene_feed_resize_lds(int32_t bg_w, int32_t bg_h, int32_t out_w, int32_t out_h,
                                  int32_t ksize_x, int32_t ksize_y, int32_t elem_size,
                                  int32_t* tile /* may be NULL */);
int ipp_scene_feed_index_map_sampled(const uint8_t* map, int64_t map_pitch, int32_t bg_w,
                                     int32_t bg_h, const int32_t* slot, int32_t n_scenes,
                                     int32_t per_scene, const int32_t* xtab, const int32_t* ytab,
                                     int32_t out_w, int32_t out_h, uint8_t* out, int64_t out_pitch,
                                     void* stream);
/* The same batch letterboxed: the composites resized with their aspect kept
 * into a rectangle of new_w x new_h at (left, top) of an out_w x out_h canvas,
 * the rest of the canvas a pad value, and the targets and the index map moved
 * and scaled to match.
 *
 * THE GEOMETRY is host arithmetic in exact integers (labels_fmt.
 * letterbox_geometry(bg_hw, size, scaleup, center, stride)); the entries take
 * any rectangle inside the canvas.  It is the usual LetterBox rule, r =
 * min(out_h / bg_h, out_w / bg_w), with min(r, 1) when scaleup is false:
 *   LIMITING AXIS: the one with the smaller ratio, compared by cross-
 *     multiplication (out_h·bg_w against out_w·bg_h); on a tie both are.  A
 *     limiting axis takes its canvas extent exactly.  With scaleup false and
 *     r >= 1 (out_h >= bg_h and out_w >= bg_w) both keep the background's.
 *   OTHER AXIS: a·b / c rounded half to even, a = its background extent, b =
 *     the limiting axis' canvas extent, c = the limiting axis' background
 *     extent: q, rem = divmod(a·b, c), plus one where 2·rem > c, or 2·rem == c
 *     and q is odd (Python's round); at least 1.
 *   STRIDE s >= 1 (the minimal rectangle): with dw = out_w - new_w, dh = out_h
 *     - new_h the canvas shrinks to out_w = new_w + dw % s, out_h = new_h +
 *     dh % s before the offsets are taken.
 *   OFFSETS: center: left = dw / 2, top = dh / 2, rounded down (what round(dw
 *     / 2 - 0.1) gives); else left = top = 0.
 *   The shrunken canvas passed back as the size gives the same rectangle
 *   unless the other axis' extent was rounded DOWN and its remainder dw % s
 *   (dh % s) is 0: then that axis fills the new canvas, becomes the limiting
 *   one, and the formerly limiting extent is computed anew (it can come out
 *   smaller by the rounding; the rectangle still fits the canvas).
 *
 * ipp_scene_feed_letterbox: in, lut, elem_size, bgr as for
 * ipp_scene_feed_resize; taps_x, taps_y: ipp_plan_resample's tables for (bg_w
 * -> new_w) and (bg_h -> new_h) with ksize_x and ksize_y, or geometry.
 * identity_taps for an axis whose sizes are equal; out = n_scenes x 3 x out_h x
 * out_w contiguous elements; pad in 0..255.  With r the H FIRST, THEN V integer
 * result of ipp_scene_feed_resize taken for (new_w, new_h):
 *   out[s][c][y][x] = lut[c][ r[y - top][x - left][ch(c)] ]   for left <= x <
 *                     left + new_w and top <= y < top + new_h,
 *   out[s][c][y][x] = lut[c][pad]                             everywhere else.
 * The table's words are copied; no float arithmetic runs.  ONE launch covers
 * the canvas: one workgroup of 256 threads per (scene, tile of tw x th canvas
 * elements), every element of out written exactly once and none outside it.
 * The part of a tile inside the rectangle is a run of at most tw x th resized
 * outputs, and the bound of ipp_scene_feed_resize holds for a run wherever it
 * starts, so the tile and the LDS bytes are those of the rectangle:
 * ipp_scene_feed_resize_lds(bg_w, bg_h, new_w, new_h, ksize_x, ksize_y,
 * elem_size, tile) states both, within IPP_FEED_RESIZE_LDS_BYTES.  A workgroup
 * whose tile lies wholly in the pad reads nothing of `in` and stages nothing;
 * pad elements go in 16-B stores at the 16-B boundaries of their plane row,
 * element by element before the first and behind the last.  As there, nothing
 * is assumed of the alignment of `in`, every window is clamped to the staged
 * span, and no byte outside the n_scenes·bg_h·bg_w·3 of `in` is read whatever
 * the tables hold.
 * IPP_E_ARG, before any launch: everything ipp_scene_feed_resize refuses, with
 * new_w, new_h in the place of out_w, out_h; new_w or new_h < 1, left or top <
 * 0, left + new_w > out_w, top + new_h > out_h; pad outside 0..255; out_w·out_h
 * >= 2^28; n_scenes·tiles >= 2^31 - 1 (the grid, tiles of the canvas).
 *
 * ipp_scene_feed_targets_letterbox: ipp_scene_feed_targets — DESCRIPTOR, KEPT,
 * ORDER, slot, count and the -1 rows exactly as there, by the same code — with
 * another ROW.  From the integer row (x0, y0, x1, y1):
 *   cx = f32( f64((x0 + x1)·new_w + 2·left·bg_w) / f64(2·bg_w·out_w) )
 *   w  = f32( f64((x1 - x0)·new_w) / f64(bg_w·out_w) )
 *   cy and h alike with y, new_h, top, bg_h and out_h.
 * Numerators and denominators are int64 products; with every side <=
 * IPP_FEED_MAX_SIDE = 2^23 they stay below 2^49 and are exact in float64.  Then
 * ONE correctly rounded float64 division and ONE round-to-nearest conversion
 * to float32 (the file is built without fast-math or reciprocal flags).  This
 * is NOT ipp_scene_feed_targets' single float32 division: even with the
 * rectangle equal to the canvas (new = out = bg, left = top = 0 included) the
 * two may differ in the last bit, since a float64 quotient rounded again to
 * float32 is not always the correctly rounded float32 quotient.  Nothing
 * depends on an order; there is no float atomic.
 * IPP_E_ARG, before any launch: what ipp_scene_feed_targets refuses; out_w or
 * out_h outside 1..IPP_FEED_MAX_SIDE; new_w or new_h < 1, left or top < 0, left
 * + new_w > out_w, top + new_h > out_h.
 *
 * ipp_scene_feed_index_map_letterbox: ipp_scene_feed_index_map_sampled with
 * xtab, ytab of new_w and new_h entries (geometry.nearest_table(bg, new)),
 * placed at (left, top):
 *   out[s][y][x] = f(map[s][ytab[y - top]][xtab[x - left]])  inside the rectangle,
 *   out[s][y][x] = 0  in the pad and in columns [out_w, out_pitch),
 * in n_scenes slots of out_h rows of out_pitch bytes, every byte of which is
 * written, in 16-B stores.  The map is read at the sampled positions only.
 * IPP_E_ARG, before any launch: what ipp_scene_feed_index_map_sampled refuses,
 * and the rectangle checks above. */
int ipp_scene_feed_letterbox(const uint8_t* in, void* out, const void* lut, const int32_t* taps_x,
                             const int32_t* taps_y, int32_t n_scenes, int32_t bg_w, int32_t bg_h,
                             int32_t new_w, int32_t new_h, int32_t left, int32_t top, int32_t out_w,
                             int32_t out_h, int32_t ksize_x, int32_t ksize_y, int32_t pad,
                             int32_t elem_size, int32_t bgr, void* stream);
int ipp_scene_feed_targets_letterbox(const int32_t* rows, const int32_t* scene_layer,
                                     const int32_t* class_ids /* may be NULL */, int32_t n_images,
                                     int32_t n_scenes, int32_t per_scene, int32_t bg_w, int32_t bg_h,
                                     int32_t min_q, int32_t new_w, int32_t new_h, int32_t left,
                                     int32_t top, int32_t out_w, int32_t out_h, float* targets,
                                     int32_t* count, int32_t* slot, void* stream);
int ipp_scene_feed_index_map_letterbox(const uint8_t* map, int64_t map_pitch, int32_t bg_w,
                                       int32_t bg_h, const int32_t* slot, int32_t n_scenes,
                                       int32_t per_scene, const int32_t* xtab, const int32_t* ytab,
                                       int32_t new_w, int32_t new_h, int32_t left, int32_t top,
                                       int32_t out_w, int32_t out_h, uint8_t* out, int64_t out_pitch,
                                       void* stream);

/* ------------------------------------------------------------------------ */
/* K10-K13: pixels_isolés.keep_largest_component                             */
/* :32 threshold(α,1,255) :35 connectedComponentsWithStats(8) :38-55 keep    */
/* largest :74-81 crop-fit (findNonZero + boundingRect).                     */
/* ------------------------------------------------------------------------ */
/* Scratch of one image inside a caller-provided byte buffer (offsets in
 * bytes, 256-B aligned; ipp_ccl_scratch_layout fills them for a w×h image
 * relative to 0 — add the image's base offset).  Per 64×64 tile: mask = 64
 * row words of fg bits (tile-major), edge = the global root of each edge
 * pixel (top, bottom, left, right × 64 int32), tile = (first entry, count).
 * P/A: int32/uint32 per run-start index (touched at component roots only);
 * ent: ent_cap {root, area, bbox} records of the components that touch a
 * tile edge (the others are final after the tile pass). */
typedef struct ipp_ccl_work {
    int64_t mask_off, edge_off, p_off, a_off, ent_off;
    int64_t ent_cap;
    int64_t tile_off;   /* per tile: component count, only root, edge flags */
    int64_t img_off;    /* per image: best closed component, kept root      */
} ipp_ccl_work;

/* Bytes of scratch for one w×h image; fills *work (may be NULL). */
int64_t ipp_ccl_scratch_layout(int32_t w, int32_t h, ipp_ccl_work* work);

/* α > 1 → 8-connected components → α := 0 outside the largest (lowest root on
 * ties) IN PLACE on 4-channel images; images without any component are left
 * unchanged.  works: device array of per-image scratch offsets into `scratch`;
 * max_ent = largest ent_cap; counts: int32[n] scratch; stats: int64[n]
 * scratch (best key = area << 32 | ~root); bbox[i] = (x0, y0, x1, y1) of the
 * kept component or (-1,-1,-1,-1) when there is none (the caller then takes
 * the α ≠ 0 bbox of the unchanged image, pixels_isolés.py:74-81). */
int ipp_ccl_keep_largest(uint8_t* img, const ipp_image_desc* descs, int32_t n_images,
                         int32_t max_w, int32_t max_h, const ipp_ccl_work* works,
                         uint8_t* scratch, int64_t max_ent, int32_t* counts, int64_t* stats,
                         int32_t* bbox, void* stream);

/* Fused config-5 chain on 3-channel BGR frames: filtres_liste's HSV mask
 * (filtres_liste.py:84-134, params as for ipp_hsv_mask with bgr = 1) → α > 1
 * components → keep the largest → crop-fit (pixels_isolés.py:29-81), written
 * as BGRA (α 255 inside the component, 0 elsewhere) at out_descs[i] (the
 * slot must hold the whole frame).  bbox as above; a frame with no kept pixel
 * gets bbox (-1,...) and no output (the reference raises there).  Frames of
 * any width; each frame's h·pitch + 18 must be below 2^32: the crop addresses
 * a frame through one buffer resource (32-bit offsets from the 16-byte
 * boundary below the frame to the dword holding its last byte).  NOT checked
 * here, the descriptors being in device memory: a larger frame is cropped
 * wrongly without an error. */
int ipp_video_keep_largest(const uint8_t* frames, const ipp_image_desc* descs, int32_t n_images,
                           int32_t max_w, int32_t max_h, const ipp_hsv_params* hsv,
                           const ipp_ccl_work* works, uint8_t* scratch, int64_t max_ent,
                           int32_t* counts, int64_t* stats, int32_t* bbox, uint8_t* out,
                           const ipp_image_desc* out_descs, void* stream);

/* Bounding box of non-zero pixels, Pillow getbbox() rule (rotations.py:99,
 * recadrages.py:70): the alpha band for 2/4-channel images, any band for
 * 1/3-channel ones (also cv2.findNonZero+boundingRect, pixels_isolés.py:77-79).
 * bbox[i] = (x0, y0, x1, y1) or (-1,-1,-1,-1) when empty. */
int ipp_alpha_bbox(const uint8_t* img, const ipp_image_desc* descs, int32_t n_images,
                   int32_t max_w, int32_t max_h, int32_t* bbox, void* stream);
/* The thresholded form, for the tight YOLO box of a pasted overlay
 * (overlays.py:139 pastes through the overlay's alpha): the box of the pixels
 * whose last band is >= alpha_min, on 2- and 4-channel images (an image with
 * another channel count has no alpha band and gets the all -1 row).
 * 1 <= alpha_min <= 255; alpha_min = 1 equals ipp_alpha_bbox on such images. */
int ipp_alpha_bbox_min(const uint8_t* img, const ipp_image_desc* descs, int32_t n_images,
                       int32_t max_w, int32_t max_h, int32_t alpha_min, int32_t* bbox,
                       void* stream);

/* ------------------------------------------------------------------------ */
/* Host-side planning (CPU).                                                 */
/* ------------------------------------------------------------------------ */
/* Pillow Resample.c precompute_coeffs + normalize_coeffs_8bpc for LANCZOS
 * (support 3): writes bounds[2*out_size] (xmin, count) followed by
 * taps[out_size*ksize] into `out` (int32); returns ksize, or the required
 * int32 count when out == NULL (as -count), or IPP_E_ARG. */
int64_t ipp_plan_lanczos(int32_t in_size, double in0, double in1, int32_t out_size,
                         int32_t* out, int64_t out_capacity);
/* The same for any of Pillow's five convolution filters (Resample.c's filter
 * functions and supports): `filter` is an IPP_RESAMPLE_* code, the layout and
 * the return convention are ipp_plan_lanczos', and ksize = 2·⌈support·max((in1
 * - in0) / out_size, 1)⌉ + 1.  IPP_RESAMPLE_LANCZOS returns exactly what
 * ipp_plan_lanczos returns.  An unknown filter is IPP_E_ARG.
 *   BOX       1 on (-0.5, 0.5], support 0.5
 *   BILINEAR  1 - |x|, support 1
 *   HAMMING   sinc(x)·(0.54 + 0.46·cos(pi·x)), support 1 (the two constants are
 *             float literals in Resample.c and are widened from float here too)
 *   BICUBIC   a = -0.5, support 2
 *   LANCZOS   sinc(x)·sinc(x / 3), support 3 */
#define IPP_RESAMPLE_BOX 0
#define IPP_RESAMPLE_BILINEAR 1
#define IPP_RESAMPLE_HAMMING 2
#define IPP_RESAMPLE_BICUBIC 3
#define IPP_RESAMPLE_LANCZOS 4
int64_t ipp_plan_resample(int32_t filter, int32_t in_size, double in0, double in1,
                          int32_t out_size, int32_t* out, int64_t out_capacity);
/* MFMA tile format of a pipe axis (v_mfma_i32_16x16x64_i8; stated in
 * csrc/ipp_pipe_layout.h): size bound in int32 for (in, out, ksize) and bound
 * on K steps per tile.  ipp_plan_mfma_tile (below) is the one host function
 * that writes the format. */
int64_t ipp_plan_mfma_size(int32_t in_size, int32_t out_size, int32_t ksize);
int32_t ipp_plan_mfma_nk_bound(int32_t in_size, int32_t out_size, int32_t ksize);
/* ksize for (in_size, out_size) without computing taps. */
int32_t ipp_plan_lanczos_ksize(double in0, double in1, int32_t out_size);

/* Alpha bbox of the rotated canvas of a fully opaque in_w×in_h image under
 * the 16.16 affine (a0..a5) on an nw×nh canvas, computed analytically per
 * row with exact integer arithmetic.  bbox = (x0, y0, x1, y1) or all -1. */
int ipp_plan_opaque_bbox(int32_t in_w, int32_t in_h, const int32_t a[6],
                         int32_t nw, int32_t nh, int32_t bbox[4]);

/* ------------------------------------------------------------------------ */
/* Batch planner of the fused pipe (ipp_plan.cpp; replaces the per-item host  */
/* loop of fused.plan_pipe).  Draws every random parameter in the order of    */
/* the reference's chained file-mode pipeline with CPython's generator        */
/* (rotations.py:89, symmetry.py:122, pipeline.py:202, overlays.py:108,       */
/* :133-134), plans each item's geometry (rotations.py:96-109,                */
/* overlays.py:106-126) and fills the pipe descriptors (grouped by background) */
/* and the per-axis records of the device tap planner.                        */
/* ------------------------------------------------------------------------ */
typedef struct ipp_pipe_plan_cfg {
    int32_t src_h, src_w, src_pitch;          /* RGB u8 sources; pitch 0 = 3·src_w */
    int32_t crop_t, crop_b, crop_l, crop_r;   /* crop_from_border margins (px)     */
    int32_t bg_h, bg_w, n_bg;
    int32_t n_sym, sym_flip[4];               /* symmetry pool (flip code per entry) */
    int32_t n_global, start, stop;            /* plan items [start, stop) of n_global */
    int32_t given;                            /* 1: items[] hold angle, ratio, sym,
                                                 bg_index, x, y (nothing is drawn) */
    int32_t n_threads;                        /* ≤ 0: all cores                    */
    int32_t ring_cols;                        /* H-pass LDS ring (≤ 0: 512); an H tile
                                                 needing a wider window is refused */
    int32_t pad_;
    uint64_t seed;                            /* |n| of random.seed(n)             */
    double angle_min, angle_max, scale_min, scale_max;
} ipp_pipe_plan_cfg;

typedef struct ipp_pipe_item {
    double angle, ratio;
    int32_t sym, bg_index, x, y;              /* sym: index into the pool          */
    int32_t rot_w, rot_h;                     /* rotated canvas (expand=True)      */
    int32_t cut_x, cut_y, cut_w, cut_h;       /* its getbbox = the cut-out         */
    int32_t ov_w, ov_h;                       /* resized overlay                   */
} ipp_pipe_item;

/* One resampling axis (2 per item: H then V) for ipp_pipe_plan_taps. */
typedef struct ipp_tap_axis {
    int32_t in_size, out_size;
    int32_t identity;     /* 1: no pass on this axis (single 2^22 tap)        */
    int32_t shift;        /* subtracted from every xmin (V axis: ybox_first)  */
    int32_t phase;        /* tile phase (V axis: y mod 16)                    */
    int32_t nkb;          /* ipp_plan_mfma_nk_bound: K-step slots per tile     */
    int32_t compact;      /* 1: tiles may use the compact block layout (H
                             axis of the pipe, see ipp_plan_mfma_tile)         */
    int32_t n_tiles;      /* (out_size + phase + 15) / 16                     */
    int64_t coef_off;     /* int32 index of the axis block in coefs           */
} ipp_tap_axis;

/* totals[] slots of ipp_plan_pipe_batch */
#define IPP_PT_COEF_WORDS 0   /* int32 size of the coefs buffer               */
#define IPP_PT_TMP_BYTES 1
#define IPP_PT_MAX_OUT_W 2
#define IPP_PT_MAX_ROWS 3
#define IPP_PT_MAX_OV_W 4
#define IPP_PT_MAX_OV_H 5
#define IPP_PT_ALGO_H 6       /* algorithmic bytes, see fused.PipePlan        */
#define IPP_PT_ALGO_V 7
#define IPP_PT_COPY_BYTES 8   /* 2 x the composite bytes the H launch copies
                                 (read + write as the V pass would move them;
                                 dense 16-B aligned images assumed)            */
#define IPP_PT_MAX_TILES 9
#define IPP_PT_ERR_ITEM 10    /* on IPP_E_RANGE: global item index and reason: */
#define IPP_PT_ERR_CODE 11    /* 1 canvas beyond 16.16, 2 ScaleAffine table,
                                 3 degenerate overlay, 4 given parameters do not
                                 fit, 5 H window beyond the LDS ring, 6 empty
                                 randint range                                 */
#define IPP_PT_COPY_READS 12  /* background bytes the H launch's grouped copy
                                 loads: one background per run of
                                 same-background items in each group of
                                 IPP_PIPE_COPY_GROUP items                     */
#define IPP_PLAN_TOTALS 16

/* Items per background-copy group of ipp_pipe_hpass_bgcopy (one shared load
 * per background vector and run of same-background items in the group). */
#define IPP_PIPE_COPY_GROUP 8
/* Widest overlay (pixels) of the pipe's V launch (ipp_pipe_vblend_bands). */
#define IPP_PIPE_MAX_OV_W 992

/* items[stop - start]: outputs (inputs too when cfg->given); descs[n] (in
 * processing order), axes[2n]; totals[IPP_PLAN_TOTALS]. */
int ipp_plan_pipe_batch(const ipp_pipe_plan_cfg* cfg, ipp_pipe_item* items, ipp_pipe_desc* descs,
                        ipp_tap_axis* axes, int64_t* totals);

/* Device tap planner (ipp_taps.hip): builds the MFMA tile format of every
 * axis (what ipp_plan_mfma_tile writes from Pillow's taps: hdr, bias,
 * blocks; tile t's blocks at uint4 offset t·nkb·192 of the axis's block area)
 * directly in `coefs` (device, IPP_PT_COEF_WORDS int32).  The taps are
 * computed in fp64 on the device; any tile holding a tap whose rounding point
 * lies within 2^-22 of a quantisation boundary is recomputed on the host with
 * the libm sin Pillow uses and copied over, so the result is bit-exact with
 * Resample.c.  scratch: device, ipp_pipe_taps_scratch_bytes(n_axes).
 * Synchronises `stream`.  stats[0] = tiles recomputed on the host, stats[1] =
 * device status (bit 0: a tile needed more K steps than nkb). */
int64_t ipp_pipe_taps_scratch_bytes(int32_t n_axes);
int ipp_pipe_plan_taps(const ipp_tap_axis* axes, int32_t n_axes, int32_t* coefs, void* scratch,
                       int64_t* stats, void* stream);
/* ipp_pipe_plan_taps with the size cap of the one packed upload of the
 * host-rebuilt tiles given (0 <= pack_cap <= the scratch's pack region, 4 MiB;
 * ipp_pipe_plan_taps passes the region size).  Rebuilt tiles whose pack
 * exceeds the cap are copied tile by tile instead; the taps are the same byte
 * for byte (tests/test_gpu_taps.py forces that path with pack_cap = 0). */
int ipp_pipe_plan_taps_cap(const ipp_tap_axis* axes, int32_t n_axes, int32_t* coefs, void* scratch,
                           int64_t* stats, int64_t pack_cap, void* stream);
/* Host restatement of one tile of that format (Resample.c taps, libm sin):
 * hdr[4], bias[16], blocks (nK·3072 bytes, ≤ blocks_cap); dense, or compact
 * (hdr[3] = 1) where axis->compact allows it: both layouts are stated in
 * csrc/ipp_pipe_layout.h. */
int ipp_plan_mfma_tile(const ipp_tap_axis* axis, int32_t t, int32_t hdr[4], int32_t bias[16],
                       uint8_t* blocks, int64_t blocks_cap);
/* Pieces of ipp_plan_pipe_batch exposed for the tests: the division-free
 * form of ipp_plan_opaque_bbox, CPython's math.hypot (vector_norm), the
 * rotation plan (out = nw, nh, a0..a5) and the first n random() values of
 * random.seed(seed). */
int ipp_plan_opaque_bbox_fast(int32_t in_w, int32_t in_h, const int32_t a[6],
                              int32_t nw, int32_t nh, int32_t bbox[4]);
double ipp_plan_py_hypot(double x, double y);
int ipp_plan_rotation(int32_t w, int32_t h, double angle, int32_t out[8]);
int ipp_plan_py_random(uint64_t seed, int32_t n, double* out);

/* ------------------------------------------------------------------------ */
/* tranfo.enhance_image (transforms/tranfo.py:37-53) on RGB images:           */
/* ImageEnhance Brightness/Contrast/Color (:38-40, Image.blend, Blend.c),     */
/* GaussianBlur (:42-44, BoxBlur.c) and the r/g/b point() LUTs (:46-51).      */
/* ------------------------------------------------------------------------ */
#define IPP_ENH_BLUR 1   /* a GaussianBlur follows (box passes, ipp_box_pass) */
#define IPP_ENH_LUT 2    /* apply the image's 3×256 LUT (after the blur)      */

typedef struct ipp_enhance_desc {
    int64_t src_off, dst_off;          /* RGB images, explicit pitches      */
    int32_t w, h, src_pitch, dst_pitch;
    float f_brightness, f_contrast, f_color;  /* float32(factor), Blend.c   */
    int32_t flags;                     /* IPP_ENH_*                          */
    int32_t box_r;                     /* box radius (int part), BoxBlur.c   */
    uint32_t box_ww, box_fw;           /* 8.24 weights of the box pass       */
    int32_t pad_;
    int64_t lut_off;                   /* byte offset of 3×256 LUT bytes     */
} ipp_enhance_desc;

/* Σ L of the brightened image per image into sums[n] (zeroed first). */
int ipp_enhance_lsum(const uint8_t* src, const ipp_enhance_desc* descs, int32_t n_images,
                     int64_t max_pixels, uint64_t* sums, void* stream);
/* brightness → contrast (mean = int(Σ/N + 0.5)) → color [→ LUT when the
 * image has IPP_ENH_LUT and no IPP_ENH_BLUR]; writes dst (dst_off/pitch). */
int ipp_enhance_color(const uint8_t* src, uint8_t* dst, const ipp_enhance_desc* descs,
                      int32_t n_images, int64_t max_pixels, const uint64_t* sums,
                      const uint8_t* luts, void* stream);
/* One BoxBlur.c pass along x (axis 0) or y (axis 1) of packed RGB planes at
 * byte offsets offs[i] (pitch 3w) in src → dst at the same offsets, or at the
 * descriptor's dst_off/dst_pitch when final_dst; luts != NULL applies the
 * LUTs (last pass).  A GaussianBlur is 3 x passes then 3 y passes. */
int ipp_box_pass(const uint8_t* src, uint8_t* dst, const ipp_enhance_desc* descs, int32_t n_images,
                 int64_t max_pixels, const int64_t* offs, int32_t axis, const uint8_t* luts,
                 int32_t final_dst, void* stream);

/* ------------------------------------------------------------------------ */
/* Baseline JPEG of RGB composites, encoded on the device                     */
/* ------------------------------------------------------------------------ */
/* The entropy-coded data of the file Pillow 12.2.0 (libjpeg-turbo 3.1) writes
 * for Image.fromarray(a).save(path, quality=q[, subsampling=0]) of an 8-bit
 * RGB image: baseline sequential, the Annex K Huffman tables, one scan, no
 * restart markers.  The header (SOI, APP0 JFIF, DQT x 2, SOF0, DHT x 4, SOS)
 * and the EOI are the host's (image_processor_pipeline_amd/jpeg.py).  This
 * project's normative definition, in exact integers (tests/jpeg_refs.py is
 * its restatement, held to the installed Pillow byte for byte):
 *
 * TABLES.  Quality q in 1..100 scales the two Annex K.1/K.2 tables t by s =
 * 5000 / q (q < 50) or 200 - 2q: (t·s + 50) / 100 clamped to 1..255.  The
 * caller passes the 2 x 64 results (luma, chroma; row-major, not zigzag).
 * COLOUR (jccolor.c, 16-bit fixed point, arithmetic >> 16):
 *   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + 128·65536 + 32767) >> 16
 *   Cr = ( 32768 R - 27439 G -  5329 B + 128·65536 + 32767) >> 16
 * SAMPLING.  IPP_JPEG_444: three full-resolution components, MCU = 8 x 8 px,
 * blocks Y Cb Cr.  IPP_JPEG_420 (Pillow's default): Cb and Cr halved both
 * ways, MCU = 16 x 16 px, blocks Y00 Y01 Y10 Y11 Cb Cr.  A chroma sample is
 * (a + b + c + d + bias) >> 2 over its 2 x 2 converted pixels, bias 1 for an
 * even chroma column and 2 for an odd one.
 * EDGES, two kinds.  (1) Replication: a component has ⌈size / 8⌉ blocks each
 * way (size = w, h for full resolution; ⌈w / 2⌉, ⌈h / 2⌉ for 4:2:0 chroma).
 * Full-resolution samples past the image repeat its last column and row.  For
 * 4:2:0 chroma the order matters, and is libjpeg's: pixel columns past w
 * repeat the last one *before* the downsample (so the bias still alternates);
 * pixel rows are repeated only to an even count (row 2cy + 1 = h reads row
 * h - 1); chroma rows past ⌈h / 2⌉ repeat the last *chroma* row — which, for
 * an even h, is not the downsample of a repeated pixel row.  (2) Dummy blocks:
 * a 4:2:0 luma block of an MCU that lies past the luma grid (w mod 16 in
 * 1..8: Y01, Y11; h mod 16 in 1..8: Y10, Y11) is not made of pixels: its AC
 * terms are 0 and its DC is the DC of the block before it in the MCU; in a
 * dummy bottom row both blocks take Y01's (jccoefct.c).
 * TRANSFORM (jfdctint.c "islow", CONST_BITS 13, PASS1_BITS 2, int32) of the
 * samples - 128, rows then columns; the result is 8 x the DCT.
 * QUANTISATION.  coef / (8·q), halves away from zero: sign · ((|coef| + 4q)
 * / 8q).  (The kernels divide by the reciprocal floor(2^26 / 8q) + 1, exact
 * for every operand below 2^26 / 8q, so below 2^15; |coef| <= 8·1024 plus the
 * passes' rounding.)
 * CODING.  Zigzag order; DC as the difference to the previous block of the
 * same component in the scan (0 for the first; dummy blocks count), category
 * = bit length of |v|, magnitude bits v (v >= 0) or v - 1 (v < 0); AC as
 * (run << 4 | category) with 0xF0 for each 16 zeros before a nonzero term and
 * 0x00 (EOB) when the block ends in zeros.  Bits are MSB first; the last byte
 * is filled with 1-bits; every 0xFF byte, that one included, is followed by a
 * 0x00 (counted in the sizes below).
 *
 * ipp_jpeg_encode: in = n_images x h x w x 3 contiguous uint8 RGB (what the V
 * launches leave).  Image i's data go to slots + i·pitch16(capacity), where
 * pitch16 rounds up to 16 B; hdr (device int32[n_images][IPP_JPEG_HDR])
 * receives {bytes, status}.  status 0: exactly `bytes` bytes were written to
 * the slot and nothing else of it.  status IPP_JPEG_OVERFLOW: the data are
 * longer than capacity, NO byte of the slot was written, and `bytes` is the
 * length found so far (the stuffed length, or the unstuffed one where that
 * alone exceeds capacity), saturated to 2^31 - 1.  Whether an image fits is
 * known after the scans and before any write to its slot.  Every header word
 * is written.  qtab: HOST uint16[2][64], read before the call returns.
 * ipp_jpeg_pack, after it on the same stream: copies image i's `bytes` bytes
 * to out + offsets[i] (device int64[n_images], computed by the caller from
 * the copied-back headers) for every image with status 0; writes nothing for
 * the others and nothing else.
 * No float anywhere.  The only atomic is an integer OR that merges the two
 * words a block's bits may share with its neighbours' in the zeroed unstuffed
 * stream: the result does not depend on any order.
 * scratch: device, 16-B aligned, ipp_jpeg_scratch_bytes(...) bytes, each part
 * rounded up to 256 B: per image and block 64 int16 coefficients (zigzag) and
 * a uint64 (AC bit length, then bit offset); per image a 16-B record, the
 * unstuffed stream (pitch16(capacity) + 16 B) and a uint32 per 4096 B of it.
 * Blocks per image: 6·⌈w / 16⌉·⌈h / 16⌉ or 3·⌈w / 8⌉·⌈h / 8⌉.
 * IPP_E_ARG, before any launch: a NULL pointer; scratch or slots not 16-B,
 * offsets not 8-B, hdr not 4-B aligned; w or h outside 1..IPP_JPEG_MAX_SIDE;
 * another sampling; capacity outside 1..IPP_JPEG_MAX_CAPACITY; a table entry
 * outside 1..255; n_images negative or > 65535 (the grid).  n_images == 0 is
 * IPP_OK, launches and writes nothing. */
#define IPP_JPEG_420 0
#define IPP_JPEG_444 1
#define IPP_JPEG_HDR 2
#define IPP_JPEG_OVERFLOW 1
#define IPP_JPEG_MAX_SIDE 16384
#define IPP_JPEG_MAX_CAPACITY 2147483632 /* 2^31 - 16: sizes fit the int32 headers */
int64_t ipp_jpeg_scratch_bytes(int32_t n_images, int32_t w, int32_t h, int32_t sampling, int64_t capacity);
int ipp_jpeg_encode(const uint8_t* in, int32_t n_images, int32_t w, int32_t h, int32_t sampling,
                    const uint16_t* qtab, uint8_t* scratch, uint8_t* slots, int64_t capacity, int32_t* hdr,
                    void* stream);
int ipp_jpeg_pack(const uint8_t* slots, int64_t capacity, const int32_t* hdr, int32_t n_images,
                  const int64_t* offsets, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------ */
/* Baseline JPEG files decoded on the device                                  */
/* ------------------------------------------------------------------------ */
/* The RGB pixels np.asarray(Image.open(f).convert("RGB")) gives with Pillow
 * 12.2.0 (libjpeg-turbo 3.1) for a baseline file: 8 bit, three components
 * YCbCr sampled 2x2/1x1/1x1 (IPP_JPEG_420) or 1x1/1x1/1x1 (IPP_JPEG_444), one
 * interleaved scan, Huffman coded, with or without restart markers.  The host
 * (jpeg.py parse_jpeg) walks the markers and refuses everything else by name;
 * the device decodes the entropy-coded span.  This project's normative
 * definition, in exact integers (tests/jpeg_decode_refs.py is its restatement,
 * held to the installed Pillow value for value; Pillow is the judge):
 *
 * CODING, undone.  Blocks in scan order as for the encoder above; in each, a
 * DC symbol (category s <= 11, then s magnitude bits: v, or v - 2^s + 1 where
 * v < 2^(s-1)) added to the previous DC of the component (0 at the start of the
 * scan and after every RSTn), then AC symbols (run << 4 | s): 0x00 ends the
 * block, 0xF0 skips 16 terms, else skip `run` and read a term of s <= 10 bits;
 * zigzag position k of the block is natural position zz[k].  The codes are
 * those of the file's own DHT tables (BITS, HUFFVAL; Annex C).  A 0x00 after a
 * 0xFF is no data.  With a restart interval of r MCUs, every r MCUs the stream
 * is padded to a byte and RSTn (n counting 0..7 and again) follows.
 * DEQUANTISE.  coefficient · table entry (the file's DQT, 8 bit), natural order.
 * INVERSE TRANSFORM (jidctint.c "islow", CONST_BITS 13, PASS1_BITS 2, int32),
 * columns first, then rows.  Of c0..c7:
 *   z1 = (c2 + c6)·4433, t2 = z1 - c6·15137, t3 = z1 + c2·6270
 *   t0 = (c0 + c4) << 13, t1 = (c0 - c4) << 13
 *   t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
 *   a0..a3 = c7, c5, c3, c1;  z1 = a0 + a3, z2 = a1 + a2, z3 = a0 + a2,
 *   z4 = a1 + a3, z5 = (z3 + z4)·9633
 *   a0 *= 2446, a1 *= 16819, a2 *= 25172, a3 *= 12299
 *   z1 *= -7373, z2 *= -20995, z3 = z3·(-16069) + z5, z4 = z4·(-3196) + z5
 *   a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4
 *   outputs 0..7 = t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1,
 *   t11 - a2, t10 - a3, each (x + 2^(s-1)) >> s with s = 11 for the columns and
 *   18 for the rows (arithmetic shift).  Then + 128, clamped to 0..255.
 *   libjpeg masks the sample before its limit table, so one outside -384..639
 *   before the clamp would wrap there.  No file an encoder writes reaches that
 *   range; such files are outside this contract and nothing is tested there.
 * UPSAMPLE, 4:2:0 only (jdsample.c).  A chroma plane is its real extent of
 * ⌈w / 2⌉ x ⌈h / 2⌉ samples; what was decoded past it is never read.  Where
 * ⌈w / 2⌉ > 2, the "fancy" triangle filter: for output row y, s[x] =
 * 3·near[x] + far[x] with near = chroma row y >> 1 and far the row above it
 * (y even) or below it (y odd), the edge row repeated at the top and bottom;
 * output column 2x = (3·s[x] + s[x-1] + 8) >> 4, column 2x + 1 = (3·s[x] +
 * s[x+1] + 7) >> 4, s repeating its edge at both ends.  Where ⌈w / 2⌉ <= 2
 * (w <= 4) libjpeg replicates instead: pixel (x, y) takes chroma (x >> 1,
 * y >> 1).  Cropped to w x h.
 * COLOUR (jdcolor.c), cb and cr less 128, arithmetic shifts, clamped to 0..255:
 *   R = Y + (( 91881·cr + 32768) >> 16)
 *   G = Y + ((-22554·cb - 46802·cr + 32768) >> 16)
 *   B = Y + ((116130·cb + 32768) >> 16)
 * No float anywhere.
 *
 * ipp_jpeg_decode: image i's entropy-coded bytes (after the SOS header, up to
 * the EOI or the end of the file) are data[span_off, span_off + span_len); no
 * byte outside the span is read; its
 * pixels go to out + out_off, rows out_pitch (>= 3w) bytes apart, 3w bytes of
 * each written and nothing else.  qtabs: device uint16[n_qtabs][64], natural
 * order; htabs: device uint8[n_htabs][16 + 256], BITS then HUFFVAL; qt / dc /
 * ac: per component (Y, Cb, Cr) the index of its table.  restart: the DRI
 * interval in MCUs, 0 for none.  Sizes, samplings and tables may differ from
 * image to image.  descs_host and descs hold the same n_images descriptors in
 * host and in device memory (one staging buffer and its copy): the host's are
 * checked before any launch, the kernels read the device's.
 * stat: device int32[n_images][IPP_JPEGD_STAT] = {status, rounds, subsequences,
 * marker status}; every word is written.  status 0: the image's pixels are
 * all written.  Nonzero: the stream is malformed and NO byte of the image's
 * output is written — IPP_JPEGD_BAD_MARKER (a marker other than RSTn, or fill
 * bytes, inside the span), _WRONG_RST (RSTn out of order), _SEG_COUNT (not
 * ⌈MCUs / restart⌉ segments), _TRUNCATED (the span ends in 0xFF), _BAD_CODE (a
 * code in no table, or a category or EOB run baseline does not have), _RUN (a
 * run past coefficient 63), _SEG_BLOCKS (a segment that ends early, inside a
 * block or an MCU, with blocks missing or left over, or with a byte or more
 * unread).  Several faults: the largest code.  rounds / subsequences: the most
 * synchronisation rounds any segment of the image took and the most
 * subsequences (of IPP_JPEGD_SUBSEQ bytes) any segment has — the decoder
 * repeats rounds until no lane's start state changes, however many that takes.
 * scratch: device, 16-B aligned; ipp_jpeg_decode_scratch_bytes fills the HOST
 * descriptors' coef_off / sub_off / seg_off (per image, each rounded up to
 * 256 B: 128 B per block; 24 B per span_len / IPP_JPEGD_SUBSEQ + segments + 1;
 * 8 B per segment) and returns the total, or IPP_E_ARG for a bad shape.
 * IPP_E_ARG, before any launch: a NULL pointer; scratch not 16-B, descs not
 * 8-B, stat not 4-B, qtabs not 2-B aligned; n_images negative or > 65535;
 * n_qtabs or n_htabs < 1; a negative size; per image: w or h outside
 * 1..IPP_JPEG_MAX_SIDE, another sampling, restart outside 0..65535, span_len
 * outside 0..IPP_JPEGD_MAX_SPAN, a span outside data, a table index outside
 * its array, out_pitch < 3w, an output outside out, scratch offsets other than
 * ipp_jpeg_decode_scratch_bytes assigns, or their total over scratch_bytes.
 * n_images == 0 is IPP_OK, launches and writes nothing. */
#define IPP_JPEGD_STAT 4
#define IPP_JPEGD_BAD_MARKER 1
#define IPP_JPEGD_WRONG_RST 2
#define IPP_JPEGD_SEG_COUNT 3
#define IPP_JPEGD_TRUNCATED 4
#define IPP_JPEGD_BAD_CODE 5
#define IPP_JPEGD_RUN 6
#define IPP_JPEGD_SEG_BLOCKS 7
#define IPP_JPEGD_MAX_SPAN 1073741824 /* 2^30 */
typedef struct ipp_jpegd_desc {
    int64_t span_off;                  /* entropy-coded bytes in data             */
    int64_t out_off;                   /* first pixel in out                      */
    int64_t coef_off, sub_off, seg_off; /* scratch parts (ipp_jpeg_decode_scratch_bytes) */
    int32_t span_len;
    int32_t w, h, sampling, restart;
    int32_t out_pitch;
    int32_t qt[3], dc[3], ac[3];
    int32_t pad_;
} ipp_jpegd_desc;
int64_t ipp_jpeg_decode_scratch_bytes(ipp_jpegd_desc* descs, int32_t n_images);
int ipp_jpeg_decode(const uint8_t* data, int64_t data_bytes, const ipp_jpegd_desc* descs_host,
                    const ipp_jpegd_desc* descs, int32_t n_images, const uint16_t* qtabs, int32_t n_qtabs,
                    const uint8_t* htabs, int32_t n_htabs, uint8_t* scratch, int64_t scratch_bytes,
                    uint8_t* out, int64_t out_bytes, int32_t* stat, void* stream);

/* ------------------------------------------------------------------------ */
/* Measurement helper (the copy-kernel ceiling of the box).     */
/* ------------------------------------------------------------------------ */
/* dst[0, nbytes) = src[0, nbytes) with 16-B non-temporal loads/stores; both
 * pointers 16-B aligned.  Not a reference call site: bench.py times it to
 * report the roofline against the HBM rate a plain copy reaches here. */
int ipp_stream_copy(const uint8_t* src, uint8_t* dst, int64_t nbytes, void* stream);

/* Library version / build info string. */
const char* ipp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* IPP_H */
