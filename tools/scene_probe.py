"""Scene batch against the flat batch of the same overlays ("Scenes").

    python tools/scene_probe.py [--scenes 1024] [--per-scene 4] [--size 1024] [--backgrounds 16]
                                [--steps 20] [--warmup 3] [--seed 0] [--simplify EPS] [--obb]

Workload: S scenes × K overlays of size² sources on size² backgrounds with the
config-3 parameters (fused.PipeConfig()), against PipeRunner.run on the flat
S·K-item batch of the same sources.  The two runs alternate step by step on
one device; every time is taken with HIP events on the current stream.  The
same steps time the label launch (ipp_pipe_scene_boxes) and the visibility-map
launch (ipp_pipe_scene_map) without and with the boxes, one after the other,
then the contour tracer (ipp_scene_contours) and its pack launch
(ipp_scene_contours_pack) on that map and those rows, with --max-edges slots
per overlay (default fused.scene_contour_capacity).  With --simplify EPS (pixels)
the same steps time the simplification of those packed polygons
(ipp_polygons_simplify) and its pack launch (ipp_polygons_simplify_pack) next
to the tracer's, and the report gains the vertices before and after and the
bytes copied back.  With --obb the same steps time the oriented boxes of those
packed polygons (ipp_polygons_obb) as well, and the report gains the bytes that
come back per overlay against the packed ring's.  A second series times each launch of the scene run on its own.  Prints one
JSON line."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--per-scene", type=int, default=4)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--backgrounds", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-edges", type=int, default=0)
    ap.add_argument("--simplify", type=float, default=None, metavar="EPS")
    ap.add_argument("--obb", action="store_true")
    args = ap.parse_args()

    import torch
    from bench import make_sources
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import fused
    from image_processor_pipeline_amd.device import _stream

    dev = torch.device("cuda:0")
    S, K, Z, nbg = args.scenes, args.per_scene, args.size, args.backgrounds
    n = S * K
    cfg = fused.PipeConfig()
    src = make_sources(0, n, Z, args.seed, dev)
    g0 = torch.Generator(device=dev)
    g0.manual_seed(1)
    bgs = torch.randint(0, 256, (nbg, Z, Z, 3), dtype=torch.uint8, device=dev, generator=g0)
    t0 = time.perf_counter()
    flat_plan = fused.plan_pipe((Z, Z), n, (Z, Z), nbg, cfg, seed=args.seed * 7919)
    t1 = time.perf_counter()
    scene_plan = fused.plan_scenes((Z, Z), S, K, (Z, Z), nbg, cfg, seed=args.seed * 7919)
    t2 = time.perf_counter()
    flat, scene = fused.PipeRunner(flat_plan, dev), fused.SceneRunner(scene_plan, dev)
    out_flat = torch.empty((n, Z, Z, 3), dtype=torch.uint8, device=dev)
    out_scene = torch.empty((S, Z, Z, 3), dtype=torch.uint8, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    # the visibility maps (at most 8 layers per scene): one buffer, written whole by every launch
    with_map = K <= N.IPP_SCENE_MAP_MAX_LAYERS
    vis = torch.empty((S, Z, fused.scene_map_pitch(Z)), dtype=torch.uint8, device=dev) if with_map else None

    # the contour tracer on the map and rows of the boxes-and-map launch; the pack's offsets come from the
    # headers of the last step (the same every step: the inputs do not change)
    import numpy as np
    max_edges = args.max_edges or fused.scene_contour_capacity(scene_plan)
    tracer = {}
    if with_map:
        nb = scene.lib.ipp_scene_contours_scratch_bytes(n, max_edges)
        tracer = dict(scratch=torch.empty(int(nb), dtype=torch.uint8, device=dev),
                      hdr=torch.zeros(N.IPP_CONTOUR_HDR * n, dtype=torch.int32, device=dev),
                      offsets=torch.zeros(n, dtype=torch.int64, device=dev),
                      verts=torch.empty(2, dtype=torch.int32, device=dev), rows=None)

    def trace():
        N.check(scene.lib.ipp_scene_contours(vis.data_ptr(), vis.shape[2], Z, Z, tracer["rows"].data_ptr(),
                                             scene._scene_layer.data_ptr(), n, S, K, max_edges,
                                             tracer["scratch"].data_ptr(), tracer["hdr"].data_ptr(), _stream(dev)),
                "ipp_scene_contours")

    def pack():
        N.check(scene.lib.ipp_scene_contours_pack(tracer["scratch"].data_ptr(), tracer["hdr"].data_ptr(),
                                                  tracer["offsets"].data_ptr(), n, max_edges,
                                                  tracer["verts"].data_ptr(), _stream(dev)),
                "ipp_scene_contours_pack")

    # the simplification of the packed polygons; its scratch and the counts are sized with the packed buffer,
    # the second pack's offsets come from the counts of the step after (the same every step)
    eps_q = None if args.simplify is None else fused.simplify_tolerance(args.simplify)
    simp = {}

    def simplify():
        N.check(scene.lib.ipp_polygons_simplify(tracer["verts"].data_ptr(), tracer["offsets"].data_ptr(),
                                                tracer["hdr"].data_ptr(), n, simp["total"], Z, Z, eps_q,
                                                simp["scratch"].data_ptr(), simp["counts"].data_ptr(), _stream(dev)),
                "ipp_polygons_simplify")

    def simplify_pack():
        N.check(scene.lib.ipp_polygons_simplify_pack(tracer["verts"].data_ptr(), tracer["offsets"].data_ptr(),
                                                     tracer["hdr"].data_ptr(), simp["scratch"].data_ptr(),
                                                     simp["counts"].data_ptr(), simp["out_offsets"].data_ptr(), n,
                                                     simp["out"].data_ptr(), _stream(dev)),
                "ipp_polygons_simplify_pack")

    # the oriented boxes of the packed polygons: scratch and records sized with the packed buffer
    obb = {}

    def oriented():
        N.check(scene.lib.ipp_polygons_obb(tracer["verts"].data_ptr(), tracer["offsets"].data_ptr(),
                                           tracer["hdr"].data_ptr(), n, obb["total"], Z, Z,
                                           obb["scratch"].data_ptr(), obb["rec"].data_ptr(), _stream(dev)),
                "ipp_polygons_obb")

    ms_obb = []
    ms_flat, ms_scene, ms_label, ms_map, ms_both, ms_trace, ms_pack = [], [], [], [], [], [], []
    ms_simp, ms_simp_pack = [], []
    hdrs = kept = None
    for step in range(args.warmup + args.steps):
        ef = timed(lambda: flat.run(src, bgs, out_flat))
        es = timed(lambda: scene.run(src, bgs, out_scene))
        el = timed(lambda: scene._launch_boxes(1, 128))
        if with_map:
            em = timed(lambda: scene._launch_map("scene_masks", 1, 128, False, vis))
            eb = timed(lambda: tracer.__setitem__("rows", scene._launch_map("scene_masks", 1, 128, True, vis)[1]))
            et = timed(trace)
            if hdrs is not None:
                ep = timed(pack)
                if args.obb:
                    eo = timed(oriented)
                if eps_q is not None:
                    ey = timed(simplify)
                    if kept is not None:
                        ez = timed(simplify_pack)
        torch.cuda.synchronize(dev)
        if with_map:
            if hdrs is not None and step >= args.warmup:
                ms_pack.append(ep[0].elapsed_time(ep[1]))
                if args.obb:
                    ms_obb.append(eo[0].elapsed_time(eo[1]))
                if eps_q is not None:
                    ms_simp.append(ey[0].elapsed_time(ey[1]))
                    if kept is not None:
                        ms_simp_pack.append(ez[0].elapsed_time(ez[1]))
            if hdrs is not None and eps_q is not None and kept is None:
                kept = simp["counts"].cpu().numpy().astype(np.int64)
                simp["out_offsets"] = torch.from_numpy(np.concatenate([[0], np.cumsum(kept)[:-1]]).astype(np.int64)).to(dev)
                simp["out"] = torch.empty(2 * max(int(kept.sum()), 1), dtype=torch.int32, device=dev)
            if hdrs is None:                  # the first step's headers size the packed buffer of all later steps
                hdrs = tracer["hdr"].cpu().numpy().reshape(n, N.IPP_CONTOUR_HDR)
                nv = hdrs[:, 3].astype(np.int64)
                tracer["offsets"] = torch.from_numpy(np.concatenate([[0], np.cumsum(nv)[:-1]]).astype(np.int64)).to(dev)
                tracer["verts"] = torch.empty(2 * max(int(nv.sum()), 1), dtype=torch.int32, device=dev)
                if args.obb:
                    obb["total"] = int(nv.sum())
                    nb = scene.lib.ipp_polygons_obb_scratch_bytes(n, obb["total"])
                    obb["scratch"] = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=dev)
                    obb["rec"] = torch.zeros(N.IPP_OBB_REC * n, dtype=torch.int32, device=dev)
                if eps_q is not None:
                    simp["total"] = int(nv.sum())
                    nb = scene.lib.ipp_polygons_simplify_scratch_bytes(n, simp["total"])
                    simp["scratch"] = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=dev)
                    simp["counts"] = torch.zeros(n, dtype=torch.int32, device=dev)
        if step >= args.warmup:
            ms_flat.append(ef[0].elapsed_time(ef[1]))
            ms_scene.append(es[0].elapsed_time(es[1]))
            ms_label.append(el[0].elapsed_time(el[1]))
            if with_map:
                ms_map.append(em[0].elapsed_time(em[1]))
                ms_both.append(eb[0].elapsed_time(eb[1]))
                ms_trace.append(et[0].elapsed_time(et[1]))

    # per launch: the scene run's own sequence, an event pair around each launch
    p, lib, st = scene_plan.pipe, scene.lib, _stream(dev)
    hsv = N.np_ptr(p.hsv)
    tmp, coefs, dp = scene.tmp.data_ptr(), scene.coefs.data_ptr(), scene._dptr
    launches = [("hpass_bgcopy(layer 0)", lambda: lib.ipp_pipe_hpass_bgcopy(
        src.data_ptr(), tmp, coefs, dp(0), S, p.max_out_w, p.max_rows, 3, hsv, p.tap_format, bgs.data_ptr(),
        out_scene.data_ptr(), st))]
    if K > 1:
        launches.append((f"hpass(layers 1..{K - 1})", lambda: lib.ipp_pipe_hpass(
            src.data_ptr(), tmp, coefs, dp(S), S * (K - 1), p.max_out_w, p.max_rows, 3, hsv, p.tap_format, st)))
    launches.append(("vblend_bands(layer 0)", lambda: lib.ipp_pipe_vblend_bands(
        tmp, bgs.data_ptr(), out_scene.data_ptr(), coefs, dp(0), S, p.bg_w, p.bg_h, p.max_ov_w, p.max_ov_h,
        p.tap_format, st)))
    for k in range(1, K):
        launches.append((f"vblend_over(layer {k})", lambda k=k: lib.ipp_pipe_vblend_over(
            tmp, out_scene.data_ptr(), coefs, dp(k * S), S, p.bg_w, p.bg_h, p.max_ov_w, p.max_ov_h, p.tap_format,
            st)))
    per = {name: [] for name, _ in launches}
    for step in range(args.warmup + args.steps):
        evs = [(name, timed(lambda fn=fn: N.check(fn(), name))) for name, fn in launches]
        torch.cuda.synchronize(dev)
        if step >= args.warmup:
            for name, (a, b) in evs:
                per[name].append(a.elapsed_time(b))

    scene_rows = tracer["rows"].cpu().numpy().reshape(n, 6) if with_map else None

    def summary(v):
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    print(json.dumps({
        "device": torch.cuda.get_device_name(dev), "scenes": S, "per_scene": K, "size": Z, "backgrounds": nbg,
        "steps": args.steps, "warmup": args.warmup,
        "plan_host_ms": {"flat": round((t1 - t0) * 1e3, 1), "scenes": round((t2 - t1) * 1e3, 1)},
        "flat_step": summary(ms_flat), "scene_step": summary(ms_scene), "label_launch": summary(ms_label),
        "map_launch": summary(ms_map) if with_map else None,
        "boxes_and_map_launch": summary(ms_both) if with_map else None,
        "map_bytes": int(vis.numel()) if with_map else 0,
        "contour_launch": summary(ms_trace) if with_map else None,
        "contour_pack_launch": summary(ms_pack) if with_map and ms_pack else None,
        "contours": None if hdrs is None else {
            "max_edges": max_edges, "largest_n_edges": int(hdrs[:, 0].max()), "largest_n_vertices": int(hdrs[:, 3].max()),
            "overflowed": int((hdrs[:, 7] & 1).sum()), "packed_bytes": int(8 * hdrs[:, 3].astype(np.int64).sum()),
            "header_bytes": int(hdrs.nbytes), "scratch_bytes": int(tracer["scratch"].numel())},
        "simplify_launch": summary(ms_simp) if ms_simp else None,
        "simplify_pack_launch": summary(ms_simp_pack) if ms_simp_pack else None,
        "simplify": None if kept is None else {
            "eps_px": args.simplify, "eps_q": eps_q, "vertices_before": int(hdrs[:, 3].astype(np.int64).sum()),
            "vertices_after": int(kept.sum()), "largest_before": int(hdrs[:, 3].max()),
            "largest_after": int(kept.max()), "largest_before_ring_after": int(kept[int(hdrs[:, 3].argmax())]), "counts_bytes": int(4 * n), "kept_bytes": int(8 * kept.sum()),
            "bytes_back": int(hdrs.nbytes + 4 * n + 8 * kept.sum()), "scratch_bytes": int(simp["scratch"].numel())},
        "obb_launch": summary(ms_obb) if ms_obb else None,
        "obb": None if not ms_obb else (lambda r: {
            "records_bytes": int(r.nbytes), "bytes_back_per_overlay": 4 * N.IPP_OBB_REC,
            "packed_bytes_per_overlay_mean": round(float(8 * hdrs[:, 3].astype(np.int64).sum()) / n, 1),
            "boxes": int((r[:, 7] >= 3).sum()), "largest_hull": int(r[:, 7].max()),
            "rows_spanned_max": int((hdrs[:, 3] > 0).any() and (scene_rows[:, 3] - scene_rows[:, 1]).max()),
            "scratch_bytes": int(obb["scratch"].numel())})(obb["rec"].cpu().numpy().reshape(n, N.IPP_OBB_REC)),
        "scene_launches": {name: summary(v) for name, v in per.items()},
        "copy_read_bytes": {"flat": flat_plan.copy_read_bytes, "scenes": scene_plan.copy_read_bytes},
        "composite_bytes": {"flat": out_flat.numel(), "scenes": out_scene.numel()},
        "scratch_label_bytes": int(scene._scratch.numel()),
    }))


if __name__ == "__main__":
    main()
