"""Timing of the device training batches ("Scenes":
ipp_scene_feed_images against the torch formulation, and the two small
launches beside the box and map launches they follow).

    python tools/feed_probe.py [--scenes 4096] [--size 1024] [--reps 20] [--warmup 3]
                               [--label-scenes 256] [--per-scene 3] [--backgrounds 16] [--seed 0] [--out FILE]

Part 1: `scenes` random composites of size² (halved until the composites, the
f16 and f32 images and the torch chain's temporaries fit in the free memory).
Three things alternate rep by rep on one device, each timed with HIP events:
  feed    ipp_scene_feed_images into f16 (9 B per pixel) and into f32 (15 B);
  torch   out.permute(0, 3, 1, 2).to(float16).sub_(mean).div_(std), what a user
          writes today;
  copy    ipp_stream_copy over 1 GiB, the copy-kernel ceiling of bench.py --full.
The kernel's images are checked against a torch gather through the same table.
Part 2: a planned batch of `label_scenes` × `per_scene` overlays after its run:
the box launch, ipp_scene_feed_targets, the map launch with boxes and
ipp_scene_feed_index_map, each alone.  Prints one JSON line (and writes it to
--out)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label-scenes", type=int, default=256)
    ap.add_argument("--per-scene", type=int, default=3)
    ap.add_argument("--backgrounds", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from bench import copy_ceiling, make_sources
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import fused
    from image_processor_pipeline_amd.device import _stream

    dev = torch.device("cuda:0")
    lib, st = N.load(), _stream(dev)
    Z = args.size
    P = Z * Z
    S = min(args.scenes, 4096)
    free = torch.cuda.mem_get_info(dev)[0]
    while S > 1 and S * P * (3 + 6 + 12 + 6 + 6) > 0.8 * free:     # composites, f16, f32, the chain's result and a temporary
        S //= 2

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    def med(v):
        return round(statistics.median(v), 4)

    # --- part 1 ---------------------------------------------------------------------------------------------
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    out = torch.randint(0, 256, (S, Z, Z, 3), dtype=torch.uint8, device=dev, generator=g)
    lut16 = fused.feed_lut(MEAN, STD, torch.float16).to(dev)
    lut32 = fused.feed_lut(MEAN, STD, torch.float32).to(dev)
    img16 = torch.empty((S, 3, Z, Z), dtype=torch.float16, device=dev)
    img32 = torch.empty((S, 3, Z, Z), dtype=torch.float32, device=dev)
    mean = torch.tensor(MEAN, dtype=torch.float16, device=dev).view(1, 3, 1, 1) * 255
    std = torch.tensor(STD, dtype=torch.float16, device=dev).view(1, 3, 1, 1) * 255

    def feed16():
        N.check(lib.ipp_scene_feed_images(out.data_ptr(), img16.data_ptr(), lut16.data_ptr(), S, Z, Z, 2, 0, st), "feed")

    def feed32():
        N.check(lib.ipp_scene_feed_images(out.data_ptr(), img32.data_ptr(), lut32.data_ptr(), S, Z, Z, 4, 0, st), "feed")

    def chain():
        return out.permute(0, 3, 1, 2).to(torch.float16).sub_(mean).div_(std)

    ev = {"feed16": [], "feed32": [], "torch": []}
    for rep in range(args.warmup + args.reps):
        for name, fn in (("feed16", feed16), ("torch", chain), ("feed32", feed32)):
            e = events(fn)
            if rep >= args.warmup:
                ev[name].append(e)
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    for c in range(3):                                               # the images are the table's entries
        for s in (0, S - 1):
            assert torch.equal(img16[s, c], lut16[c][out[s, :, :, c].long()])
            assert torch.equal(img32[s, c], lut32[c][out[s, :, :, c].long()])
    del img32
    torch.cuda.empty_cache()
    ceiling = copy_ceiling(dev)

    def gbps(bytes_per_pixel, t):
        return S * P * bytes_per_pixel / (t * 1e-3) / 1e9

    t16, t32, tch = statistics.median(ms["feed16"]), statistics.median(ms["feed32"]), statistics.median(ms["torch"])
    res = {
        "images": f"{S} composites of {Z}x{Z}", "reps": args.reps,
        "feed_f16_ms": {"median": med(ms["feed16"]), "min": round(min(ms["feed16"]), 4), "max": round(max(ms["feed16"]), 4)},
        "feed_f32_ms": {"median": med(ms["feed32"]), "min": round(min(ms["feed32"]), 4), "max": round(max(ms["feed32"]), 4)},
        "torch_chain_f16_ms": {"median": med(ms["torch"]), "min": round(min(ms["torch"]), 4),
                               "max": round(max(ms["torch"]), 4)},
        "torch_over_feed_f16": round(tch / t16, 2),
        "feed_f16_GBps": round(gbps(9, t16), 1), "feed_f32_GBps": round(gbps(15, t32), 1),
        "copy_ceiling_GBps": round(ceiling, 1),
        "feed_f16_frac_of_copy_ceiling": round(gbps(9, t16) / ceiling, 4),
        "feed_f32_frac_of_copy_ceiling": round(gbps(15, t32) / ceiling, 4),
        "feed_f16_Mpix_per_s": round(S * P / (t16 * 1e-3) / 1e6, 1),
    }
    del out, img16
    torch.cuda.empty_cache()

    # --- part 2 ---------------------------------------------------------------------------------------------
    LS, K, nbg = args.label_scenes, args.per_scene, args.backgrounds
    src = make_sources(0, LS * K, Z, args.seed, dev)
    g.manual_seed(1)
    bgs = torch.randint(0, 256, (nbg, Z, Z, 3), dtype=torch.uint8, device=dev, generator=g)
    plan = fused.plan_scenes((Z, Z), LS, K, (Z, Z), nbg, fused.PipeConfig(), seed=args.seed * 7919)
    runner = fused.SceneRunner(plan, dev)
    comp = torch.empty((LS, Z, Z, 3), dtype=torch.uint8, device=dev)
    runner.run(src, bgs, comp)
    fd = runner.feed(comp, mean=MEAN, std=STD, index_map=True)
    torch.cuda.synchronize()
    buf, rows = runner._launch_map("feed_probe", 1, 128, True, None)
    ibuf = torch.empty_like(buf)
    tg, cnt, slot = torch.empty_like(fd.targets), torch.empty_like(fd.count), torch.empty_like(fd.slot)

    def k_targets():
        N.check(lib.ipp_scene_feed_targets(rows.data_ptr(), runner._scene_layer.data_ptr(), None, LS * K, LS, K, Z, Z, 0,
                                           tg.data_ptr(), cnt.data_ptr(), slot.data_ptr(), st), "targets")

    def k_index():
        N.check(lib.ipp_scene_feed_index_map(buf.data_ptr(), buf.shape[2], Z, Z, slot.data_ptr(), LS, K, ibuf.data_ptr(),
                                             st), "index_map")

    parts = {"box_launch": lambda: runner._launch_boxes(1, 128), "feed_targets": k_targets,
             "map_launch_with_boxes": lambda: runner._launch_map("feed_probe", 1, 128, True, buf),
             "feed_index_map": k_index}
    ev2 = {k: [] for k in parts}
    for rep in range(args.warmup + args.reps):
        for name, fn in parts.items():
            e = events(fn)
            if rep >= args.warmup:
                ev2[name].append(e)
    torch.cuda.synchronize()
    assert torch.equal(tg, fd.targets) and torch.equal(slot, fd.slot) and torch.equal(ibuf, fd.index_map._base)
    res["labels"] = f"{LS} scenes x {K} layers, {Z}x{Z} backgrounds, {int(cnt.cpu()[0])} targets"
    for name, v in ev2.items():
        t = [a.elapsed_time(b) for a, b in v]
        res[name + "_ms"] = {"median": med(t), "min": round(min(t), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
