"""Timing of the resizing device training batches ("Scenes":
ipp_scene_feed_resize against the chain a user writes without it).

    python tools/feed_resize_probe.py [--scenes 1024] [--size 1024] [--out-size 640] [--reps 20] [--warmup 3]
                                      [--seed 0] [--out FILE]

`scenes` random composites of size² (halved until the composites, the full-size
f16 images, the small ones and the chain's temporaries fit in the free memory).
Four things alternate rep by rep on one device, each timed with HIP events:
  resize_bilinear, resize_lanczos   ipp_scene_feed_resize into f16 at out-size²
          (3 B in and 6·(out/size)² B out per composite pixel);
  chain   ipp_scene_feed_images into full-size f16, then
          torch.nn.functional.interpolate(size=..., mode="bilinear",
          antialias=True): what a user writes today (3 + 6 B, then 6 B in and
          6·(out/size)² B out);
  copy    ipp_stream_copy over 1 GiB, the copy-kernel ceiling of bench.py --full.
The kernel's first and last images are checked against Pillow's resize of the
same composites through the same table.  Prints one JSON line (and writes it
to --out)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out-size", type=int, default=640)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from bench import copy_ceiling
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import fused
    from image_processor_pipeline_amd import geometry as G
    from image_processor_pipeline_amd.device import _stream, _to_dev

    dev = torch.device("cuda:0")
    lib, st = N.load(), _stream(dev)
    Z, O = args.size, args.out_size
    P, Q = Z * Z, O * O
    S = args.scenes
    free = torch.cuda.mem_get_info(dev)[0]
    while S > 1 and S * (P * (3 + 6) + Q * (6 + 6 + 12)) > 0.7 * free:  # composites, full f16, two small, the chain's temporaries
        S //= 2

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    comp = torch.randint(0, 256, (S, Z, Z, 3), dtype=torch.uint8, device=dev, generator=g)
    lut = fused.feed_lut(MEAN, STD, torch.float16).to(dev)
    full = torch.empty((S, 3, Z, Z), dtype=torch.float16, device=dev)
    small = torch.empty((S, 3, O, O), dtype=torch.float16, device=dev)
    taps = {}
    for name in ("bilinear", "lanczos"):
        k, t = G.resample_taps(name, Z, O)
        taps[name] = (k, _to_dev(t, dev).view(torch.int32))

    def resize(name):
        k, t = taps[name]
        N.check(lib.ipp_scene_feed_resize(comp.data_ptr(), small.data_ptr(), lut.data_ptr(), t.data_ptr(), t.data_ptr(), S,
                                          Z, Z, O, O, k, k, 2, 0, st), "ipp_scene_feed_resize")

    def chain():
        N.check(lib.ipp_scene_feed_images(comp.data_ptr(), full.data_ptr(), lut.data_ptr(), S, Z, Z, 2, 0, st), "feed")
        return torch.nn.functional.interpolate(full, size=(O, O), mode="bilinear", antialias=True)

    todo = (("resize_bilinear", lambda: resize("bilinear")), ("chain", chain), ("resize_lanczos", lambda: resize("lanczos")))
    ev = {name: [] for name, _ in todo}
    for rep in range(args.warmup + args.reps):
        for name, fn in todo:
            e = events(fn)
            if rep >= args.warmup:
                ev[name].append(e)
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}

    from PIL import Image
    for name, flt in (("lanczos", Image.Resampling.LANCZOS), ("bilinear", Image.Resampling.BILINEAR)):
        resize(name)
        for s in (0, S - 1):
            pil = np.asarray(Image.fromarray(comp[s].cpu().numpy()).resize((O, O), flt))
            exp = torch.stack([lut[c][torch.from_numpy(pil[:, :, c].astype(np.int64)).to(dev)] for c in range(3)])
            assert torch.equal(small[s], exp), (name, s)
    del full, small
    torch.cuda.empty_cache()
    ceiling = copy_ceiling(dev)

    k_bytes = S * (3 * P + 6 * Q)
    c_bytes = S * (3 * P + 6 * P + 6 * P + 6 * Q)
    res = {"images": f"{S} composites of {Z}x{Z} -> {O}x{O} f16", "reps": args.reps,
           "tile_lds": {n: int(lib.ipp_scene_feed_resize_lds(Z, Z, O, O, taps[n][0], taps[n][0], 2, None)) for n in taps},
           "ksize": {n: taps[n][0] for n in taps}, "copy_ceiling_GBps": round(ceiling, 1)}
    for name, nbytes in (("resize_bilinear", k_bytes), ("resize_lanczos", k_bytes), ("chain", c_bytes)):
        t = statistics.median(ms[name])
        gbps = nbytes / (t * 1e-3) / 1e9
        res[name] = {"median_ms": round(t, 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                     "bytes_per_composite_pixel": round(nbytes / (S * P), 2), "GBps": round(gbps, 1),
                     "frac_of_copy_ceiling": round(gbps / ceiling, 4),
                     "Mpix_per_s": round(S * P / (t * 1e-3) / 1e6, 1)}
    for name in ("resize_bilinear", "resize_lanczos"):
        res[f"chain_over_{name}"] = round(statistics.median(ms["chain"]) / statistics.median(ms[name]), 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
