"""Timing of the letterboxed device training batches ("Scenes":
ipp_scene_feed_letterbox and ipp_scene_feed_targets_letterbox against the form
composed from the entries of before and torch).

    python tools/feed_letterbox_probe.py [--scenes 256] [--out-size 640] [--reps 30] [--warmup 5] [--seed 0]
                                         [--step-seconds 240] [--out FILE]

Two geometries, each in a child process of its own that is ended after
--step-seconds: `scenes` random composites of 1024 x 1024 (the workload's; the
rectangle is the whole 640² canvas) and of 1920 x 1080 (640 x 360 at top 140),
into f16, BILINEAR and LANCZOS.  Per geometry and filter two things alternate
rep by rep on one device, each timed with HIP events:
  letterbox  ipp_scene_feed_letterbox into the canvas, then
             ipp_scene_feed_targets_letterbox: two launches;
  composed   ipp_scene_feed_resize into a temporary of the rectangle's size, a
             new canvas filled plane by plane with the pad's table word (what
             torch.full launches; the three words differ), the slice copy,
             ipp_scene_feed_targets, and the rows moved and scaled column by
             column with torch ops (float32; no stated rounding rule).
The canvases of the two must be equal bit for bit.  Prints one JSON line per
geometry (and appends them to --out)."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CASES = {"1024x1024": (1024, 1024), "1920x1080": (1920, 1080)}
K_LAYERS, PAD = 4, 114


def run_case(args):
    import numpy as np
    import torch
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import fused
    from image_processor_pipeline_amd import geometry as G
    from image_processor_pipeline_amd.device import _stream, _to_dev

    dev = torch.device("cuda:0")
    lib, st = N.load(), _stream(dev)
    bw, bh = CASES[args.case]
    S, K = args.scenes, K_LAYERS
    geo = fused.letterbox_geometry((bh, bw), args.out_size)
    rect = (geo.new_w, geo.new_h, geo.left, geo.top, geo.out_w, geo.out_h)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    comp = torch.randint(0, 256, (S, bh, bw, 3), dtype=torch.uint8, device=dev, generator=g)
    lut = fused.feed_lut(MEAN, STD, torch.float16).to(dev)
    canvas = torch.empty((S, 3, geo.out_h, geo.out_w), dtype=torch.float16, device=dev)
    small = torch.empty((S, 3, geo.new_h, geo.new_w), dtype=torch.float16, device=dev)
    # rows of S·K boxes inside the background, all visible; descriptors in scene, layer order
    rng = np.random.default_rng(args.seed)
    x0, y0 = rng.integers(0, bw - 1, S * K), rng.integers(0, bh - 1, S * K)
    x1, y1 = x0 + 1 + rng.integers(0, bw - x0 - 1), y0 + 1 + rng.integers(0, bh - y0 - 1)
    area = (x1 - x0) * (y1 - y0)
    rows = _to_dev(np.stack([x0, y0, x1, y1, area, area], axis=1).astype(np.int32), dev).view(torch.int32)
    q = np.arange(S * K)
    scene_layer = _to_dev(np.stack([q // K, q % K], axis=1).astype(np.int32), dev).view(torch.int32)
    targets = torch.empty((S * K, 6), dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    slot = torch.empty((S, K), dtype=torch.int32, device=dev)
    taps = {}
    for name in ("bilinear", "lanczos"):
        taps[name] = tuple((k, _to_dev(t, dev).view(torch.int32)) for k, t in (
            G.identity_taps(n) if n == m else G.resample_taps(name, n, m) for n, m in ((bw, geo.new_w), (bh, geo.new_h))))
    pad_words = [float(v) for v in lut[:, PAD].cpu()]

    def letterbox(name):
        (kx, tx), (ky, ty) = taps[name]
        N.check(lib.ipp_scene_feed_letterbox(comp.data_ptr(), canvas.data_ptr(), lut.data_ptr(), tx.data_ptr(),
                                             ty.data_ptr(), S, bw, bh, *rect, kx, ky, PAD, 2, 0, st), "letterbox")
        N.check(lib.ipp_scene_feed_targets_letterbox(rows.data_ptr(), scene_layer.data_ptr(), None, S * K, S, K, bw, bh, 0,
                                                     *rect, targets.data_ptr(), count.data_ptr(), slot.data_ptr(), st),
                "targets_letterbox")
        return canvas

    def composed(name):
        (kx, tx), (ky, ty) = taps[name]
        N.check(lib.ipp_scene_feed_resize(comp.data_ptr(), small.data_ptr(), lut.data_ptr(), tx.data_ptr(), ty.data_ptr(),
                                          S, bw, bh, geo.new_w, geo.new_h, kx, ky, 2, 0, st), "resize")
        out = torch.empty((S, 3, geo.out_h, geo.out_w), dtype=torch.float16, device=dev)
        for c in range(3):                                      # torch.full's fill, one per plane: the pad words differ
            out[:, c].fill_(pad_words[c])
        out[:, :, geo.top:geo.top + geo.new_h, geo.left:geo.left + geo.new_w] = small
        N.check(lib.ipp_scene_feed_targets(rows.data_ptr(), scene_layer.data_ptr(), None, S * K, S, K, bw, bh, 0,
                                           targets.data_ptr(), count.data_ptr(), slot.data_ptr(), st), "targets")
        kept = targets[:, 0] >= 0                               # the unused rows stay -1
        targets[:, 2] = torch.where(kept, targets[:, 2] * (geo.new_w / geo.out_w) + geo.left / geo.out_w, targets[:, 2])
        targets[:, 3] = torch.where(kept, targets[:, 3] * (geo.new_h / geo.out_h) + geo.top / geo.out_h, targets[:, 3])
        targets[:, 4] = torch.where(kept, targets[:, 4] * (geo.new_w / geo.out_w), targets[:, 4])
        targets[:, 5] = torch.where(kept, targets[:, 5] * (geo.new_h / geo.out_h), targets[:, 5])
        return out

    def timed(fn, name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(name)
        b.record()
        return a, b

    res = {"case": f"{S} composites of {bw}x{bh} -> {geo.new_w}x{geo.new_h} at ({geo.left}, {geo.top}) of "
                   f"{geo.out_w}x{geo.out_h} f16, {S * K} rows", "reps": args.reps}
    P, Q, R = bw * bh, geo.out_w * geo.out_h, geo.new_w * geo.new_h
    model = {"letterbox": 3 * P + 6 * Q, "composed": 3 * P + 6 * R + 6 * Q + 6 * R + 6 * R}
    for name in ("bilinear", "lanczos"):
        assert torch.equal(letterbox(name).view(torch.int16), composed(name).view(torch.int16)), name
        ev = {"letterbox": [], "composed": []}
        for rep in range(args.warmup + args.reps):
            for what, fn in (("letterbox", letterbox), ("composed", composed)):
                e = timed(fn, name)
                if rep >= args.warmup:
                    ev[what].append(e)
        torch.cuda.synchronize()
        ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
        r = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                 "bytes_per_composite_pixel": round(model[k] / P, 3)} for k, v in ms.items()}
        r["composed_over_letterbox"] = round(statistics.median(ms["composed"]) / statistics.median(ms["letterbox"]), 3)
        res[name] = r
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--out-size", type=int, default=640)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", choices=list(CASES), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case:
        return run_case(args)
    lines = []
    for case in CASES:      # one fresh process per geometry; the first that fails or runs out of time ends the probe
        cmd = [sys.executable, str(Path(__file__).resolve()), "--case", case] + [
            f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("scenes", "out_size", "reps", "warmup", "seed")]
        done = subprocess.run(cmd, timeout=args.step_seconds, capture_output=True, text=True, cwd=str(ROOT))
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            sys.exit(f"{case}: exit status {done.returncode}")
        lines.append(done.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
