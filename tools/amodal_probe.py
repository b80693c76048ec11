"""The amodal launch against the map launch it extends ("Amodal labels").

    python tools/amodal_probe.py [--scenes 1024] [--per-scene 4] [--size 1024] [--backgrounds 16]
                                 [--steps 20] [--warmup 3] [--seed 0]

Workload: tools/scene_probe.py's — S scenes × K overlays of size² sources on
size² backgrounds with the config-3 parameters.  After one scene run, every
step times, one after the other on the current stream with HIP events:
ipp_pipe_scene_map with the rows (the parent's boxes-and-map call),
ipp_pipe_scene_amodal with every output (arows, occ, presence map, rows,
visibility map), and ipp_pipe_scene_amodal with arows and occ alone.  Checks
that the visible outputs of the two entries are identical, and prints one JSON
line."""
import argparse
import json
import statistics
import sys
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
    args = ap.parse_args()

    import torch
    from bench import make_sources
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import fused
    from image_processor_pipeline_amd.device import _stream

    dev = torch.device("cuda:0")
    S, K, Z, nbg = args.scenes, args.per_scene, args.size, args.backgrounds
    n = S * K
    src = make_sources(0, n, Z, args.seed, dev)
    g0 = torch.Generator(device=dev)
    g0.manual_seed(1)
    bgs = torch.randint(0, 256, (nbg, Z, Z, 3), dtype=torch.uint8, device=dev, generator=g0)
    plan = fused.plan_scenes((Z, Z), S, K, (Z, Z), nbg, fused.PipeConfig(), seed=args.seed * 7919)
    scene = fused.SceneRunner(plan, dev)
    out = torch.empty((S, Z, Z, 3), dtype=torch.uint8, device=dev)
    scene.run(src, bgs, out)
    scene._scene_scratch("amodal_probe")
    p, lib, st = plan.pipe, scene.lib, _stream(dev)
    pitch = fused.scene_map_pitch(Z)
    vis, vis2, amap = (torch.empty((S, Z, pitch), dtype=torch.uint8, device=dev) for _ in range(3))
    rows, rows2, arows = (torch.empty(6 * n, dtype=torch.int32, device=dev) for _ in range(3))
    occ = torch.empty((S, 2, K, K), dtype=torch.int32, device=dev)
    head = (scene.tmp.data_ptr(), scene.coefs.data_ptr(), scene._dptr(0), scene._scene_layer.data_ptr(), n, S, K,
            p.bg_w, p.bg_h, p.max_ov_w, p.max_ov_h, 1, 128, p.tap_format, scene._scratch.data_ptr())

    def map_rows():
        N.check(lib.ipp_pipe_scene_map(*head, rows.data_ptr(), vis.data_ptr(), pitch, st), "ipp_pipe_scene_map")

    def amodal_all():
        N.check(lib.ipp_pipe_scene_amodal(*head, arows.data_ptr(), occ.data_ptr(), amap.data_ptr(), rows2.data_ptr(),
                                          vis2.data_ptr(), pitch, st), "ipp_pipe_scene_amodal")

    def amodal_counts():
        N.check(lib.ipp_pipe_scene_amodal(*head, arows.data_ptr(), occ.data_ptr(), None, None, None, pitch, st),
                "ipp_pipe_scene_amodal")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    calls = (("map_with_rows", map_rows), ("amodal_all_outputs", amodal_all), ("amodal_rows_and_occ", amodal_counts))
    ms = {name: [] for name, _ in calls}
    for step in range(args.warmup + args.steps):
        evs = [(name, timed(fn)) for name, fn in calls]
        torch.cuda.synchronize(dev)
        if step >= args.warmup:
            for name, (a, b) in evs:
                ms[name].append(a.elapsed_time(b))
    amodal_all()
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(rows, rows2)) and bool(torch.equal(vis, vis2))
    o = occ.cpu().numpy()

    def summary(v):
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    print(json.dumps({
        "device": torch.cuda.get_device_name(dev), "scenes": S, "per_scene": K, "size": Z, "backgrounds": nbg,
        "steps": args.steps, "warmup": args.warmup, **{name: summary(v) for name, v in ms.items()},
        "ratio_all_over_map": round(statistics.median(ms["amodal_all_outputs"]) /
                                    statistics.median(ms["map_with_rows"]), 3),
        "visible_outputs_identical": same, "map_bytes": int(vis.numel()),
        "pairs_covering": int(sum((o[:, 0, k, j] > 0).sum() for k in range(K) for j in range(k + 1, K))),
    }))
    if not same:
        sys.exit("the visible rows or map of the two entries differ")


if __name__ == "__main__":
    main()
