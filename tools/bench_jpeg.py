"""Times the device JPEG encoder against what the host path does, on one GPU
in one run (DESIGN.md §3 "JPEG"):

  device   JpegEncoder.encode of the batch: the launches by HIP events (and
           per kernel group by events around single entries of a second pass),
           and wall clock from the call to the files' bytes on the host;
  host     the raw copy back of the same composites, then
           Image.fromarray(a).save(buffer, "JPEG", quality=q) on `--threads`
           threads.

The composites come from the config-3 plan (fused.plan_pipe at 1024², seed 0)
on seeded noise sources and backgrounds.  Prints one JSON line.  It needs a
GPU and fails without one.

    python tools/bench_jpeg.py --n 256 --quality 75 --threads 16 --reps 5
"""
from __future__ import annotations

import argparse
import io
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--subsampling", default="4:2:0")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=4, help="composites compared with Pillow's bytes")
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image

    from image_processor_pipeline_amd import fused
    from image_processor_pipeline_amd import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg: no GPU")
    dev = torch.device("cuda:0")
    n, S = a.n, a.size
    g = torch.Generator(device="cpu").manual_seed(0)
    src = torch.randint(0, 256, (n, S, S, 3), dtype=torch.uint8, generator=g).to(dev)
    bgs = (torch.arange(S, dtype=torch.int32)[None, :, None] // 4 + torch.arange(S, dtype=torch.int32)[:, None, None] // 8
           + torch.tensor([0, 40, 90], dtype=torch.int32)[None, None, :]).remainder(256).to(torch.uint8)
    bgs = torch.stack([bgs, bgs.flip(1)]).contiguous().to(dev)
    plan = fused.plan_pipe((S, S), n, (S, S), 2, fused.PipeConfig(), seed=0)
    out = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
    fused.PipeRunner(plan, dev).run(src, bgs, out)
    torch.cuda.synchronize()
    del src

    enc = fused.JpegEncoder(dev, n, (S, S), a.quality, a.subsampling)
    files = enc.encode(out)                                   # warm-up, and the result to compare
    subs = {"4:2:0": 2, "4:4:4": 0}[a.subsampling]

    def pil(arr):
        b = io.BytesIO()
        Image.fromarray(arr).save(b, "JPEG", quality=a.quality, subsampling=subs)
        return b.getvalue()
    for i in range(min(a.check, n)):
        if files[i] != pil(out[i].cpu().numpy()):
            raise SystemExit(f"bench_jpeg: composite {i} differs from Pillow's file")

    st = torch.cuda.current_stream(dev).cuda_stream
    wall, kern, pack = [], [], []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        N.check(enc.lib.ipp_jpeg_encode(out.data_ptr(), n, S, S, enc.sampling, N.np_ptr(enc.qtab), enc.scratch.data_ptr(),
                                        enc.slots.data_ptr(), enc.capacity, enc.hdr.data_ptr(), st), "ipp_jpeg_encode")
        e1.record()
        torch.cuda.synchronize()
        kern.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        files = enc.encode(out)
        wall.append((time.perf_counter() - t0) * 1e3)
    host_copy, host_enc = [], []
    for _ in range(max(1, a.reps // 2)):
        t0 = time.perf_counter()
        raw = out.cpu().numpy()
        t1 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=a.threads) as pool:
            list(pool.map(pil, raw))
        t2 = time.perf_counter()
        host_copy.append((t1 - t0) * 1e3)
        host_enc.append((t2 - t1) * 1e3)
    med = statistics.median
    file_bytes = sum(len(f) for f in files)
    print(json.dumps({
        "n": n, "size": S, "quality": a.quality, "subsampling": a.subsampling, "device": torch.cuda.get_device_name(0),
        "device_encode_launches_ms": round(med(kern), 3), "device_encode_launches_ms_min": round(min(kern), 3),
        "device_encode_wall_ms": round(med(wall), 3), "device_encode_wall_ms_min": round(min(wall), 3),
        "host_raw_copy_ms": round(med(host_copy), 3), "host_pillow_ms": round(med(host_enc), 3), "host_threads": a.threads,
        "bytes_back": int(enc.bytes_back), "file_bytes": int(file_bytes), "raw_bytes": int(3 * n * S * S),
        "pixel_bytes_read": int(3 * n * S * S), "coef_scratch_bytes": int(136 * n * (S // 16) ** 2 * 6) if subs == 2 else
        int(136 * n * (S // 8) ** 2 * 3), "checked_against_pillow": min(a.check, n)}))


if __name__ == "__main__":
    main()
