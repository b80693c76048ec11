"""Scaffolding shared by the GPU tests of the scenes: the device, uploads, one
scene batch after its run, and the contour tracer driven through its two C
entries.  Imported after ``pytest.importorskip("torch")``."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import scene_refs as SR

DEV = "cuda:0"


def require_fused():
    """The ``fused`` module, or a skip without a GPU (each file's ``fused`` fixture)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from image_processor_pipeline_amd import fused as F
    return F


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_dev_copy(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared cases are read-only)


def current_stream():
    return torch.cuda.current_stream().cuda_stream


def same_polys(got, exp):
    assert len(got) == len(exp)
    for gs, es in zip(got, exp):
        assert len(gs) == len(es)
        for g, e in zip(gs, es):
            assert (g is None) == (e is None)
            if g is not None:
                assert g.dtype == np.int32 and g.shape == e.shape and np.array_equal(g, e)


class SceneBatch:
    """One planned scene batch (src, bgs, plan, cfg) after its run into an
    `out` pre-filled with 77, with the oracle's overlays."""

    def __init__(self, fused, batch):
        self.fused = fused
        self.src, self.bgs, self.plan, self.cfg = batch
        self.runner = fused.SceneRunner(self.plan, DEV)
        self.dsrc, self.dbgs = to_dev_copy(self.src), to_dev_copy(self.bgs)
        self.out = torch.full((self.plan.n_scenes,) + self.bgs.shape[1:], 77, dtype=torch.uint8, device=DEV)
        self.runner.run(self.dsrc, self.dbgs, self.out)
        self.overlays = SR.scene_overlays(self.src, self.plan, self.cfg)


def trace_contours(lib, case, max_edges, poison, slack):
    """Both C entries of the tracer on a handmade case (tests/contour_refs.py).
    The scratch is pre-filled with 0xA5, the headers and the vertex buffer with
    `poison`; the vertex buffer has `slack` pairs after the polygons.  Returns
    hdr (n, 8), verts (-1, 2), offsets, total on the host and d_hdr, d_verts,
    the device buffers."""
    from image_processor_pipeline_amd import _native as N
    n = len(case.rows)
    nb = lib.ipp_scene_contours_scratch_bytes(n, max_edges)
    assert nb == (32 * n + 255) // 256 * 256 + 2 * n * max_edges * 32          # the documented formula
    scratch = torch.full((nb,), 0xA5, dtype=torch.uint8, device=DEV)
    vis, rows, sl = to_dev_copy(case.vis), to_dev_copy(case.rows), to_dev_copy(case.scene_layer)
    hdr = torch.full((n * 8,), poison, dtype=torch.int32, device=DEV)
    N.check(lib.ipp_scene_contours(vis.data_ptr(), case.pitch, case.bg_w, case.bg_h, rows.data_ptr(), sl.data_ptr(),
                                   n, case.n_scenes, case.per_scene, max_edges, scratch.data_ptr(), hdr.data_ptr(),
                                   current_stream()), "ipp_scene_contours")
    h = hdr.cpu().numpy().reshape(n, 8)
    nv = h[:, 3].astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(nv)[:-1]]).astype(np.int64)
    total = int(nv.sum())
    verts = torch.full((2 * max(total + slack, 1),), poison, dtype=torch.int32, device=DEV)
    N.check(lib.ipp_scene_contours_pack(scratch.data_ptr(), hdr.data_ptr(), to_dev_copy(offsets).data_ptr(), n,
                                        max_edges, verts.data_ptr(), current_stream()), "ipp_scene_contours_pack")
    return SimpleNamespace(hdr=h, verts=verts.cpu().numpy().reshape(-1, 2), offsets=offsets, total=total,
                           d_hdr=hdr, d_verts=verts)
