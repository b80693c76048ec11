"""Register/scratch budget of the label kernels (ipp_label.hip): no VGPR
spills and no scratch in ipp_pipe_overlay_bbox's and ipp_alpha_bbox_min's
kernels.  Compiles the file to ISA (CPU only) and reads the amdhsa metadata,
as tests/test_kernel_resources.py does for the pipe."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "image_processor_pipeline_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, str(ROOT))
from tools import kernel_res  # noqa: E402

KERNELS = ("k_pipe_overlay_bbox", "k_alpha_bbox_min")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_label_kernels_no_spills_no_scratch(tmp_path):
    out = tmp_path / "ipp_label.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}",
                    f"-I{CSRC}", "-S", "--cuda-device-only", str(CSRC / "ipp_label.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    seen = set()
    for k in kernel_res.kernels(str(out)):
        name = k.get("name") or ""
        hit = [h for h in KERNELS if h in name]
        if not hit:
            continue
        seen.add(hit[0])
        assert int(k.get("vgpr_spill_count", 0)) == 0, name
        assert int(k.get("sgpr_spill_count", 0)) == 0, name
        assert int(k.get("private_segment_fixed_size", 0)) == 0, name
        assert "scratch_" not in kernel_res.body(text, name), name
    assert seen == set(KERNELS)
    # the box kernel runs its taps on the matrix cores
    assert "v_mfma_i32_16x16x64_i8" in kernel_res.body(text, next(
        k["name"] for k in kernel_res.kernels(str(out)) if "k_pipe_overlay_bbox" in (k.get("name") or "")))
