"""Register/scratch/LDS budget of the scene kernels: the in-place V kernel
(ipp_pipe.hip k_pipe_vblend_over) and ipp_pipe_scene_boxes' kernels
(ipp_label.hip).  Compiles to ISA (CPU only) and reads the amdhsa metadata, as
tests/test_label_kernel_resources.py does; a resource check only."""
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

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

LDS_MAX = 64 * 1024


def _kernels(name: str, tmp_path: Path):
    built = ROOT / "build" / "obj" / f"{name}.s"
    src = CSRC / f"{name}.hip"
    deps = [src] + list(CSRC.glob("*.h")) + [ROOT / "include" / "ipp.h"]
    path = built
    if not (built.exists() and built.stat().st_mtime >= max(d.stat().st_mtime for d in deps)):
        path = tmp_path / f"{name}.s"
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}",
                        f"-I{CSRC}", "-S", "--cuda-device-only", str(src), "-o", str(path)], check=True,
                       capture_output=True)
    return list(kernel_res.kernels(str(path))), path.read_text()


def _clean(k, text):
    name = k["name"]
    assert int(k.get("vgpr_spill_count", 0)) == 0, name
    assert int(k.get("sgpr_spill_count", 0)) == 0, name
    assert int(k.get("private_segment_fixed_size", 0)) == 0, name
    assert "scratch_" not in kernel_res.body(text, name), name
    assert int(k.get("group_segment_fixed_size", 0)) <= LDS_MAX, name


def test_inplace_v_kernel_matches_its_sibling(tmp_path):
    ks, text = _kernels("ipp_pipe", tmp_path)
    over = {k["name"]: k for k in ks if "k_pipe_vblend_over" in (k.get("name") or "")}
    sib = {k["name"]: k for k in ks if "k_pipe_vblend_mfma" in (k.get("name") or "")}
    assert len(over) == 2 and len(sib) == 2                    # MAGIC and the reciprocal form of each
    for name, k in over.items():
        _clean(k, text)
        twin = next(s for n, s in sib.items() if ("ILb1E" in n) == ("ILb1E" in name))     # same MAGIC flag
        # the same static LDS (both take their rows as dynamic LDS sized by the
        # host from one formula) and the same occupancy class (≤ 160 registers
        # per lane: 3 waves per SIMD)
        assert int(k["group_segment_fixed_size"]) == int(twin["group_segment_fixed_size"]), name
        regs = int(k["vgpr_count"]) + int(k.get("agpr_count", 0))
        assert regs <= 160, (name, regs)


def test_scene_label_kernels_no_spills_no_scratch(tmp_path):
    ks, text = _kernels("ipp_label", tmp_path)
    want = ("k_scene_init", "k_scene_alpha", "k_scene_visible", "k_scene_finish")
    seen = set()
    for k in ks:
        hit = [w for w in want if w in (k.get("name") or "")]
        if hit:
            seen.add(hit[0])
            _clean(k, text)
    assert seen == set(want)
