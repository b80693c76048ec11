"""The emitted ISA of a kernel file, for the tests that read it (resource
budgets from the amdhsa metadata through tools/kernel_res, the gather-hazard
check through tools/asm_hazard): one hipcc command line, CPU only, and each
file compiled at most once per process."""
import functools
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "image_processor_pipeline_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, str(ROOT))
from tools import kernel_res  # noqa: E402

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

LDS_MAX = 64 * 1024


def compile_isa(src: Path, out: Path, inc: Path = CSRC, extra=()) -> None:
    """Device code of `src` as gfx950 assembly in `out`; `inc` holds the csrc
    headers, `extra` is further compiler flags."""
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}",
                    f"-I{inc}", *extra, "-S", "--cuda-device-only", str(src), "-o", str(out)], check=True,
                   capture_output=True)


@functools.lru_cache(maxsize=None)
def isa(name: str):
    """(path, text, kernels) of csrc/<name>.hip's ISA: the build's
    build/obj/<name>.s where it is newer than the file and every header,
    compiled here otherwise."""
    path = ROOT / "build" / "obj" / f"{name}.s"
    src = CSRC / f"{name}.hip"
    deps = [src] + list(CSRC.glob("*.h")) + [ROOT / "include" / "ipp.h"]
    if not (path.exists() and path.stat().st_mtime >= max(d.stat().st_mtime for d in deps)):
        path = Path(tempfile.mkdtemp(prefix="kernel_isa_")) / f"{name}.s"
        compile_isa(src, path)
    return path, path.read_text(), list(kernel_res.kernels(str(path)))


def clean(k, text):
    """No spill, no private segment, no scratch access, LDS within a CU's."""
    name = k["name"]
    assert int(k.get("vgpr_spill_count", 0)) == 0, name
    assert int(k.get("sgpr_spill_count", 0)) == 0, name
    assert int(k.get("private_segment_fixed_size", 0)) == 0, name
    assert "scratch_" not in kernel_res.body(text, name), name
    assert int(k.get("group_segment_fixed_size", 0)) <= LDS_MAX, name
