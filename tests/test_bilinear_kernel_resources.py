"""k_rotate_bilinear (ipp_bilinear.hip) is bit-exact with Pillow only while no
multiply-add of its double arithmetic is fused: Geometry.c's a0·x + a1·y + a2
and a + (b - a)·d round after every operation, and the truncation to uint8
exposes the last bit.  The file's ``#pragma clang fp contract(off)`` is what
holds that wherever the file is compiled without the Makefile's
``-ffp-contract=off`` (as tests/kernel_isa.py does), so the emitted ISA is
read here: no fused multiply-add of any width in the kernel, and — the control
— at least one as soon as the pragma is gone and contraction is allowed.
CPU only."""
import shutil

from tests.kernel_isa import CSRC, clean, compile_isa, isa, needs_hipcc
from tools import kernel_res

pytestmark = needs_hipcc

KERNEL = "k_rotate_bilinear"
PRAGMA = "#pragma clang fp contract(off)"


def _fused(text: str, name: str):
    """Instructions of kernel `name` whose mnemonic names a fused multiply-add
    (v_fma_*, v_fmac_*, v_fmamk_*, v_pk_fma_*, ...)."""
    out = []
    for line in kernel_res.body(text, name).splitlines():
        tok = line.split(";")[0].split()
        if tok and not tok[0].startswith(".") and not tok[0].endswith(":") and "fma" in tok[0]:
            out.append(line.strip())
    return out


def _kernel(ks):
    found = [k for k in ks if KERNEL in (k.get("name") or "")]
    assert len(found) == 1, [k.get("name") for k in ks]
    return found[0]


def test_rotate_bilinear_has_no_fused_multiply_add():
    _, text, ks = isa("ipp_bilinear")
    k = _kernel(ks)
    clean(k, text)
    body = kernel_res.body(text, k["name"])
    assert "v_mul_f64" in body and "v_add_f64" in body          # the double arithmetic is there to be fused
    assert _fused(text, k["name"]) == []


def test_contraction_would_fuse_it(tmp_path):
    """The control: the same file without the pragma, contraction allowed."""
    src = (CSRC / "ipp_bilinear.hip").read_text()
    assert src.count(PRAGMA) == 1
    for h in CSRC.glob("*.h"):
        shutil.copy(h, tmp_path / h.name)
    (tmp_path / "ipp_bilinear.hip").write_text(src.replace(PRAGMA, ""))
    out = tmp_path / "ipp_bilinear.s"
    compile_isa(tmp_path / "ipp_bilinear.hip", out, tmp_path, extra=("-ffp-contract=fast",))
    text = out.read_text()
    k = _kernel(list(kernel_res.kernels(str(out))))
    assert _fused(text, k["name"]), "contraction allowed and nothing fused: the check above proves nothing"
