"""Static guard of the H pass's hand-waited gathers (gather
waits).  k_pipe_hpass2 issues its source gathers by inline asm and waits for
them by hand; a compiler copy, read or spill of a gather register before the
wait that names it would carry stale bytes.  tools/asm_hazard.py checks the
emitted ISA of every instantiation (control-flow-aware); this test runs it on
the build's ipp_pipe.s and on a mutation of the source that drops the
end-of-phase-2 waits (the round-2 structure: the next chunk's sets stayed in
flight across the loop's back edge, where the compiler copies them)."""
import re
import shutil

from tests.kernel_isa import CSRC, compile_isa, isa, needs_hipcc
from tools import asm_hazard


@needs_hipcc
def test_hpass_gathers_never_touched_in_flight(capsys):
    path = isa("ipp_pipe")[0]
    for pattern, least in (("k_pipe_hpass2", 24),):
        rc = asm_hazard.main(str(path), pattern)
        out = capsys.readouterr().out
        n = int(re.search(r"(\d+) kernels checked", out).group(1))
        assert n >= least, out     # every NR / zones / channels instantiation
        assert rc == 0, out        # no in-flight register touched, no scratch


@needs_hipcc
def test_checker_flags_waits_left_to_the_back_edge(tmp_path, capsys):
    src = (CSRC / "ipp_pipe.hip").read_text()
    waits = ("        asm_wait(RA.p, RA.live ? 4 * RB.live : -1);\n"
             "        asm_wait(RB.p, RB.live ? 0 : -1);\n        if (!more) break;")
    assert waits in src
    mutated = src.replace(waits, "        if (!more) break;")
    d = tmp_path / "mut"
    d.mkdir()
    for h in CSRC.glob("*.h"):
        shutil.copy(h, d)
    (d / "ipp_pipe.hip").write_text(mutated)
    compile_isa(d / "ipp_pipe.hip", d / "ipp_pipe.s", d)
    rc = asm_hazard.main(str(d / "ipp_pipe.s"))
    out = capsys.readouterr().out
    assert rc == 1 and "in-flight gather register" in out, out
