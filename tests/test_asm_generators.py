"""The generators of the assembly kernels (fidget_amd/csrc/gen_*.py) as a program: a run depends on nothing an earlier run left behind,
its kernels are the ones the library looks up, and an experiment switch it does not know ends it.  CPU only: the generators are run on
the offsets.json and trans_funcs.s the build leaves in csrc/_gen.  (That a change of the generators leaves the code object's bytes alone
is tools/gen_identity.py's business; what the bytes do, the emulator tests' - tests/test_emu_*.py.)"""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
TRANS = os.path.join(CSRC, "_gen", "trans_funcs.s")


@pytest.fixture(scope="module")
def gen():
    """(gen_asm, gen_interp, offsets)"""
    if CSRC not in sys.path:       # (it stays there: generate() imports the other generators when it runs)
        sys.path.insert(0, CSRC)
    import gen_asm
    import gen_interp
    with open(os.path.join(CSRC, "_gen", "offsets.json")) as f:
        return gen_asm, gen_interp, json.load(f)


@pytest.fixture(scope="module")
def two_runs(gen):
    """the product build's text, generated twice in this process (a run of its own each: no switch of the environment applies)"""
    gen_asm, gen_interp, off = gen
    return [gen_interp.generate(off, TRANS, a=gen_asm.Asm()) for _ in range(2)]


def test_a_second_run_in_the_process_gives_the_same_text(two_runs):
    """(the list of the embedded copies of the compiled routines, which fh_trans_probe is generated from, was a module's: a second run
    found the first run's copies in it)"""
    assert two_runs[0] == two_runs[1]
    assert two_runs[0].count(".amdhsa_kernel ") == 18


def test_the_kernels_are_the_ones_the_library_looks_up(two_runs, gen):
    """amdhsa.kernels' names = FH_ASM_NAMES (capi_core.hpp), as sets; and a build without the routines holds the rest"""
    with open(os.path.join(CSRC, "capi_core.hpp")) as f:
        m = re.search(r"FH_ASM_NAMES\[FH_ASM_COUNT\]\s*=\s*\{(.*?)\};", f.read(), re.S)
    wanted = re.findall(r'"(\w+)"', m.group(1))
    assert len(wanted) == len(set(wanted)) == 18
    names = lambda text: re.findall(r"^    \.name:\s+(\w+)$", text[text.index("amdhsa.kernels:"):], re.M)
    got = names(two_runs[0])
    assert len(got) == len(set(got)) and set(got) == set(wanted)
    gen_asm, gen_interp, off = gen
    plain = names(gen_interp.generate(off, None, a=gen_asm.Asm()))
    assert set(plain) == {n for n in wanted if not n.endswith("_t") and n != "fh_trans_probe"}


@pytest.mark.parametrize("text, unknown", [("nowork", "nowork"), ("nosqrt,nosuchswitch", "nosuchswitch"), ("twicesqr", "twicesqr"),
                                           ("vgpr", "vgpr"), ("nomod", "nomod")])
def test_an_unknown_switch_ends_the_run(gen, monkeypatch, text, unknown):
    gen_asm, gen_interp, off = gen
    with pytest.raises(SystemExit, match=f"'{unknown}'"):
        gen_asm.parse_switches(text)
    monkeypatch.setenv("FH_EXP", text)
    with pytest.raises(SystemExit, match=f"'{unknown}'"):
        gen_interp.generate(off, TRANS)


def test_the_known_switches_are_taken(gen):
    gen_asm = gen[0]
    known = ["nosqrt", "twicesqrt", "nosin", "noexp", "twiceexp", "nodiv", "nofastdiv", "twicediv", "nodelta", "file64", "vgpr160", "nointerp",
             "compiledsincos", "prune_nolive", "twiceln", "noatan"]
    assert gen_asm.parse_switches(",".join(known)) == set(known)
    assert gen_asm.parse_switches("") == set()
    a = gen_asm.Asm(gen_asm.parse_switches("nodiv,vgpr160"))
    assert a.vgpr_switch() == 160 and gen_asm.Asm().vgpr_switch() is None
