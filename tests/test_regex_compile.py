"""The regular-expression compiler (zarc_amd/csrc/zre_compile.h) without an engine: zarc_gpu_regex_compile is handle-less, so the table it
makes is walked here on the CPU, in Python, the way the kernels walk it -- a line's bytes from the last to the first -- and compared with
Python's `re` (regex_cases.positions).  A fault found here is the compiler's, one found only in test_regex.py a kernel's.
tests/host/regex_compile_test.cpp is the compiler alone, as a stand-alone program: no library, no Python, no GPU."""
import os
import re
import subprocess

import pytest

import regex_cases as zr
from zarc_amd import _lib
from zarc_amd.engine import regex_compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def compile_fn(emu_lib_path):
    lib = _lib.load(emu_lib_path)
    return lambda rx, icase=False: regex_compile(lib, rx, icase)


def test_compile_random_tables_against_re(compile_fn):
    zr.check_random_tables(compile_fn)


def test_compile_state_counts(compile_fn):
    for m in (1, 2, 17, 62):                                                # a literal of m bytes: m + 1 states
        assert compile_fn(re.escape(bytes(range(0x80, 0x80 + m))))[0] == m + 1
    assert compile_fn(b".{4}a")[0] == 32 and compile_fn(b"a")[0] == 2
    assert compile_fn(b"[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}")[0] == 14   # the dotted quad fits with room to spare
    assert compile_fn(b"(GET|POST) /api")[0] == compile_fn(b"(POST|GET) /api")[0]      # minimised: the order of the branches does not matter
    assert compile_fn(b"x$$") == compile_fn(b"x$") and compile_fn(b"^^x") == compile_fn(b"^x") and compile_fn(b"(x)") == compile_fn(b"x")
    for rx in (b"abc", b"^a.*b$", b"[^a]+x", b"\\w+@\\w+\\.com$"):
        assert zr.accept_ok(compile_fn(rx))
        assert zr.accept_ok(compile_fn(rx, True))


def test_compile_walks_like_re(compile_fn):
    text = b"GET /api/v1 200 17 ms\nPOST /API/v2 500 1200 ms\r\nget /other 404 3 ms \n\nimport os\n import re\nerror: db timeout\nerror timeout error\n" \
           b"10.0.0.1 x\n999.1.22.333\n1.2.3\n\x00\xff\x80 \t.\nAx bx Cx dx @[ `{\nxx"
    cases = (b"error.*timeout", b"^import ", b"[0-9]+ ms$", b"(GET|POST) /api", b"[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}", b".", b"x$", b"^x", b"^$|x",
             b"\\S+\\s\\S+$", b"[\\x80-\\xff]+", b"\\0.", b"[a-c]x", b"[^a-c]x", b"@\\[|`\\{", b"(^| )[0-9]+( |$)", b"m?s$", b"\\d{3,}", b"\\t\\.")
    for rx in cases:
        for icase in (False, True):
            if rx == b"^$|x": continue
            got = zr.walk_table(compile_fn(rx, icase), text)
            assert got == zr.positions(text, rx, icase), (rx, icase, got[:5])
    zr.refused(lambda: compile_fn(b"^$|x"), _lib.E_PARAM, "offset 0:")


def test_compile_refusals(compile_fn):
    for rx, at in zr.BAD:
        zr.refused(lambda: compile_fn(rx), _lib.E_PARAM, "regex: offset %d:" % at)
    zr.refused(lambda: compile_fn(b".{7}a"), _lib.E_UNSUPPORTED, "needs 256 states", "limit is 64")
    zr.refused(lambda: compile_fn(re.escape(bytes(range(0x80, 0x80 + 100)))), _lib.E_UNSUPPORTED, "needs 101 states")
    zr.refused(lambda: compile_fn(b"(a{255}){255}"), _lib.E_UNSUPPORTED, "states")
    assert compile_fn(b"a" * 62)[0] == 63 and compile_fn(b"(((((((((a)))))))))")[0] == 2


def test_compile_standalone_program(tmp_path):
    exe = str(tmp_path / "regex_compile_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "zarc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "regex_compile_test.cpp"), "-o", exe])
    exprs = [b"abc", b"error.*timeout", b"^import ", b"[0-9]+ ms$", b"(GET|POST) /api", b".{4}a", b".{7}a", b"a*", b"(", b"[b-a]", b"a{3,2}", b"\\b", b"a**",
             b"\xff\xfe+", b"[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}", b"a{1,255}b", b"(a|b|c|d|e|f|g|h){1,200}z", b"((a*)*)*b", b"x" * 1025]
    src = tmp_path / "exprs.txt"
    src.write_bytes(b"\n".join(exprs) + b"\n")
    out = subprocess.run([exe, str(src)], stdout=subprocess.PIPE, check=True).stdout.split(b"\n")[:-1]
    assert len(out) == len(exprs)
    word = [o.split(b" ")[0] for o in out]
    assert word == [b"ok"] * 6 + [b"E_UNSUPPORTED"] + [b"E_PARAM"] * 6 + [b"ok", b"ok", b"E_UNSUPPORTED", b"E_UNSUPPORTED", b"ok", b"E_PARAM"], out
    assert out[0] == b"ok 4 0 1" and out[5].startswith(b"ok 32 ") and out[14].startswith(b"ok 14 ") and b"offset 1:" in out[9] and b"needs 257 states" in out[15]
    folded = subprocess.run([exe, str(src), "-i"], stdout=subprocess.PIPE, check=True).stdout.split(b"\n")[:-1]
    assert [o.split(b" ")[0] for o in folded] == word
