"""The forward table of zarc_gpu_regex_compile_ends (zarc_amd/csrc/zre_compile.h) without an engine: the call is handle-less, so the table is
walked here on the CPU, in Python, the way zarc_matches_*_regex walk it -- from a match's first byte towards the line's end -- and the end it
gives for every matching start position is compared with E(s) of the reference (only_cases.regex_end: Python's `re` with the rest of the
line pinned by a look-ahead).  A fault found here is the compiler's, one found only in test_only.py a kernel's.
The backward table of zarc_gpu_regex_compile must not have changed: tests/golden/regex_tables_before_only.json holds the SHA-256 of the
table the commit before this call existed made of every expression test_regex_compile.py compiles."""
import hashlib
import json
import os
import random
import re

import pytest

import only_cases as oc
import regex_cases as zr
from zarc_amd import _lib
from zarc_amd.engine import regex_compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALKS_LIKE_RE = (b"error.*timeout", b"^import ", b"[0-9]+ ms$", b"(GET|POST) /api", b"[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}", b".", b"x$", b"^x",
                 b"\\S+\\s\\S+$", b"[\\x80-\\xff]+", b"\\0.", b"[a-c]x", b"[^a-c]x", b"@\\[|`\\{", b"(^| )[0-9]+( |$)", b"m?s$", b"\\d{3,}", b"\\t\\.")
STATE_COUNTS = (b".{4}a", b"a", b"(GET|POST) /api", b"(POST|GET) /api", b"x$$", b"x$", b"^^x", b"^x", b"(x)", b"x", b"abc", b"^a.*b$", b"[^a]+x", b"\\w+@\\w+\\.com$",
                b"a" * 62, b"(((((((((a)))))))))") + tuple(re.escape(bytes(range(0x80, 0x80 + m))) for m in (1, 2, 17, 62))
TEXT = (b"GET /api/v1 200 17 ms\nPOST /API/v2 500 1200 ms\r\nget /other 404 3 ms \n\nimport os\n import re\nerror: db timeout\nerror timeout error\n"
        b"10.0.0.1 x\n999.1.22.333\n1.2.3\n\x00\xff\x80 \t.\nAx bx Cx dx @[ `{\nxx")


@pytest.fixture(scope="module")
def lib(emu_lib_path):
    return _lib.load(emu_lib_path)


def table_end(table, line, s):
    """E(s) as the forward table gives it, or None: the walk of include/zarc_gpu.h, zarc_gpu_regex_compile_ends"""
    states, start, accept, delta = table
    dead = states - 1
    q, end = (delta[start * 256 + 0x0A] if s == 0 else start), None
    for j in range(s, len(line)):
        q = delta[q * 256 + line[j]]
        if q == dead: break
        if accept[q] & 1 or (accept[q] & 2 and j + 1 == len(line)): end = j + 1
    return end


def table_ok(table):
    states, start, accept, delta = table
    dead = states - 1
    first = delta[start * 256 + 0x0A]
    if states == 1: return start == 0 and accept[0] == 0 and not any(delta)          # an expression that matches nothing (c^): DEAD alone
    # (start == dead: a match starts at a line's first byte or nowhere, as with ^bb)
    return (2 <= states <= 64 and start <= dead and first < states and max(delta) < states and accept[dead] == 0 and accept[start] == 0
            and all(delta[dead * 256 + b] == dead for b in range(256) if b != 0x0A) and all(delta[q * 256 + 0x0A] == dead for q in range(states) if q != start))


def check_lines(lib, rx, lines, icase=False):
    """-> the starts compared"""
    table = regex_compile(lib, rx, icase, ends=True)
    assert table_ok(table), (rx, table[0])
    n = 0
    for line in lines:
        for s in zr.positions(line, rx, icase):
            assert table_end(table, line, s) == oc.regex_end(line, s, rx, icase), (rx, icase, line, s)
            n += 1
    return n


def test_ends_random_expressions_against_re(lib):
    exprs = zr.random_cases()[0]
    rnd = random.Random(zr.SEED + 9)
    lines = [bytes(rnd.choice(b"aabbc.") for _ in range(rnd.randrange(0, 14))) for _ in range(60)] + [b"abcabcabcabcabcabcabcab", b"a" * 20, b""]
    total = sum(check_lines(lib, e, lines) for e in exprs)
    assert total > 50 * len(exprs)


def test_ends_leftmost_longest_expressions(lib):
    lines = oc.SMALL.split(b"\n")
    for rx in oc.REGEXES + (b"a[^z]*z", b"id=[0-9]+", b"[a-z]+cr ", b"(a|b)*a(a|b){4}", b"x($|g)", b"(^|g)x", b"^(a|b)+$", b"^^a$$|b"):
        assert check_lines(lib, rx, lines + [b"az" + b"a" * 50, b"gx xg x", b"abba", b"id=12 id=x id=0007", b"odnwnecr xcr cr "]) >= 1, rx
    for rx in WALKS_LIKE_RE:
        for icase in (False, True):
            assert check_lines(lib, rx, TEXT.split(b"\n"), icase) >= 1, rx
    assert check_lines(lib, b"ab", [b"xAbaB"], icase=True) == 2


def test_ends_refusals(lib):
    fn = lambda rx: regex_compile(lib, rx, ends=True)
    for rx, at in zr.BAD:                                                   # refusals and messages are zarc_gpu_regex_compile's
        zr.refused(lambda: fn(rx), _lib.E_PARAM, "regex: offset %d:" % at)
    # an expression the backward table has room for and the forward table has not: the message gives the number needed
    assert regex_compile(lib, b"(a|b)*a(a|b){6}")[0] <= 64
    zr.refused(lambda: fn(b"(a|b)*a(a|b){6}"), _lib.E_UNSUPPORTED, "needs 129 states", "limit is 64")
    assert fn(b"(a|b)*a(a|b){4}")[0] == 33                                  # which of the last five bytes were an a: 2^5 states (`start` is the one without any), and DEAD
    assert fn(b".{7}a")[0] == 10 and fn(b"a")[0] == 3                       # what the backward table cannot hold is a chain forwards
    assert fn(b"a" * 62)[0] == 64
    zr.refused(lambda: fn(b"a" * 63), _lib.E_UNSUPPORTED, "needs 65 states")


def test_backward_tables_are_what_they_were(lib):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "regex_tables_before_only.json")))
    exprs = [(e, False) for e in zr.random_cases()[0]] + [(e, ic) for e in WALKS_LIKE_RE + STATE_COUNTS for ic in (False, True)]
    assert len(want) == len(set(exprs)) > 350
    for rx, icase in exprs:
        states, start, accept, delta = regex_compile(lib, rx, icase)
        got = hashlib.sha256(b"%d %d " % (states, start) + accept + delta).hexdigest()
        assert got == want["%s %d" % (rx.hex(), icase)], (rx, icase)
