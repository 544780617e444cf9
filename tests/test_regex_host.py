"""FrameReader::search_regex_content_frames and lines_regex_content_frames of the C++ host mirror (zarc_amd/host/zarc_host.hpp) on 1, 2 and
4 handles: identical results (tests/host/regex_frames_test.cpp checks that, built here with g++), and what one handle answers equals
Python's `re` over the entries' bytes, line by line (regex_cases.positions)."""
import os
import subprocess

import pytest

import lines_cases as lc
import regex_cases as zr
import search_cases as sc
import set_cases as zs
from zarc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "regex_frames_test.cpp")
EXPRS = [b"Zarc.*Needle$|^odn", b"[a-z]+, ?[a-z]+ sj", b"\xfe[N-P]e+dle"]


def build(out_dir, lib_dir, lib_name):
    exe = os.path.join(str(out_dir), "regex_frames_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, SRC, "-L" + lib_dir, "-l" + lib_name,
                           "-Wl,-rpath," + lib_dir, "-pthread"])
    return exe


def entries(corpus):
    sizes = (0, 1, 300, 70000, 200000, 65536, 5000, 131073, 65543, 9)
    ents = [corpus.entry(9700 + i, n, 0 if n > 1000 else i & 3) for i, n in enumerate(sizes)]
    needle = b" Zarc then \xfeNeedle\n"
    for i, e in enumerate(ents):
        if len(e) >= 65543: ents[i] = sc.plant(e, needle, [65536 - 15, len(e) - len(needle)])   # across the slice boundary, and at the frame's end
        if len(e) == 5000: ents[i] = sc.plant(sc.plant(e, needle, [15]), needle.upper(), [1000])
    return ents


def run_case(exe, tmp_path, corpus, env, groups):
    ents = entries(corpus)
    d = tmp_path / "entries"
    d.mkdir()
    for i, e in enumerate(ents): (d / str(i)).write_bytes(e)
    (d / "expressions").write_bytes(b"".join(p + b"\n" for p in EXPRS))
    out = subprocess.check_output([exe, str(d), str(len(ents))], timeout=900, env=env).decode().splitlines()
    assert any(l.startswith("regex frames OK") for l in out)
    seen = 0
    for x, rx in enumerate(EXPRS):
        for icase in (False, True):
            for g in groups:
                assert "search_regex_content_frames %d%s on %d device(s) OK" % (x, " (icase)" if icase else "", g) in out
            R = [tuple(int(v) for v in l.split()[3:]) for l in out if l.startswith("R %d %d " % (x, icase))]
            L = [tuple(int(v) for v in l.split()[3:]) for l in out if l.startswith("L %d %d " % (x, icase))]
            assert len(R) == len(ents)
            want_lines = []
            for i, e in enumerate(ents):
                _, status, count, first, lines = R[i]
                if i == 7:
                    assert (status, count, first, lines) == (_lib.FRAME_SRCSIZE, 0, -1, 0)
                    want_lines.append([])
                    continue
                pos = zr.positions(e, rx, icase)
                assert status == (_lib.FRAME_DIGEST if i == 4 else _lib.FRAME_OK)
                assert (count, first) == (len(pos), pos[0] if pos else -1), (rx, icase, i)
                want_lines.append(zs.ref_lines(e, pos))
                assert lines == len(want_lines[-1]), (rx, icase, i)
                seen += count
            exp = lc.deliver(ents, want_lines, max_lines=3, max_line=64, rec_cap=7)    # the caps the program asks for
            assert L == [(i, s, l, no, m, len(t)) for i, s, l, no, m, t in exp], (rx, icase)
    assert seen > 20


def test_regex_content_frames_emulated(emu_lib_path, tmp_path, corpus):
    exe = build(tmp_path, os.path.dirname(emu_lib_path), "zarc_gpu_emu")
    run_case(exe, tmp_path, corpus, dict(os.environ, HIPEMU_DEVICES="4"), (1, 2, 4))


@pytest.mark.gpu
def test_regex_content_frames_gpu(tmp_path, corpus):
    exe = build(tmp_path, os.path.join(ROOT, "zarc_amd"), "zarc_gpu")
    run_case(exe, tmp_path, corpus, None, (1,))
