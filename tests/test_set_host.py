"""FrameReader::search_set_content_frames and lines_set_content_frames of the C++ host mirror (zarc_amd/host/zarc_host.hpp) on 1, 2 and 4
handles: identical results and identical summed hits (tests/host/set_frames_test.cpp checks that, built here with g++), and what one
handle answers equals Python's `re` over the entries' bytes (set_cases.ref)."""
import os
import subprocess

import pytest

import lines_cases as lc
import search_cases as sc
import set_cases as zs
from zarc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "set_frames_test.cpp")
NEEDLE = b"\x01Zarc\xfeNeedle"
PATS = [NEEDLE, b"Needle", b"zarc", b"\xfeN", b"the", NEEDLE]              # a prefix relation, a suffix, a duplicate, short ones


def build(out_dir, lib_dir, lib_name):
    exe = os.path.join(str(out_dir), "set_frames_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, SRC, "-L" + lib_dir, "-l" + lib_name,
                           "-Wl,-rpath," + lib_dir, "-pthread"])
    return exe


def entries(corpus):
    sizes = (0, 1, 300, 70000, 200000, 65536, 5000, 131073, 65543, 9)
    ents = [corpus.entry(9700 + i, n, 0 if n > 1000 else i & 3) for i, n in enumerate(sizes)]
    for i, e in enumerate(ents):
        if len(e) >= 65543: ents[i] = sc.plant(e, NEEDLE, [65536 - 5, len(e) - len(NEEDLE)])
        if len(e) == 5000: ents[i] = sc.plant(sc.plant(e, NEEDLE, [15]), NEEDLE.upper(), [1000])
    return ents


def run_case(exe, tmp_path, corpus, env, groups):
    ents = entries(corpus)
    d = tmp_path / "entries"
    d.mkdir()
    for i, e in enumerate(ents): (d / str(i)).write_bytes(e)
    (d / "patterns").write_bytes(b"".join(p + b"\n" for p in PATS))
    out = subprocess.check_output([exe, str(d), str(len(ents))], timeout=900, env=env).decode().splitlines()
    for g in groups:
        assert "search_set_content_frames on %d device(s) OK" % g in out and "search_set_content_frames (icase) on %d device(s) OK" % g in out
    assert any(l.startswith("set frames OK") for l in out)
    for icase in (False, True):
        R = [tuple(int(v) for v in l.split()[2:]) for l in out if l.startswith("R %d " % icase)]
        L = [tuple(int(v) for v in l.split()[2:]) for l in out if l.startswith("L %d " % icase)]
        H = [int(v) for v in next(l for l in out if l.startswith("H %d" % icase)).split()[2:]]
        assert len(R) == len(ents)
        want_hits, want_lines = [0] * len(PATS), []
        for i, e in enumerate(ents):
            _, status, count, first, which, lines = R[i]
            if i == 7:
                assert (status, count, first, which, lines) == (_lib.FRAME_SRCSIZE, 0, -1, -1, 0)
                want_lines.append([])
                continue
            c, f, w, per, union = zs.ref(e, PATS, icase)
            assert status == (_lib.FRAME_DIGEST if i == 4 else _lib.FRAME_OK)
            assert (count, first, which) == (c, -1 if f is None else f, -1 if w is None else w), (icase, i)
            want_hits = [a + b for a, b in zip(want_hits, per)]
            want_lines.append(zs.ref_lines(e, union))
            assert lines == len(want_lines[-1]), (icase, i)
        assert H == want_hits and H[0] == H[5] == (7 if icase else 6)   # 2 + 2 + 1 (the two copies overlap in the 65543-byte entry) + 1, and the upper-case copy
        exp = lc.deliver(ents, want_lines, max_lines=3, max_line=64, rec_cap=7)    # the caps the program asks for
        assert L == [(i, s, l, no, m, len(t)) for i, s, l, no, m, t in exp] and len(L) == 7      # nine lines pass max_lines: rec_cap cuts them, over the handles as on one


def test_set_content_frames_emulated(emu_lib_path, tmp_path, corpus):
    exe = build(tmp_path, os.path.dirname(emu_lib_path), "zarc_gpu_emu")
    run_case(exe, tmp_path, corpus, dict(os.environ, HIPEMU_DEVICES="4"), (1, 2, 4))


@pytest.mark.gpu
def test_set_content_frames_gpu(tmp_path, corpus):
    exe = build(tmp_path, os.path.join(ROOT, "zarc_amd"), "zarc_gpu")
    run_case(exe, tmp_path, corpus, None, (1,))
