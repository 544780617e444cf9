"""The LineSelect argument of FrameReader's lines calls in the C++ host mirror (zarc_amd/host/zarc_host.hpp) on 1, 2 and 4 handles: identical
hit lines, selected lines and records under every cap and for all three matchers, the verdict and counts of search_content_frames, the lines
of a plain host scan (tests/host/select_frames_test.cpp, built here with g++)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "select_frames_test.cpp")
SELECTIONS = (b"-B 2 -A 2", b"-v -B 0 -A 0", b"-v -B 1 -A 3", b"-B 4294967295 -A 0", b"-B 0 -A 1")


def build(out_dir, lib_dir, lib_name):
    exe = os.path.join(str(out_dir), "select_frames_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, SRC, "-L" + lib_dir, "-l" + lib_name,
                           "-Wl,-rpath," + lib_dir, "-pthread"])
    return exe


def test_select_content_frames_emulated(emu_lib_path, tmp_path):
    exe = build(tmp_path, os.path.dirname(emu_lib_path), "zarc_gpu_emu")
    out = subprocess.check_output([exe], timeout=900, env=dict(os.environ, HIPEMU_DEVICES="4"))
    for g in (1, 2, 4):
        for s in SELECTIONS:
            assert b"select %s on %d device(s) OK" % (s, g) in out
    assert b"select frames OK" in out


@pytest.mark.gpu
def test_select_content_frames_gpu(tmp_path):
    exe = build(tmp_path, os.path.join(ROOT, "zarc_amd"), "zarc_gpu")
    out = subprocess.check_output([exe], timeout=600)
    assert all(b"select %s on 1 device(s) OK" % s in out for s in SELECTIONS) and b"select frames OK" in out
