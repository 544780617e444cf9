"""FrameReader::matches_content_frames of the C++ host mirror (zarc_amd/host/zarc_host.hpp) on 1, 2 and 4 handles: identical lines, matches
and match records under every pair of caps and for all three matchers, the verdict, counts and lines of lines_content_frames, the matches of
a plain host scan (tests/host/only_frames_test.cpp, built here with g++)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "only_frames_test.cpp")
CAPS = 9


def build(out_dir, lib_dir, lib_name):
    exe = os.path.join(str(out_dir), "only_frames_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, SRC, "-L" + lib_dir, "-l" + lib_name,
                           "-Wl,-rpath," + lib_dir, "-pthread"])
    return exe


def test_only_content_frames_emulated(emu_lib_path, tmp_path):
    exe = build(tmp_path, os.path.dirname(emu_lib_path), "zarc_gpu_emu")
    out = subprocess.check_output([exe], timeout=900, env=dict(os.environ, HIPEMU_DEVICES="4"))
    for g in (1, 2, 4):
        for k in range(CAPS):
            assert b"only caps %d on %d device(s) OK" % (k, g) in out
    assert b"only frames OK" in out


@pytest.mark.gpu
def test_only_content_frames_gpu(tmp_path):
    exe = build(tmp_path, os.path.join(ROOT, "zarc_amd"), "zarc_gpu")
    out = subprocess.check_output([exe], timeout=600)
    assert all(b"only caps %d on 1 device(s) OK" % k in out for k in range(CAPS)) and b"only frames OK" in out
