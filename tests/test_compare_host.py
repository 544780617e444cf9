"""FrameReader::compare_content_frames of the C++ host mirror (zarc_amd/host/zarc_host.hpp) on 1, 2 and 4 handles: identical results, the
verdict of check_content_frames, the results of a plain host walk of both sides (tests/host/compare_frames_test.cpp, built here with g++)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "compare_frames_test.cpp")


def build(out_dir, lib_dir, lib_name):
    exe = os.path.join(str(out_dir), "compare_frames_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, SRC, "-L" + lib_dir, "-l" + lib_name,
                           "-Wl,-rpath," + lib_dir, "-pthread"])
    return exe


def test_compare_content_frames_emulated(emu_lib_path, tmp_path):
    exe = build(tmp_path, os.path.dirname(emu_lib_path), "zarc_gpu_emu")
    out = subprocess.check_output([exe], timeout=900, env=dict(os.environ, HIPEMU_DEVICES="4"))
    for g in (1, 2, 4):
        assert b"compare_content_frames on %d device(s) OK" % g in out
    assert b"compare frames OK" in out


@pytest.mark.gpu
def test_compare_content_frames_gpu(tmp_path):
    exe = build(tmp_path, os.path.join(ROOT, "zarc_amd"), "zarc_gpu")
    out = subprocess.check_output([exe], timeout=600)
    assert b"compare_content_frames on 1 device(s) OK" in out and b"compare frames OK" in out
