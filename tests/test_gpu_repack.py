"""zarc_gpu_repack_batch* on the MI355X: the cases of test_repack.py on the product library at full size and over the full source x target
matrix, plus what only the GPU can show -- the real-data items and the diagnostic twin (libzarc_gpu_diag.so) in a child process, whose
fault injection makes the read-back check fail."""
import glob
import os
import subprocess

import pytest

import repack_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_gpu_repack_equals_pack_of_unpack_on_libzstd_frames(engine, oracle, corpus, libzstds, golden_frames):
    rc.check_golden(engine, oracle, corpus, libzstds, golden_frames)


@pytest.fixture(scope="module")
def want_cache():
    return {}   # pack of the same content at the same target, asked for by six sources


@pytest.mark.parametrize("source", rc.MODES, ids=rc.MODE_ID)
def test_gpu_repack_equals_pack_of_unpack_on_own_frames(engine, oracle, corpus, libzstds, source, want_cache):
    rc.check_own_frames(engine, oracle, corpus, libzstds, True, source, rc.MODES, want_cache)


def test_gpu_repack_equals_pack_of_unpack_on_real_data(engine, oracle, libzstds, real_items):
    rc.check_real_items(engine, oracle, libzstds, real_items)


def test_gpu_repack_the_error_list_among_good_frames(engine, oracle, corpus, libzstds, golden_frames):
    rc.check_errors(engine, oracle, corpus, libzstds, golden_frames)


def test_gpu_repack_copy_counters_and_device_form(engine, oracle, corpus):
    rc.check_device_form(engine, oracle, corpus)


def test_gpu_repack_in_bounded_scratch(engine, corpus):
    rc.check_bounded_scratch(engine, corpus, big=True)


def test_gpu_repack_large_frames_among_small(engine, oracle, corpus, libzstds, libzstd15):
    rc.check_large_among_small(engine, oracle, corpus, libzstds, libzstd15, big=True)


def test_gpu_repack_carries_the_checksum(engine, oracle, corpus, libzstds, libzstd15):
    rc.check_checksum_carried(engine, oracle, corpus, libzstds, libzstd15)


def test_gpu_repack_arguments(engine):
    rc.check_arguments(engine)


def test_gpu_repack_check_switch_changes_no_output(engine, corpus):
    rc.check_switch_changes_nothing(engine, corpus, big=True)


@pytest.fixture(scope="module")
def diag_lib_path():
    """the diagnostic twin of the product library (make DIAG=1): built when it is missing or older than a source"""
    csrc = os.path.join(ROOT, "zarc_amd", "csrc")
    path = os.path.join(ROOT, "zarc_amd", "libzarc_gpu_diag.so")
    srcs = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(ROOT, "include", "zarc_gpu.h"), os.path.join(csrc, "Makefile")]
    if not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["make", "-s", "-C", csrc, "DIAG=1", "-j16"])
    return path


def test_gpu_repack_the_check_fires(diag_lib_path):
    rc.check_the_check_fires(diag_lib_path)
