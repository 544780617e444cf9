"""zarc_gpu_repack_batch* on the CPU build of the same kernel and engine sources (HIP emulator; a diagnostic build, so the fault injection of
the read-back check is there).  test_gpu_repack.py runs the same cases on the MI355X at full size.  The emulator's encoder is slow, so
the source x target matrix is thinned here: every mode is a source once and a target at least twice."""
import pytest

import repack_cases as rc
from zarc_amd import _lib


def test_emu_repack_equals_pack_of_unpack_on_libzstd_frames(emu_engine, oracle, corpus, libzstds, golden_frames):
    rc.check_golden(emu_engine, oracle, corpus, libzstds, golden_frames, limit=140000, every_target=False)


@pytest.mark.parametrize("source", rc.MODES, ids=rc.MODE_ID)
def test_emu_repack_equals_pack_of_unpack_on_own_frames(emu_engine, oracle, corpus, libzstds, source):
    rc.check_own_frames(emu_engine, oracle, corpus, libzstds, False, source, rc.thinned_targets(source))


def test_emu_repack_the_error_list_among_good_frames(emu_engine, oracle, corpus, libzstds, golden_frames):
    rc.check_errors(emu_engine, oracle, corpus, libzstds, golden_frames)


def test_emu_repack_copy_counters_and_device_form(emu_engine, oracle, corpus):
    rc.check_device_form(emu_engine, oracle, corpus)


def test_emu_repack_in_bounded_scratch(emu_engine, corpus):
    rc.check_bounded_scratch(emu_engine, corpus, big=False)


def test_emu_repack_large_frames_among_small(emu_engine, oracle, corpus, libzstds, libzstd15):
    rc.check_large_among_small(emu_engine, oracle, corpus, libzstds, libzstd15, big=False)


def test_emu_repack_carries_the_checksum(emu_engine, oracle, corpus, libzstds, libzstd15):
    rc.check_checksum_carried(emu_engine, oracle, corpus, libzstds, libzstd15)


def test_emu_repack_arguments(emu_engine):
    rc.check_arguments(emu_engine)


def test_emu_repack_check_switch_changes_no_output(emu_engine, corpus):
    rc.check_switch_changes_nothing(emu_engine, corpus, big=False)


def test_emu_repack_the_check_fires(emu_lib_path):
    rc.check_the_check_fires(emu_lib_path)


def test_repack_is_exported():
    assert "zarc_gpu_repack_batch" in _lib.EXPORTS and "zarc_gpu_repack_batch_device" in _lib.EXPORTS
