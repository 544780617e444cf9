"""zarc_gpu_verify_batch*, the copy counters and the read-back check of pack on the CPU build of the same kernel and engine sources (HIP
emulator; a diagnostic build, so the fault injection of the check is there).  test_gpu_verify.py runs the same cases on the MI355X."""
import pytest

import verify_cases as vc
from zarc_amd import Engine, _lib


def test_emu_verify_equals_unpack_on_libzstd_frames(emu_engine, oracle, corpus, golden_frames):
    vc.check_golden(emu_engine, oracle, corpus, golden_frames, limit=140000)


def test_emu_verify_equals_unpack_on_the_error_list(emu_engine, oracle, corpus, golden_frames):
    vc.check_errors(emu_engine, oracle, corpus, golden_frames)


@pytest.mark.parametrize("mode", vc.MODES, ids=lambda m: "level%d_split%d_%s" % (m[0], m[1], "zstd" if m[2] else "store"))
def test_emu_verify_equals_unpack_on_own_frames(emu_engine, oracle, corpus, mode):
    vc.check_own_frames(emu_engine, oracle, corpus, big=False, modes=(mode,))


def test_emu_verify_equals_unpack_on_the_mixed_batch(emu_engine, oracle, corpus):
    vc.check_mixed(emu_engine, oracle, corpus, 1500)


def test_emu_verify_equals_unpack_on_frames_in_pieces(emu_engine, oracle, corpus, libzstd15):
    vc.check_pieces(emu_engine, oracle, corpus, libzstd15)


def test_emu_verify_device_form(emu_engine, oracle, corpus, golden_frames):
    vc.check_device_form(emu_engine, oracle, corpus, golden_frames)


def test_emu_verify_arguments(emu_engine):
    vc.check_arguments(emu_engine)


def test_emu_copy_counters_of_pack(emu_engine, corpus):
    vc.check_pack_counters(emu_engine, corpus)


def test_emu_copy_counters_name_the_path(emu_lib_path, emu_engine, corpus, monkeypatch):
    ents = [corpus.entry(60 + i, 20000 + 3000 * i, -1) for i in range(6)]
    frames = [f for f, _ in emu_engine.pack(ents)]
    raw_lens = [len(e) for e in ents]
    vc.check_path_counters(emu_engine, frames, raw_lens, ents, direct_expected=False)            # pageable caller memory
    monkeypatch.setenv("HIPEMU_ALL_PINNED", "1")
    e = Engine(0, emu_lib_path)
    try:
        e.set_parameter(_lib.PX_ZERO_COPY, 1)
        vc.check_path_counters(e, frames, raw_lens, ents, direct_expected=True)
        e.set_parameter(_lib.PX_ZERO_COPY, 0)
        vc.check_path_counters(e, frames, raw_lens, ents, direct_expected=False)
    finally:
        e.close()


def test_emu_verify_in_bounded_scratch(emu_engine, oracle, corpus):
    vc.check_bounded_scratch(emu_engine, oracle, corpus)


def test_emu_check_switch_changes_no_output(emu_engine, emu_lib_path, corpus):
    fresh = Engine(0, emu_lib_path)
    fresh.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    try:
        vc.check_switch_changes_nothing(emu_engine, fresh, corpus, big=False)
    finally:
        fresh.close()


def test_emu_the_check_fires(emu_lib_path):
    vc.check_the_check_fires(emu_lib_path)
