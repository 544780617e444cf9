"""zarc_gpu_compare_batch* on the CPU build of the same kernel and engine sources (HIP emulator).  test_gpu_compare.py runs the same cases
on the MI355X.  The reference of every expected value is Python on the source bytes (compare_cases.ref_cmp).
Where the encoder is not the subject the batches are packed in store mode here (search_cases.pack)."""
import compare_cases as cc


def test_emu_compare_slice_step_and_wave_seams(emu_engine, corpus):
    cc.check_seams(emu_engine, corpus, compress=False)


def test_emu_compare_lengths(emu_engine, corpus):
    cc.check_lengths(emu_engine, corpus, compress=False)


def test_emu_compare_shifted_tail(emu_engine, corpus):
    cc.check_shifted(emu_engine, corpus, compress=False)


def test_emu_compare_carry_paths(emu_engine, corpus):
    cc.check_carry(emu_engine, corpus, compress=False)


def test_emu_compare_random_edits(emu_engine):
    cc.check_random(emu_engine, compress=False)


def test_emu_compare_bad_frames(emu_engine, oracle, corpus, golden_frames):
    cc.check_bad_frames(emu_engine, oracle, corpus, golden_frames, compress=False)


def test_emu_compare_cut_invariance_forms_handles_and_counters(emu_engine, corpus):
    cc.check_cut_invariance(emu_engine, corpus, compress=False)


def test_emu_compare_arguments(emu_engine, corpus):
    cc.check_arguments(emu_engine, corpus)
