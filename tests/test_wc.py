"""zarc_gpu_count_batch* on the CPU build of the same kernel and engine sources (HIP emulator).  test_gpu_wc.py runs the same cases on the
MI355X.  The reference of every expected value is Python on the source bytes (wc_cases.ref_wc).
Where the encoder is not the subject the batches are packed in store mode here (search_cases.pack)."""
import wc_cases as wc


def test_emu_wc_slice_step_and_wave_seams(emu_engine, corpus):
    wc.check_seams(emu_engine, corpus, compress=False)


def test_emu_wc_longest_line(emu_engine):
    wc.check_longest(emu_engine, compress=False)


def test_emu_wc_ends_of_content(emu_engine, corpus):
    wc.check_ends(emu_engine, corpus, compress=False)


def test_emu_wc_carry_paths(emu_engine, corpus):
    wc.check_carry(emu_engine, corpus, compress=False)


def test_emu_wc_lines_of_equal_lengths(emu_engine):
    wc.check_random(emu_engine, compress=False)


def test_emu_wc_many_small_and_bad_frames(emu_engine, oracle, corpus, golden_frames):
    wc.check_many_small(emu_engine, oracle, corpus, golden_frames, compress=False)


def test_emu_wc_cut_invariance_forms_and_counters(emu_engine, corpus):
    wc.check_cut_invariance(emu_engine, corpus, compress=False)


def test_emu_wc_arguments(emu_engine, corpus):
    wc.check_arguments(emu_engine, corpus)
