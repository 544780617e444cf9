"""zarc_gpu_search_lines_batch* on the CPU build of the same kernel and engine sources (HIP emulator).  test_gpu_lines.py runs the same
cases on the MI355X.  The reference of every expected value is Python on the source bytes (lines_cases.ref_lines).
Where the encoder is not the subject the batches are packed in store mode here (search_cases.pack)."""
import lines_cases as lc


def test_emu_lines_slice_boundaries(emu_engine, corpus):
    lc.check_boundaries(emu_engine, corpus, compress=False)


def test_emu_lines_degenerate_frames(emu_engine, corpus):
    lc.check_degenerate(emu_engine, corpus, compress=False)


def test_emu_lines_neighbours_share_no_line(emu_engine, corpus):
    lc.check_neighbours(emu_engine, corpus, compress=False)


def test_emu_lines_many_small_frames(emu_engine, corpus):
    lc.check_many_small(emu_engine, corpus)


def test_emu_lines_overlap_is_one_line(emu_engine):
    lc.check_overlap(emu_engine, compress=False)


def test_emu_lines_case_folding(emu_engine, corpus):
    lc.check_case_folding(emu_engine, corpus, compress=False)


def test_emu_lines_needle_lengths(emu_engine, corpus):
    lc.check_needle_lengths(emu_engine, corpus, compress=False)


def test_emu_lines_caps_and_delivery_rule(emu_engine, corpus):
    lc.check_caps(emu_engine, corpus, compress=False)


def test_emu_lines_in_bounded_scratch(emu_engine, corpus):
    lc.check_bounded_scratch(emu_engine, corpus, compress=False)


def test_emu_lines_device_form_and_counters(emu_engine, corpus):
    lc.check_device_form(emu_engine, corpus, compress=False)


def test_emu_lines_verdicts_equal_verify_and_search(emu_engine, oracle, corpus, golden_frames):
    lc.check_verdicts(emu_engine, oracle, corpus, golden_frames)


def test_emu_lines_frames_in_pieces(emu_engine, oracle, corpus, golden_frames):
    lc.check_pieces(emu_engine, oracle, corpus, golden_frames)


def test_emu_lines_arguments(emu_engine, corpus):
    lc.check_arguments(emu_engine, corpus)
