"""zarc_gpu_search_batch* on the CPU build of the same kernel and engine sources (HIP emulator).  test_gpu_search.py runs the same cases
on the MI355X.  The reference of every expected value is Python's `re` (search_cases.ref).
Where the encoder is not the subject the batches are packed in store mode here (search_cases.pack); the small-frame, pieces and verdict cases
search compressed frames, the engine's own and libzstd's."""
import search_cases as sc


def test_emu_search_boundaries(emu_engine, corpus):
    sc.check_boundaries(emu_engine, corpus, compress=False)


def test_emu_search_needle_lengths(emu_engine, corpus):
    sc.check_needle_lengths(emu_engine, corpus, compress=False)


def test_emu_search_neighbours_never_complete_a_match(emu_engine, corpus):
    sc.check_neighbours(emu_engine, corpus, compress=False)


def test_emu_search_overlap_and_worst_case(emu_engine):
    sc.check_overlap(emu_engine, compress=False)


def test_emu_search_case_folding(emu_engine, corpus):
    sc.check_case_folding(emu_engine, corpus, compress=False)


def test_emu_search_many_small_frames(emu_engine, corpus):
    sc.check_many_small(emu_engine, corpus)


def test_emu_search_frames_in_pieces(emu_engine, oracle, corpus, golden_frames):
    sc.check_pieces(emu_engine, oracle, corpus, golden_frames)


def test_emu_search_verdicts_equal_verify(emu_engine, oracle, corpus, golden_frames):
    sc.check_verdicts(emu_engine, oracle, corpus, golden_frames)


def test_emu_search_in_bounded_scratch(emu_engine, corpus):
    sc.check_bounded_scratch(emu_engine, corpus, compress=False)


def test_emu_search_device_form_and_counters(emu_engine, corpus):
    sc.check_device_form(emu_engine, corpus, compress=False)


def test_emu_search_arguments(emu_engine, corpus):
    sc.check_arguments(emu_engine, corpus)
