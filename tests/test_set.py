"""zarc_gpu_search_set_* on the CPU build of the same kernel and engine sources (HIP emulator).  test_gpu_set.py runs the same cases on
the MI355X.  The reference of every expected value is Python's `re` (set_cases.ref).
Where the encoder is not the subject the batches are packed in store mode here (search_cases.pack); the small-frame, pieces and verdict cases
search compressed frames, the engine's own and libzstd's."""
import set_cases as zs


def test_emu_set_of_one_pattern_is_search(emu_engine, corpus):
    zs.check_one_pattern(emu_engine, corpus, compress=False)


def test_emu_set_mixed_classes(emu_engine, corpus):
    zs.check_mixed_classes(emu_engine, corpus, compress=False)


def test_emu_set_frame_end_is_per_pattern(emu_engine, corpus):
    zs.check_frame_end(emu_engine, corpus, compress=False)


def test_emu_set_shared_keys(emu_engine, corpus):
    zs.check_shared_keys(emu_engine, corpus, compress=False)


def test_emu_set_full_set(emu_engine, corpus):
    zs.check_full_set(emu_engine, corpus, compress=False)


def test_emu_set_overlap_and_worst_case(emu_engine):
    zs.check_overlap(emu_engine, compress=False)


def test_emu_set_case_folding(emu_engine, corpus):
    zs.check_case_folding(emu_engine, corpus, compress=False)


def test_emu_set_many_small_frames(emu_engine, corpus):
    zs.check_many_small(emu_engine, corpus)


def test_emu_set_verdicts_equal_verify(emu_engine, oracle, corpus, golden_frames):
    zs.check_verdicts(emu_engine, oracle, corpus, golden_frames)


def test_emu_set_in_bounded_scratch(emu_engine, corpus):
    zs.check_bounded_scratch(emu_engine, corpus, compress=False)


def test_emu_set_device_form_and_counters(emu_engine, corpus):
    zs.check_device_form(emu_engine, corpus, compress=False)


def test_emu_set_arguments(emu_engine, corpus):
    zs.check_arguments(emu_engine, corpus)


def test_emu_set_frames_in_pieces(emu_engine, oracle, corpus, golden_frames):
    zs.check_pieces(emu_engine, oracle, corpus, golden_frames)


def test_emu_set_lines(emu_engine, corpus):
    zs.check_lines(emu_engine, corpus, compress=False)


def test_emu_set_lines_caps(emu_engine, corpus):
    zs.check_lines_caps(emu_engine, corpus, compress=False)
