"""zarc_gpu_search_regex_* on the CPU build of the same kernel and engine sources (HIP emulator).  test_gpu_regex.py runs the same cases on
the MI355X.  The reference of every expected value is Python's `re`, line by line (regex_cases.positions).
Where the encoder is not the subject the batches are packed in store mode here (search_cases.pack); the small-frame and verdict cases search
compressed frames, the engine's own and libzstd's."""
import regex_cases as zr


def test_emu_regex_literal_is_search(emu_engine, corpus):
    zr.check_literal(emu_engine, corpus, compress=False)


def test_emu_regex_state_across_chunks_and_slices(emu_engine):
    zr.check_boundaries(emu_engine, compress=False)


def test_emu_regex_anchors(emu_engine):
    zr.check_anchors(emu_engine, compress=False)


def test_emu_regex_classes(emu_engine):
    zr.check_classes(emu_engine, compress=False)


def test_emu_regex_quantifiers(emu_engine):
    zr.check_quantifiers(emu_engine, compress=False)


def test_emu_regex_refusals(emu_engine, corpus):
    zr.check_refusals(emu_engine, corpus)


def test_emu_regex_random_differential(emu_engine):
    zr.check_random(emu_engine, compress=False)


def test_emu_regex_verdicts_equal_verify(emu_engine, oracle, corpus, golden_frames):
    zr.check_verdicts(emu_engine, oracle, corpus, golden_frames)


def test_emu_regex_in_bounded_scratch(emu_engine, corpus):
    zr.check_bounded_scratch(emu_engine, corpus, compress=False)


def test_emu_regex_device_form_and_counters(emu_engine, corpus):
    zr.check_device_form(emu_engine, corpus, compress=False)


def test_emu_regex_many_small_frames(emu_engine, corpus):
    zr.check_many_small(emu_engine, corpus)


def test_emu_regex_lines_caps(emu_engine, corpus):
    zr.check_lines_caps(emu_engine, corpus, compress=False)
