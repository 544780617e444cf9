"""zarc_gpu_read_ranges_batch* on the CPU build of the same kernel and engine sources (HIP emulator).  test_gpu_range.py runs the same cases
on the MI355X.  The reference of every expected value is Python on the source bytes (range_cases.ref_range).
Where the encoder is not the subject the batches are packed in store mode here (search_cases.pack)."""
import range_cases as rc


def test_emu_range_slice_and_chunk_boundaries(emu_engine, corpus):
    rc.check_boundaries(emu_engine, corpus, compress=False)


def test_emu_range_frames_of_many_slices(emu_engine, corpus):
    rc.check_large(emu_engine, corpus, compress=False)


def test_emu_range_ends_of_content(emu_engine):
    rc.check_ends(emu_engine, compress=False)


def test_emu_range_arithmetic_saturates(emu_engine, corpus):
    rc.check_arithmetic(emu_engine, corpus, compress=False)


def test_emu_range_gather_alignment_and_canaries(emu_engine, corpus):
    rc.check_alignment(emu_engine, corpus, compress=False)


def test_emu_range_caps_and_continuation(emu_engine, corpus):
    rc.check_caps(emu_engine, corpus, compress=False)


def test_emu_range_cut_invariance_forms_and_counters(emu_engine, corpus):
    rc.check_cut_invariance(emu_engine, corpus, compress=False)


def test_emu_range_many_small_and_bad_frames(emu_engine, oracle, corpus, golden_frames):
    rc.check_many_small(emu_engine, oracle, corpus, golden_frames, compress=False)


def test_emu_range_arguments(emu_engine, corpus):
    rc.check_arguments(emu_engine, corpus)
