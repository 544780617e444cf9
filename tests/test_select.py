"""zarc_gpu_select_lines_batch* (grep -v, -A / -B / -C on the device) on the CPU build of the same kernel and engine sources (HIP emulator).
test_gpu_select.py runs the same cases on the MI355X.  The reference of every expected value is Python on the source bytes
(select_cases.ref_select).  Where the encoder is not the subject the batches are packed in store mode here (search_cases.pack)."""
import select_cases as zc


def test_emu_select_context_across_a_slice_boundary(emu_engine):
    zc.check_boundaries(emu_engine, compress=False)


def test_emu_select_context_across_whole_slices(emu_engine):
    zc.check_whole_slices(emu_engine, compress=False)


def test_emu_select_line_over_three_slices(emu_engine):
    zc.check_long_line(emu_engine, compress=False)


def test_emu_select_merging_edges_and_invert(emu_engine):
    zc.check_small(emu_engine, compress=False)


def test_emu_select_a_slice_of_newlines(emu_engine):
    zc.check_newlines_only(emu_engine, compress=False)


def test_emu_select_equivalence(emu_engine, corpus):
    zc.check_equivalence(emu_engine, corpus, compress=False)


def test_emu_select_66_slices(emu_engine):
    zc.check_66_slices(emu_engine, compress=False)


def test_emu_select_many_small_frames(emu_engine, oracle, corpus, golden_frames):
    zc.check_many_small(emu_engine, oracle, corpus, golden_frames)


def test_emu_select_caps_and_delivery_rule(emu_engine):
    zc.check_caps(emu_engine, compress=False)


def test_emu_select_in_bounded_scratch_and_chunks(emu_engine, corpus):
    zc.check_bounded_scratch(emu_engine, corpus, compress=False)


def test_emu_select_frames_in_pieces(emu_engine, oracle, corpus, golden_frames):
    zc.check_pieces(emu_engine, oracle, corpus, golden_frames)


def test_emu_select_device_form_and_counters(emu_engine):
    zc.check_device_form(emu_engine, compress=False)


def test_emu_select_arguments(emu_engine):
    zc.check_arguments(emu_engine)
