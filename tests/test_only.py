"""zarc_gpu_search_matches_batch* (grep -o on the device) on the CPU build of the same kernel and engine sources (HIP emulator).
test_gpu_only.py runs the same cases on the MI355X.  The reference of every expected value is Python on the source bytes
(only_cases.ref_frame).  Where the encoder is not the subject the batches are packed in store mode here (search_cases.pack)."""
import only_cases as oc


def test_emu_only_leftmost_longest(emu_engine):
    oc.check_leftmost_longest(emu_engine, compress=False)


def test_emu_only_matches_at_a_slice_boundary(emu_engine):
    oc.check_boundaries(emu_engine, compress=False)


def test_emu_only_matches_at_the_frames_end(emu_engine):
    oc.check_frame_end(emu_engine, compress=False)


def test_emu_only_line_over_three_slices(emu_engine):
    oc.check_long_line(emu_engine, compress=False)


def test_emu_only_equivalences(emu_engine, corpus):
    oc.check_equivalences(emu_engine, corpus, compress=False)


def test_emu_only_caps_and_both_delivery_rules(emu_engine):
    oc.check_caps(emu_engine, compress=False)


def test_emu_only_cut_invariance(emu_engine, corpus):
    oc.check_cut_invariance(emu_engine, corpus, compress=False)


def test_emu_only_many_small_and_bad_frames(emu_engine, oracle, corpus, golden_frames):
    oc.check_many_small(emu_engine, oracle, corpus, golden_frames)


def test_emu_only_arguments(emu_engine):
    oc.check_arguments(emu_engine)
