"""zarc_gpu_search_matches_batch* on the MI355X: the cases of test_only.py on the product library."""
import pytest

import only_cases as oc

pytestmark = pytest.mark.gpu


def test_gpu_only_leftmost_longest(engine):
    oc.check_leftmost_longest(engine)


def test_gpu_only_matches_at_a_slice_boundary(engine):
    oc.check_boundaries(engine)


def test_gpu_only_matches_at_the_frames_end(engine):
    oc.check_frame_end(engine)


def test_gpu_only_line_over_three_slices(engine):
    oc.check_long_line(engine)


def test_gpu_only_equivalences(engine, corpus):
    oc.check_equivalences(engine, corpus)


def test_gpu_only_caps_and_both_delivery_rules(engine):
    oc.check_caps(engine)


def test_gpu_only_cut_invariance(engine, corpus):
    oc.check_cut_invariance(engine, corpus)


def test_gpu_only_many_small_and_bad_frames(engine, oracle, corpus, golden_frames):
    oc.check_many_small(engine, oracle, corpus, golden_frames)


def test_gpu_only_arguments(engine):
    oc.check_arguments(engine)
