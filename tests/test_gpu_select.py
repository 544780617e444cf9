"""zarc_gpu_select_lines_batch* on the MI355X: the cases of test_select.py on the product library."""
import pytest

import select_cases as zc

pytestmark = pytest.mark.gpu


def test_gpu_select_context_across_a_slice_boundary(engine):
    zc.check_boundaries(engine)


def test_gpu_select_context_across_whole_slices(engine):
    zc.check_whole_slices(engine)


def test_gpu_select_line_over_three_slices(engine):
    zc.check_long_line(engine)


def test_gpu_select_merging_edges_and_invert(engine):
    zc.check_small(engine)


def test_gpu_select_a_slice_of_newlines(engine):
    zc.check_newlines_only(engine)


def test_gpu_select_equivalence(engine, corpus):
    zc.check_equivalence(engine, corpus)


def test_gpu_select_66_slices(engine):
    zc.check_66_slices(engine)


def test_gpu_select_many_small_frames(engine, oracle, corpus, golden_frames):
    zc.check_many_small(engine, oracle, corpus, golden_frames)


def test_gpu_select_caps_and_delivery_rule(engine):
    zc.check_caps(engine)


def test_gpu_select_in_bounded_scratch_and_chunks(engine, corpus):
    zc.check_bounded_scratch(engine, corpus)


def test_gpu_select_frames_in_pieces(engine, oracle, corpus, golden_frames):
    zc.check_pieces(engine, oracle, corpus, golden_frames)


def test_gpu_select_device_form_and_counters(engine):
    zc.check_device_form(engine)


def test_gpu_select_arguments(engine):
    zc.check_arguments(engine)
