"""zarc_gpu_search_lines_batch* on the MI355X: the cases of test_lines.py on the product library, plus the real-data items."""
import pytest

import lines_cases as lc

pytestmark = pytest.mark.gpu


def test_gpu_lines_slice_boundaries(engine, corpus):
    lc.check_boundaries(engine, corpus)


def test_gpu_lines_degenerate_frames(engine, corpus):
    lc.check_degenerate(engine, corpus)


def test_gpu_lines_neighbours_share_no_line(engine, corpus):
    lc.check_neighbours(engine, corpus)


def test_gpu_lines_many_small_frames(engine, corpus):
    lc.check_many_small(engine, corpus)


def test_gpu_lines_overlap_is_one_line(engine):
    lc.check_overlap(engine)


def test_gpu_lines_case_folding(engine, corpus):
    lc.check_case_folding(engine, corpus)


def test_gpu_lines_needle_lengths(engine, corpus):
    lc.check_needle_lengths(engine, corpus)


def test_gpu_lines_caps_and_delivery_rule(engine, corpus):
    lc.check_caps(engine, corpus)


def test_gpu_lines_in_bounded_scratch(engine, corpus):
    lc.check_bounded_scratch(engine, corpus)


def test_gpu_lines_device_form_and_counters(engine, corpus):
    lc.check_device_form(engine, corpus)


def test_gpu_lines_verdicts_equal_verify_and_search(engine, oracle, corpus, golden_frames):
    lc.check_verdicts(engine, oracle, corpus, golden_frames)


def test_gpu_lines_frames_in_pieces(engine, oracle, corpus, golden_frames):
    lc.check_pieces(engine, oracle, corpus, golden_frames)


def test_gpu_lines_arguments(engine, corpus):
    lc.check_arguments(engine, corpus)


def test_gpu_lines_real_data(engine, real_items):
    lc.check_real_items(engine, real_items)
