"""zarc_gpu_search_batch* on the MI355X: the cases of test_search.py on the product library, plus the real-data items and the check that
the product library reads no environment variable."""
import pytest

import search_cases as sc
import verify_cases as vc

pytestmark = pytest.mark.gpu


def test_gpu_search_boundaries(engine, corpus):
    sc.check_boundaries(engine, corpus)


def test_gpu_search_needle_lengths(engine, corpus):
    sc.check_needle_lengths(engine, corpus)


def test_gpu_search_neighbours_never_complete_a_match(engine, corpus):
    sc.check_neighbours(engine, corpus)


def test_gpu_search_overlap_and_worst_case(engine):
    sc.check_overlap(engine)


def test_gpu_search_case_folding(engine, corpus):
    sc.check_case_folding(engine, corpus)


def test_gpu_search_many_small_frames(engine, corpus):
    sc.check_many_small(engine, corpus)


def test_gpu_search_frames_in_pieces(engine, oracle, corpus, golden_frames):
    sc.check_pieces(engine, oracle, corpus, golden_frames)


def test_gpu_search_verdicts_equal_verify(engine, oracle, corpus, golden_frames):
    sc.check_verdicts(engine, oracle, corpus, golden_frames)


def test_gpu_search_in_bounded_scratch(engine, corpus):
    sc.check_bounded_scratch(engine, corpus)


def test_gpu_search_device_form_and_counters(engine, corpus):
    sc.check_device_form(engine, corpus)


def test_gpu_search_arguments(engine, corpus):
    sc.check_arguments(engine, corpus)


def test_gpu_search_real_data(engine, real_items):
    sc.check_real_items(engine, real_items)


def test_gpu_search_product_library_reads_no_variable(engine):
    assert hasattr(engine.lib, "zarc_gpu_search_batch")
    vc.check_product_reads_no_variable(engine.lib_path)
