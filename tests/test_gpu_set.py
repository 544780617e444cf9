"""zarc_gpu_search_set_* on the MI355X: the cases of test_set.py on the product library, plus the real-data items and the check that the
product library reads no environment variable."""
import pytest

import set_cases as zs
import verify_cases as vc

pytestmark = pytest.mark.gpu


def test_gpu_set_of_one_pattern_is_search(engine, corpus):
    zs.check_one_pattern(engine, corpus)


def test_gpu_set_mixed_classes(engine, corpus):
    zs.check_mixed_classes(engine, corpus)


def test_gpu_set_frame_end_is_per_pattern(engine, corpus):
    zs.check_frame_end(engine, corpus)


def test_gpu_set_shared_keys(engine, corpus):
    zs.check_shared_keys(engine, corpus)


def test_gpu_set_full_set(engine, corpus):
    zs.check_full_set(engine, corpus)


def test_gpu_set_overlap_and_worst_case(engine):
    zs.check_overlap(engine)


def test_gpu_set_case_folding(engine, corpus):
    zs.check_case_folding(engine, corpus)


def test_gpu_set_many_small_frames(engine, corpus):
    zs.check_many_small(engine, corpus)


def test_gpu_set_verdicts_equal_verify(engine, oracle, corpus, golden_frames):
    zs.check_verdicts(engine, oracle, corpus, golden_frames)


def test_gpu_set_in_bounded_scratch(engine, corpus):
    zs.check_bounded_scratch(engine, corpus)


def test_gpu_set_device_form_and_counters(engine, corpus):
    zs.check_device_form(engine, corpus)


def test_gpu_set_arguments(engine, corpus):
    zs.check_arguments(engine, corpus)


def test_gpu_set_frames_in_pieces(engine, oracle, corpus, golden_frames):
    zs.check_pieces(engine, oracle, corpus, golden_frames)


def test_gpu_set_lines(engine, corpus):
    zs.check_lines(engine, corpus)


def test_gpu_set_lines_caps(engine, corpus):
    zs.check_lines_caps(engine, corpus)


def test_gpu_set_real_data(engine, real_items):
    zs.check_real_items(engine, real_items)


def test_gpu_set_product_library_reads_no_variable(engine):
    assert hasattr(engine.lib, "zarc_gpu_search_set_batch")
    vc.check_product_reads_no_variable(engine.lib_path)
