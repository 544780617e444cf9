"""zarc_gpu_search_regex_* on the MI355X: the cases of test_regex.py on the product library, plus the real-data items and the check that the
product library reads no environment variable."""
import pytest

import regex_cases as zr
import verify_cases as vc

pytestmark = pytest.mark.gpu


def test_gpu_regex_literal_is_search(engine, corpus):
    zr.check_literal(engine, corpus)


def test_gpu_regex_state_across_chunks_and_slices(engine):
    zr.check_boundaries(engine)


def test_gpu_regex_anchors(engine):
    zr.check_anchors(engine)


def test_gpu_regex_classes(engine):
    zr.check_classes(engine)


def test_gpu_regex_quantifiers(engine):
    zr.check_quantifiers(engine)


def test_gpu_regex_refusals(engine, corpus):
    zr.check_refusals(engine, corpus)


def test_gpu_regex_random_differential(engine):
    zr.check_random(engine)


def test_gpu_regex_verdicts_equal_verify(engine, oracle, corpus, golden_frames):
    zr.check_verdicts(engine, oracle, corpus, golden_frames)


def test_gpu_regex_in_bounded_scratch(engine, corpus):
    zr.check_bounded_scratch(engine, corpus)


def test_gpu_regex_device_form_and_counters(engine, corpus):
    zr.check_device_form(engine, corpus)


def test_gpu_regex_many_small_frames(engine, corpus):
    zr.check_many_small(engine, corpus)


def test_gpu_regex_lines_caps(engine, corpus):
    zr.check_lines_caps(engine, corpus)


def test_gpu_regex_real_data(engine, real_items):
    zr.check_real_items(engine, real_items)


def test_gpu_regex_product_library_reads_no_variable(engine):
    assert hasattr(engine.lib, "zarc_gpu_search_regex_batch")
    vc.check_product_reads_no_variable(engine.lib_path)
