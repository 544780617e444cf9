"""zarc_gpu_read_ranges_batch* on the MI355X: the cases of test_range.py on the product library, through the encoder's compressed frames."""
import pytest

import range_cases as rc

pytestmark = pytest.mark.gpu


def test_gpu_range_slice_and_chunk_boundaries(engine, corpus):
    rc.check_boundaries(engine, corpus)


def test_gpu_range_frames_of_many_slices(engine, corpus):
    rc.check_large(engine, corpus)


def test_gpu_range_ends_of_content(engine):
    rc.check_ends(engine)


def test_gpu_range_arithmetic_saturates(engine, corpus):
    rc.check_arithmetic(engine, corpus)


def test_gpu_range_gather_alignment_and_canaries(engine, corpus):
    rc.check_alignment(engine, corpus)


def test_gpu_range_caps_and_continuation(engine, corpus):
    rc.check_caps(engine, corpus)


def test_gpu_range_cut_invariance_forms_and_counters(engine, corpus):
    rc.check_cut_invariance(engine, corpus)


def test_gpu_range_many_small_and_bad_frames(engine, oracle, corpus, golden_frames):
    rc.check_many_small(engine, oracle, corpus, golden_frames)


def test_gpu_range_arguments(engine, corpus):
    rc.check_arguments(engine, corpus)
