"""zarc_gpu_count_batch* on the MI355X: the cases of test_wc.py on the product library, through the encoder's compressed frames."""
import pytest

import wc_cases as wc

pytestmark = pytest.mark.gpu


def test_gpu_wc_slice_step_and_wave_seams(engine, corpus):
    wc.check_seams(engine, corpus)


def test_gpu_wc_longest_line(engine):
    wc.check_longest(engine)


def test_gpu_wc_ends_of_content(engine, corpus):
    wc.check_ends(engine, corpus)


def test_gpu_wc_carry_paths(engine, corpus):
    wc.check_carry(engine, corpus)


def test_gpu_wc_lines_of_equal_lengths(engine):
    wc.check_random(engine)


def test_gpu_wc_many_small_and_bad_frames(engine, oracle, corpus, golden_frames):
    wc.check_many_small(engine, oracle, corpus, golden_frames)


def test_gpu_wc_cut_invariance_forms_and_counters(engine, corpus):
    wc.check_cut_invariance(engine, corpus)


def test_gpu_wc_arguments(engine, corpus):
    wc.check_arguments(engine, corpus)
