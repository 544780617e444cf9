"""zarc_gpu_compare_batch* on the MI355X: the cases of test_compare.py on the product library, through the encoder's compressed frames and
through store-mode frames."""
import pytest

import compare_cases as cc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("compress", (True, False), ids=("compressed", "stored"))
def test_gpu_compare_slice_step_and_wave_seams(engine, corpus, compress):
    cc.check_seams(engine, corpus, compress)


@pytest.mark.parametrize("compress", (True, False), ids=("compressed", "stored"))
def test_gpu_compare_lengths(engine, corpus, compress):
    cc.check_lengths(engine, corpus, compress)


@pytest.mark.parametrize("compress", (True, False), ids=("compressed", "stored"))
def test_gpu_compare_shifted_tail(engine, corpus, compress):
    cc.check_shifted(engine, corpus, compress)


def test_gpu_compare_carry_paths(engine, corpus):
    cc.check_carry(engine, corpus)


@pytest.mark.parametrize("compress", (True, False), ids=("compressed", "stored"))
def test_gpu_compare_random_edits(engine, compress):
    cc.check_random(engine, compress)


def test_gpu_compare_bad_frames(engine, oracle, corpus, golden_frames):
    cc.check_bad_frames(engine, oracle, corpus, golden_frames)


def test_gpu_compare_cut_invariance_forms_handles_and_counters(engine, corpus):
    cc.check_cut_invariance(engine, corpus)


def test_gpu_compare_arguments(engine, corpus):
    cc.check_arguments(engine, corpus)
