"""A zarc_gpu_search_set_lines_* call cut by the scratch budget and the staging chunk, on the MI355X: the case of test_set_cut.py on the
product library."""
import pytest

import set_cut_cases as zc

pytestmark = pytest.mark.gpu


def test_gpu_set_lines_cut_invariance(engine, corpus):
    zc.check_lines_cut_invariance(engine, corpus)
