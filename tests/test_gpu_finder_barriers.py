"""The tile loop's removed barriers on the MI355X: the cases of finder_barrier_cases.py on the product library.  A wave that runs
ahead of where a barrier used to hold it must find every value it takes from another wave final, and must overwrite nothing a slower
wave still reads: otherwise a frame differs from the model's."""
import pytest

import finder_barrier_cases as fb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def made(corpus):
    return {g: make(corpus) for g, make in fb.GROUPS.items()}


@pytest.mark.parametrize("group,level", fb.plan())
def test_gpu_finder_barriers(engine, oracle, made, group, level):
    fb.check_frames(engine, oracle, made[group], level)
