"""The match finder's memory requests on the MI355X: the cases of finder_wait_cases.py on the product library.  A request that is
consumed before it has arrived, or a parked word that is taken for another tile's, gives a frame that differs from the model's.
The first three tests together are finder_wait_cases.check(engine, ..., many=1500), one test per pair of its plan()."""
import pytest

import finder_wait_cases as fw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def made(corpus):
    return {g: make(corpus) for g, make in fw.GROUPS.items()}


@pytest.mark.parametrize("group", [g for g, level in fw.plan() if level == 3])
def test_gpu_finder_waits_level3(engine, oracle, libzstds, made, group):
    fw.check_frames(engine, oracle, libzstds, made[group], level=3)


@pytest.mark.parametrize("group,level", [(g, level) for g, level in fw.plan() if level != 3])
def test_gpu_finder_waits_fast_and_deep(engine, oracle, libzstds, made, group, level):
    fw.check_frames(engine, oracle, libzstds, made[group], level=level)


def test_gpu_finder_waits_many_frames_both_orders(engine, oracle, corpus, libzstds):
    fw.check_many(engine, oracle, libzstds, corpus, 1500)


def test_gpu_finder_waits_positions_past_2g(engine):
    fw.check_positions_past_2g(engine)
