"""The backward offers of the match finder on the MI355X: the cases of finder_offer_cases.py on the product library.  Two offers that
meet at one target, offers cut at the start of a tile, a block or a wave, the far candidates' long reach over a wave edge and a wave
in which every position offers must give the frames the model gives."""
import pytest

import finder_offer_cases as fo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def made(corpus):
    return {g: make(corpus) for g, make in fo.GROUPS.items()}


@pytest.mark.parametrize("group,level", fo.plan())
def test_gpu_finder_offers(engine, oracle, made, group, level):
    fo.check_frames(engine, oracle, made[group], level)
