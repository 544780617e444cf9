"""The backward offers of the match finder on the emulator build (finder_offer_cases.py): every frame bit-identical to the model at
levels 1, 3, 9 and 15, and the cases checked against the model alone.  test_gpu_finder_offers.py runs the same cases on the device.

dense_offers was built for a finder that packs a wave's offering positions into one pass and goes round again for more than 64 of
them; the finder here makes one pass per chunk and has no such loop, so there is no second round to witness.  What the case shows
is checked from the model's side: check_cases_bite counts the adopted matches in the copy (at least 40 of 48: five positions in six
of a span of 128 take the match the position behind them offered).  Counted once with a temporary ballot in front of the offers in
the emulator build (not committed): over the six entries nine (wave, tile) pairs hold 117 to 123 offering positions of 128, so both
positions of nearly every lane offer."""
import pytest

import finder_offer_cases as fo


@pytest.fixture(scope="module")
def made(corpus):
    return {g: make(corpus) for g, make in fo.GROUPS.items()}


def test_finder_offer_cases_bite(oracle, made):
    fo.check_cases_bite(oracle, made)


@pytest.mark.parametrize("group,level", fo.plan())
def test_emu_finder_offers(emu_engine, oracle, made, group, level):
    fo.check_frames(emu_engine, oracle, made[group], level)
