"""The tile loop's removed barriers on the emulator build (finder_barrier_cases.py).  The emulator runs threads as fibres up to the next
barrier or wave collective, so a wave that no barrier holds back runs ahead of its neighbours: a value taken from another wave before
it is final, or overwritten while another wave still needs it, gives a frame that differs from the model's.
test_gpu_finder_barriers.py runs the same cases on the device."""
import pytest

import finder_barrier_cases as fb


@pytest.fixture(scope="module")
def made(corpus):
    return {g: make(corpus) for g, make in fb.GROUPS.items()}


def test_finder_barrier_cases_bite(oracle, made):
    fb.check_cases_bite(oracle, made)


@pytest.mark.parametrize("group,level", fb.plan())
def test_emu_finder_barriers(emu_engine, oracle, made, group, level):
    fb.check_frames(emu_engine, oracle, made[group], level)
