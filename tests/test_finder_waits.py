"""The match finder's request bookkeeping on the emulator build: which tile a parked window word or far entries asked for ahead belong
to, on every path that leaves a tile, a block, a segment or a frame early (finder_wait_cases.py).  The emulator runs the lanes one after
another, so it cannot see a request that is consumed too early: test_gpu_finder_waits.py runs the same cases on the device.
The three tests together are finder_wait_cases.check(emu_engine, ..., many=42), one test per pair of its plan()."""
import pytest

import finder_wait_cases as fw


@pytest.fixture(scope="module")
def made(corpus):
    return {g: make(corpus) for g, make in fw.GROUPS.items()}


@pytest.mark.parametrize("group", [g for g, level in fw.plan() if level == 3])
def test_emu_finder_waits_level3(emu_engine, oracle, libzstds, made, group):
    fw.check_frames(emu_engine, oracle, libzstds, made[group], level=3)


@pytest.mark.parametrize("group,level", [(g, level) for g, level in fw.plan() if level != 3])
def test_emu_finder_waits_fast_and_deep(emu_engine, oracle, libzstds, made, group, level):
    fw.check_frames(emu_engine, oracle, libzstds, made[group], level=level)


def test_emu_finder_waits_many_frames_both_orders(emu_engine, oracle, corpus, libzstds):
    fw.check_many(emu_engine, oracle, libzstds, corpus, 42)
