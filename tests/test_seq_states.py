"""zarc_zge_seq_states on the emulator build (seq_states_cases.py): every frame bit-identical to the model with
ZARC_GPU_PX_SEQ_STATES at 0, at 1 and at the capacities, and the cases checked against the model alone.  test_gpu_seq_states.py runs
the same cases on the device, and alone the text frames of 16 blocks and more and the mixed batch (seq_states_cases.plan).  The emulator
build is a diagnostic build: it counts the blocks whose states the state kernel computes, which test_emu_states_taken holds against
the model's frames -- the byte checks alone cannot tell a state path that ran from one that did not.

Mutants tried once on the emulator build, none committed; each failed cases of this file:
  chains run first to last (sequence index done + e instead of nseq - 1 - done - e in the state kernel)
  the first symbol's init state left out (the chain starts from state 0)
  the final states of OF and ML swapped in pass 2's flush of given states
  the run rule ignoring one type's mode (ML)."""
import re

import pytest

import seq_states_cases as sc
from zarc_amd import _lib


def test_seq_states_cases_bite(oracle, corpus):
    sc.check_cases_bite(oracle, corpus)


@pytest.mark.parametrize("group,level,px", sc.plan(emu=True))
def test_emu_seq_states(emu_engine, oracle, corpus, group, level, px):
    sc.check_frames(emu_engine, oracle, corpus, group, level, px)


@pytest.mark.parametrize("group,k,px", sc.TAKEN_CASES)
def test_emu_states_taken(emu_engine, oracle, corpus, capfd, monkeypatch, group, k, px):
    """The state path is taken where the plan says so, not only harmless: the diagnostic build (the emulator build is one) counts the
    blocks whose states zarc_zge_seq_states computes and prints the count with the stage clocks; it must equal what runs_of() reads
    off the model's frame -- none below the minimum run, none above the capacity, none with the switch off."""
    raw = sc.made(corpus, group)[k]
    monkeypatch.setenv("ZARC_GPU_DBG", "1024")
    counts = {}
    for value in ((px, 0) if group == "uneven_run" else (px,)):   # (the switch at 0 once: it launches no state kernel at all)
        emu_engine.set_parameter(_lib.PX_SEQ_STATES, value)
        capfd.readouterr()
        try:
            frame = emu_engine.pack([raw])[0][0]
        finally:
            emu_engine.set_parameter(_lib.PX_SEQ_STATES, 1)
        counts[value] = sum(int(n) for n in re.findall(r"seq-states blocks (\d+)", capfd.readouterr().err))
        assert frame == sc.model(oracle, corpus, group, 3)[k], (group, k, value)
    assert counts[px] == sc.taken_expected(oracle, corpus, group, k, px), (group, k, px, counts)
    assert counts.get(0, 0) == 0, (group, k, counts)
