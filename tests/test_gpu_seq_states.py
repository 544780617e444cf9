"""zarc_zge_seq_states on the MI355X: the cases of seq_states_cases.py on the product library.  Runs below, at and above the
minimum, rounds that end on and next to a multiple of 64 sequences, blocks of very different sequence counts in one run, runs that
restart behind a raw, an RLE, an empty and an unproven block, a type in RLE mode, blocks above the capacity, and all of it in one
batch must give the frames the model gives, whatever ZARC_GPU_PX_SEQ_STATES says."""
import pytest

import seq_states_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group,level,px", sc.plan())
def test_gpu_seq_states(engine, oracle, corpus, group, level, px):
    sc.check_frames(engine, oracle, corpus, group, level, px)
