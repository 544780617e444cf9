"""Block splitting (ZARC_GPU_PX_BLOCK_SPLIT) on the MI355X: the checks of test_split.py on the product library, plus what only the GPU
can show -- its own decoder on its own uneven blocks in a large mixed batch, and the ratio table of the real-data items."""
import os

import pytest

import parity_cases as pc
import split_cases as sc
import splitmodel
from zarc_amd import Engine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    return splitmodel.SplitModel()


def test_gpu_parameter_is_known_and_checked(engine):
    lib, h = engine.lib, engine.h
    assert lib.zarc_gpu_set_parameter(h, 9007, 1) == _lib.OK
    assert lib.zarc_gpu_set_parameter(h, 9007, 2) == _lib.E_PARAM
    assert lib.zarc_gpu_set_parameter(h, 9007, -1) == _lib.E_PARAM
    assert lib.zarc_gpu_set_parameter(h, 9007, 0) == _lib.OK


def test_gpu_switch_off_changes_nothing(engine, oracle, corpus):
    fresh = Engine(0)
    fresh.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    try:
        sc.check_switch_off_unchanged(engine, fresh, oracle, corpus, big=True)
    finally:
        fresh.close()


@pytest.mark.parametrize("level", [1, 3, 9, 15])
def test_gpu_split_frames_equal_the_model_and_decode_everywhere(engine, oracle, corpus, libzstds, model, level):
    cases = sc.split_inputs(corpus, big=True)
    blocks = sc.check_frames(engine, oracle, model, libzstds, cases, level=level)
    assert len(cases["sharp_halves"]) <= 65536 and blocks["sharp_halves"] > 1
    assert blocks["many_pieces"] > (len(cases["many_pieces"]) + 65535) // 65536
    if level == 3:
        keep = ["sharp_halves", "many_pieces", "size_0", "size_65537", "one_byte", "five_mib"]
        sc.check_frames(engine, oracle, model, libzstds, {k: cases[k] for k in keep}, level=3, checksum=0)


def test_gpu_store_mode_ignores_the_switch(engine, corpus):
    ents = [corpus.entry(320, 200000, 0), sc.sharp_halves(corpus), b""]
    engine.enable_compression(False)
    try:
        off = engine.pack(ents)
        with sc.split_on(engine):
            on = engine.pack(ents)
    finally:
        engine.enable_compression(True)
    assert on == off


def test_gpu_many_small_frames_split(engine, oracle, corpus):
    """The 70 000-frame mixed batch of parity_cases with the switch on: the decoder's 64-slot trips over its own encoder's frames."""
    with sc.split_on(engine):
        pc.check_many_frames_with_turned_down_ones(engine, oracle, corpus, 70000)


def test_gpu_split_ratio_on_real_data(engine, libzstd15, real_items, tmp_path):
    """No item larger with the switch on, every item inside the existing bounds, the ELF / machine-code / JSON items strictly smaller in
    sum.  The per-item table is printed, and written as realdata_split.json into the directory ZARC_TEST_OUT names (the run that
    made profiles/r05_realdata_split.json), else into pytest's temporary directory."""
    out_dir = os.environ.get("ZARC_TEST_OUT") or str(tmp_path)
    sc.check_ratio(engine, libzstd15, real_items, "MI355X", os.path.join(out_dir, "realdata_split.json"))
