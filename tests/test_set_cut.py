"""A zarc_gpu_search_set_lines_* call cut by the scratch budget and the staging chunk, on the CPU build of the same kernel and engine
sources (HIP emulator).  test_gpu_set_cut.py runs the same case on the MI355X."""
import set_cut_cases as zc


def test_emu_set_lines_cut_invariance(emu_engine, corpus):
    zc.check_lines_cut_invariance(emu_engine, corpus, compress=False)
