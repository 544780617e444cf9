"""The ABI of the count call: both symbols in the product library, the size of zarc_gpu_wc, the timer numbers.  Needs no device."""
import ctypes
import os
import re

from zarc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wc_symbols_are_exported():
    lib = ctypes.CDLL(os.path.join(ROOT, "zarc_amd", "libzarc_gpu.so"))
    for name in ("zarc_gpu_count_batch", "zarc_gpu_count_batch_device"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def test_wc_record_is_64_bytes():
    assert ctypes.sizeof(_lib.Wc) == 64
    assert [f[0] for f in _lib.Wc._fields_] == ["lines", "words", "chars", "max_line", "max_line_start", "max_line_no", "reserved"]
    assert _lib.Wc.max_line_no.offset == 40 and _lib.Wc.reserved.offset == 48


def test_wc_timer_numbers_match_the_header():
    assert (_lib.T_WC, _lib.T_COUNT) == (13, 14)
    header = open(os.path.join(ROOT, "include", "zarc_gpu.h")).read()
    assert re.search(r"ZARC_GPU_T_WC = 13,", header) and re.search(r"ZARC_GPU_T_COUNT = 14\b", header)
    assert re.search(r"\} zarc_gpu_wc;\s*/\* 64 bytes \*/", header)
