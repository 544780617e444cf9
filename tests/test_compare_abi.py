"""The ABI of the compare call: its symbols in the product library, the layout of zarc_gpu_cmp, its constants, and the timer enum that
did not grow.  Needs no device."""
import ctypes
import os
import re

from zarc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compare_symbols_are_exported():
    lib = ctypes.CDLL(os.path.join(ROOT, "zarc_amd", "libzarc_gpu.so"))
    for name in ("zarc_gpu_compare_batch", "zarc_gpu_compare_batch_device", "zarc_gpu_last_compare_ms"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def test_compare_record_is_64_bytes():
    assert ctypes.sizeof(_lib.Cmp) == 64
    assert [f[0] for f in _lib.Cmp._fields_] == ["relation", "byte_a", "byte_b", "reserved0", "prefix", "line", "differing", "suffix", "reserved"]
    assert (_lib.Cmp.byte_b.offset, _lib.Cmp.prefix.offset, _lib.Cmp.suffix.offset, _lib.Cmp.reserved.offset) == (8, 16, 40, 48)


def test_compare_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "zarc_gpu.h")).read()
    for name in ("NONE", "EQUAL", "DIFFER", "FRAME_IS_PREFIX", "OTHER_IS_PREFIX"):
        m = re.search(r"ZARC_GPU_CMP_%s = (\d+)\b" % name, header)
        assert m and int(m.group(1)) == getattr(_lib, "CMP_" + name), name
    assert (_lib.CMP_NONE, _lib.CMP_EQUAL, _lib.CMP_DIFFER, _lib.CMP_FRAME_IS_PREFIX, _lib.CMP_OTHER_IS_PREFIX) == (0, 1, 2, 3, 4)
    assert re.search(r"#define ZARC_GPU_CMP_EOF 256u", header) and _lib.CMP_EOF == 256
    assert re.search(r"\} zarc_gpu_cmp;\s*/\* 64 bytes \*/", header)


def test_compare_leaves_the_timer_enum_and_the_abi_version():
    header = open(os.path.join(ROOT, "include", "zarc_gpu.h")).read()
    assert _lib.T_COUNT == 14 and re.search(r"ZARC_GPU_T_COUNT = 14\b", header)
    assert _lib.ABI_VERSION == 2 and re.search(r"#define ZARC_GPU_ABI_VERSION 2\b", header)
