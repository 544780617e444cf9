"""ctypes binding of tests/support/split_model.c: the CPU statement of the encoder with block splitting on (test infrastructure only)."""
import ctypes
import os
import subprocess

import harness

ROOT = harness.ROOT


def _build():
    d = os.path.join(ROOT, "tests", "support", "_build")
    os.makedirs(d, exist_ok=True)
    so = os.path.join(d, "libsplitmodel.so")
    srcs = [os.path.join(ROOT, "tests", "support", "split_model.c"), os.path.join(ROOT, "oracle", "zstd_enc_model.c"),
            os.path.join(ROOT, "oracle", "zge_model.h"), os.path.join(ROOT, "oracle", "oracle.h"), os.path.join(ROOT, "oracle", "xxh64_ref.c")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c99", "-I", os.path.join(ROOT, "oracle"), "-o", so, srcs[0], srcs[4]])
    return so


class SplitModel:
    def __init__(self):
        self.lib = m = ctypes.CDLL(_build())
        m.zge_bound.restype = ctypes.c_size_t
        m.zge_bound.argtypes = [ctypes.c_size_t]
        m.zge_default_params.argtypes = [ctypes.POINTER(harness.ZgeParams), ctypes.c_int]
        m.zge_split_encode_frame.argtypes = [ctypes.POINTER(harness.ZgeParams), ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint32)]
        m.split_model_tune.argtypes = [ctypes.c_int, ctypes.c_int]

    def tune(self, chunks, piece_cost):
        self.lib.split_model_tune(chunks, piece_cost)

    def encode(self, data, level=3, checksum=1, blocks=False):
        p = harness.ZgeParams()
        self.lib.zge_default_params(ctypes.byref(p), level)
        p.checksum = checksum
        cap = self.lib.zge_bound(len(data))
        dst = ctypes.create_string_buffer(cap)
        ol, nb = ctypes.c_size_t(), ctypes.c_uint32()
        rc = self.lib.zge_split_encode_frame(ctypes.byref(p), bytes(data), len(data), dst, cap, ctypes.byref(ol), ctypes.byref(nb))
        assert rc == 0, rc
        return (dst.raw[:ol.value], nb.value) if blocks else dst.raw[:ol.value]


def count_blocks(frame):
    """Number of Zstandard blocks of one frame (walks the block headers)."""
    d = frame[4]
    fcs_flag, single, dict_flag = d >> 6, (d >> 5) & 1, d & 3
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[dict_flag] + ((1 if single else 0) if fcs_flag == 0 else (1 << fcs_flag))
    n = 0
    while True:
        h = frame[pos] | (frame[pos + 1] << 8) | (frame[pos + 2] << 16)
        last, typ, size = h & 1, (h >> 1) & 3, h >> 3
        pos += 3 + (1 if typ == 1 else size)
        n += 1
        if last:
            return n
