"""zarc_gpu_verify_batch*, the copy counters and the read-back check of pack on the MI355X: the cases of test_verify.py on the product
library at full size, plus what only the GPU can show -- the real-data items, page-locked caller memory, and the diagnostic twin
(libzarc_gpu_diag.so) whose fault injection makes the check fail."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

import verify_cases as vc
from zarc_amd import Engine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_gpu_verify_equals_unpack_on_libzstd_frames(engine, oracle, corpus, golden_frames):
    vc.check_golden(engine, oracle, corpus, golden_frames)


def test_gpu_verify_equals_unpack_on_the_error_list(engine, oracle, corpus, golden_frames):
    vc.check_errors(engine, oracle, corpus, golden_frames)


@pytest.mark.parametrize("mode", vc.MODES, ids=lambda m: "level%d_split%d_%s" % (m[0], m[1], "zstd" if m[2] else "store"))
def test_gpu_verify_equals_unpack_on_own_frames(engine, oracle, corpus, mode):
    vc.check_own_frames(engine, oracle, corpus, big=True, modes=(mode,))


def test_gpu_verify_equals_unpack_on_the_mixed_batch(engine, oracle, corpus):
    vc.check_mixed(engine, oracle, corpus, 70000)


def test_gpu_verify_equals_unpack_on_frames_in_pieces(engine, oracle, corpus, libzstd15):
    vc.check_pieces(engine, oracle, corpus, libzstd15)


def test_gpu_verify_equals_unpack_on_real_data(engine, oracle, real_items):
    vc.check_real_items(engine, oracle, real_items)


def test_gpu_verify_device_form(engine, oracle, corpus, golden_frames):
    vc.check_device_form(engine, oracle, corpus, golden_frames)


def test_gpu_verify_arguments(engine):
    vc.check_arguments(engine)


def test_gpu_copy_counters_of_pack(engine, corpus):
    vc.check_pack_counters(engine, corpus)


def test_gpu_copy_counters_name_the_path(engine, corpus):
    """Pageable caller memory goes through the ring.  One hipHostMalloc'd block that holds entries, frame slots, frames and outputs in
    runs of 6 MiB (above the default threshold of ZARC_GPU_PX_ZERO_COPY) goes directly, every byte; with the switch at 0 none does."""
    n, size = 6, 6 << 20
    ents = [corpus.entry(9100 + i, size, 3) for i in range(n)]           # incompressible: the frames are runs of 6 MiB as well
    frames = [f for f, _ in engine.pack(ents)]
    vc.check_path_counters(engine, frames, [size] * n, ents, direct_expected=False)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipHostMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    hip.hipHostFree.argtypes = [ctypes.c_void_p]
    cap = sum(engine.bound(size) for _ in range(n))
    flen = [len(f) for f in frames]
    total = n * size + cap + sum((l + 15) // 16 * 16 for l in flen) + n * size + 4096
    base = ctypes.c_void_p()
    assert hip.hipHostMalloc(ctypes.byref(base), total, 0) == 0
    try:
        at = base.value
        src = [at + i * size for i in range(n)]; at += n * size
        dst = at; at += cap
        fr = []
        for l in flen:
            fr.append(at); at += (l + 15) // 16 * 16
        out = [at + i * size for i in range(n)]
        for p, e in zip(src, ents): ctypes.memmove(p, e, size)
        for p, f in zip(fr, frames): ctypes.memmove(p, f, len(f))
        lib, h = engine.lib, engine.h
        szs = lambda v: (ctypes.c_size_t * n)(*v)
        vps = lambda v: (ctypes.c_void_p * n)(*v)
        dig = np.zeros((n, 32), dtype=np.uint8); pdig = dig.ctypes.data_as(ctypes.c_void_p)
        st = (ctypes.c_int * n)()
        for zero_copy, direct in ((None, True), (0, False)):
            if zero_copy is not None: engine.set_parameter(_lib.PX_ZERO_COPY, zero_copy)
            try:
                dst_off, dst_len = szs([0] * n), szs([0] * n)
                assert lib.zarc_gpu_pack_batch(h, n, vps(src), szs([size] * n), ctypes.c_void_p(dst), cap, dst_off, dst_len, pdig, st) == 0
                h2d, d2h, ring, dr = vc.copy_counters(engine)
                assert h2d == n * size and d2h == sum(dst_len) == sum(flen) and ring + dr == h2d + d2h and dr == (h2d + d2h if direct else 0)
                assert [ctypes.string_at(dst + dst_off[i], dst_len[i]) for i in range(n)] == frames
                assert lib.zarc_gpu_verify_batch(h, n, vps(fr), szs(flen), szs([size] * n), None, pdig, st) == 0 and list(st) == [0] * n
                h2d, d2h, ring, dr = vc.copy_counters(engine)
                assert h2d == sum(flen) and d2h == 0 and ring + dr == h2d and dr == (h2d if direct else 0)
                assert lib.zarc_gpu_unpack_batch(h, n, vps(fr), szs(flen), szs([size] * n), vps(out), None, pdig, st) == 0 and list(st) == [0] * n
                h2d, d2h, ring, dr = vc.copy_counters(engine)
                assert h2d == sum(flen) and d2h == n * size and ring + dr == h2d + d2h and dr == (h2d + d2h if direct else 0)
                assert [ctypes.string_at(out[i], size) for i in range(n)] == ents
            finally:
                engine.set_parameter(_lib.PX_ZERO_COPY, 4096)
    finally:
        hip.hipHostFree(base)


def test_gpu_verify_in_bounded_scratch(engine, oracle, corpus):
    vc.check_bounded_scratch(engine, oracle, corpus)


def test_gpu_check_switch_changes_no_output(engine, corpus):
    fresh = Engine(0)
    fresh.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    try:
        vc.check_switch_changes_nothing(engine, fresh, corpus, big=True)
    finally:
        fresh.close()


def test_gpu_check_passes_a_large_mixed_batch(engine, corpus):
    """the check over many small entries and a few large ones (slices of one workgroup each, parts under a scratch budget): no false alarm"""
    ents = [corpus.entry(9300 + i, (5 << 20) + 17 * i, i % 4) for i in range(3)] + [corpus.entry(9400 + i, 1 + (i * 7919) % 9000, i % 4) for i in range(30000)] + [b""]
    plain = engine.pack(ents)
    for budget in (0, 64):
        engine.set_parameter(_lib.PX_SCRATCH_MB, budget)
        try:
            with vc.settings(engine, check=1):
                assert engine.pack(ents) == plain
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)


@pytest.fixture(scope="module")
def diag_lib_path():
    """the diagnostic twin of the product library (make DIAG=1): built when it is missing or older than a source"""
    csrc = os.path.join(ROOT, "zarc_amd", "csrc")
    path = os.path.join(ROOT, "zarc_amd", "libzarc_gpu_diag.so")
    srcs = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(ROOT, "include", "zarc_gpu.h"), os.path.join(csrc, "Makefile")]
    if not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["make", "-s", "-C", csrc, "DIAG=1", "-j16"])
    return path


def test_gpu_the_check_fires(diag_lib_path):
    vc.check_the_check_fires(diag_lib_path)


def test_gpu_product_library_reads_no_variable(engine):
    vc.check_product_reads_no_variable(engine.lib_path)
