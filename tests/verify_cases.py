"""Checks of zarc_gpu_verify_batch*, zarc_gpu_last_copy_bytes and the read-back check of pack (ZARC_GPU_PX_CHECK_FRAMES), shared by
the emulator tests (test_verify.py) and the GPU tests (test_gpu_verify.py).  Every comparison is equality: verify must judge a frame
exactly as unpack does, and the check must change nothing but the time.

Run as a script (`python verify_cases.py LIB MODE`) this file is the child process of check_the_check_fires: the fault injection of the
diagnostic build is steered by environment variables, which the library reads when the call runs."""
import ctypes
import json
import os
import random
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    for p in (ROOT, os.path.join(HERE, "support"), os.path.join(HERE, "golden")):
        sys.path.insert(0, p)

import make_golden  # noqa: E402
import parity_cases as pc  # noqa: E402
from zarc_amd import _lib  # noqa: E402

DECODED = (_lib.FRAME_OK, _lib.FRAME_DIGEST, _lib.FRAME_CHECKSUM)  # unpack delivers the bytes of these (engine.hip: copy_out)


# ---- raw calls: return codes and every output array, where Engine's wrappers raise or drop them -----------------------------------
def _ptrs(bufs):
    n = len(bufs)
    return (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs]), (ctypes.c_size_t * n)(*[len(b) for b in bufs])


def raw_pack(engine, entries, seen=None):
    """-> (rc, frames, digests, statuses, dst_lens); frames[i] is None where dst_len[i] == 0 and the entry is not empty input"""
    n = len(entries)
    bufs = [bytes(e) for e in entries]
    ptrs, lens = _ptrs(bufs)
    cap = sum(engine.bound(len(b)) for b in bufs)
    dst = np.zeros(max(cap, 1), dtype=np.uint8)
    dst_off, dst_len = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    dig = np.zeros((n, 32), dtype=np.uint8)
    status = (ctypes.c_int * n)()
    if seen is None:
        rc = engine.lib.zarc_gpu_pack_batch(engine.h, n, ptrs, lens, dst.ctypes.data_as(ctypes.c_void_p), cap, dst_off, dst_len,
                                            dig.ctypes.data_as(ctypes.c_void_p), status)
    else:
        def known(_ctx, d, i):
            key = bytes(d[:32])
            if key in seen:
                return 1
            seen.add(key)
            return 0
        cb = _lib.KNOWN_FN(known)
        rc = engine.lib.zarc_gpu_pack_batch_dedup(engine.h, n, ptrs, lens, dst.ctypes.data_as(ctypes.c_void_p), cap, dst_off, dst_len,
                                                  dig.ctypes.data_as(ctypes.c_void_p), status, cb, None)
    frames = [bytes(dst[dst_off[i]:dst_off[i] + dst_len[i]]) if dst_len[i] else None for i in range(n)]
    return rc, frames, [bytes(d) for d in dig], [int(s) for s in status], [int(x) for x in dst_len]


def copy_counters(engine):
    return tuple(engine.copy_bytes(w) for w in (_lib.C_H2D, _lib.C_D2H, _lib.C_RING, _lib.C_DIRECT))


# ---- 1 + 2. verify equals unpack, and nothing comes out ------------------------------------------------------------------------------
def check_verify_equals_unpack(engine, oracle, frames, raw_lens, expect, raws=None, tag=""):
    """statuses equal element for element, digests equal, decodable frames carry the BLAKE3 of their content; and the copy counters of
    both calls: verify moves the frames in and nothing out, unpack moves the decoded bytes out as well"""
    want = engine.unpack(frames, raw_lens, expect)
    h2d_u, d2h_u, ring_u, direct_u = copy_counters(engine)
    got = engine.verify(frames, raw_lens, expect)
    h2d_v, d2h_v, ring_v, direct_v = copy_counters(engine)
    assert [g[1] for g in got] == [w[2] for w in want], tag
    assert [g[0] for g in got] == [w[1] for w in want], tag
    if raws is not None:
        for i, (dig, st) in enumerate(got):
            if st in DECODED and raws[i] is not None and raw_lens[i] == len(raws[i]):
                assert dig == oracle.blake3(raws[i]), (tag, i)
    total_in = sum(len(f) for f in frames)
    assert d2h_v == 0 and h2d_v == total_in, (tag, h2d_v, d2h_v)
    assert h2d_u == total_in and d2h_u == sum(int(r) for r, w in zip(raw_lens, want) if w[2] in DECODED), (tag, h2d_u, d2h_u)
    assert ring_v + direct_v == h2d_v + d2h_v and ring_u + direct_u == h2d_u + d2h_u, tag
    return got


def golden_set(corpus, oracle, golden_frames, limit=None):
    d, m = golden_frames
    sel = m["frames"] if limit is None else [f for f in m["frames"] if f["raw_len"] <= limit]
    cache, frames, raws = {}, [], []
    for fr in sel:
        name = fr["recipe"]
        if name not in cache:
            cache[name] = make_golden.recipe_bytes(m["recipes"][name], corpus)
        frames.append(open(os.path.join(d, fr["file"]), "rb").read())
        raws.append(cache[name])
    return frames, [len(r) for r in raws], [oracle.blake3(r) for r in raws], raws


def check_golden(engine, oracle, corpus, golden_frames, limit=None):
    frames, raw_lens, expect, raws = golden_set(corpus, oracle, golden_frames, limit)
    assert len(frames) > 20
    got = check_verify_equals_unpack(engine, oracle, frames, raw_lens, expect, raws, "golden")
    assert all(st == _lib.FRAME_OK for _, st in got)
    # expect = None works: the digest is still delivered, nothing is compared
    got = check_verify_equals_unpack(engine, oracle, frames[:9], raw_lens[:9], None, raws[:9], "golden, no expect")
    assert all(st == _lib.FRAME_OK for _, st in got)


def error_list(oracle, corpus, golden_frames):
    """the seven frames of parity_cases.check_unpack_errors"""
    d, m = golden_frames
    fr = next(f for f in m["frames"] if f["recipe"] == "text300" and f["level"] == 3 and f["checksum"] == 1 and f["libzstd"].startswith("1.5"))
    good = open(os.path.join(d, fr["file"]), "rb").read()
    raw = make_golden.recipe_bytes(m["recipes"]["text300"], corpus)
    bad_ck = bytearray(good); bad_ck[-1] ^= 0x40
    bad_magic = bytearray(good); bad_magic[0] ^= 1
    corrupt = bytearray(good); corrupt[12] ^= 0xFF; corrupt[13] ^= 0xFF
    frames = [good, bytes(bad_ck), bytes(bad_magic), good[:-7], bytes(corrupt), good, good]
    expect = [oracle.blake3(raw)] * 5 + [bytes(32), oracle.blake3(raw)]
    return frames, [len(raw)] * 6 + [len(raw) + 1], expect, [raw] * 7


def check_errors(engine, oracle, corpus, golden_frames):
    frames, raw_lens, expect, raws = error_list(oracle, corpus, golden_frames)
    got = check_verify_equals_unpack(engine, oracle, frames, raw_lens, expect, raws, "errors")
    st = [s for _, s in got]
    assert st[0] == _lib.FRAME_OK and st[1] == _lib.FRAME_CHECKSUM and st[2] == _lib.FRAME_BAD_MAGIC
    assert st[3] != _lib.FRAME_OK and st[4] != _lib.FRAME_OK
    assert st[5] == _lib.FRAME_DIGEST and got[5][0] == oracle.blake3(raws[5])   # reported; the digest is that of what was decoded
    assert st[6] == _lib.FRAME_SRCSIZE


class settings:
    """with settings(engine, level=.., split=.., compress=.., ...): parameters set, and everything back afterwards"""

    def __init__(self, engine, level=3, split=0, compress=True, check=0, chunk=0, groups=0):
        self.e, self.v = engine, (level, split, compress, check, chunk, groups)

    def _set(self, level, split, compress, check, chunk, groups):
        self.e.set_parameter(_lib.P_COMPRESSION_LEVEL, level)
        self.e.set_parameter(_lib.PX_BLOCK_SPLIT, split)
        self.e.enable_compression(compress)
        self.e.set_parameter(_lib.PX_CHECK_FRAMES, check)
        self.e.set_parameter(_lib.PX_STAGE_CHUNK, chunk)
        self.e.set_parameter(_lib.PX_DEC_GROUPS, groups)

    def __enter__(self):
        self._set(*self.v)
        return self.e

    def __exit__(self, *a):
        self._set(3, 0, True, 0, 0, 0)


# (level, block splitting, compression): levels 1, 3, 9, 15, with 9007 on, store mode
MODES = ((1, 0, True), (3, 0, True), (9, 0, True), (15, 0, True), (3, 1, True), (3, 0, False))


def check_own_frames(engine, oracle, corpus, big, modes=MODES):
    cases = pc.encode_cases(corpus, big)
    names = list(cases)
    raws = [cases[k] for k in names]
    for level, split, compress in modes:
        with settings(engine, level=level, split=split, compress=compress):
            packed = engine.pack(raws)
        got = check_verify_equals_unpack(engine, oracle, [f for f, _ in packed], [len(r) for r in raws], [d for _, d in packed], raws,
                                         "own frames %r" % ((level, split, compress),))
        assert all(st == _lib.FRAME_OK for _, st in got), (level, split, compress)


def mixed_batch(engine, corpus, n):
    """the inputs of parity_cases.check_many_frames_with_turned_down_ones"""
    rnd = random.Random(11)
    ents = [corpus.entry(5000 + i, rnd.choice((0, 1, 9, 40, 130, 700, 2500)), i % 4) for i in range(n)]
    packed = engine.pack(ents)
    frames, digests, raw_lens = [f for f, _ in packed], [d for _, d in packed], [len(e) for e in ents]
    bad = {}
    for i in range(3, n, 37):
        kind = (i // 37) % 4
        f = bytearray(frames[i])
        if kind == 0: f[0] ^= 1; bad[i] = "magic"
        elif kind == 1 and len(f) > 9: f = f[:-3]; bad[i] = "trunc"
        elif kind == 2: raw_lens[i] += 1; bad[i] = "size"
        elif kind == 3: digests[i] = bytes(32); bad[i] = "digest"
        frames[i] = bytes(f)
    return frames, raw_lens, digests, ents, bad


def check_mixed(engine, oracle, corpus, n):
    frames, raw_lens, digests, ents, bad = mixed_batch(engine, corpus, n)
    got = check_verify_equals_unpack(engine, oracle, frames, raw_lens, digests, ents, "mixed")
    for i, (dig, st) in enumerate(got):
        why = bad.get(i)
        if why is None: assert st == _lib.FRAME_OK, i
        elif why == "magic": assert st == _lib.FRAME_BAD_MAGIC, i
        elif why == "trunc": assert st != _lib.FRAME_OK, i
        elif why == "size": assert st == _lib.FRAME_SRCSIZE, i


def check_pieces(engine, oracle, corpus, libzstd15):
    """the inputs of test_emu_frame_pass_in_pieces: frames above 4 MiB, alone and among small ones, one and two size groups"""
    text = corpus.entry(5151, (4 << 20) + 700000, 0)
    rnd = corpus.entry(5152, (4 << 20) + 300001, 3)
    small = corpus.entry(5153, 90000, 1)
    own = engine.pack([text])[0][0]
    frames = [libzstd15.compress(text, 3, 1), libzstd15.compress(rnd, 3, 1), own, libzstd15.compress(small, 3, 1)]
    raws = [text, rnd, text, small]
    bad = bytearray(frames[0]); bad[len(bad) // 2] ^= 0x55
    tiny = [corpus.entry(5200 + i, 40 + 37 * i, i % 4) for i in range(70)]
    tframes = [f for f, _ in engine.pack(tiny)]
    mixed_f = tframes[:30] + [own] + tframes[30:] + [frames[1]]
    mixed_r = tiny[:30] + [text] + tiny[30:] + [rnd]
    for g in (0, 2):
        with settings(engine, groups=g):
            got = check_verify_equals_unpack(engine, oracle, frames, [len(r) for r in raws], [oracle.blake3(r) for r in raws], raws, "pieces %d" % g)
            assert all(st == _lib.FRAME_OK for _, st in got)
            got = check_verify_equals_unpack(engine, oracle, [bytes(bad), frames[1]], [len(text), len(rnd)], [oracle.blake3(text), oracle.blake3(rnd)], None,
                                             "pieces, corrupt %d" % g)
            assert got[0][1] != _lib.FRAME_OK and got[1][1] == _lib.FRAME_OK
            got = check_verify_equals_unpack(engine, oracle, mixed_f, [len(r) for r in mixed_r], [oracle.blake3(r) for r in mixed_r], mixed_r, "pieces, mixed %d" % g)
            assert all(st == _lib.FRAME_OK for _, st in got)


def check_real_items(engine, oracle, real_items):
    raws = [v for v in real_items.values()]
    for level in (3, 9):
        with settings(engine, level=level):
            packed = engine.pack(raws)
        got = check_verify_equals_unpack(engine, oracle, [f for f, _ in packed], [len(r) for r in raws], [d for _, d in packed], raws, "real items")
        assert all(st == _lib.FRAME_OK for _, st in got)


def _arena(engine, blobs):
    off, pos = [], 0
    for b in blobs:
        off.append(pos)
        pos += (len(b) + 15) // 16 * 16
    d = engine.malloc(pos + _lib.PAD + 256)
    for b, o in zip(blobs, off):
        if b:
            engine.h2d(d + o, b)
    return d, off, pos


def check_device_form(engine, oracle, corpus, golden_frames):
    """verify_device against unpack_device on the error list and a few of the engine's own frames; device forms count no copies"""
    frames, raw_lens, expect, raws = error_list(oracle, corpus, golden_frames)
    own = [corpus.entry(300 + i, n, i % 4) for i, n in enumerate((0, 1, 70000, 200000, 5))]
    packed = engine.pack(own)
    frames += [f for f, _ in packed]; raw_lens += [len(r) for r in own]; expect += [d for _, d in packed]
    d_frames, foff, _ = _arena(engine, frames)
    doff, pos = [], 0
    for r in raw_lens:
        doff.append(pos)
        pos += (r + 15) // 16 * 16
    d_dst = engine.malloc(pos + _lib.PAD + 256)
    try:
        exp = np.frombuffer(b"".join(expect), dtype=np.uint8)
        flen = [len(f) for f in frames]
        dig_u, st_u = engine.unpack_device(d_frames, foff, flen, d_dst, doff, raw_lens, exp)
        assert copy_counters(engine) == (0, 0, 0, 0)
        dig_v, st_v = engine.verify_device(d_frames, foff, flen, raw_lens, exp)
        assert copy_counters(engine) == (0, 0, 0, 0)
        assert list(st_v) == list(st_u) and bytes(dig_v) == bytes(dig_u)
        assert list(st_v[:3]) == [_lib.FRAME_OK, _lib.FRAME_CHECKSUM, _lib.FRAME_BAD_MAGIC] and st_v[5] == _lib.FRAME_DIGEST and st_v[6] == _lib.FRAME_SRCSIZE
        assert all(s == _lib.FRAME_OK for s in st_v[7:])
        dig_n, st_n = engine.verify_device(d_frames, foff, flen, raw_lens, None)
        assert [s for s in st_n] == [s if s != _lib.FRAME_DIGEST else _lib.FRAME_OK for s in st_u]
        assert engine.kernel_ms(_lib.T_DECODE) >= 0 and engine.kernel_ms(_lib.T_DEC_FRAMES) >= 0   # the decoder's entries, as for unpack
    finally:
        engine.free(d_frames)
        engine.free(d_dst)


def check_arguments(engine):
    """n = 0 is OK; NULL arguments and frames of 4 GiB and more are refused as unpack refuses them"""
    lib, h = engine.lib, engine.h
    c = ctypes
    frame = b"\x28\xb5\x2f\xfd\x20\x00\x01\x00\x00"
    ptrs, lens = _ptrs([frame])
    rl = (c.c_size_t * 1)(0)
    dig = np.zeros((1, 32), dtype=np.uint8)
    pdig = dig.ctypes.data_as(c.c_void_p)
    st = (c.c_int * 1)()
    out = np.zeros(16, dtype=np.uint8)
    optrs = (c.c_void_p * 1)(out.ctypes.data)
    assert lib.zarc_gpu_verify_batch(h, 0, None, None, None, None, None, None) == _lib.OK
    assert lib.zarc_gpu_verify_batch_device(h, 0, None, None, None, None, None, None, None) == _lib.OK
    assert lib.zarc_gpu_verify_batch(h, 1, ptrs, lens, rl, None, pdig, st) == lib.zarc_gpu_unpack_batch(h, 1, ptrs, lens, rl, optrs, None, pdig, st) == _lib.OK
    for args_v, args_u in ((([None, lens, rl, None, pdig, st]), [None, lens, rl, optrs, None, pdig, st]),
                           ([ptrs, None, rl, None, pdig, st], [ptrs, None, rl, optrs, None, pdig, st]),
                           ([ptrs, lens, None, None, pdig, st], [ptrs, lens, None, optrs, None, pdig, st]),
                           ([ptrs, lens, rl, None, None, st], [ptrs, lens, rl, optrs, None, None, st]),
                           ([ptrs, lens, rl, None, pdig, None], [ptrs, lens, rl, optrs, None, pdig, None])):
        assert lib.zarc_gpu_verify_batch(h, 1, *args_v) == lib.zarc_gpu_unpack_batch(h, 1, *args_u) == _lib.E_PARAM
    nullp = (c.c_void_p * 1)(None)
    assert lib.zarc_gpu_verify_batch(h, 1, nullp, lens, rl, None, pdig, st) == _lib.E_PARAM
    big = (c.c_size_t * 1)(0xFFFFFFF0)
    assert lib.zarc_gpu_verify_batch(h, 1, ptrs, lens, big, None, pdig, st) == lib.zarc_gpu_unpack_batch(h, 1, ptrs, lens, big, optrs, None, pdig, st) == _lib.E_UNSUPPORTED
    assert lib.zarc_gpu_verify_batch(h, 1, ptrs, big, rl, None, pdig, st) == _lib.E_UNSUPPORTED
    u64 = lambda v: (c.c_uint64 * 1)(v)
    dummy = c.c_void_p(16)  # never dereferenced: the call is refused before
    assert lib.zarc_gpu_verify_batch_device(h, 1, dummy, u64(0), u64(9), u64(0xFFFFFFF0), None, pdig, st) == _lib.E_UNSUPPORTED
    assert lib.zarc_gpu_verify_batch_device(h, 1, None, u64(0), u64(9), u64(0), None, pdig, st) == _lib.E_PARAM
    assert lib.zarc_gpu_verify_batch_device(h, 1, dummy, u64(0), u64(9), u64(0), None, None, st) == _lib.E_PARAM
    assert lib.zarc_gpu_last_copy_bytes(h, 4) == 0 and lib.zarc_gpu_last_copy_bytes(h, -1) == 0
    assert lib.zarc_gpu_error_name(_lib.E_CHECK) == b"Frame failed its read-back check"


# ---- 2. copy counters of pack ----------------------------------------------------------------------------------------------------------
def check_pack_counters(engine, corpus):
    a, b, c = corpus.entry(80, 30000, 0), corpus.entry(81, 70000, 1), corpus.entry(82, 5000, 2)
    for chunk in (0, 20000):
        with settings(engine, chunk=chunk):
            ents = [a, b, c, b""]
            rc, frames, _, _, dlen = raw_pack(engine, ents)
            assert rc == 0
            h2d, d2h, ring, direct = copy_counters(engine)
            assert h2d == sum(len(e) for e in ents) and d2h == sum(dlen) and ring + direct == h2d + d2h
            # hash first, half of the batch duplicates: the duplicates come in (they are hashed on the device) and nothing of them goes out
            ents = [a, b, a, c, b, c, a, b]
            rc, frames, _, st, dlen = raw_pack(engine, ents, seen=set())
            assert rc == 0 and st == [0, 0, 8, 0, 8, 8, 8, 8] and [x for x, s in zip(dlen, st) if s == 8] == [0] * 5
            h2d, d2h, ring, direct = copy_counters(engine)
            assert h2d == sum(len(e) for e in ents) and d2h == sum(dlen) and ring + direct == h2d + d2h
    engine.blake3([a, b])
    assert copy_counters(engine)[:2] == (len(a) + len(b), 0)


def check_path_counters(engine, frames, raw_lens, entries, direct_expected):
    """which way the content went: with page-locked caller memory and zero copy on, every byte directly; otherwise none"""
    for call in ("verify", "unpack", "pack"):
        if call == "verify": engine.verify(frames, raw_lens)
        elif call == "unpack": engine.unpack(frames, raw_lens)
        else: engine.pack(entries)
        h2d, d2h, ring, direct = copy_counters(engine)
        assert ring + direct == h2d + d2h and h2d > 0, call
        assert direct == (h2d + d2h if direct_expected else 0), (call, h2d, d2h, ring, direct)


# ---- 3. bounded scratch -----------------------------------------------------------------------------------------------------------------
def check_bounded_scratch(engine, oracle, corpus):
    raws = [corpus.entry(7000 + i, 512 << 10, i % 4) for i in range(24)] + [corpus.entry(7100, 3 << 20, 0)]
    packed = engine.pack(raws)
    frames, raw_lens, expect = [f for f, _ in packed], [len(r) for r in raws], [d for _, d in packed]
    frames[3] = frames[3][:-1]          # and something to tell apart
    expect[7] = bytes(32)
    free = engine.verify(frames, raw_lens, expect)
    engine.set_parameter(_lib.PX_SCRATCH_MB, 2)
    try:
        bounded = engine.verify(frames, raw_lens, expect)
        assert copy_counters(engine)[:2] == (sum(len(f) for f in frames), 0)
    finally:
        engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
    assert bounded == free
    assert [st for _, st in free] == [0 if i not in (3, 7) else (free[3][1] if i == 3 else _lib.FRAME_DIGEST) for i in range(25)] and free[3][1] != 0
    for i, (dig, st) in enumerate(free):
        if i != 3:
            assert dig == oracle.blake3(raws[i])


# ---- 4. check off changes nothing; check on changes nothing but time ------------------------------------------------------------------
def _pack_all_ways(engine, corpus, ents, device=True):
    """host and device forms, plain and dedup: everything a caller gets back"""
    out = {}
    out["host"] = raw_pack(engine, ents)
    out["host_dedup"] = raw_pack(engine, ents, seen=set())
    if not device:
        return out
    d_src, off, pos = _arena(engine, ents)
    cap = sum(engine.bound(len(e)) for e in ents)
    d_dst = engine.malloc(cap + 256)
    try:
        for name, seen in (("device", None), ("device_dedup", set())):
            lens = [len(e) for e in ents]
            if seen is None: dst_off, dst_len, dig, st = engine.pack_device(d_src, off, lens, d_dst, cap)
            else: dst_off, dst_len, dig, st = engine.pack_device_dedup(d_src, off, lens, d_dst, cap, seen)
            blob = engine.d2h(d_dst, cap)
            out[name] = ([bytes(blob[int(o):int(o) + int(l)]) if l else None for o, l in zip(dst_off, dst_len)], bytes(dig), list(st), list(dst_len))
    finally:
        engine.free(d_src)
        engine.free(d_dst)
    return out


def check_switch_changes_nothing(engine, fresh, corpus, big):
    if big: a, b, c, r = corpus.entry(80, 30000, 0), corpus.entry(81, 70000, 1), corpus.entry(82, 3 << 20, 2), corpus.entry(83, 100000, 3)
    else: a, b, c, r = corpus.entry(80, 9000, 0), corpus.entry(81, 20000, 1), corpus.entry(82, 70000, 2), corpus.entry(83, 12000, 3)
    ents = [a, b, a, c, b"", r, b, corpus.entry(84, 1, 0)]
    assert engine.lib.zarc_gpu_set_parameter(engine.h, _lib.PX_CHECK_FRAMES, 2) == _lib.E_PARAM
    assert engine.lib.zarc_gpu_set_parameter(engine.h, _lib.PX_CHECK_FRAMES, -1) == _lib.E_PARAM
    for level, split, compress in MODES:
        for chunk in (0, 65536 if big else 16384):   # (the device forms have no chunks: they run with the first value only)
            res = []
            for e, check in ((fresh, None), (engine, 0), (engine, 1)):
                with settings(e, level=level, split=split, compress=compress, check=check or 0, chunk=chunk) if check is not None else _fresh(e, level, split, compress, chunk):
                    res.append(_pack_all_ways(e, corpus, ents, device=chunk == 0))
            assert res[0] == res[1] == res[2], (level, split, compress, chunk)
            assert res[2]["host"][0] == 0 and res[2]["host_dedup"][3] == [0, 0, 8, 0, 0, 0, 8, 0]
            assert chunk or res[2]["device_dedup"][2] == [0, 0, 8, 0, 0, 0, 8, 0]


class _fresh:
    """the handle that never heard of 9008: everything but that id"""

    def __init__(self, e, level, split, compress, chunk):
        self.e, self.v = e, (level, split, compress, chunk)

    def __enter__(self):
        level, split, compress, chunk = self.v
        self.e.set_parameter(_lib.P_COMPRESSION_LEVEL, level); self.e.set_parameter(_lib.PX_BLOCK_SPLIT, split)
        self.e.enable_compression(compress); self.e.set_parameter(_lib.PX_STAGE_CHUNK, chunk)

    def __exit__(self, *a):
        self.e.set_parameter(_lib.P_COMPRESSION_LEVEL, 3); self.e.set_parameter(_lib.PX_BLOCK_SPLIT, 0)
        self.e.enable_compression(True); self.e.set_parameter(_lib.PX_STAGE_CHUNK, 0)


# ---- 5. the check fires ---------------------------------------------------------------------------------------------------------------
def fire_batch(corpus):
    """eight entries; entry 5 is 100 000 incompressible bytes: a flipped body byte lies in a raw block and must change the decoded bytes"""
    ents = [corpus.entry(8000 + i, 20000 + 9000 * i, i % 3) for i in range(8)]
    ents[5] = corpus.entry(8005, 100000, 3)
    return ents


def _child_main(lib_path, check):
    import harness
    from zarc_amd import Engine
    e = Engine(0, lib_path)
    e.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    e.set_parameter(_lib.PX_CHECK_FRAMES, int(check))
    rc, frames, digs, st, dlen = raw_pack(e, fire_batch(harness.Corpus()))
    print(json.dumps({"rc": rc, "status": st, "dst_len": dlen, "message": e.lib.zarc_gpu_last_error(e.h).decode(), "name": e.lib.zarc_gpu_error_name(rc).decode()}))


def run_child(lib_path, check, env_extra):
    env = dict(os.environ)
    env.pop("ZARC_GPU_CHECK_FLIP_BODY", None); env.pop("ZARC_GPU_CHECK_FLIP_TAIL", None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), lib_path, str(check)], env=env, stdout=subprocess.PIPE, check=True, timeout=900).stdout
    return json.loads(out.decode().strip().splitlines()[-1])


def check_the_check_fires(diag_lib_path):
    import re
    r = run_child(diag_lib_path, 1, {})
    assert r["rc"] == 0 and r["status"] == [0] * 8, r
    good_len = r["dst_len"]
    r = run_child(diag_lib_path, 1, {"ZARC_GPU_CHECK_FLIP_BODY": "5"})
    assert r["rc"] == _lib.E_CHECK and r["name"] == "Frame failed its read-back check", r
    assert r["status"] == [0, 0, 0, 0, 0, _lib.FRAME_CORRUPT, 0, 0] and r["dst_len"][5] == 0 and r["dst_len"][:5] == good_len[:5], r
    m = re.search(r"entry (\d+) .*byte (\d+)", r["message"])
    assert m and int(m.group(1)) == 5 and int(m.group(2)) < 100000, r
    r = run_child(diag_lib_path, 1, {"ZARC_GPU_CHECK_FLIP_TAIL": "5"})
    assert r["rc"] == _lib.E_CHECK and r["status"] == [0, 0, 0, 0, 0, _lib.FRAME_CORRUPT, 0, 0], r
    assert re.search(r"entry 5\b", r["message"]) and "trailer" in r["message"], r
    r = run_child(diag_lib_path, 0, {"ZARC_GPU_CHECK_FLIP_BODY": "5", "ZARC_GPU_CHECK_FLIP_TAIL": "5"})
    assert r["rc"] == 0 and r["status"] == [0] * 8 and r["dst_len"] == good_len, r      # the check did not run


def check_product_reads_no_variable(lib_path):
    r = run_child(lib_path, 1, {"ZARC_GPU_CHECK_FLIP_BODY": "5", "ZARC_GPU_CHECK_FLIP_TAIL": "5"})
    assert r["rc"] == 0 and r["status"] == [0] * 8, r


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])
