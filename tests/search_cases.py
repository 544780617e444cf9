"""Checks of zarc_gpu_search_batch*, shared by the emulator tests (test_search.py) and the GPU tests (test_gpu_search.py).

The reference for every expected value is Python's `re` on the CPU, over the bytes the frames were packed from -- never the engine:
    count = len(re.findall(b"(?=" + re.escape(p) + b")", d, flags))      (overlapping occurrences count)
    first = re.search(re.escape(p), d, flags)
with flags = re.I for the case-folding search (a bytes pattern folds ASCII letters only).  Every comparison is equality."""
import ctypes
import os
import re

import numpy as np

import make_golden
import verify_cases as vc
from zarc_amd import _lib

SLICE = 65536  # zarc_search_scan: start positions per workgroup


def ref(d, p, icase=False):
    """-> (count, first or None) of the fixed byte string p in d"""
    flags = re.I if icase else 0
    m = re.search(re.escape(p), d, flags)
    return len(re.findall(b"(?=" + re.escape(p) + b")", d, flags)), (m.start() if m else None)


def plant(raw, needle, offsets):
    b = bytearray(raw)
    for o in offsets:
        b[o:o + len(needle)] = needle
    assert len(b) == len(raw)
    return bytes(b)


def pack(engine, raws, level=3, compress=True):
    """-> (frames, raw_lens, digests).  The emulator tests pack their large batches in store mode (compress=False) where the encoder is not
    the subject -- its match finder runs at 100 KB/s there: the decoded bytes lie in the scratch exactly as those of compressed frames do."""
    with vc.settings(engine, level=level, compress=compress):
        packed = engine.pack(raws)
    return [f for f, _ in packed], [len(r) for r in raws], [d for _, d in packed]


def check_search(engine, packed, raws, needle, icase=False, tag=""):
    """one search call over a packed batch against the reference; every frame is good, so every verdict is OK.  -> [(count, first)]"""
    frames, raw_lens, digests = packed
    got = engine.search(frames, raw_lens, needle, icase=icase, expect=digests)
    assert len(got) == len(raws)
    for i, (st, dig, count, first) in enumerate(got):
        assert st == _lib.FRAME_OK and dig == digests[i], (tag, i, st)
        assert (count, first) == ref(raws[i], needle, icase), (tag, i, len(raws[i]), needle, icase)
    return [(g[2], g[3]) for g in got]


# ---- 1. boundaries: 16-byte steps, slices, the frame's end --------------------------------------------------------------------------
NEEDLE7 = b"\x01Zq~\x02Kx"
LEN1 = 3 * SLICE + 1000
OFFSETS1 = [0, 1, 15, 16, 17] + [SLICE - k for k in range(1, 8)] + [SLICE, 2 * SLICE - 3, LEN1 - 7]


def check_boundaries(engine, corpus, compress=True):
    text = corpus.entry(4000, LEN1, 0)
    assert ref(text, NEEDLE7) == (0, None)
    raws = [plant(text, NEEDLE7, OFFSETS1)]                                 # all of them in one frame (later ones overwrite overlapped earlier ones)
    raws += [plant(text, NEEDLE7, [o]) for o in OFFSETS1]                   # ... and every offset alone
    raws.append(plant(corpus.entry(4001, 5000, 0), NEEDLE7[:6], [5000 - 6]))  # ends with the first 6 bytes: must not match there
    raws += [NEEDLE7[:-1], NEEDLE7, b"", NEEDLE7 + NEEDLE7[:3], b"x" + NEEDLE7]  # shorter than the needle, exactly it, empty, ...
    got = check_search(engine, pack(engine, raws, compress=compress), raws, NEEDLE7, tag="boundaries")
    assert got[0][0] >= 6 and got[0][1] == 1                               # (offset 0's copy is overwritten by offset 1's)
    assert [g for g in got[1:1 + len(OFFSETS1)]] == [(1, o) for o in OFFSETS1]
    n = 1 + len(OFFSETS1)
    assert got[n:] == [(0, None), (0, None), (1, 0), (0, None), (1, 0), (1, 1)]


NEEDLE_LENS = (1, 2, 3, 4, 5, 16, 17, 255, 256)


def needle_of(m):
    return bytes((i * 89 + m * 7) % 127 + 128 for i in range(m))           # bytes >= 0x80: not in the corpus text


def check_needle_lengths(engine, corpus, compress=True):
    """needles of every length class, each across a 16-byte step, across a slice boundary, at the frame's very end -- and cut short by it"""
    length = 2 * SLICE + 500
    raws, want = [], []
    for j, m in enumerate(NEEDLE_LENS):
        nd = needle_of(m)
        offs = [16 * 1000 - (1 if m > 1 else 0), SLICE - max(1, m // 2), length - m]
        if m == 1: offs += [SLICE - 1, SLICE, 15, 16]
        raws.append(plant(corpus.entry(4100 + j, length, 0), nd, offs))
        want.append(len(set(offs)))
        raws.append(plant(corpus.entry(4150 + j, length, 0), nd[:m - 1] if m > 1 else b"", [length - (m - 1)]))  # all but the last byte at the end
    packed = pack(engine, raws, compress=compress)
    for j, m in enumerate(NEEDLE_LENS):
        got = check_search(engine, packed, raws, needle_of(m), tag="needle of %d" % m)
        assert got[2 * j][0] == want[j] and got[2 * j + 1] == (0, None), (m, got[2 * j], got[2 * j + 1])


# ---- 2. neighbours in the scratch ----------------------------------------------------------------------------------------------------
def check_neighbours(engine, corpus, compress=True):
    """64 frames of exactly 4096 bytes lie back to back in the decoder's scratch, whatever order it puts them in; each begins with
    needle[k:] and ends with needle[:k], so every neighbour pair would complete a match across a frame's end"""
    needle = b"\xf1NEEDLE\xf2"
    for k in (1, 4, len(needle) - 1):
        raws = []
        for i in range(64):
            b = bytearray(corpus.entry(4200 + i, 4096, 0))
            b[:len(needle) - k] = needle[k:]
            b[4096 - k:] = needle[:k]
            raws.append(bytes(b))
        got = check_search(engine, pack(engine, raws, compress=compress), raws, needle, tag="neighbours k=%d" % k)
        assert got == [(0, None)] * 64


# ---- 3. overlap and the worst case ---------------------------------------------------------------------------------------------------
def check_overlap(engine, compress=True):
    raws = [b"a" * 200000, b"abab" * 30000]
    packed = pack(engine, raws, compress=compress)
    for m in (1, 4, 256):
        got = check_search(engine, packed, raws, b"a" * m, tag="run, %d" % m)
        assert got[0] == (200000 - m + 1, 0)
    got = check_search(engine, packed, raws, b"ababa", tag="abab")
    assert got == [(0, None), (2 * 30000 - 2, 0)]


# ---- 4. case folding -----------------------------------------------------------------------------------------------------------------
def check_case_folding(engine, corpus, compress=True):
    text = corpus.entry(4300, 70000, 0)
    raws = [
        plant(text, b"hello WORLD", [5]) + b"HELLO world" + text[:777] + b"hElLo wOrLd" + b"Hello World",
        b"0123{A4567{a89`A@a" * 200,                     # '{' is '[' + 0x20, '`' is '@' + 0x20: not letters, never folded
        b"xx[Ayy[azz" * 50,
        plant(text, b"\xc4B\xe4", [100, SLICE - 1]) + b"\xe4b\xc4..\xc4b\xc4..\xe4B\xe4..\xc4b\xe4",   # 0xC4 / 0xE4 differ by 0x20 as well
        b"`Z@" * 33 + b"@z`",
    ]
    packed = pack(engine, raws, compress=compress)
    res = {}
    for needle in (b"Hello World", b"[a", b"\xc4b\xe4", b"@z`", b"{A"):
        for icase in (False, True):
            res[needle, icase] = check_search(engine, packed, raws, needle, icase, tag="case %r %r" % (needle, icase))
    assert res[b"Hello World", False][0] == (1, len(raws[0]) - 11) and res[b"Hello World", True][0] == (4, 5)
    assert res[b"[a", False][1] == res[b"[a", True][1] == (0, None)        # planted "{A": only the letter folds, so still no match
    assert res[b"[a", False][2][0] == 50 and res[b"[a", True][2][0] == 100
    assert res[b"\xc4b\xe4", False][3][0] == 1 and res[b"\xc4b\xe4", True][3][0] == 3
    assert res[b"@z`", False][4] == (1, 99) and res[b"@z`", True][4] == (1, 99)
    assert res[b"{A", True][1][0] == 400 and res[b"{A", False][1][0] == 200


# ---- 5. many small frames ------------------------------------------------------------------------------------------------------------
def small_entries(corpus, n=3000):
    return [corpus.entry(4400 + i, (i * 7919) % 301, i % 4) for i in range(n)]


def check_many_small(engine, corpus):
    raws = small_entries(corpus)
    needle = raws[0 + 4 * 20][40:42]                                        # two bytes of a text entry
    assert len(needle) == 2
    for compress in (True, False):
        got = check_search(engine, pack(engine, raws, compress=compress), raws, needle, tag="small, compress %r" % compress)
        assert sum(c for c, _ in got) > 10 and sum(c == 0 for c, _ in got) > 10


# ---- 6. frames in pieces, other encoders' frames -------------------------------------------------------------------------------------
def check_pieces(engine, oracle, corpus, golden_frames):
    d, m = golden_frames
    raws, frames = [corpus.entry(4500, (4 << 20) + 17, 0)], []
    frames.append(pack(engine, raws)[0][0])
    for name in ("text300", "records200k", "lz300k"):
        fr = next(f for f in m["frames"] if f["recipe"] == name and f["level"] == 3 and f["checksum"] == 1 and f["libzstd"].startswith("1.5"))
        frames.append(open(os.path.join(d, fr["file"]), "rb").read())
        raws.append(make_golden.recipe_bytes(m["recipes"][name], corpus))
    packed = (frames, [len(r) for r in raws], [oracle.blake3(r) for r in raws])
    for i, r in enumerate(raws):
        at = len(r) // 2
        needle = r[at:at + (9, 3, 6, 5)[i]]
        got = check_search(engine, packed, raws, needle, tag="pieces %d" % i)
        assert got[i][0] >= 1


# ---- 7. verdict parity and bad frames ------------------------------------------------------------------------------------------------
def check_verdicts(engine, oracle, corpus, golden_frames):
    frames, raw_lens, expect, raws = vc.error_list(oracle, corpus, golden_frames)
    good = [corpus.entry(4600 + i, 30000 + i, 0) for i in range(2)]
    needle = raws[0][150:155]
    good = [plant(g, needle, [77, 20000]) for g in good]
    gf, gl, gd = pack(engine, good)
    frames, raw_lens, expect, raws = [gf[0]] + frames + [gf[1]], [gl[0]] + raw_lens + [gl[1]], [gd[0]] + expect + [gd[1]], [good[0]] + raws + [good[1]]
    for exp in (expect, None):
        want = engine.verify(frames, raw_lens, exp)
        got = engine.search(frames, raw_lens, needle, expect=exp)
        assert [(dig, st) for st, dig, _, _ in got] == want
        st = [g[0] for g in got]
        assert st[0] == st[1] == st[8] == _lib.FRAME_OK and st[2] == _lib.FRAME_CHECKSUM and st[3] == _lib.FRAME_BAD_MAGIC and st[7] == _lib.FRAME_SRCSIZE
        assert st[6] == (_lib.FRAME_DIGEST if exp else _lib.FRAME_OK)
        for i, (s, _, count, first) in enumerate(got):
            if s in (_lib.FRAME_OK, _lib.FRAME_DIGEST):
                assert (count, first) == ref(raws[i], needle) and count >= 1, i   # a digest mismatch is searched: unpack delivers its bytes
            else:
                assert (count, first) == (0, None), i
        assert sum(s in (_lib.FRAME_OK, _lib.FRAME_DIGEST) for s in st) == 4


# ---- 8. bounded scratch --------------------------------------------------------------------------------------------------------------
def check_bounded_scratch(engine, corpus, compress=True):
    raws = small_entries(corpus) + [corpus.entry(4700 + i, 1 << 20, i) for i in range(3)]
    needle = raws[80][40:42]
    packed = pack(engine, raws, compress=compress)
    free = check_search(engine, packed, raws, needle, tag="budget 0")
    t_free = engine.kernel_ms(_lib.T_SEARCH)
    for mb in (2, 1):                                                      # (check_bounded_scratch of verify_cases runs under 2): two parts and more
        engine.set_parameter(_lib.PX_SCRATCH_MB, mb)
        try:
            assert check_search(engine, packed, raws, needle, tag="budget %d" % mb) == free
            assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in packed[0]), 0)
            assert engine.kernel_ms(_lib.T_SEARCH) > 0 and t_free > 0
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)


# ---- 9. device form and counters -----------------------------------------------------------------------------------------------------
def check_device_form(engine, corpus, compress=True):
    raws = [plant(corpus.entry(4800 + i, n, i % 4), NEEDLE7, [n // 3] if n > 30 else []) for i, n in enumerate((0, 1, 70000, 200000, 5, 7, 65536 + 7, 4096))]
    raws[5] = NEEDLE7
    frames, raw_lens, digests = packed = pack(engine, raws, compress=compress)
    host = engine.search(frames, raw_lens, NEEDLE7, expect=digests)
    assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in frames), 0)
    h2d, d2h, ring, direct = vc.copy_counters(engine)
    assert ring + direct == h2d
    assert engine.kernel_ms(_lib.T_SEARCH) > 0 and engine.kernel_ms(_lib.T_TOTAL) >= engine.kernel_ms(_lib.T_SEARCH)
    assert engine.kernel_ms(_lib.T_BLAKE3) >= 0 and engine.kernel_ms(_lib.T_DECODE) >= 0
    check_search(engine, packed, raws, NEEDLE7, tag="device form, host")
    d_frames, foff, _ = vc._arena(engine, frames)
    try:
        exp = np.frombuffer(b"".join(digests), dtype=np.uint8)
        for icase in (False, True):
            dev = engine.search_device(d_frames, foff, [len(f) for f in frames], raw_lens, NEEDLE7, icase=icase, expect=exp)
            assert vc.copy_counters(engine) == (0, 0, 0, 0)
            assert engine.kernel_ms(_lib.T_SEARCH) > 0
            assert dev == engine.search(frames, raw_lens, NEEDLE7, icase=icase, expect=digests)
        assert engine.search_device(d_frames, foff, [len(f) for f in frames], raw_lens, NEEDLE7, expect=exp) == host
        engine.verify_device(d_frames, foff, [len(f) for f in frames], raw_lens, exp)
        assert engine.kernel_ms(_lib.T_SEARCH) in (0.0, -1.0)             # an unused timer, as after any call that does not search
    finally:
        engine.free(d_frames)
    engine.verify(frames, raw_lens, digests)
    assert engine.kernel_ms(_lib.T_SEARCH) in (0.0, -1.0)
    engine.unpack(frames, raw_lens, digests)
    assert engine.kernel_ms(_lib.T_SEARCH) in (0.0, -1.0)


# ---- 10. arguments -------------------------------------------------------------------------------------------------------------------
def check_arguments(engine, corpus):
    lib, h = engine.lib, engine.h
    c = ctypes
    raw = plant(corpus.entry(4900, 5000, 0), NEEDLE7, [1234])
    frames, raw_lens, digests = pack(engine, [raw])
    ptrs, lens = vc._ptrs(frames)
    rl = (c.c_size_t * 1)(len(raw))
    dig = np.zeros((1, 32), dtype=np.uint8)
    pdig = dig.ctypes.data_as(c.c_void_p)
    st, cnt, fst = (c.c_int * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)()
    pat = c.cast(c.c_char_p(NEEDLE7), c.c_void_p)
    long_pat = c.cast(c.c_char_p(b"p" * 300), c.c_void_p)

    def host(n=1, ptrs=ptrs, lens=lens, rl=rl, pat=pat, m=7, flags=0, pdig=pdig, st=st, cnt=cnt, fst=fst):
        return lib.zarc_gpu_search_batch(h, n, ptrs, lens, rl, None, pat, m, flags, pdig, st, cnt, fst)
    assert host() == _lib.OK and (st[0], cnt[0], fst[0]) == (0, 1, 1234)
    assert host(pat=None) == host(m=0) == host(pat=long_pat, m=257) == _lib.E_PARAM
    assert host(pat=long_pat, m=256) == _lib.OK and (cnt[0], fst[0]) == (0, _lib.SEARCH_NONE)
    assert host(flags=2) == host(flags=3) == host(flags=0x80000000) == _lib.E_PARAM
    assert host(st=None) == host(cnt=None) == host(fst=None) == host(pdig=None) == _lib.E_PARAM
    assert host(ptrs=None) == host(lens=None) == host(rl=None) == _lib.E_PARAM
    assert host(n=0, ptrs=None, lens=None, rl=None) == _lib.OK
    big = (c.c_size_t * 1)(0xFFFFFFF0)
    assert host(rl=big) == host(lens=big) == _lib.E_UNSUPPORTED
    u64 = lambda v: (c.c_uint64 * 1)(v)
    dummy = c.c_void_p(16)  # never dereferenced: the call is refused before

    def dev(n=1, base=dummy, off=u64(0), fl=u64(9), rl=u64(0), pat=pat, m=7, flags=0, pdig=pdig, st=st, cnt=cnt, fst=fst):
        return lib.zarc_gpu_search_batch_device(h, n, base, off, fl, rl, None, pat, m, flags, pdig, st, cnt, fst)
    assert dev(n=0, base=None, off=None, fl=None, rl=None) == _lib.OK
    assert dev(base=None) == dev(off=None) == dev(fl=None) == dev(rl=None) == _lib.E_PARAM
    assert dev(pat=None) == dev(m=0) == dev(m=257) == dev(flags=4) == _lib.E_PARAM
    assert dev(st=None) == dev(cnt=None) == dev(fst=None) == dev(pdig=None) == _lib.E_PARAM
    assert dev(rl=u64(0xFFFFFFF0)) == dev(fl=u64(1 << 32)) == _lib.E_UNSUPPORTED
    # ... and the handle still works
    assert host(flags=_lib.SEARCH_ICASE) == _lib.OK and (st[0], cnt[0], fst[0]) == (0, 1, 1234)
    assert engine.search(frames, raw_lens, NEEDLE7, expect=digests) == [(0, digests[0], 1, 1234)]


# ---- 13. real data (GPU) -------------------------------------------------------------------------------------------------------------
def check_real_items(engine, real_items):
    raws = list(real_items.values())
    packed = pack(engine, raws)
    for i, r in enumerate(raws):
        needle = r[len(r) // 2:len(r) // 2 + 4]
        got = check_search(engine, packed, raws, needle, tag="real item %d" % i)
        assert got[i][0] >= 1
