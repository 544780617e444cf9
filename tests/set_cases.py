"""Checks of zarc_gpu_search_set_* (a set of fixed strings searched in one pass), shared by the emulator tests (test_set.py) and the GPU
tests (test_gpu_set.py).

The reference for every expected value is Python's `re` on the CPU, over the bytes the frames were packed from -- never the engine.  Per
pattern it gives the set of start positions
    {m.start() for m in re.finditer(b"(?=" + re.escape(p) + b")", d, flags)}        (flags = re.I for the case-folding search)
and nothing else filters them: the frame-end rule is per pattern because `re` sees one frame's bytes at a time.  The union of those sets
gives count and first, the lowest index whose set holds `first` gives which, the sets' sizes summed over the frames give hits, and the
lowest union position inside a line gives the line's record.  Every comparison is equality."""
import bisect
import ctypes
import os
import random
import re

import numpy as np

import lines_cases as lc
import make_golden
import search_cases as sc
import verify_cases as vc
from zarc_amd import _lib

S = sc.SLICE
LEN1 = 3 * S + 1000            # the largest frame of these cases (but the one multi-MiB frame of the pieces case)
DECODED = (_lib.FRAME_OK, _lib.FRAME_DIGEST)


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def positions(d, p, icase=False):
    return {m.start() for m in re.finditer(b"(?=" + re.escape(p) + b")", d, re.I if icase else 0)}


def ref(d, pats, icase=False):
    """-> (count, first, which, per-pattern counts, sorted union) of the set in one frame's bytes"""
    pos = [positions(d, p, icase) for p in pats]
    union = sorted(set().union(*pos))
    first = union[0] if union else None
    which = next(k for k, s in enumerate(pos) if first in s) if union else None
    return len(union), first, which, [len(s) for s in pos], union


def ref_lines(d, union):
    """-> [(start, length, number, match)] of the lines that hold a position of the sorted list `union`"""
    out, pos, no = [], 0, 1
    for piece in d.split(b"\n"):
        j = bisect.bisect_left(union, pos)
        if j < len(union) and union[j] < pos + len(piece): out.append((pos, len(piece), no, union[j]))
        pos += len(piece) + 1; no += 1
    return out


def check_set(engine, packed, raws, pats, icase=False, tag="", call=None, refs=None):
    """one search_set call over a packed batch of good frames against the reference -> (results, hits)"""
    frames, raw_lens, digests = packed
    call = call or (lambda: engine.search_set(frames, raw_lens, pats, icase=icase, expect=digests))
    results, hits = call()
    assert len(results) == len(raws) and len(hits) == len(pats)
    want_hits = [0] * len(pats)
    for i, (st, dig, count, first, which) in enumerate(results):
        c, f, w, per, _ = refs[i] if refs else ref(raws[i], pats, icase)
        assert st == _lib.FRAME_OK and dig == digests[i], (tag, i, st)
        assert (count, first, which) == (c, f, w), (tag, i, len(raws[i]), (count, first, which), (c, f, w))
        want_hits = [a + b for a, b in zip(want_hits, per)]
    assert hits == want_hits, (tag, [(k, a, b) for k, (a, b) in enumerate(zip(hits, want_hits)) if a != b][:8])
    return results, hits


# ---- 1. a set of one pattern is the one-pattern search -------------------------------------------------------------------------------
def one_pattern_frames(corpus):
    """the frames of search_cases.check_boundaries and check_needle_lengths"""
    text = corpus.entry(4000, sc.LEN1, 0)
    raws = [sc.plant(text, sc.NEEDLE7, sc.OFFSETS1)] + [sc.plant(text, sc.NEEDLE7, [o]) for o in sc.OFFSETS1]
    raws.append(sc.plant(corpus.entry(4001, 5000, 0), sc.NEEDLE7[:6], [5000 - 6]))
    raws += [sc.NEEDLE7[:-1], sc.NEEDLE7, b"", sc.NEEDLE7 + sc.NEEDLE7[:3], b"x" + sc.NEEDLE7]
    length = 2 * S + 500
    for j, m in enumerate(sc.NEEDLE_LENS):
        nd = sc.needle_of(m)
        offs = [16 * 1000 - (1 if m > 1 else 0), S - max(1, m // 2), length - m]
        if m == 1: offs += [S - 1, S, 15, 16]
        raws.append(sc.plant(corpus.entry(4100 + j, length, 0), nd, offs))
        raws.append(sc.plant(corpus.entry(4150 + j, length, 0), nd[:m - 1] if m > 1 else b"", [length - (m - 1)]))
    return raws


def check_one_pattern(engine, corpus, compress=True):
    raws = one_pattern_frames(corpus)
    frames, raw_lens, digests = packed = sc.pack(engine, raws, compress=compress)
    seen = 0
    for p in [sc.needle_of(m) for m in sc.NEEDLE_LENS] + [sc.NEEDLE7]:
        one = engine.search(frames, raw_lens, p, expect=digests)
        res, hits = engine.search_set(frames, raw_lens, [p], expect=digests)
        assert [r[:4] for r in res] == one, len(p)
        assert [r[4] for r in res] == [0 if r[2] else None for r in res]
        assert hits == [sum(r[2] for r in one)]
        for i, r in enumerate(raws):                                        # ... and both are the reference's
            assert one[i][2:] == sc.ref(r, p), (len(p), i)
        seen += hits[0]
    assert seen > 40


# ---- 2. every length class in one set ------------------------------------------------------------------------------------------------
def mixed_set():
    """lengths 256, 255, 17, 16, 5, 4, 3, 2, 1 in this order, bytes >= 0x80; the 17- and 5-byte ones are prefixes of the 256-byte one (and
    sc.needle_of(2) happens to be one as well), so a planted long pattern is a match of several patterns at one position"""
    base = sc.needle_of(256)
    return [base, sc.needle_of(255), base[:17], sc.needle_of(16), base[:5], sc.needle_of(4), sc.needle_of(3), sc.needle_of(2), sc.needle_of(1)]


def check_mixed_classes(engine, corpus, compress=True):
    pats = mixed_set()
    assert sorted(len(p) for p in pats) == sorted(sc.NEEDLE_LENS)
    raws = []
    for j, p in enumerate(pats):
        m = len(p)
        for f in range(3):                                                  # S - k for k = 0 .. 7, each at a slice boundary of its own
            offs = [b * S - (3 * f + b - 1) for b in (1, 2, 3) if 3 * f + b - 1 <= 7]
            if f == 0: offs.append(16 * 1000 - (1 if m > 1 else 0))         # across a 16-byte step
            if f == 1: offs.append(LEN1 - m)                                # the frame's very end
            raws.append(sc.plant(corpus.entry(6000 + 3 * j + f, LEN1, 0), p, offs))
    two = sc.plant(corpus.entry(6100, 9000, 0), pats[2], [100])             # the 17-byte one: the 5- and the 2-byte one match there too
    two = sc.plant(two, pats[0], [5000])                                    # the 256-byte one: four patterns at one position
    raws += [two, pats[0][:255], pats[4][:4] + b"x", b"", pats[8]]
    packed = sc.pack(engine, raws, compress=compress)
    res, hits = check_set(engine, packed, raws, pats, tag="mixed classes")
    n = len(pats) * 3
    assert res[n][2:] == (res[n][2], 100, 2)                                # the lowest index of those that match at 100
    assert res[n + 1][3:] == (0, 2) and res[n + 2][3:] == (0, 7) and res[n + 3][2:] == (0, None, None) and res[n + 4][2:] == (1, 0, 8)
    assert all(h >= 10 for h in hits)
    only_long = [p for p in pats if len(p) >= 4]                            # a set without the short classes
    check_set(engine, packed, raws, only_long, tag="classes of 4 and more")
    check_set(engine, packed, raws, pats[6:], tag="short classes only")


# ---- 3. the frame's end is per pattern -----------------------------------------------------------------------------------------------
def check_frame_end(engine, corpus, compress=True):
    long_p = bytes(range(0xA0, 0xB1))
    short_p = long_p[:5]
    assert len(long_p) == 17
    body = corpus.entry(6200, 5000, 0)
    raws = [body + long_p[:16], body + long_p, body + long_p[:4], long_p[:16], short_p, long_p[:4]]
    res, hits = check_set(engine, sc.pack(engine, raws, compress=compress), raws, [long_p, short_p], tag="frame end")
    assert res[0][2:] == (1, 5000, 1) and res[1][2:] == (1, 5000, 0) and res[2][2:] == (0, None, None)
    assert res[3][2:] == (1, 0, 1) and res[4][2:] == (1, 0, 1) and res[5][2:] == (0, None, None)
    assert hits == [1, 4]
    needle = b"\xf1NEEDLE\xf2"                                             # search_cases.check_neighbours: 64 frames of 4096 bytes back to back
    for k in (1, 4, len(needle) - 1):
        raws = []
        for i in range(64):
            b = bytearray(corpus.entry(4200 + i, 4096, 0))
            b[:len(needle) - k] = needle[k:]
            b[4096 - k:] = needle[:k]
            raws.append(bytes(b))
        _, hits = check_set(engine, sc.pack(engine, raws, compress=compress), raws, [needle, needle[1:], needle[:-1]], tag="neighbours k=%d" % k)
        assert hits[0] == 0


# ---- 4. patterns that share their key ------------------------------------------------------------------------------------------------
def check_shared_keys(engine, corpus, compress=True):
    head = b"\xe1\xe2\xe3\xe4"
    rnd = random.Random(4)
    pats = [head + bytes([0x80 + i // 100, 0x80 + i % 100]) + bytes(rnd.randrange(0x80, 0x100) for _ in range(i % 23)) for i in range(300)]
    text = corpus.entry(6300, S + 5000, 0)
    raw = sc.plant(text, head + b"zz", [50, S - 2])                         # the key alone: a candidate of 300 patterns, a match of none
    for n, i in enumerate((0, 7, 150, 299, 22, 23)):
        raw = sc.plant(raw, pats[i], [1000 + 700 * n, S - 3 + 64 * n + 700])
    raws = [raw, text, head, pats[299]]
    _, hits = check_set(engine, sc.pack(engine, raws, compress=compress), raws, pats, tag="300 patterns, one key")
    assert sum(hits) >= 13 and hits[299] == 3
    # prefixes of one another: the union counts a position once, every pattern counts its own
    pats = [b"a", b"ab", b"abc", b"abcd", b"abcde", b"abcdefghi"]
    raws = [b"xxabcdefghixx abcd a" * 3 + b"abcdefgh", b"abcdefghi", b"bcdefghi", b"ab" * 40000]
    res, hits = check_set(engine, sc.pack(engine, raws, compress=compress), raws, pats, tag="prefixes")
    assert hits == [10 + 1 + 40000, 7 + 1 + 40000, 7 + 1, 7 + 1, 4 + 1, 3 + 1] and res[0][2:] == (10, 2, 0) and res[3][2] == 40000
    # the same pattern twice
    res, hits = check_set(engine, sc.pack(engine, raws, compress=compress), raws, [b"abcd", b"bc", b"abcd"], tag="twice")
    assert hits[0] == hits[2] == 8 and res[1][4] == 0 and res[2][4] == 1


# ---- 5. the fullest set --------------------------------------------------------------------------------------------------------------
_full = {}


def full_set(corpus):
    """1024 seeded patterns of lengths 1 .. 256 (bytes >= 0x80), about 40 of them planted in three frames of ~200 KB; -> (pats, raws, refs).
    The reference of this case takes its time (3072 passes of `re`): it is computed once and shared."""
    if not _full:
        rnd = random.Random(5)
        lens = [1, 2, 3, 4, 5, 255, 256] * 4 + [rnd.randrange(1, 257) for _ in range(1024 - 28)]
        pats = [bytes(rnd.randrange(0x80, 0x100) for _ in range(m)) for m in lens]
        raws = []
        for f in range(3):
            raw = corpus.entry(6400 + f, 200000 + 1000 * f, 0)
            for n in range(14):
                p = pats[(f * 14 + n) * 24 % 1024]
                raw = sc.plant(raw, p, [3000 + 14000 * n, len(raw) - len(p)] if n == f else [3000 + 14000 * n])
            raws.append(raw)
        _full["v"] = (pats, raws, [ref(r, pats) for r in raws])
    return _full["v"]


def check_full_set(engine, corpus, compress=True):
    pats, raws, refs = full_set(corpus)
    assert len(pats) == _lib.SEARCH_MAX_SET
    packed = sc.pack(engine, raws, compress=compress)
    _, hits = check_set(engine, packed, raws, pats, tag="1024 patterns", refs=refs)
    assert sum(h > 0 for h in hits) >= 40
    try:
        engine.search_set(packed[0], packed[1], pats + [b"one more"], expect=packed[2])
        assert False, "1025 patterns were accepted"
    except Exception as e:
        assert getattr(e, "code", None) == _lib.E_PARAM
    check_set(engine, packed, raws, pats, tag="... and the handle still works", refs=refs)


# ---- 6. overlap and the worst case ---------------------------------------------------------------------------------------------------
def check_overlap(engine, compress=True):
    raws = [b"a" * 200000, b"abab" * 30000]
    pats = [b"a", b"aa", b"aaaa", b"a" * 256, b"ababa"]
    res, hits = check_set(engine, sc.pack(engine, raws, compress=compress), raws, pats, tag="runs")
    assert [r[2:] for r in res] == [(200000, 0, 0), (60000, 0, 0)]
    assert hits == [200000 + 60000, 199999, 199997, 200000 - 255, 2 * 30000 - 2]
    res, hits = check_set(engine, sc.pack(engine, raws, compress=compress), raws, pats[1:], tag="runs, without the single byte")
    assert [r[2:] for r in res] == [(199999, 0, 0), (59998, 0, 3)]


# ---- 7. case folding -----------------------------------------------------------------------------------------------------------------
def check_case_folding(engine, corpus, compress=True):
    text = corpus.entry(4300, 70000, 0)
    raws = [                                                               # search_cases.check_case_folding's frames
        sc.plant(text, b"hello WORLD", [5]) + b"HELLO world" + text[:777] + b"hElLo wOrLd" + b"Hello World",
        b"0123{A4567{a89`A@a" * 200,
        b"xx[Ayy[azz" * 50,
        sc.plant(text, b"\xc4B\xe4", [100, S - 1]) + b"\xe4b\xc4..\xc4b\xc4..\xe4B\xe4..\xc4b\xe4",
        b"`Z@" * 33 + b"@z`",
    ]
    pats = [b"Hello World", b"hELLO wORLD", b"[a", b"{A", b"\xc4b\xe4"]
    packed = sc.pack(engine, raws, compress=compress)
    res, hits = check_set(engine, packed, raws, pats, icase=False, tag="case, exact")
    assert hits == [1, 0, 50, 200, 1] and res[0][2:] == (1, len(raws[0]) - 11, 0)
    res, hits = check_set(engine, packed, raws, pats, icase=True, tag="case, folded")
    assert hits[0] == hits[1] == 4 and res[0][2:] == (4, 5, 0)              # the two spellings match at the same positions: each counts once
    assert hits[2:] == [100, 400, 3] and res[1][2] == 400 and res[2][2] == 100


# ---- 8. many small frames ------------------------------------------------------------------------------------------------------------
def small_set(raws):
    """eight needles of 2 .. 5 bytes cut from the entries"""
    pick = [r for r in raws if len(r) > 120][:40:5]
    return [r[40 + 3 * k:40 + 3 * k + 2 + k % 4] for k, r in enumerate(pick)]


def check_many_small(engine, corpus):
    raws = sc.small_entries(corpus)
    pats = small_set(raws)
    assert len(pats) == 8 and sorted(set(len(p) for p in pats)) == [2, 3, 4, 5]
    refs = [ref(r, pats) for r in raws]
    for compress in (True, False):
        res, hits = check_set(engine, sc.pack(engine, raws, compress=compress), raws, pats, tag="small, compress %r" % compress, refs=refs)
        assert sum(r[2] > 0 for r in res) > 10 and sum(r[2] == 0 for r in res) > 10 and all(h > 0 for h in hits)


# ---- 9. verdicts ---------------------------------------------------------------------------------------------------------------------
def check_verdicts(engine, oracle, corpus, golden_frames):
    frames, raw_lens, expect, raws = vc.error_list(oracle, corpus, golden_frames)
    good = [corpus.entry(4600 + i, 30000 + i, 0) for i in range(2)]
    pats = [raws[0][150:155], raws[0][200:203], b"\xfe\xfd"]
    good = [sc.plant(g, pats[0], [77, 20000]) for g in good]
    gf, gl, gd = sc.pack(engine, good)
    frames, raw_lens, expect, raws = [gf[0]] + frames + [gf[1]], [gl[0]] + raw_lens + [gl[1]], [gd[0]] + expect + [gd[1]], [good[0]] + raws + [good[1]]
    for exp in (expect, None):
        want = engine.verify(frames, raw_lens, exp)
        got, hits = engine.search_set(frames, raw_lens, pats, expect=exp)
        assert [(dig, st) for st, dig, _, _, _ in got] == want
        st = [g[0] for g in got]
        assert st[0] == st[1] == st[8] == _lib.FRAME_OK and st[2] == _lib.FRAME_CHECKSUM and st[3] == _lib.FRAME_BAD_MAGIC and st[7] == _lib.FRAME_SRCSIZE
        assert st[6] == (_lib.FRAME_DIGEST if exp else _lib.FRAME_OK)       # the DIGEST frame is searched
        want_hits = [0] * len(pats)
        for i, (s, _, count, first, which) in enumerate(got):
            if s in DECODED:
                c, f, w, per, _ = ref(raws[i], pats)
                assert (count, first, which) == (c, f, w) and count >= 1, i
                want_hits = [a + b for a, b in zip(want_hits, per)]
            else:
                assert (count, first, which) == (0, None, None), i
        assert sum(s in DECODED for s in st) == 4
        assert hits == want_hits and hits[2] == 0                           # frames that did not decode add nothing


# ---- 10. bounded scratch -------------------------------------------------------------------------------------------------------------
def check_bounded_scratch(engine, corpus, compress=True):
    raws = sc.small_entries(corpus) + [corpus.entry(4700 + i, 1 << 20, i) for i in range(3)]
    pats = small_set(raws)[:4] + [raws[-3][5000:5007]]
    packed = sc.pack(engine, raws, compress=compress)
    refs = [ref(r, pats) for r in raws]
    free = check_set(engine, packed, raws, pats, tag="budget 0", refs=refs)
    assert engine.kernel_ms(_lib.T_SEARCH) > 0
    for mb in (2, 1):
        engine.set_parameter(_lib.PX_SCRATCH_MB, mb)
        try:
            assert check_set(engine, packed, raws, pats, tag="budget %d" % mb, refs=refs) == free
            assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in packed[0]), 0)
            assert engine.kernel_ms(_lib.T_SEARCH) > 0
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
    engine.verify(packed[0][:5], packed[1][:5], packed[2][:5])
    assert engine.kernel_ms(_lib.T_SEARCH) in (0.0, -1.0)                  # an unused timer after a call that does not search


# ---- 11. the device form -------------------------------------------------------------------------------------------------------------
def check_device_form(engine, corpus, compress=True):
    raws = [sc.plant(corpus.entry(4800 + i, n, i % 4), sc.NEEDLE7, [n // 3] if n > 30 else []) for i, n in enumerate((0, 1, 70000, 200000, 5, 7, 65536 + 7, 4096))]
    raws[5] = sc.NEEDLE7
    pats = [sc.NEEDLE7, b"The", sc.NEEDLE7[:3], raws[2][100:104]]
    frames, raw_lens, digests = packed = sc.pack(engine, raws, compress=compress)
    host = {}
    for icase in (False, True):
        host[icase] = check_set(engine, packed, raws, pats, icase=icase, tag="host form %r" % icase)
        h2d, d2h, ring, direct = vc.copy_counters(engine)
        assert (h2d, d2h) == (sum(len(f) for f in frames), 0) and ring + direct == h2d
        assert engine.kernel_ms(_lib.T_SEARCH) > 0 and engine.kernel_ms(_lib.T_TOTAL) >= engine.kernel_ms(_lib.T_SEARCH)
    d_frames, foff, _ = vc._arena(engine, frames)
    try:
        exp = np.frombuffer(b"".join(digests), dtype=np.uint8)
        for icase in (False, True):
            dev = engine.search_set_device(d_frames, foff, [len(f) for f in frames], raw_lens, pats, icase=icase, expect=exp)
            assert vc.copy_counters(engine) == (0, 0, 0, 0)
            assert engine.kernel_ms(_lib.T_SEARCH) > 0
            assert dev == host[icase]
        engine.verify_device(d_frames, foff, [len(f) for f in frames], raw_lens, exp)
        assert engine.kernel_ms(_lib.T_SEARCH) in (0.0, -1.0)
    finally:
        engine.free(d_frames)


# ---- 12. arguments -------------------------------------------------------------------------------------------------------------------
def raw_set(pats, count=None, null=(), lens=None):
    """a zarc_gpu_pattern_set over pats, bent as asked: count, members to pass as NULL, other lengths"""
    ps = _lib.PatternSet.of(pats)
    if lens is not None:
        for k, v in enumerate(lens): ps._len[k] = v
    if count is not None: ps.count = count
    for name in null: setattr(ps, name, None)
    return ps


def check_arguments(engine, corpus):
    lib, h = engine.lib, engine.h
    c = ctypes
    P, OK = _lib.E_PARAM, _lib.OK
    raw = sc.plant(corpus.entry(4900, 5000, 0), sc.NEEDLE7, [1234])
    frames, raw_lens, digests = packed = sc.pack(engine, [raw])
    ptrs, lens = vc._ptrs(frames)
    rl = (c.c_size_t * 1)(len(raw))
    dig = np.zeros((1, 32), dtype=np.uint8)
    pdig = dig.ctypes.data_as(c.c_void_p)
    st, cnt, fst, wch, hits, lines = (c.c_int * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1024)(), (c.c_uint64 * 1)()
    good = raw_set([sc.NEEDLE7, b"\xf0q"])
    many = [b"%04d" % k for k in range(1025)]
    bad_sets = [None, raw_set([b"x"], null=("bytes",)), raw_set([b"x"], null=("off",)), raw_set([b"x"], null=("len",)), raw_set([b"x"], count=0),
                raw_set(many), raw_set([b"x", b"yy"], lens=[1, 0]), raw_set([b"x", b"y" * 300], lens=[1, 257])]
    nl_sets = [raw_set([b"ab", b"a\nb"]), raw_set([b"\n"]), raw_set([b"x", b"y", b"zz\n"])]
    ref_of = lambda s: c.byref(s) if s is not None else None

    def host(n=1, ptrs=ptrs, lens=lens, rl=rl, s=good, flags=0, pdig=pdig, st=st, cnt=cnt, fst=fst, wch=wch, hits=hits):
        return lib.zarc_gpu_search_set_batch(h, n, ptrs, lens, rl, None, ref_of(s), flags, pdig, st, cnt, fst, wch, hits)
    assert host() == OK and (st[0], cnt[0], fst[0], wch[0], hits[0], hits[1]) == (0, 1, 1234, 0, 1, 0)
    assert [host(s=s) for s in bad_sets] == [P] * len(bad_sets)
    assert host(s=raw_set(many[:1024])) == OK and host(s=raw_set([b"y" * 256])) == OK and (cnt[0], fst[0], wch[0]) == (0, _lib.SEARCH_NONE, _lib.SEARCH_NONE)
    assert host(s=nl_sets[0]) == OK                                         # a 0x0A is refused by the lines form only
    assert host(flags=2) == host(flags=3) == host(flags=0x80000000) == P
    assert host(st=None) == host(cnt=None) == host(fst=None) == host(pdig=None) == host(wch=None) == P
    assert host(hits=None) == OK and (cnt[0], wch[0]) == (1, 0)
    assert host(ptrs=None) == host(lens=None) == host(rl=None) == P
    hits[0] = hits[1] = 77
    assert host(n=0, ptrs=None, lens=None, rl=None) == OK and (hits[0], hits[1]) == (0, 0)   # n == 0: hits zeroed ...
    assert host(n=0, s=bad_sets[4]) == host(n=0, s=None) == host(n=0, wch=None) == P           # ... and the set validated all the same
    big = (c.c_size_t * 1)(0xFFFFFFF0)
    assert host(rl=big) == host(lens=big) == _lib.E_UNSUPPORTED
    u64 = lambda v: (c.c_uint64 * 1)(v)
    dummy = c.c_void_p(16)  # never dereferenced: the call is refused before

    def dev(n=1, base=dummy, off=u64(0), fl=u64(9), rl=u64(0), s=good, flags=0, pdig=pdig, st=st, cnt=cnt, fst=fst, wch=wch, hits=hits):
        return lib.zarc_gpu_search_set_batch_device(h, n, base, off, fl, rl, None, ref_of(s), flags, pdig, st, cnt, fst, wch, hits)
    hits[0] = 77
    assert dev(n=0, base=None, off=None, fl=None, rl=None) == OK and hits[0] == 0
    assert dev(base=None) == dev(off=None) == dev(fl=None) == dev(rl=None) == P
    assert [dev(s=s) for s in bad_sets] == [P] * len(bad_sets) and dev(flags=4) == P
    assert dev(st=None) == dev(cnt=None) == dev(fst=None) == dev(pdig=None) == dev(wch=None) == P
    assert dev(rl=u64(0xFFFFFFF0)) == dev(fl=u64(1 << 32)) == _lib.E_UNSUPPORTED
    # the lines forms
    rec, ru, tu = (_lib.Line * 4)(), c.c_size_t(77), c.c_size_t(77)
    text = np.zeros(64, dtype=np.uint8)
    ptext = text.ctypes.data_as(c.c_void_p)

    def hl(n=1, ptrs=ptrs, lens=lens, rl=rl, s=good, flags=0, max_line=16, pdig=pdig, st=st, cnt=cnt, fst=fst, wch=wch, hits=hits, lines=lines, rec=rec, rec_cap=4,
           ru=c.byref(ru), text=ptext, text_cap=64, tu=c.byref(tu)):
        return lib.zarc_gpu_search_set_lines_batch(h, n, ptrs, lens, rl, None, ref_of(s), flags, 0, max_line, pdig, st, cnt, fst, wch, hits, lines, rec, rec_cap, ru,
                                                   text, text_cap, tu)

    def dl(n=1, base=dummy, off=u64(0), fl=u64(9), rl=u64(0), s=good, flags=0, max_line=16, pdig=pdig, st=st, cnt=cnt, fst=fst, wch=wch, hits=hits, lines=lines, rec=rec,
           rec_cap=4, ru=c.byref(ru), text=dummy, text_cap=64, tu=c.byref(tu)):
        return lib.zarc_gpu_search_set_lines_batch_device(h, n, base, off, fl, rl, None, ref_of(s), flags, 0, max_line, pdig, st, cnt, fst, wch, hits, lines, rec,
                                                          rec_cap, ru, text, text_cap, tu)
    want = lc.ref_lines(raw, sc.NEEDLE7)
    assert hl() == OK and (ru.value, tu.value, lines[0], cnt[0], wch[0]) == (1, min(want[0][1], 16), 1, 1, 0) and rec[0].match == 1234
    assert hl(rec_cap=0, rec=None, text=None) == OK and (ru.value, tu.value, lines[0]) == (0, 0, 1)
    for f in (hl, dl):
        assert [f(s=s) for s in bad_sets + nl_sets] == [P] * (len(bad_sets) + 3), f.__name__
        assert f(flags=2) == f(max_line=0) == f(max_line=65537) == P
        assert f(st=None) == f(cnt=None) == f(fst=None) == f(pdig=None) == f(wch=None) == f(lines=None) == f(ru=None) == f(tu=None) == f(rec=None) == f(text=None) == P
        assert f(text_cap=63) == _lib.E_DSTSIZE
        assert f(n=0, s=nl_sets[1]) == P
    assert hl(ptrs=None) == hl(lens=None) == hl(rl=None) == dl(base=None) == dl(off=None) == dl(fl=None) == dl(rl=None) == P
    ru.value = tu.value = hits[0] = 77
    assert hl(n=0, ptrs=None, lens=None, rl=None) == OK and (ru.value, tu.value, hits[0]) == (0, 0, 0)
    assert dl(n=0, base=None, off=None, fl=None, rl=None) == OK
    assert hl(rl=big) == hl(lens=big) == dl(rl=u64(0xFFFFFFF0)) == dl(fl=u64(1 << 32)) == _lib.E_UNSUPPORTED
    # ... and the handle still works
    assert host(flags=_lib.SEARCH_ICASE) == OK and (st[0], cnt[0], fst[0], wch[0], hits[0]) == (0, 1, 1234, 0, 1)
    assert engine.search_set(frames, raw_lens, [b"\xf0q", sc.NEEDLE7], expect=digests) == ([(0, digests[0], 1, 1234, 1)], [0, 1])
    assert engine.search(frames, raw_lens, sc.NEEDLE7, expect=digests) == [(0, digests[0], 1, 1234)]


# ---- 13. frames in pieces, other encoders' frames ------------------------------------------------------------------------------------
def check_pieces(engine, oracle, corpus, golden_frames):
    d, m = golden_frames
    raws, frames = [corpus.entry(4500, (4 << 20) + 17, 0)], []
    frames.append(sc.pack(engine, raws)[0][0])
    for name in ("text300", "records200k", "lz300k"):
        fr = next(f for f in m["frames"] if f["recipe"] == name and f["level"] == 3 and f["checksum"] == 1 and f["libzstd"].startswith("1.5"))
        frames.append(open(os.path.join(d, fr["file"]), "rb").read())
        raws.append(make_golden.recipe_bytes(m["recipes"][name], corpus))
    packed = (frames, [len(r) for r in raws], [oracle.blake3(r) for r in raws])
    pats = [r[len(r) // 2:len(r) // 2 + (9, 3, 6, 5)[i]] for i, r in enumerate(raws)]   # one needle from each
    res, hits = check_set(engine, packed, raws, pats, tag="pieces")
    assert all(r[2] >= 1 for r in res) and all(x >= 1 for x in hits)


# ---- 14. lines -----------------------------------------------------------------------------------------------------------------------
N2 = b"\xf3QZ\xf4"              # the second needle of the lines cases: not in the corpus text, no 0x0A


def check_set_lines(engine, packed, raws, pats, icase=False, max_lines=0, max_line=4096, rec_cap=None, tag="", call=None):
    """one search_set_lines call against the reference built from the union positions -> (results, records, hits)"""
    frames, raw_lens, digests = packed
    refs = [ref(r, pats, icase) for r in raws]
    want = [ref_lines(r, rf[4]) for r, rf in zip(raws, refs)]
    cap = sum(len(w) for w in want) + 1 if rec_cap is None else rec_cap
    call = call or (lambda **kw: engine.search_set_lines(frames, raw_lens, pats, expect=digests, **kw))
    results, records, hits = call(icase=icase, max_lines=max_lines, max_line=max_line, rec_cap=cap)
    assert len(results) == len(raws)
    for i, (st, dig, count, first, which, lines) in enumerate(results):
        assert st == _lib.FRAME_OK and dig == digests[i], (tag, i, st)
        assert (count, first, which) == refs[i][:3], (tag, i)
        assert lines == len(want[i]), (tag, i, lines, len(want[i]))
    assert hits == [sum(rf[3][k] for rf in refs) for k in range(len(pats))], tag
    exp = lc.deliver(raws, want, max_lines, max_line, cap)
    assert len(records) == len(exp), (tag, len(records), len(exp))
    for g, e in zip(records, exp):
        assert g == e, (tag, g[:5], e[:5])                                  # (rec.match: the lowest union position of the line)
    return results, records, hits


def lines_frames(corpus):
    """lines_cases.boundary_frames with a second needle among the first: lines that hold both, lines that hold one, and a match of each on
    either side of a slice boundary"""
    raws = lc.boundary_frames(corpus)
    raws[0] = sc.plant(raws[0], N2, [S - 60])           # the line starts in slice 0: N2 in front of the boundary, the first needle behind it
    raws[3] = sc.plant(raws[3], N2, [S + 10])           # both needles in the line behind the two 0x0A
    raws[4] = sc.plant(raws[4], N2, [S - 30, S - 5])    # N2 alone in the line that ends at S - 1 (its second copy ends right there); the first needle alone behind it
    raws[5] = sc.plant(raws[5], N2, [S + 1])            # the first needle ends at S - 1, 0x0A at S, N2 opens the next slice's first line
    raws[7] = sc.plant(raws[7], N2, [2 * S - 2])        # N2 alone, across a boundary
    return raws


def check_lines(engine, corpus, compress=True):
    raws = lines_frames(corpus)
    packed = sc.pack(engine, raws, compress=compress)
    _, recs, hits = check_set_lines(engine, packed, raws, [lc.NEEDLE, N2], tag="two needles")
    by = lambda i: [r[1:5] for r in recs if r[0] == i]
    assert len(by(0)) == 1 and by(0)[0][3] == S - 60                        # one line, its lowest match is the second needle's
    assert [r[3] for r in by(4)] == [S - 30, S] and [r[3] for r in by(5)] == [S - 7, S + 1]
    assert hits[1] == 6
    check_set_lines(engine, packed, raws, [N2, lc.NEEDLE, N2[:2]], tag="three, other order")
    one = engine.search_lines(packed[0], packed[1], lc.NEEDLE, expect=packed[2], rec_cap=64)
    res, recs, hits = engine.search_set_lines(packed[0], packed[1], [lc.NEEDLE], expect=packed[2], rec_cap=64)
    assert ([r[:4] + r[5:] for r in res], recs) == one and hits == [sum(r[2] for r in one[0])]   # a set of one pattern is search_lines
    # the device form
    d_frames, foff, _ = vc._arena(engine, packed[0])
    try:
        exp = np.frombuffer(b"".join(packed[2]), dtype=np.uint8)
        dev_call = lambda **kw: engine.search_set_lines_device(d_frames, foff, [len(f) for f in packed[0]], packed[1], [lc.NEEDLE, N2], expect=exp, **kw)
        for kw in ({}, {"max_lines": 1}, {"rec_cap": 3}, {"max_line": 17}):
            dev = check_set_lines(engine, packed, raws, [lc.NEEDLE, N2], tag="device form %r" % kw, call=dev_call, **kw)
            assert vc.copy_counters(engine) == (0, 0, 0, 0) and engine.kernel_ms(_lib.T_LINES) > 0
            assert dev == check_set_lines(engine, packed, raws, [lc.NEEDLE, N2], tag="host form %r" % kw, **kw)
            h2d, d2h, _, _ = vc.copy_counters(engine)
            assert (h2d, d2h) == (sum(len(f) for f in packed[0]), sum(len(r[5]) for r in dev[1]))
    finally:
        engine.free(d_frames)


def check_lines_caps(engine, corpus, compress=True):
    """lines_cases.check_caps with a set: the caps count lines of the union"""
    big = b"".join(b"line %d %s\n" % (k, lc.NEEDLE if k % 3 else N2) for k in range(1000))
    small = [sc.plant(corpus.entry(5400 + i, 3000, 0), (lc.NEEDLE, N2)[i % 2], [100 + 900 * k for k in range(i)]) for i in range(4)]
    raws = [small[1], big, small[0], small[3], b"", small[2]]
    packed = sc.pack(engine, raws, compress=compress)
    pats = [lc.NEEDLE, N2]
    full = [len(ref_lines(r, ref(r, pats)[4])) for r in raws]
    assert full[1] == 1000
    for max_lines in (0, 1, 7):
        total = sum(min(n, max_lines or n) for n in full)
        for rec_cap in (0, 1, total, total - 1):
            res, recs, _ = check_set_lines(engine, packed, raws, pats, max_lines=max_lines, rec_cap=rec_cap, tag="caps %d %d" % (max_lines, rec_cap))
            assert [r[5] for r in res] == full and len(recs) == min(total, rec_cap)
    long_line = corpus.entry(5450, 70000, 0).replace(b"\n", b" ")
    Q, Q2 = b"\xf7", b"\xf8\xf9"
    raws2 = [b"\n".join([b"", Q, Q2 + b"x" * 14, b"y" * 16 + Q, long_line[:100] + Q2 + long_line[102:], b""])]
    packed2 = sc.pack(engine, raws2, compress=compress)
    for max_line in (1, 16, 17, 65536):
        _, recs, _ = check_set_lines(engine, packed2, raws2, [Q, Q2], max_line=max_line, rec_cap=5, tag="max_line %d" % max_line)
        assert [(r[2], len(r[5])) for r in recs] == [(n, min(n, max_line)) for n in (1, 16, 17, 70000)]
    # text_cap below rec_cap * max_line: E_DSTSIZE, as for the one-pattern call (check_arguments has the one-byte-short case of both forms)
    c = ctypes
    ps = _lib.PatternSet.of([Q, Q2])
    ptrs, lens = vc._ptrs(packed2[0])
    out = [(c.c_uint64 * 1)() for _ in range(5)]
    dig, st, rec, ru, tu = np.zeros((1, 32), dtype=np.uint8), (c.c_int * 1)(), (_lib.Line * 64)(), c.c_size_t(), c.c_size_t()
    text = np.zeros(64 * 16, dtype=np.uint8)
    for rec_cap, max_line, text_cap, rc in ((5, 16, 79, _lib.E_DSTSIZE), (1, 1, 0, _lib.E_DSTSIZE), (2 ** 62, 65536, (2 ** 62 * 65536 - 1) % 2 ** 64, _lib.E_DSTSIZE),
                                            (4, 16, 64, _lib.OK)):
        assert engine.lib.zarc_gpu_search_set_lines_batch(engine.h, 1, ptrs, lens, (c.c_size_t * 1)(len(raws2[0])), None, c.byref(ps), 0, 0, max_line,
                                                          dig.ctypes.data_as(c.c_void_p), st, out[0], out[1], out[2], out[3], out[4], rec, rec_cap, c.byref(ru),
                                                          text.ctypes.data_as(c.c_void_p), text_cap, c.byref(tu)) == rc, (rec_cap, max_line)
    assert ru.value == 4 and out[4][0] == 4


# ---- 17. real data (GPU) -------------------------------------------------------------------------------------------------------------
def check_real_items(engine, real_items):
    """16 needles of 4 .. 12 bytes cut from the items' middles, all items in one batch"""
    raws = list(real_items.values())
    pats = [raws[k % len(raws)][len(raws[k % len(raws)]) // 2 + 97 * (k // len(raws)):][:4 + k % 9] for k in range(16)]
    assert all(4 <= len(p) <= 12 for p in pats)
    res, hits = check_set(engine, sc.pack(engine, raws), raws, pats, tag="real items")
    assert all(h >= 1 for h in hits) and sum(r[2] >= 1 for r in res) >= min(len(raws), 16)
