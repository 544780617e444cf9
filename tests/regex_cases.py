"""Checks of zarc_gpu_search_regex_* (regular expressions matched on the device), shared by the emulator tests (test_regex.py), the GPU tests
(test_gpu_regex.py) and the compiler's tests (test_regex_compile.py).

The reference for every expected value is Python's `re` on the CPU, over the bytes the frames were packed from -- never the engine.  Matching
is per line: per line of a frame the reference is
    {m.start() for m in re.finditer(b"(?=(?:" + R + b"))", line, flags)}            (flags = re.I for the case-folding search)
shifted by the line's offset.  Whether a match exists at a position does not depend on leftmost-longest or backtracking order, so `re`, POSIX
and the engine agree on it.  The sorted positions give count and first, the lowest position inside a line gives the line's record
(set_cases.ref_lines), lines_cases.deliver applies the delivery rule.  Every comparison is equality."""
import ctypes
import random
import re

import numpy as np

import lines_cases as lc
import search_cases as sc
import set_cases as zs
import verify_cases as vc
from zarc_amd import _lib

S = sc.SLICE
LEN1 = 3 * S + 1000            # the largest frame of these cases
DECODED = (_lib.FRAME_OK, _lib.FRAME_DIGEST)
MAX_LITERAL = 62               # a literal of m bytes needs m + 1 states; the issue draws the line at 62


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def positions(d, rx, icase=False):
    """the sorted matching start positions of the expression in one frame's bytes"""
    prog = re.compile(b"(?=(?:" + rx + b"))", re.I if icase else 0)
    out, pos = [], 0
    for line in d.split(b"\n"):
        out += [pos + m.start() for m in prog.finditer(line)]
        pos += len(line) + 1
    return out


def ref(d, rx, icase=False):
    p = positions(d, rx, icase)
    return len(p), (p[0] if p else None)


def check_regex(engine, packed, raws, rx, icase=False, tag="", call=None, refs=None):
    """one search_regex call over a packed batch of good frames against the reference -> [(count, first)]"""
    frames, raw_lens, digests = packed
    call = call or (lambda: engine.search_regex(frames, raw_lens, rx, icase=icase, expect=digests))
    got = call()
    assert len(got) == len(raws)
    for i, (st, dig, count, first) in enumerate(got):
        assert st == _lib.FRAME_OK and dig == digests[i], (tag, rx, i, st)
        want = refs[i] if refs else ref(raws[i], rx, icase)
        assert (count, first) == want, (tag, rx, icase, i, len(raws[i]), (count, first), want)
    return [(g[2], g[3]) for g in got]


def check_regex_lines(engine, packed, raws, rx, icase=False, max_lines=0, max_line=4096, rec_cap=None, tag="", call=None):
    """one search_regex_lines call against the reference -> (results, records)"""
    frames, raw_lens, digests = packed
    pos = [positions(r, rx, icase) for r in raws]
    want = [zs.ref_lines(r, p) for r, p in zip(raws, pos)]
    cap = sum(len(w) for w in want) + 1 if rec_cap is None else rec_cap
    call = call or (lambda **kw: engine.search_regex_lines(frames, raw_lens, rx, expect=digests, **kw))
    results, records = call(icase=icase, max_lines=max_lines, max_line=max_line, rec_cap=cap)
    assert len(results) == len(raws)
    for i, (st, dig, count, first, lines) in enumerate(results):
        assert st == _lib.FRAME_OK and dig == digests[i], (tag, rx, i, st)
        assert (count, first) == (len(pos[i]), pos[i][0] if pos[i] else None), (tag, rx, i, (count, first))
        assert lines == len(want[i]), (tag, rx, i, lines, len(want[i]))
    exp = lc.deliver(raws, want, max_lines, max_line, cap)
    assert len(records) == len(exp), (tag, rx, len(records), len(exp))
    for g, e in zip(records, exp):
        assert g == e, (tag, rx, g[:5], e[:5])
    return results, records


def check_both(engine, packed, raws, rx, icase=False, tag=""):
    got = check_regex(engine, packed, raws, rx, icase, tag)
    res, recs = check_regex_lines(engine, packed, raws, rx, icase, tag=tag + ", lines")
    assert [(r[2], r[3]) for r in res] == got
    return got, recs


def refused(call, code, *needles):
    try:
        call()
    except _lib.ZarcGpuError as e:
        assert e.code == code, (e.code, code, str(e))
        for s in needles: assert s in str(e), (s, str(e))
        return str(e)
    assert False, "not refused: %r" % (needles,)


def noise(seed, n, alphabet=b"deghijklmnpq  ", line=48):
    """n bytes over `alphabet` with a 0x0A every `line` bytes on average (0: none)"""
    rnd = random.Random(seed)
    b = bytearray(rnd.choice(alphabet) for _ in range(n))
    if line:
        k = rnd.randrange(1, 2 * line)
        while k < n:
            b[k] = 0x0A
            k += rnd.randrange(1, 2 * line)
    return bytes(b)


def blank(raw, lo, hi, fill=0x20):
    """no 0x0A in [lo, hi)"""
    return raw[:lo] + raw[lo:hi].replace(b"\n", bytes([fill])) + raw[hi:]


# ---- 1. a literal is the fixed-string search -----------------------------------------------------------------------------------------
def check_literal(engine, corpus, compress=True):
    raws = zs.one_pattern_frames(corpus)
    frames, raw_lens, digests = sc.pack(engine, raws, compress=compress)
    seen = 0
    for p in [sc.needle_of(m) for m in sc.NEEDLE_LENS] + [sc.NEEDLE7]:
        assert b"\n" not in p
        rx = re.escape(p)
        for icase in (False, True):
            if len(p) > MAX_LITERAL:                                        # exactly this split: longer literals need more than 64 states
                refused(lambda: engine.search_regex(frames, raw_lens, rx, icase=icase, expect=digests), _lib.E_UNSUPPORTED, "states")
                refused(lambda: engine.search_regex_lines(frames, raw_lens, rx, icase=icase, expect=digests), _lib.E_UNSUPPORTED, "states")
                continue
            one = engine.search(frames, raw_lens, p, icase=icase, expect=digests)
            assert engine.search_regex(frames, raw_lens, rx, icase=icase, expect=digests) == one, (len(p), icase)
            if not icase or p == sc.NEEDLE7:                                # (the folded lines form: once, with the needle that holds letters)
                assert engine.search_regex_lines(frames, raw_lens, rx, icase=icase, expect=digests, rec_cap=256) == \
                    engine.search_lines(frames, raw_lens, p, icase=icase, expect=digests, rec_cap=256), (len(p), icase)
            seen += sum(r[2] for r in one)
    assert seen > 60
    folded = sc.plant(corpus.entry(4300, 70000, 0), b"hello WORLD", [5, S - 4]) + b"HELLO world"
    fr = sc.pack(engine, [folded], compress=compress)
    assert engine.search_regex(fr[0], fr[1], b"Hello World", icase=True, expect=fr[2]) == engine.search(fr[0], fr[1], b"Hello World", icase=True, expect=fr[2])
    assert engine.search_regex(fr[0], fr[1], b"Hello World", icase=True, expect=fr[2])[0][2:] == (3, 5)


# ---- 2. state across chunk and slice boundaries --------------------------------------------------------------------------------------
BOUNDARY_RX = (b"foo.*bar", b"a[^x]*z", b"ab+c")


def boundary_frames():
    """the alphabet of the noise holds none of a b c f o r x z: every match is planted"""
    out = []
    # 0: heads in slice 0, tails in slice 1, one line across the boundary
    f = blank(blank(noise(1, LEN1), S - 400, S + 400), 2 * S - 400, 2 * S + 400)
    f = sc.plant(f, b"foo", [S - 100]); f = sc.plant(f, b"bar", [S + 50])
    f = sc.plant(f, b"a", [S - 300]); f = sc.plant(f, b"z", [S + 200]); f = sc.plant(f, b"a" + b"b" * 300 + b"c", [2 * S - 150])
    out.append(f)
    # 1: heads in slice 0, tails in slice 2, slice 1 without any 0x0A (its table is used)
    f = blank(noise(2, LEN1), S - 300, 2 * S + 300)
    f = sc.plant(f, b"foo", [S - 120]); f = sc.plant(f, b"bar", [2 * S + 100]); f = sc.plant(f, b"a", [S - 50, S + 7]); f = sc.plant(f, b"z", [2 * S + 30])
    f = sc.plant(f, b"abc", [2 * S - 2, 2 * S + 5]); f = sc.plant(f, b"x", [2 * S + 200]); f = sc.plant(f, b"a", [2 * S + 150])
    out.append(f)
    # 2: no 0x0A at all
    f = noise(3, LEN1, line=0)
    f = sc.plant(f, b"foo", [10, 70000]); f = sc.plant(f, b"bar", [LEN1 - 100]); f = sc.plant(f, b"a", [5]); f = sc.plant(f, b"z", [LEN1 - 1])
    f = sc.plant(f, b"abbc", [254, 255, 256 * 9 - 1, S - 2, 2 * S - 1][::2]); f = sc.plant(f, b"x", [3 * S])
    out.append(f)
    # 3: a 0x0A at S - 1, a match start at S; 4: a 0x0A at S, a match that ends in front of it, one that starts behind it, a head it cuts off
    f = blank(noise(4, LEN1), S - 40, S + 40)
    out.append(sc.plant(sc.plant(f, b"\n", [S - 1]), b"abc foo bar az", [S]))
    out.append(sc.plant(sc.plant(sc.plant(f, b"\n", [S]), b"abbc", [S - 4, S + 1]), b"ab", [S - 8]))
    # 5: a match start at S - 1 in a line that goes on behind S
    out.append(sc.plant(sc.plant(f, b"abbbc", [S - 1]), b"foo bar", [S - 20]))
    # 6: match starts at positions 255, 256 and 257 of a chunk
    f = noise(5, 40000)
    out.append(sc.plant(f, b"abc", [10 * 256 + 255, 20 * 256 + 256, 30 * 256 + 257]))
    # 7: lines of 0, 1, 255, 256 and 257 bytes, matching and not
    lines = []
    fit = lambda head, fill, tail, n: (head + fill * max(n - len(head) - len(tail), 0) + tail)[:n]
    for n in (0, 1, 255, 256, 257):
        lines += [b"z" * n, fit(b"a", b"g", b"z", n), fit(b"ab", b"b", b"c", n), fit(b"foo", b"h", b"bar", n)]
    out.append(b"\n".join(lines * 3))
    # 8 ..: exactly S, S + 1, 1 and 0 bytes; a frame of one slice among the others
    f = sc.plant(blank(noise(6, S + 1), S - 30, S + 1), b"abbc", [S - 4])
    out += [f[:S], sc.plant(f, b"c", [S]), b"a", b"", sc.plant(noise(7, 3000), b"foo then bar az abc", [1000])]
    return out


def check_boundaries(engine, compress=True):
    raws = boundary_frames()
    packed = sc.pack(engine, raws, compress=compress)
    for rx in BOUNDARY_RX:
        got, recs = check_both(engine, packed, raws, rx, tag="boundaries")
        assert sum(c for c, _ in got) >= 8, (rx, got)
    got = check_regex(engine, packed, raws, b"foo.*bar", tag="boundaries")
    assert got[0] == (1, S - 100) and got[1] == (1, S - 120) and got[2] == (2, 10)      # the tails lie one and two slices behind the heads
    got = check_regex(engine, packed, raws, b"ab+c", tag="boundaries")
    assert got[3][1] == S and got[5][1] == S - 1 and got[4] == (2, S - 4) and got[6] == (3, 10 * 256 + 255) and got[8] == (1, S - 4)


# ---- 3. anchors ----------------------------------------------------------------------------------------------------------------------
ANCHOR_RX = (b"^x", b"x$", b"^x$", b"^(a|b)+$", b"x$|^y", b"^^x$$", b"(^|g)x", b"x($|g)")


def anchor_frames():
    f = blank(noise(8, 2 * S + 500), S - 40, S + 40)
    f = sc.plant(f, b"\nx\n", [S - 1])                                      # behind a 0x0A that is a slice's last byte
    f = sc.plant(f, b"\nabab\n", [2 * S - 3])                               # a line of a and b across a boundary
    g = sc.plant(blank(noise(9, S + 300), S - 40, S + 40), b"\ny", [S - 1])
    return [b"x", b"x\n", b"\nx", b"x\r\n", b"y", b"xx\n\nx\ny\nab\nabc\nba\n\nyx\nxy", b"x\n\nx", b"ax\nxa\nx", f, g, f[:S] + b"x", f[:S - 1] + b"\nx\n",
            b"gx\nxg\nhx"]


def check_anchors(engine, compress=True):
    raws = anchor_frames()
    packed = sc.pack(engine, raws, compress=compress)
    for rx in ANCHOR_RX:
        check_both(engine, packed, raws, rx, tag="anchors")
    got = check_regex(engine, packed, raws, b"^x$", tag="anchors")
    assert got[:5] == [(1, 0), (1, 0), (1, 1), (0, None), (0, None)] and got[8] == (1, S) and got[6] == (2, 0)
    assert check_regex(engine, packed, raws, b"x$|^y", tag="anchors")[9] == (1, S)


# ---- 4. classes ----------------------------------------------------------------------------------------------------------------------
def check_classes(engine, compress=True):
    every = bytes(range(256))
    raws = [every * 3, b"b\nb\n\nbb", b"-\n-\n--", b"7\n7", every + b"Hello hELLO AX bx Cx dx ax\n@[ `{ `[ @{ @{\nab]c-x\\d a-z 1.5 \t\x41\n" + every[::-1]]
    packed = sc.pack(engine, raws, compress=compress)
    got = check_regex(engine, packed, raws, b".", tag="dot")
    assert got[0] == (3 * 255, 0)                                           # 0x00, 0x0D, 0x80 .. 0xFF, and never 0x0A
    for rx in (b"..", b"[^a][^a]", b"\\S\\S", b"\\D\\D", b"\\W\\W", b"[^a]", b"\\s", b"\\d+", b"\\w+\\W"):
        check_both(engine, packed, raws, rx, tag="classes")
    assert check_regex(engine, packed, raws, b"[^a][^a]", tag="classes")[1] == (1, 5)   # only the line feed separates the pieces
    assert [c for c, _ in check_regex(engine, packed, raws, b"\\W\\W", tag="classes")[2:3]] == [1]
    for rx in (b"[a-c]+", b"[\\x80-\\xff]", b"\\x41", b"[\\]\\-x]", b"[]a]", b"[^]a]b", b"[a\\-z]", b"[\\d.]+", b"\\.", b"\\t", b"[\\x00-\\x20]", b"\\0", b"[b-]x", b"[\\Wa]b"):
        check_regex(engine, packed, raws, rx, tag="classes")
    for rx in (b"hello", b"[a-c]x", b"[^a-c]x", b"@\\[", b"`\\{", b"[@`][\\[{]", b"H[D-F]L+O"):
        for icase in (False, True):
            check_regex(engine, packed, raws, rx, icase=icase, tag="icase")
    assert check_regex(engine, packed, raws, b"hello", icase=True)[4][0] == 2 and check_regex(engine, packed, raws, b"[a-c]x", icase=True)[4][0] == 4
    assert check_regex(engine, packed, raws, b"@\\[", icase=True)[4][0] == 1 and check_regex(engine, packed, raws, b"`\\{", icase=True)[4][0] == 1


# ---- 5. quantifiers and structure ----------------------------------------------------------------------------------------------------
def check_quantifiers(engine, compress=True):
    raws = [noise(20 + k, 5000 + 777 * k, alphabet=b"aabbcde", line=(9, 40, 300)[k % 3]) for k in range(5)] + [b"aaaa", b"aab", b"ababcde cdcde e abe", b"abcd"]
    packed = sc.pack(engine, raws, compress=compress)
    for rx in (b"a{3}", b"a{2,}", b"a{1,3}b", b"(ab|cd)+e", b"((a|b)c)+d", b"(a(b(c|d))?)+e", b"(a|ab)(c|bcd)", b"a{0}b", b"(ab){2,3}c", b"a?b?c", b"(a|b|c){4}d", b"ab|abc|abcd"):
        check_both(engine, packed, raws, rx, tag="quantifiers")
    assert check_regex(engine, packed, raws, b"(a|ab)(c|bcd)")[8] == (1, 0)            # two ways to match at one position: it counts once
    assert check_regex(engine, packed, raws, b"a{3}")[5] == (2, 0) and check_regex(engine, packed, raws, b"a{1,3}b")[6] == (2, 0)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
BAD = (  # (expression, the offset its message names)
    (b"(ab", 0), (b"ab)", 2), (b"a[bc", 1), (b"*a", 0), (b"a|+b", 2), (b"a**", 2), (b"a{2}{3}", 4), (b"ab{", 2), (b"ab{x}", 2), (b"a{3,2}", 1), (b"a{,2}", 1),
    (b"a{256}", 1), (b"[b-a]", 1), (b"", 0), (b"a" * 1025, 1024), (b"a\\b", 1), (b"(a)\\1", 3), (b"\\Aa", 0), (b"a\\z", 1), (b"a*?", 2), (b"a+?", 2), (b"a??", 2),
    (b"a{2}?", 4), (b"a++", 2), (b"a\nb", 1), (b"a\\nb", 1), (b"[a\n]", 2), (b"a*", 0), (b"x|", 0), (b"()", 0), (b"^$", 0), (b"(a|)", 0), (b"^*a", 1), (b"a\\", 1),
    (b"(?:a)", 1), (b"\\x4", 0),
)


def check_refusals(engine, corpus):
    raw = sc.plant(corpus.entry(4900, 5000, 0), sc.NEEDLE7, [1234])
    frames, raw_lens, digests = sc.pack(engine, [raw])
    for rx, at in BAD:
        for call in (lambda: engine.search_regex(frames, raw_lens, rx, expect=digests), lambda: engine.search_regex_lines(frames, raw_lens, rx, expect=digests),
                     lambda: engine.search_regex([], [], rx), lambda: engine.regex_compile(rx)):   # n == 0: the expression is validated all the same
            refused(call, _lib.E_PARAM, "offset %d:" % at)
    assert engine.regex_compile(b".{4}a")[0] == 32
    for call in (lambda: engine.regex_compile(b".{7}a"), lambda: engine.search_regex(frames, raw_lens, b".{7}a", expect=digests), lambda: engine.search_regex([], [], b".{7}a")):
        refused(call, _lib.E_UNSUPPORTED, "256 states")
    refused(lambda: engine.regex_compile(b".{12}a"), _lib.E_UNSUPPORTED, "more than 4096 states")
    assert engine.search_regex([], [], b"ab+c") == [] and engine.search_regex_lines([], [], b"ab+c") == ([], [])
    # missing arrays and unknown flag bits, as zarc_gpu_search_batch refuses them
    lib, h, c = engine.lib, engine.h, ctypes
    P, OK = _lib.E_PARAM, _lib.OK
    ptrs, lens = vc._ptrs(frames)
    rl = (c.c_size_t * 1)(len(raw))
    dig = np.zeros((1, 32), dtype=np.uint8)
    pdig = dig.ctypes.data_as(c.c_void_p)
    st, cnt, fst, lines = (c.c_int * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)()
    rx = c.cast(c.c_char_p(re.escape(sc.NEEDLE7)), c.c_void_p)
    m = len(re.escape(sc.NEEDLE7))

    def host(n=1, ptrs=ptrs, lens=lens, rl=rl, rx=rx, m=m, flags=0, pdig=pdig, st=st, cnt=cnt, fst=fst):
        return lib.zarc_gpu_search_regex_batch(h, n, ptrs, lens, rl, None, rx, m, flags, pdig, st, cnt, fst)
    assert host() == OK and (st[0], cnt[0], fst[0]) == (0, 1, 1234)
    assert host(flags=2) == host(flags=3) == host(flags=0x80000000) == host(rx=None) == host(m=0) == P
    assert host(st=None) == host(cnt=None) == host(fst=None) == host(pdig=None) == host(ptrs=None) == host(lens=None) == host(rl=None) == P
    assert host(n=0, ptrs=None, lens=None, rl=None) == OK and host(n=0, st=None) == P
    big = (c.c_size_t * 1)(0xFFFFFFF0)
    assert host(rl=big) == host(lens=big) == _lib.E_UNSUPPORTED
    u64 = lambda v: (c.c_uint64 * 1)(v)
    dummy = c.c_void_p(16)  # never dereferenced: the call is refused before

    def dev(n=1, base=dummy, off=u64(0), fl=u64(9), rl=u64(0), rx=rx, m=m, flags=0, pdig=pdig, st=st, cnt=cnt, fst=fst):
        return lib.zarc_gpu_search_regex_batch_device(h, n, base, off, fl, rl, None, rx, m, flags, pdig, st, cnt, fst)
    assert dev(n=0, base=None, off=None, fl=None, rl=None) == OK
    assert dev(base=None) == dev(off=None) == dev(fl=None) == dev(rl=None) == dev(flags=4) == dev(rx=None) == P
    assert dev(st=None) == dev(cnt=None) == dev(fst=None) == dev(pdig=None) == P
    assert dev(rl=u64(0xFFFFFFF0)) == dev(fl=u64(1 << 32)) == _lib.E_UNSUPPORTED
    rec, ru, tu = (_lib.Line * 4)(), c.c_size_t(77), c.c_size_t(77)
    text = np.zeros(64, dtype=np.uint8)
    ptext = text.ctypes.data_as(c.c_void_p)

    def hl(n=1, ptrs=ptrs, lens=lens, rl=rl, rx=rx, m=m, flags=0, max_line=16, pdig=pdig, st=st, cnt=cnt, fst=fst, lines=lines, rec=rec, rec_cap=4, ru=c.byref(ru), text=ptext,
           text_cap=64, tu=c.byref(tu)):
        return lib.zarc_gpu_search_regex_lines_batch(h, n, ptrs, lens, rl, None, rx, m, flags, 0, max_line, pdig, st, cnt, fst, lines, rec, rec_cap, ru, text, text_cap, tu)

    def dl(n=1, base=dummy, off=u64(0), fl=u64(9), rl=u64(0), rx=rx, m=m, flags=0, max_line=16, pdig=pdig, st=st, cnt=cnt, fst=fst, lines=lines, rec=rec, rec_cap=4,
           ru=c.byref(ru), text=dummy, text_cap=64, tu=c.byref(tu)):
        return lib.zarc_gpu_search_regex_lines_batch_device(h, n, base, off, fl, rl, None, rx, m, flags, 0, max_line, pdig, st, cnt, fst, lines, rec, rec_cap, ru, text,
                                                            text_cap, tu)
    assert hl() == OK and (ru.value, lines[0], cnt[0]) == (1, 1, 1) and rec[0].match == 1234
    assert hl(rec_cap=0, rec=None, text=None) == OK and (ru.value, tu.value, lines[0]) == (0, 0, 1)
    for f in (hl, dl):
        assert f(flags=2) == f(max_line=0) == f(max_line=65537) == f(rx=None) == f(m=0) == P, f.__name__
        assert f(st=None) == f(cnt=None) == f(fst=None) == f(pdig=None) == f(lines=None) == f(ru=None) == f(tu=None) == f(rec=None) == f(text=None) == P
        assert f(text_cap=63) == _lib.E_DSTSIZE
    assert hl(ptrs=None) == hl(lens=None) == hl(rl=None) == dl(base=None) == dl(off=None) == dl(fl=None) == dl(rl=None) == P
    ru.value = tu.value = 77
    assert hl(n=0, ptrs=None, lens=None, rl=None) == OK and (ru.value, tu.value) == (0, 0)
    assert dl(n=0, base=None, off=None, fl=None, rl=None) == OK
    assert hl(rl=big) == hl(lens=big) == dl(rl=u64(0xFFFFFFF0)) == dl(fl=u64(1 << 32)) == _lib.E_UNSUPPORTED
    # ... and the handle still works
    assert engine.search_regex(frames, raw_lens, re.escape(sc.NEEDLE7), expect=digests) == [(0, digests[0], 1, 1234)]
    assert engine.search(frames, raw_lens, sc.NEEDLE7, expect=digests) == [(0, digests[0], 1, 1234)]


# ---- 7. random differential ----------------------------------------------------------------------------------------------------------
SEED, RANDOM_COUNT, MAX_POSITIONS = 20261018, 320, 5
_random = {}


def _gen(rnd, budget, state, top=False):
    """-> (text, positions after counted repetitions are expanded, can match empty with anchors counted as empty).  state["wide"]: an
    unbounded repetition of more than one distinct byte has been used -- at most one per expression, so that the reference's backtracking
    stays polynomial on long lines."""
    kind = rnd.random()
    if budget <= 1 or kind < 0.30:
        k = rnd.random()
        if k < 0.12: return rnd.choice((b"^", b"$")), 1, True
        atom = rnd.choice((b"a", b"b", b"c", b"a", b"b", b".", b"[ab]", b"[^a]", b"[a-c]", b"\\."))
        return atom, 1, False
    if kind < 0.55:                                                          # concatenation
        left = rnd.randrange(1, budget)
        a, b = _gen(rnd, left, state), _gen(rnd, budget - left, state)
        return a[0] + b[0], a[1] + b[1], a[2] and b[2]
    if kind < 0.72:                                                          # alternation (in a group unless at the top)
        left = rnd.randrange(1, budget)
        a, b = _gen(rnd, left, state), _gen(rnd, budget - left, state)
        text = a[0] + b"|" + b[0]
        return (text if top else b"(" + text + b")"), a[1] + b[1], a[2] or b[2]
    q = rnd.choice((b"*", b"+", b"?", b"{2}", b"{1,2}", b"{0,3}", b"{2,}", b"{1,}", b"{3}"))
    unbounded = q in (b"*", b"+", b"{2,}", b"{1,}")
    copies = {b"*": 1, b"+": 1, b"?": 1, b"{2}": 2, b"{1,2}": 2, b"{0,3}": 3, b"{2,}": 2, b"{1,}": 1, b"{3}": 3}[q]
    if budget // copies < 1 or (unbounded and state["bounded"]): return _gen(rnd, 1, state)
    if unbounded:                                                            # its body: one literal, or once per expression anything without a repetition of its own
        if state["wide"] or rnd.random() < 0.5:
            atom = rnd.choice((b"a", b"b", b"c"))
            return atom + q, copies, q in (b"*",)
        state["wide"] = True
        body = rnd.choice((b".", b"[ab]", b"[^a]", b"(ab)", b"(a|b)", b"(ab|c)", b"(a.)"))
        n = {b".": 1, b"[ab]": 1, b"[^a]": 1, b"(ab)": 2, b"(a|b)": 2, b"(ab|c)": 3, b"(a.)": 2}[body]
        if n * copies > budget: body, n = b".", 1
        return body + q, n * copies, q == b"*"
    state["bounded"] += copies > 1                                           # (no unbounded repetition inside a counted one: the reference would take n^copies steps)
    inner = _gen(rnd, budget // copies, state)
    state["bounded"] -= copies > 1
    low = {b"?": 0, b"{2}": 2, b"{1,2}": 1, b"{0,3}": 0, b"{3}": 3}[q]
    return b"(" + inner[0] + b")" + q, inner[1] * copies, low == 0 or inner[2]


def random_cases():
    """-> (expressions, frames, per expression the reference of every frame); generated once, shared by the compiler's and the engine's tests"""
    if not _random:
        rnd = random.Random(SEED)
        exprs = []
        while len(exprs) < RANDOM_COUNT:
            text, npos, empty = _gen(rnd, rnd.randrange(1, MAX_POSITIONS + 1), {"wide": False, "bounded": 0}, top=True)
            if empty or npos > MAX_POSITIONS or text in exprs: continue      # (regenerated, not counted)
            exprs.append(text)
        frames = [noise(SEED + 1, 3000, alphabet=b"abc", line=6), noise(SEED + 2, 5000, alphabet=b"aabc", line=40), noise(SEED + 3, 4000, alphabet=b"abbc", line=400),
                  b"\n".join(noise(SEED + 4 + k, n, alphabet=b"abc", line=0) for k, n in enumerate((0, 1, 2, 700, 3, 255, 256, 257, 0, 0, 5))), b"abc", b"\n\n", b""]
        _random["v"] = (exprs, frames, [[ref(f, e) for f in frames] for e in exprs])
    return _random["v"]


def walk_table(table, d):
    """the table zarc_gpu_regex_compile made, walked over one frame's bytes as the kernels walk it: from the last byte to the first"""
    states, start, accept, delta = table
    out, q = [], start
    for p in range(len(d) - 1, -1, -1):
        q = delta[q * 256 + d[p]]
        if accept[q] & 1 or (accept[q] & 2 and (p == 0 or d[p - 1] == 0x0A)): out.append(p)
    out.reverse()
    return out


def check_random_tables(compile_fn):
    exprs, frames, refs = random_cases()
    most = 0
    for e, want in zip(exprs, refs):
        try:
            table = compile_fn(e)
        except _lib.ZarcGpuError as err:
            assert False, "seed %d: %r was refused: %s" % (SEED, e, err)
        assert 1 <= table[0] <= 2 ** MAX_POSITIONS and table[1] < table[0] and accept_ok(table), (SEED, e, table[0])
        most = max(most, table[0])
        for f, w in zip(frames, want):
            p = walk_table(table, f)
            assert (len(p), p[0] if p else None) == w, "seed %d: %r on a frame of %d bytes: table %r, re %r" % (SEED, e, len(f), (len(p), p[:3]), w)
    assert most >= 8


def accept_ok(table):
    states, start, accept, delta = table
    return accept[start] == 0 and all(delta[q * 256 + 0x0A] == start for q in range(states)) and max(delta) < states


def check_random(engine, compress=True):
    exprs, frames, refs = random_cases()
    packed = sc.pack(engine, frames, compress=compress)
    for k, (e, want) in enumerate(zip(exprs, refs)):
        try:
            if k % 4:
                check_regex(engine, packed, frames, e, tag="seed %d" % SEED, refs=want)
            else:
                check_regex_lines(engine, packed, frames, e, tag="seed %d" % SEED)
        except _lib.ZarcGpuError as err:
            assert False, "seed %d: %r was refused: %s" % (SEED, e, err)


# ---- 8. the surrounding contract -----------------------------------------------------------------------------------------------------
def check_verdicts(engine, oracle, corpus, golden_frames):
    frames, raw_lens, expect, raws = vc.error_list(oracle, corpus, golden_frames)
    good = [sc.plant(corpus.entry(4600 + i, 30000 + i, 0), b"zq77 then 12 ms", [77, 20000]) for i in range(2)]
    gf, gl, gd = sc.pack(engine, good)
    frames, raw_lens, expect, raws = [gf[0]] + frames + [gf[1]], [gl[0]] + raw_lens + [gl[1]], [gd[0]] + expect + [gd[1]], [good[0]] + raws + [good[1]]
    rx = b"[a-z]+[0-9]+ .*[0-9] ms|^[A-Za-z]+ "
    for exp in (expect, None):
        want = engine.verify(frames, raw_lens, exp)
        got = engine.search_regex(frames, raw_lens, rx, expect=exp)
        res, recs = engine.search_regex_lines(frames, raw_lens, rx, expect=exp, rec_cap=20000)
        assert [(dig, st) for st, dig, _, _ in got] == want and [r[:4] for r in res] == got
        st = [g[0] for g in got]
        assert st[0] == st[1] == st[8] == _lib.FRAME_OK and st[2] == _lib.FRAME_CHECKSUM and st[3] == _lib.FRAME_BAD_MAGIC and st[7] == _lib.FRAME_SRCSIZE
        assert st[6] == (_lib.FRAME_DIGEST if exp else _lib.FRAME_OK)       # the DIGEST frame is searched
        pos = [positions(raws[i], rx) if s in DECODED else [] for i, s in enumerate(st)]
        assert [(g[2], g[3]) for g in got] == [(len(p), p[0] if p else None) for p in pos] and sum(s in DECODED for s in st) == 4
        lines = [zs.ref_lines(r, p) for r, p in zip(raws, pos)]
        assert [r[4] for r in res] == [len(l) for l in lines] and lines[0] and lines[8]
        assert recs == lc.deliver(raws, lines)                              # corrupt and mis-sized frames: count 0 and no record


def check_bounded_scratch(engine, corpus, compress=True):
    raws = sc.small_entries(corpus)[:600] + [corpus.entry(4700 + i, 1 << 20, i) for i in range(3)]
    rx = b"odnw[a-z]+ sj |^[a-z]+ kio$"                                        # (words of the synthetic corpus)
    packed = sc.pack(engine, raws, compress=compress)
    total = sum(len(zs.ref_lines(r, positions(r, rx))) for r in raws)
    assert total > 50
    rec_cap = total - 5
    free = check_regex_lines(engine, packed, raws, rx, rec_cap=rec_cap, tag="budget 0")
    free_counts = check_regex(engine, packed, raws, rx, tag="budget 0")
    assert engine.kernel_ms(_lib.T_SEARCH) > 0
    for mb in (2, 1):
        engine.set_parameter(_lib.PX_SCRATCH_MB, mb)
        try:
            assert check_regex_lines(engine, packed, raws, rx, rec_cap=rec_cap, tag="budget %d" % mb) == free
            assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in packed[0]), sum(len(r[5]) for r in free[1]))
            assert engine.kernel_ms(_lib.T_LINES) > 0 and engine.kernel_ms(_lib.T_SEARCH) > 0
            assert check_regex(engine, packed, raws, rx, tag="budget %d" % mb) == free_counts
            assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in packed[0]), 0)
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
    engine.verify(packed[0][:5], packed[1][:5], packed[2][:5])
    assert engine.kernel_ms(_lib.T_SEARCH) in (0.0, -1.0)


def check_device_form(engine, corpus, compress=True):
    raws = [sc.plant(corpus.entry(4800 + i, n, i % 4), b"GET /api/v1 200 17 ms", [n // 3, n // 2] if n > 60 else []) for i, n in enumerate((0, 1, 70000, 200000, 5, 7, S + 7, 4096))]
    rx = b"(GET|POST) /api.* [0-9]+ ms"
    frames, raw_lens, digests = packed = sc.pack(engine, raws, compress=compress)
    host = check_regex(engine, packed, raws, rx, tag="host form")
    h2d, d2h, ring, direct = vc.copy_counters(engine)
    assert (h2d, d2h) == (sum(len(f) for f in frames), 0) and ring + direct == h2d and sum(c for c, _ in host) >= 6
    assert engine.kernel_ms(_lib.T_SEARCH) > 0 and engine.kernel_ms(_lib.T_TOTAL) >= engine.kernel_ms(_lib.T_SEARCH)
    host_lines = check_regex_lines(engine, packed, raws, rx, tag="host form")
    h2d, d2h, _, _ = vc.copy_counters(engine)
    assert (h2d, d2h) == (sum(len(f) for f in frames), sum(len(r[5]) for r in host_lines[1])) and d2h > 0
    assert engine.kernel_ms(_lib.T_LINES) > 0
    d_frames, foff, _ = vc._arena(engine, frames)
    try:
        exp = np.frombuffer(b"".join(digests), dtype=np.uint8)
        flen = [len(f) for f in frames]
        for icase in (False, True):
            dev = check_regex(engine, packed, raws, rx.lower(), icase=icase, tag="device form", call=lambda: engine.search_regex_device(d_frames, foff, flen, raw_lens, rx.lower(), icase=icase, expect=exp))
            assert vc.copy_counters(engine) == (0, 0, 0, 0) and engine.kernel_ms(_lib.T_SEARCH) > 0
            assert (dev == host) == icase
        dev_call = lambda **kw: engine.search_regex_lines_device(d_frames, foff, flen, raw_lens, rx, expect=exp, **kw)
        for kw in ({}, {"max_lines": 1}, {"rec_cap": 3}, {"max_line": 17}):
            dev = check_regex_lines(engine, packed, raws, rx, tag="device form %r" % kw, call=dev_call, **kw)
            assert vc.copy_counters(engine) == (0, 0, 0, 0) and engine.kernel_ms(_lib.T_LINES) > 0
            assert dev == check_regex_lines(engine, packed, raws, rx, tag="host form %r" % kw, **kw)
        engine.verify_device(d_frames, foff, flen, raw_lens, exp)
        assert engine.kernel_ms(_lib.T_SEARCH) in (0.0, -1.0) and engine.kernel_ms(_lib.T_LINES) in (0.0, -1.0)
    finally:
        engine.free(d_frames)


def check_many_small(engine, corpus):
    raws = sc.small_entries(corpus)
    raws = raws[:400] + [b"", b"e", b"\n", b"sj"]
    rx = b"sj [a-z]+ |[0-9]{2,}$"
    pos = [positions(r, rx) for r in raws]
    refs = [(len(p), p[0] if p else None) for p in pos]
    assert sum(c > 0 for c, _ in refs) > 10 and sum(c == 0 for c, _ in refs) > 10
    for compress in (True, False):
        packed = sc.pack(engine, raws, compress=compress)
        check_regex(engine, packed, raws, rx, tag="small, compress %r" % compress, refs=refs)
    check_regex_lines(engine, packed, raws, rx, tag="small, lines")


def check_lines_caps(engine, corpus, compress=True):
    big = b"".join(b"line %d %s\n" % (k, b"took 17 ms" if k % 3 else b"took 5 s") for k in range(1000))
    small = [sc.plant(corpus.entry(5400 + i, 3000, 0), b"took 99 ms", [100 + 900 * k for k in range(i)]) for i in range(4)]
    raws = [small[1], big, small[0], small[3], b"", small[2]]
    rx = b"took [0-9]+ m?s$|took [0-9]+ ms"
    packed = sc.pack(engine, raws, compress=compress)
    full = [len(zs.ref_lines(r, positions(r, rx))) for r in raws]
    assert full[1] == 1000
    for max_lines in (0, 1, 7):
        total = sum(min(n, max_lines or n) for n in full)
        for rec_cap in (0, 1, total, total - 1):
            res, recs = check_regex_lines(engine, packed, raws, rx, max_lines=max_lines, rec_cap=rec_cap, tag="caps %d %d" % (max_lines, rec_cap))
            assert [r[4] for r in res] == full and len(recs) == min(total, rec_cap)
    long_line = corpus.entry(5450, 70000, 0).replace(b"\n", b" ")
    raws2 = [b"\n".join([b"", b"Q", b"Qx" + b"x" * 14, b"y" * 16 + b"Q", long_line[:100] + b"QQ" + long_line[102:], b""])]
    assert b"Q" not in long_line
    packed2 = sc.pack(engine, raws2, compress=compress)
    for max_line in (1, 16, 17, 65536):
        _, recs = check_regex_lines(engine, packed2, raws2, b"Q+x?", max_line=max_line, rec_cap=5, tag="max_line %d" % max_line)
        assert [(r[2], len(r[5])) for r in recs] == [(n, min(n, max_line)) for n in (1, 16, 17, 70000)]


# ---- real data (GPU) -----------------------------------------------------------------------------------------------------------------
def check_real_items(engine, real_items):
    raws = list(real_items.values())
    packed = sc.pack(engine, raws)
    for rx, icase in ((b"[A-Za-z_]+\\(.*\\)", False), (b"^ *(#|//|/\\*)", False), (b"the [a-z]+ of", True)):
        got = check_regex(engine, packed, raws, rx, icase=icase, tag="real items")
        assert sum(c for c, _ in got) >= 1
    check_regex_lines(engine, packed, raws, b"[0-9]+\\.[0-9]+", rec_cap=2000, tag="real items, lines")
