"""Checks of zarc_gpu_search_lines_batch*, shared by the emulator tests (test_lines.py) and the GPU tests (test_gpu_lines.py).

The reference for every expected value is Python on the bytes the frames were packed from -- never the engine: ref_lines() for the lines,
search_cases.ref() for count and first, deliver() for the delivery rule.  Every comparison is equality.
A line is a maximal run of bytes without 0x0A; its number is 1 + the 0x0A bytes in front of it; it matches when a match starts in it."""
import ctypes
import os
import re

import numpy as np

import make_golden
import search_cases as sc
import verify_cases as vc
from zarc_amd import _lib

S = sc.SLICE
NEEDLE = sc.NEEDLE7            # bytes the corpus text does not hold, no 0x0A among them
LEN1 = 3 * S + 1000            # the largest frame of these cases (but the one multi-MiB frame of the pieces case)


def ref_lines(d, p, icase=False):
    out, pos, no = [], 0, 1
    for piece in d.split(b"\n"):
        m = re.search(re.escape(p), piece, re.I if icase else 0)
        if m: out.append((pos, len(piece), no, pos + m.start()))
        pos += len(piece) + 1; no += 1
    return out          # (start, length, number, match); an empty last piece never matches


def deliver(raws, want, max_lines=0, max_line=4096, rec_cap=None):
    """the delivery rule: frames in batch order, per frame the first min(lines, max_lines or all, what rec_cap leaves) lines"""
    out, left = [], (sum(len(w) for w in want) if rec_cap is None else rec_cap)
    for i, w in enumerate(want):
        d = min(len(w), max_lines or len(w), left)
        out += [(i, s, l, no, m, raws[i][s:s + min(l, max_line)]) for s, l, no, m in w[:d]]
        left -= d
    return out


def check_lines(engine, packed, raws, needle, icase=False, max_lines=0, max_line=4096, rec_cap=None, tag="", call=None, statuses=None):
    """one search_lines call over a packed batch against the reference.  rec_cap None: room for every line.  -> (results, records)"""
    frames, raw_lens, digests = packed
    want = [ref_lines(r, needle, icase) for r in raws]
    cap = sum(len(w) for w in want) + 1 if rec_cap is None else rec_cap
    call = call or (lambda **kw: engine.search_lines(frames, raw_lens, needle, expect=digests, **kw))
    results, records = call(icase=icase, max_lines=max_lines, max_line=max_line, rec_cap=cap)
    assert len(results) == len(raws)
    for i, (st, dig, count, first, lines) in enumerate(results):
        assert st == _lib.FRAME_OK and dig == digests[i], (tag, i, st)
        assert (count, first) == sc.ref(raws[i], needle, icase), (tag, i)
        assert lines == len(want[i]), (tag, i, lines, len(want[i]))
    exp = deliver(raws, want, max_lines, max_line, cap)
    assert len(records) == len(exp), (tag, len(records), len(exp))
    for g, e in zip(records, exp):
        assert g == e, (tag, g[:5], e[:5])
    return results, records


def blank(b, lo, hi):
    """the text's own newlines in [lo, hi) become spaces"""
    b[lo:hi] = bytes(b[lo:hi]).replace(b"\n", b" ")


# ---- 1. slice boundaries -------------------------------------------------------------------------------------------------------------
def boundary_frames(corpus):
    """Every scenario alone in a frame of LEN1 bytes, around the boundary B = S (the spanning line: S and 2S), and all of them together.
    A line that crosses a boundary and a 0x0A next to the same boundary exclude each other, so the scenarios need six boundaries and a frame
    of LEN1 bytes has three: the combination is three frames of one batch."""
    text = corpus.entry(5000, LEN1, 0)
    assert sc.ref(text, NEEDLE) == (0, None) and text.count(b"\n") > 100

    def starts_then_matches(b, B):      # a line that starts in the slice in front of B and matches only behind B
        b[B - 100] = 10; b[B + 50:B + 57] = NEEDLE; b[B + 500] = 10
    def matches_in_both(b, B):          # one line with a match on either side of B
        b[B - 100] = 10; b[B - 50:B - 43] = NEEDLE; b[B + 50:B + 57] = NEEDLE; b[B + 500] = 10
    def spans_three(b, B):              # slices k .. k+2, no 0x0A in slice k+1, matches in k and k+2: one line, `match` in slice k
        blank(b, B - 2000, B + S + 2000)
        b[B - 100] = 10; b[B - 50:B - 43] = NEEDLE; b[B + S + 50:B + S + 57] = NEEDLE; b[B + S + 500] = 10
    def two_newlines(b, B):             # 0x0A at B-1 and at B, matches around them
        b[B - 1] = 10; b[B] = 10; b[B - 20:B - 13] = NEEDLE; b[B + 1:B + 8] = NEEDLE
    def match_behind_newline(b, B):     # a match starting at B right behind a 0x0A at B-1
        b[B - 1] = 10; b[B:B + 7] = NEEDLE
    def match_before_newline(b, B):     # a match ending at B-1 right before a 0x0A at B
        b[B - 7:B] = NEEDLE; b[B] = 10
    def last_line_open(b, B):           # a match in the frame's last line, no final 0x0A
        blank(b, LEN1 - 200, LEN1); b[LEN1 - 300] = 10; b[LEN1 - 7:] = NEEDLE
    def last_line_closed(b, B):         # ... and with one
        blank(b, LEN1 - 200, LEN1); b[LEN1 - 300] = 10; b[LEN1 - 8:LEN1 - 1] = NEEDLE; b[LEN1 - 1] = 10

    def frame(*plan):
        b = bytearray(text)
        for _, B in plan: blank(b, B - 2000, B + 2000)
        for f, B in plan: f(b, B)
        assert len(b) == LEN1
        return bytes(b)
    alone = [starts_then_matches, matches_in_both, spans_three, two_newlines, match_behind_newline, match_before_newline, last_line_open, last_line_closed]
    raws = [frame((f, S)) for f in alone]
    raws.append(frame((spans_three, S), (match_behind_newline, 3 * S), (last_line_open, 0)))
    raws.append(frame((starts_then_matches, S), (match_before_newline, 2 * S), (two_newlines, 3 * S), (last_line_closed, 0)))
    raws.append(frame((matches_in_both, S), (match_behind_newline, 2 * S), (match_before_newline, 3 * S)))
    return raws


def check_boundaries(engine, corpus, compress=True):
    raws = boundary_frames(corpus)
    _, recs = check_lines(engine, sc.pack(engine, raws, compress=compress), raws, NEEDLE, tag="boundaries")
    by = lambda i: [r[1:5] for r in recs if r[0] == i]
    assert [len(by(i)) for i in range(8)] == [1, 1, 1, 2, 1, 1, 1, 1]
    assert by(0)[0][0] == S - 99 and by(0)[0][3] == S + 50                   # starts in slice 0, matches in slice 1
    assert by(1)[0][3] == S - 50 and by(1)[0][1] == 599                      # two matches, one line
    assert by(2)[0][:2] == (S - 99, S + 599) and by(2)[0][3] == S - 50       # the line spans slice 1 entirely
    assert [r[0] for r in by(3)] == [by(3)[0][0], S + 1] and by(3)[1][2] == by(3)[0][2] + 2   # an empty line lies between them
    assert by(4)[0][0] == by(4)[0][3] == S
    assert by(5)[0][3] == S - 7 and by(5)[0][0] + by(5)[0][1] == S
    assert by(6)[0][0] + by(6)[0][1] == LEN1 and by(7)[0][0] + by(7)[0][1] == LEN1 - 1
    assert [len(by(i)) for i in (8, 9, 10)] == [3, 5, 3]


# ---- 2. degenerate frames ------------------------------------------------------------------------------------------------------------
def check_degenerate(engine, corpus, compress=True):
    flat = bytearray(corpus.entry(5100, 2 * S + 500, 0))
    blank(flat, 0, len(flat))
    flat = sc.plant(bytes(flat), NEEDLE, [100, S - 3, 2 * S + 493])
    crlf = b"abc\r\nxx " + NEEDLE + b" yy\r\n\r\n" + NEEDLE + b"\r\nend"
    raws = [b"", b"\n" * 70000, flat, NEEDLE, NEEDLE + b"\n", crlf, b"\n" + NEEDLE, b"\n\n"]
    _, recs = check_lines(engine, sc.pack(engine, raws, compress=compress), raws, NEEDLE, tag="degenerate")
    assert [r[:5] for r in recs if r[0] == 2] == [(2, 0, 2 * S + 500, 1, 100)]  # three matches, one line: the whole frame
    assert [r[:5] for r in recs if r[0] in (3, 4)] == [(3, 0, 7, 1, 0), (4, 0, 7, 1, 0)]
    assert [r[5] for r in recs if r[0] == 5] == [b"xx " + NEEDLE + b" yy\r", NEEDLE + b"\r"]   # the 0x0D stays in the line
    assert [r[3] for r in recs if r[0] in (5, 6)] == [2, 4, 2]
    assert len(recs) == 6


# ---- 3. neighbours in the scratch ----------------------------------------------------------------------------------------------------
def check_neighbours(engine, corpus, compress=True):
    """64 frames of exactly 4096 bytes back to back in the scratch: each ends in an open matching line (no final 0x0A) and begins with a
    matching first line.  Numbers restart at 1, no line is merged across two frames or counted twice."""
    raws = []
    for i in range(64):
        b = bytearray(corpus.entry(5200 + i, 4096, 0))
        blank(b, 0, 200); blank(b, 3896, 4096)
        b[:7] = NEEDLE; b[100] = 10; b[3900] = 10; b[4096 - 7:] = NEEDLE
        raws.append(bytes(b))
    res, recs = check_lines(engine, sc.pack(engine, raws, compress=compress), raws, NEEDLE, tag="neighbours")
    assert [r[4] for r in res] == [2] * 64
    assert [r[:4] for r in recs[:2]] == [(0, 0, 100, 1), (0, 3901, 195, raws[0].count(b"\n") + 1)]
    assert all(recs[2 * i][3] == 1 for i in range(64))


def small_needle(raws):
    r = raws[80]
    at = next(k for k in range(30, len(r) - 2) if b"\n" not in r[k:k + 2])
    return r[at:at + 2]


def check_many_small(engine, corpus):
    raws = sc.small_entries(corpus)
    needle = small_needle(raws)
    for compress in (True, False):
        res, recs = check_lines(engine, sc.pack(engine, raws, compress=compress), raws, needle, tag="small, compress %r" % compress)
        assert len(recs) > 10 and sum(r[4] == 0 for r in res) > 10


# ---- 4. several matches per line, overlap, case folding ------------------------------------------------------------------------------
def check_overlap(engine, compress=True):
    cut = bytearray(b"abab" * 30000)
    for k in range(99, len(cut), 100): cut[k] = 10
    raws = [b"abab" * 30000, bytes(cut), b"a" * 70001]
    packed = sc.pack(engine, raws, compress=compress)
    res, recs = check_lines(engine, packed, raws, b"ababa", tag="abab")
    assert [r[4] for r in res] == [1, 1200, 0] and recs[0][:5] == (0, 0, 120000, 1, 0)
    res, _ = check_lines(engine, packed, raws, b"a", tag="a")
    assert [r[4] for r in res] == [1, 1200, 1]


def check_case_folding(engine, corpus, compress=True):
    """the inputs of search_cases.check_case_folding, a 0x0A planted every 61 bytes where it breaks none of the planted strings"""
    text = corpus.entry(4300, 70000, 0)
    raws = [
        sc.plant(text, b"hello WORLD", [5]) + b"HELLO world" + text[:777] + b"hElLo wOrLd" + b"Hello World",
        b"0123{A4567{a89`A@a" * 200,
        b"xx[Ayy[azz" * 50,
        sc.plant(text, b"\xc4B\xe4", [100, S - 1]) + b"\xe4b\xc4..\xc4b\xc4..\xe4B\xe4..\xc4b\xe4",
        b"`Z@" * 33 + b"@z`",
    ]
    cut = []
    for r in raws:
        b = bytearray(r)
        for k in range(60, len(b), 61):
            if b[k] in b"0123456789xyz.,;": b[k] = 10
        cut.append(bytes(b))
    packed = sc.pack(engine, cut, compress=compress)
    n = {}
    for needle in (b"Hello World", b"[a", b"\xc4b\xe4", b"@z`", b"{A"):
        for icase in (False, True):
            res, _ = check_lines(engine, packed, cut, needle, icase, tag="case %r %r" % (needle, icase))
            n[needle, icase] = [r[4] for r in res]
    assert n[b"Hello World", True][0] > n[b"Hello World", False][0] >= 1   # (the four spellings stand far apart: four lines)
    assert n[b"[a", True][2] >= n[b"[a", False][2] >= 1 and n[b"[a", True][1] == 0
    assert n[b"{A", True][1] > 0


NEEDLE_LENS = (1, 4, 5, 17, 256)


def check_needle_lengths(engine, corpus, compress=True):
    length = 2 * S + 500
    raws = []
    for j, m in enumerate(NEEDLE_LENS):
        nd = sc.needle_of(m)
        offs = [16 * 1000 - (1 if m > 1 else 0), S - max(1, m // 2), length - m]
        raws.append(sc.plant(corpus.entry(5300 + j, length, 0), nd, offs))
    packed = sc.pack(engine, raws, compress=compress)
    for j, m in enumerate(NEEDLE_LENS):
        res, _ = check_lines(engine, packed, raws, sc.needle_of(m), tag="needle of %d" % m)
        assert res[j][4] >= 2


# ---- 5. caps -------------------------------------------------------------------------------------------------------------------------
def check_caps(engine, corpus, compress=True):
    big = b"".join(b"line %d %s\n" % (k, NEEDLE) for k in range(1000))
    small = [sc.plant(corpus.entry(5400 + i, 3000, 0), NEEDLE, [100 + 900 * k for k in range(i)]) for i in range(4)]
    raws = [small[1], big, small[0], small[3], b"", small[2]]
    packed = sc.pack(engine, raws, compress=compress)
    want = [ref_lines(r, NEEDLE) for r in raws]
    assert len(want[1]) == 1000
    full = [len(w) for w in want]
    for max_lines in (0, 1, 7):
        total = sum(min(len(w), max_lines or len(w)) for w in want)
        for rec_cap in (0, 1, total, total - 1):
            res, recs = check_lines(engine, packed, raws, NEEDLE, max_lines=max_lines, rec_cap=rec_cap, tag="caps %d %d" % (max_lines, rec_cap))
            assert [r[4] for r in res] == full                              # lines[] is all of them, whatever the caps
            assert len(recs) == min(total, rec_cap)
    # max_line against lines of 0, 1, 16, 17 and 70 000 bytes
    long_line = corpus.entry(5450, 70000, 0).replace(b"\n", b" ")
    Q = b"\xf7"
    raws2 = [b"\n".join([b"", Q, Q + b"x" * 15, b"y" * 16 + Q, long_line[:100] + Q + long_line[101:], b""])]
    assert Q not in long_line
    packed2 = sc.pack(engine, raws2, compress=compress)
    for max_line in (1, 16, 17, 65536):
        _, recs = check_lines(engine, packed2, raws2, Q, max_line=max_line, rec_cap=5, tag="max_line %d" % max_line)
        assert [(r[2], len(r[5])) for r in recs] == [(n, min(n, max_line)) for n in (1, 16, 17, 70000)]
    # text_cap one byte short of rec_cap * max_line
    for rec_cap, max_line, rc in ((5, 16, _lib.E_DSTSIZE), (1, 1, _lib.E_DSTSIZE), (2 ** 62, 65536, _lib.E_DSTSIZE)):
        assert raw_call(engine, packed2, Q, rec_cap=rec_cap, max_line=max_line, text_cap=(rec_cap * max_line - 1) % 2 ** 64, alloc=64)[0] == rc
    assert raw_call(engine, packed2, Q, rec_cap=4, max_line=16, text_cap=64, alloc=64)[0] == _lib.OK


def raw_call(engine, packed, pat, m=None, flags=0, max_lines=0, max_line=4096, rec_cap=4, text_cap=None, alloc=None, n=None, frame_len=None, **null):
    """zarc_gpu_search_lines_batch through ctypes; null: names of arguments to pass as NULL; alloc: records to really allocate when rec_cap
    is a number no buffer can have (the call is refused before it writes).  -> (rc, rec_used, text_used, lines)"""
    c = ctypes
    frames, raw_lens, _ = packed
    ptrs, lens = vc._ptrs(frames)
    if frame_len is not None: lens = (c.c_size_t * len(frames))(*frame_len)
    rl = (c.c_size_t * len(frames))(*raw_lens)
    dig = np.zeros((len(frames), 32), dtype=np.uint8)
    st, cnt, fst, lines = (c.c_int * len(frames))(), (c.c_uint64 * len(frames))(), (c.c_uint64 * len(frames))(), (c.c_uint64 * len(frames))()
    nrec = rec_cap if alloc is None else alloc
    rec = (_lib.Line * max(nrec, 1))()
    text = np.zeros(max(nrec * min(max_line, 65536), 1), dtype=np.uint8)
    ru, tu = c.c_size_t(77), c.c_size_t(77)
    a = dict(ptrs=ptrs, lens=lens, rl=rl, dig=dig.ctypes.data_as(c.c_void_p), st=st, cnt=cnt, fst=fst, lines=lines, rec=rec, ru=c.byref(ru),
             text=text.ctypes.data_as(c.c_void_p), tu=c.byref(tu))
    for k in null: a[k] = None
    rc = engine.lib.zarc_gpu_search_lines_batch(engine.h, len(frames) if n is None else n, a["ptrs"], a["lens"], a["rl"], None,
                                                c.cast(c.c_char_p(pat), c.c_void_p) if pat is not None else None, len(pat) if m is None else m, flags, max_lines,
                                                max_line, a["dig"], a["st"], a["cnt"], a["fst"], a["lines"], a["rec"], rec_cap, a["ru"], a["text"],
                                                rec_cap * max_line if text_cap is None else text_cap, a["tu"])
    return rc, ru.value, tu.value, list(lines)


# ---- 6. bounded scratch and forms ----------------------------------------------------------------------------------------------------
def check_bounded_scratch(engine, corpus, compress=True):
    raws = sc.small_entries(corpus) + [corpus.entry(4700 + i, 1 << 20, i) for i in range(3)]
    needle = small_needle(raws)
    packed = sc.pack(engine, raws, compress=compress)
    total = sum(len(ref_lines(r, needle)) for r in raws)
    in_big = len(ref_lines(raws[-3], needle))
    assert total > 200 and in_big > 20
    rec_cap = total - in_big // 2 - len(ref_lines(raws[-1], needle)) - len(ref_lines(raws[-2], needle))   # runs out inside the first large frame
    free = check_lines(engine, packed, raws, needle, rec_cap=rec_cap, tag="budget 0")
    assert len(free[1]) == rec_cap and free[1][-1][0] == len(raws) - 3
    for mb in (2, 1):                                                      # two parts and more: the remainder of rec_cap crosses their boundaries
        engine.set_parameter(_lib.PX_SCRATCH_MB, mb)
        try:
            assert check_lines(engine, packed, raws, needle, rec_cap=rec_cap, tag="budget %d" % mb) == free
            assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in packed[0]), sum(len(r[5]) for r in free[1]))
            assert engine.kernel_ms(_lib.T_LINES) > 0
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)


def check_device_form(engine, corpus, compress=True):
    raws = [sc.plant(corpus.entry(4800 + i, n, i % 4), NEEDLE, [n // 3, n // 2] if n > 30 else []) for i, n in enumerate((0, 1, 70000, 200000, 5, 7, S + 7, 4096))]
    raws[5] = NEEDLE
    frames, raw_lens, digests = packed = sc.pack(engine, raws, compress=compress)
    host = check_lines(engine, packed, raws, NEEDLE, tag="host form")
    h2d, d2h, ring, direct = vc.copy_counters(engine)
    assert (h2d, d2h) == (sum(len(f) for f in frames), sum(len(r[5]) for r in host[1])) and d2h > 0 and ring + direct == h2d + d2h
    assert engine.kernel_ms(_lib.T_LINES) > 0 and engine.kernel_ms(_lib.T_SEARCH) > 0
    assert engine.kernel_ms(_lib.T_TOTAL) >= engine.kernel_ms(_lib.T_LINES)
    d_frames, foff, _ = vc._arena(engine, frames)
    try:
        exp = np.frombuffer(b"".join(digests), dtype=np.uint8)
        dev_call = lambda **kw: engine.search_lines_device(d_frames, foff, [len(f) for f in frames], raw_lens, NEEDLE, expect=exp, **kw)
        for kw in ({}, {"icase": True}, {"max_lines": 1}, {"rec_cap": 3}, {"max_line": 17}):
            dev = check_lines(engine, packed, raws, NEEDLE, tag="device form %r" % kw, call=dev_call, **kw)
            assert engine.kernel_ms(_lib.T_LINES) > 0
            assert dev == check_lines(engine, packed, raws, NEEDLE, tag="host form %r" % kw, **kw)
        dev_call(rec_cap=64)
        assert vc.copy_counters(engine) == (0, 0, 0, 0)
        assert dev_call(rec_cap=64) == host
        engine.verify_device(d_frames, foff, [len(f) for f in frames], raw_lens, exp)
        assert engine.kernel_ms(_lib.T_LINES) in (0.0, -1.0)
        engine.search_device(d_frames, foff, [len(f) for f in frames], raw_lens, NEEDLE, expect=exp)
        assert engine.kernel_ms(_lib.T_LINES) in (0.0, -1.0)
    finally:
        engine.free(d_frames)
    for other in (lambda: engine.verify(frames, raw_lens, digests), lambda: engine.search(frames, raw_lens, NEEDLE, expect=digests),
                  lambda: engine.unpack(frames, raw_lens, digests)):
        other()
        assert engine.kernel_ms(_lib.T_LINES) in (0.0, -1.0)               # an unused timer, as T_SEARCH after a call that does not search


# ---- 7. verdict parity ---------------------------------------------------------------------------------------------------------------
def check_verdicts(engine, oracle, corpus, golden_frames):
    frames, raw_lens, expect, raws = vc.error_list(oracle, corpus, golden_frames)
    good = [corpus.entry(4600 + i, 30000 + i, 0) for i in range(2)]
    needle = next(raws[0][k:k + 5] for k in range(150, 400) if b"\n" not in raws[0][k:k + 5])
    good = [sc.plant(g, needle, [77, 20000]) for g in good]
    gf, gl, gd = sc.pack(engine, good)
    frames, raw_lens, expect, raws = [gf[0]] + frames + [gf[1]], [gl[0]] + raw_lens + [gl[1]], [gd[0]] + expect + [gd[1]], [good[0]] + raws + [good[1]]
    for exp in (expect, None):
        want = engine.verify(frames, raw_lens, exp)
        srch = engine.search(frames, raw_lens, needle, expect=exp)
        res, recs = engine.search_lines(frames, raw_lens, needle, expect=exp, rec_cap=10000)
        assert [(dig, st) for st, dig, _, _, _ in res] == want              # status and digest equal verify's
        assert [r[:4] for r in res] == srch                                 # count and first equal search's
        decoded = [i for i, r in enumerate(res) if r[0] in (_lib.FRAME_OK, _lib.FRAME_DIGEST)]
        assert len(decoded) == 4 and (res[6][0] == _lib.FRAME_DIGEST) == (exp is not None)   # the DIGEST frame is delivered
        lines = [ref_lines(raws[i], needle) if i in decoded else [] for i in range(len(raws))]
        assert [r[4] for r in res] == [len(l) for l in lines] and all(len(lines[i]) >= 1 for i in decoded)
        assert recs == deliver(raws, lines)                                 # undecoded frames: 0 lines and no record


# ---- 8. other encoders' frames, frames in pieces -------------------------------------------------------------------------------------
def check_pieces(engine, oracle, corpus, golden_frames):
    d, m = golden_frames
    raws, frames = [corpus.entry(4500, (4 << 20) + 17, 0)], []
    frames.append(sc.pack(engine, raws)[0][0])
    for name in ("text300", "records200k", "lz300k"):
        fr = next(f for f in m["frames"] if f["recipe"] == name and f["level"] == 3 and f["checksum"] == 1 and f["libzstd"].startswith("1.5"))
        frames.append(open(os.path.join(d, fr["file"]), "rb").read())
        raws.append(make_golden.recipe_bytes(m["recipes"][name], corpus))
    packed = (frames, [len(r) for r in raws], [oracle.blake3(r) for r in raws])
    for i, r in enumerate(raws):
        at = next(k for k in range(len(r) // 2, len(r)) if b"\n" not in r[k:k + 9])
        needle = r[at:at + (9, 3, 6, 5)[i]]
        res, _ = check_lines(engine, packed, raws, needle, max_lines=50, max_line=256, rec_cap=120, tag="pieces %d" % i)
        assert res[i][4] >= 1


# ---- 9. arguments --------------------------------------------------------------------------------------------------------------------
def check_arguments(engine, corpus):
    c = ctypes
    raw = sc.plant(corpus.entry(4900, 5000, 0), NEEDLE, [1234])
    packed = sc.pack(engine, [raw])
    want = ref_lines(raw, NEEDLE)
    ok = raw_call(engine, packed, NEEDLE)
    assert ok == (_lib.OK, 1, want[0][1], [1])
    P = _lib.E_PARAM
    assert [raw_call(engine, packed, NEEDLE, **{k: None})[0] for k in ("lines", "ru", "tu", "rec", "text")] == [P] * 5
    assert raw_call(engine, packed, NEEDLE, rec_cap=0, rec=None, text=None) == (_lib.OK, 0, 0, [1])      # a counting call
    assert [raw_call(engine, packed, NEEDLE, max_line=v)[0] for v in (0, 65537, 2 ** 63)] == [P] * 3
    assert raw_call(engine, packed, NEEDLE, max_line=65536, rec_cap=2)[0] == _lib.OK
    assert [raw_call(engine, packed, p)[0] for p in (b"a\nb", b"\n", b"ab\n")] == [P] * 3
    # ... and everything search refuses
    assert raw_call(engine, packed, None, m=7)[0] == raw_call(engine, packed, NEEDLE, m=0)[0] == raw_call(engine, packed, b"p" * 300, m=257)[0] == P
    assert [raw_call(engine, packed, NEEDLE, flags=f)[0] for f in (2, 3, 0x80000000)] == [P] * 3
    assert [raw_call(engine, packed, NEEDLE, **{k: None})[0] for k in ("st", "cnt", "fst", "dig", "ptrs", "lens", "rl")] == [P] * 7
    assert raw_call(engine, packed, NEEDLE, n=0, ptrs=None, lens=None, rl=None)[:3] == (_lib.OK, 0, 0)
    assert raw_call(engine, (packed[0], [0xFFFFFFF0], packed[2]), NEEDLE)[0] == raw_call(engine, packed, NEEDLE, frame_len=[0xFFFFFFF0])[0] == _lib.E_UNSUPPORTED
    # the device form
    lib, h = engine.lib, engine.h
    u64 = lambda v: (c.c_uint64 * 1)(v)
    dig = np.zeros((1, 32), dtype=np.uint8)
    pdig = dig.ctypes.data_as(c.c_void_p)
    st, cnt, fst, lines = (c.c_int * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)()
    rec, ru, tu = (_lib.Line * 4)(), c.c_size_t(), c.c_size_t()
    pat = c.cast(c.c_char_p(NEEDLE), c.c_void_p)
    dummy = c.c_void_p(16)  # never dereferenced: the call is refused before

    def dev(n=1, base=dummy, off=u64(0), fl=u64(9), rl=u64(0), pat=pat, m=7, flags=0, max_line=16, pdig=pdig, st=st, cnt=cnt, fst=fst, lines=lines, rec=rec, rec_cap=4,
            ru=c.byref(ru), text=dummy, text_cap=64, tu=c.byref(tu)):
        return lib.zarc_gpu_search_lines_batch_device(h, n, base, off, fl, rl, None, pat, m, flags, 0, max_line, pdig, st, cnt, fst, lines, rec, rec_cap, ru, text, text_cap, tu)
    assert dev(n=0, base=None, off=None, fl=None, rl=None) == _lib.OK
    assert dev(base=None) == dev(off=None) == dev(fl=None) == dev(rl=None) == P
    assert dev(pat=None) == dev(m=0) == dev(m=257) == dev(flags=4) == dev(max_line=0) == dev(max_line=65537) == P
    assert dev(st=None) == dev(cnt=None) == dev(fst=None) == dev(pdig=None) == dev(lines=None) == dev(ru=None) == dev(tu=None) == dev(rec=None) == dev(text=None) == P
    assert dev(pat=c.cast(c.c_char_p(b"abc\ndef"), c.c_void_p)) == P
    assert dev(text_cap=63) == _lib.E_DSTSIZE
    assert dev(rl=u64(0xFFFFFFF0)) == dev(fl=u64(1 << 32)) == _lib.E_UNSUPPORTED
    # ... and the handle still works
    assert raw_call(engine, packed, NEEDLE) == ok
    res, recs = engine.search_lines(packed[0], packed[1], NEEDLE, expect=packed[2])
    assert res == [(0, packed[2][0], 1, 1234, 1)] and recs == deliver([raw], [want])


# ---- 10. real data (GPU) -------------------------------------------------------------------------------------------------------------
def check_real_items(engine, real_items):
    """a 4-byte needle from the middle of each item, searched in that item and its neighbour (the reference walks every line of what is
    searched: over all pairs of items it would take the time of the whole suite)"""
    raws = list(real_items.values())
    frames, raw_lens, digests = sc.pack(engine, raws)
    for i, r in enumerate(raws):
        at = next(k for k in range(len(r) // 2, len(r)) if b"\n" not in r[k:k + 4])
        needle = r[at:at + 4]
        pick = [i, (i + 1) % len(raws)]
        packed = ([frames[k] for k in pick], [raw_lens[k] for k in pick], [digests[k] for k in pick])
        res, _ = check_lines(engine, packed, [raws[k] for k in pick], needle, max_lines=100, max_line=512, rec_cap=150, tag="real item %d" % i)
        assert res[0][4] >= 1
