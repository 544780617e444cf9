"""Checks of zarc_gpu_select_lines_batch* (grep's -v and -A / -B / -C), shared by the emulator tests (test_select.py) and the GPU tests
(test_gpu_select.py).

The reference of every expected value is Python on the bytes the frames were packed from -- never the engine: the lines are the pieces
between 0x0A bytes (an empty last piece dropped), M comes from lines_cases.ref_lines, set_cases.ref_lines or regex_cases.positions, H and S
follow include/zarc_gpu.h word for word, lines_cases.deliver is the delivery rule.  Every comparison is equality, and every scenario asserts
on the reference side that it is not vacuous."""
import bisect
import ctypes

import numpy as np

import lines_cases as lc
import regex_cases as rc
import search_cases as sc
import set_cases as zs
import verify_cases as vc
from zarc_amd import _lib

S = sc.SLICE
NEEDLE = sc.NEEDLE7            # bytes no frame of these cases holds unless planted, no 0x0A among them
LEN1 = 3 * S + 1000
FIXED, SET, REGEX = _lib.MATCH_FIXED, _lib.MATCH_SET, _lib.MATCH_REGEX
RX = rc.re.escape(NEEDLE)      # the needle as an expression
ALL = 0xFFFFFFFF
DECODED = (_lib.FRAME_OK, _lib.FRAME_DIGEST)


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def all_lines(d):
    pieces = d.split(b"\n")
    if pieces[-1] == b"": pieces.pop()
    out, pos = [], 0
    for no, p in enumerate(pieces, 1):
        out.append((pos, len(p), no))
        pos += len(p) + 1
    return out


def matching(d, kind, what, icase=False):
    """-> {line number: lowest matching start position} and (count, first[, which]) of the plain search"""
    if kind == FIXED:
        return {no: m for _, _, no, m in lc.ref_lines(d, what, icase)}, sc.ref(d, what, icase)
    if kind == SET:
        count, first, which, _, union = zs.ref(d, what, icase)
        return {no: m for _, _, no, m in zs.ref_lines(d, union)}, (count, first, which)
    pos = rc.positions(d, what, icase)
    return {no: m for _, _, no, m in zs.ref_lines(d, pos)}, (len(pos), pos[0] if pos else None)


def ref_select(d, kind, what, icase=False, invert=False, before=0, after=0):
    """-> (|H|, S as [(start, length, number, match or None)], the plain search's answer)"""
    lines = all_lines(d)
    M, plain = matching(d, kind, what, icase)
    H = [no for _, _, no in lines if (no in M) != invert]
    sel = []
    for s, l, no in lines:
        j = bisect.bisect_right(H, no)                 # H[j-1] <= no < H[j]
        if (j > 0 and no - H[j - 1] <= after) or (j < len(H) and H[j] - no <= before):
            sel.append((s, l, no, M.get(no)))
    return len(H), sel, plain


def call_host(engine, packed, kind, what):
    frames, raw_lens, digests = packed
    return lambda **kw: engine.select_lines(frames, raw_lens, kind, what, expect=digests, **kw)


def check_select(engine, packed, raws, kind, what, icase=False, invert=False, before=0, after=0, max_lines=0, max_line=4096, rec_cap=None, tag="", call=None):
    """one select_lines call over a packed batch of good frames against the reference.  rec_cap None: room for every selected line.
    -> (results, records, reference S per frame)"""
    digests = packed[2]
    refs = [ref_select(r, kind, what, icase, invert, before, after) for r in raws]
    want = [r[1] for r in refs]
    cap = sum(len(w) for w in want) + 1 if rec_cap is None else rec_cap
    call = call or call_host(engine, packed, kind, what)
    results, records, _ = call(icase=icase, invert=invert, before=before, after=after, max_lines=max_lines, max_line=max_line, rec_cap=cap)
    assert len(results) == len(raws)
    for i, res in enumerate(results):
        assert res[0] == _lib.FRAME_OK and res[1] == digests[i], (tag, i, res[0])
        assert tuple(res[2:-2]) == tuple(refs[i][2]), (tag, i, res[2:-2], refs[i][2])               # count, first[, which]: the plain search's
        assert (res[-2], res[-1]) == (refs[i][0], len(want[i])), (tag, i, res[-2:], refs[i][0], len(want[i]))
    exp = lc.deliver(raws, want, max_lines, max_line, cap)
    assert len(records) == len(exp), (tag, len(records), len(exp))
    for g, e in zip(records, exp):
        assert g == e, (tag, g[:5], e[:5])
    return results, records, want


def text_frame(n, seed=0, final_newline=False):
    """n bytes of lines of 20 to 90 bytes that hold their own number; no needle, no final 0x0A unless asked for"""
    out, k, total = [], 0, 0
    while total < n:
        ln = b"line %07d " % k + b"abcdefghijklmnopqrstuvwxyz"[: (k * 7 + seed) % 26] * 3
        ln = ln[:20 + (k * 13 + seed * 5) % 71] + b"\n"
        out.append(ln); total += len(ln); k += 1
    b = bytearray(b"".join(out)[:n])
    if b and b[-1] == 10 and not final_newline: b[-1] = 0x2E
    if b and final_newline: b[-1] = 10
    return b


def blank(b, lo, hi):
    b[lo:hi] = bytes(b[lo:hi]).replace(b"\n", b" ")


def kinds():
    return ((FIXED, NEEDLE), (SET, [NEEDLE]), (REGEX, RX))


# ---- 1. context across a slice boundary ----------------------------------------------------------------------------------------------
def boundary_frames():
    """B = S.  Per position of a 0x0A right at the boundary (B-1: the line ends in slice 0; B: it ends in slice 1 with all its bytes in
    slice 0) a frame whose hit is the line in front of that 0x0A and one whose hit is the line behind it"""
    raws = []
    for nl in (S - 1, S):
        for hit_before in (True, False):
            b = text_frame(LEN1, seed=nl + hit_before)
            blank(b, S - 200, S + 200)
            b[S - 150] = 10; b[nl] = 10; b[S + 150] = 10
            at = nl - 40 if hit_before else nl + 10
            b[at:at + 7] = NEEDLE
            raws.append(bytes(b))
    return raws


def check_boundaries(engine, compress=True):
    raws = boundary_frames()
    packed = sc.pack(engine, raws, compress=compress)
    for kind, what in kinds():
        for before, after in ((0, 2), (2, 0), (3, 3)):
            _, recs, want = check_select(engine, packed, raws, kind, what, before=before, after=after, tag="boundary %d %d %d" % (kind, before, after))
            for i, w in enumerate(want):
                hit = next(x for x in w if x[3] is not None)
                assert sum(x[3] is not None for x in w) == 1 and len(w) == 1 + before + after
                if after and i % 2 == 0: assert hit[0] < S and any(x[0] >= S and x[2] > hit[2] for x in w), i        # context on the far side of the boundary
                if before and i % 2 == 1: assert hit[0] >= S and any(x[0] + x[1] <= S and x[2] < hit[2] for x in w), i


# ---- 2. context across whole slices ---------------------------------------------------------------------------------------------------
def check_whole_slices(engine, compress=True):
    """slice 1 holds three long lines and no hit; `after` from a hit in slice 0 and `before` from a hit in slice 2 meet and overlap in it"""
    b = text_frame(LEN1, seed=3)
    blank(b, S - 500, 2 * S + 500)
    for p in (S - 400, S - 300, S + 20000, S + 40000, S + 60000, 2 * S + 300, 2 * S + 400): b[p] = 10
    b[S - 350:S - 343] = NEEDLE            # the line S-399 .. S-300
    b[2 * S + 350:2 * S + 357] = NEEDLE    # the line 2S+301 .. 2S+400
    raws = [bytes(b)]
    packed = sc.pack(engine, raws, compress=compress)
    for kind, what in kinds():
        for before, after in ((3, 3), (2, 2), (1, 4), (4, 1)):
            _, recs, want = check_select(engine, packed, raws, kind, what, before=before, after=after, tag="whole slices %d" % kind)
            w = want[0]
            assert [x[3] is not None for x in w].count(True) == 2
            inner = [x for x in w if S <= x[0] < 2 * S]
            assert len(inner) >= 2 and len({x[2] for x in w}) == len(w) == len(recs)               # every line once
            assert [x[2] for x in w] == list(range(w[0][2], w[0][2] + len(w)))                       # the two groups have merged


# ---- 3. a line over three slices -----------------------------------------------------------------------------------------------------
def check_long_line(engine, compress=True):
    def frame(needle_in_long, needle_next):
        b = text_frame(LEN1, seed=5)
        blank(b, S - 2000, 2 * S + 2000)
        b[S - 100] = 10; b[2 * S + 500] = 10; b[2 * S + 600] = 10
        if needle_in_long: b[S - 50:S - 43] = NEEDLE; b[2 * S + 50:2 * S + 57] = NEEDLE
        if needle_next: b[2 * S + 520:2 * S + 527] = NEEDLE
        return bytes(b)
    raws = [frame(False, True), frame(False, False), frame(True, False)]
    packed = sc.pack(engine, raws, compress=compress)
    long_line = (S - 99, S + 599)
    for kind, what in kinds():
        # as a context line: the hit is the line behind it
        _, recs, want = check_select(engine, (packed[0][:1], packed[1][:1], packed[2][:1]), raws[:1], kind, what, before=1, tag="long context")
        assert [(x[0], x[1]) for x in want[0]][0] == long_line and want[0][0][3] is None and len(recs) == 2
        # as a hit under INVERT: max_lines cuts behind it
        no = all_lines(raws[1])
        k = next(i for i, x in enumerate(no) if (x[0], x[1]) == long_line)
        _, recs, want = check_select(engine, (packed[0][1:2], packed[1][1:2], packed[2][1:2]), raws[1:2], kind, what, invert=True, max_lines=k + 2, tag="long inverted")
        assert sum((r[1], r[2]) == long_line for r in recs) == 1 and len(recs) == k + 2
        # as a matching context line under INVERT: its match is the lowest, in the first of its slices
        _, recs, want = check_select(engine, (packed[0][2:], packed[1][2:], packed[2][2:]), raws[2:], kind, what, invert=True, before=1, after=1, tag="long matching context")
        mine = [r for r in recs if (r[1], r[2]) == long_line]
        assert len(mine) == 1 and mine[0][4] == S - 50


# ---- 4. merging, 5. frame edges, 6. INVERT: small frames, every matcher ---------------------------------------------------------------
def numbered(hits, n, final_newline=True, empty=()):
    """n lines, the needle in those whose number is in hits, the lines in `empty` empty"""
    body = b"\n".join(b"" if k in empty else (b"row %d " % k + (NEEDLE if k in hits else b"plain")) for k in range(1, n + 1))
    return body + (b"\n" if final_newline else b"")


def check_small(engine, compress=True):
    raws = [
        numbered({5, 7}, 20),                       # hits two lines apart
        numbered({10, 14}, 30),                     # line 12: after-context of one hit and before-context of the next
        numbered({1}, 12),                          # a hit on line 1
        numbered({12}, 12), numbered({12}, 12, final_newline=False),   # a hit on the last line
        numbered(set(), 9),                         # no line matches
        numbered(set(range(1, 10)), 9),             # every line matches
        b"", b"\n", b"\n\n\n",
        numbered({3, 4, 5}, 8, empty={2, 6}),
        NEEDLE, NEEDLE + b"\n", b"\n" + NEEDLE,
    ]
    packed = sc.pack(engine, raws, compress=compress)
    n = {}
    for kind, what in kinds():
        for invert, before, after in ((False, 3, 3), (False, 2, 2), (False, 5, 0), (False, 0, 5), (False, ALL, ALL), (True, 0, 0), (True, 1, 1), (True, ALL, 0),
                                      (False, 0, ALL), (True, 2, 0)):
            res, recs, want = check_select(engine, packed, raws, kind, what, invert=invert, before=before, after=after, tag="small %d %r %d %d" % (kind, invert, before, after))
            n[invert, before, after] = [(r[-2], r[-1]) for r in res]
            if kind == FIXED:                       # count and first are the plain search's under INVERT too
                assert [r[:4] for r in res] == engine.search(packed[0], packed[1], NEEDLE, expect=packed[2])
        assert n[False, 3, 3][0] == (2, 9) and n[False, 2, 2][1] == (2, 9)            # merged groups: hit beats context, no line twice
        assert n[False, 5, 0][2] == (1, 1) and n[False, 0, 5][3] == n[False, 0, 5][4] == (1, 1)
        assert n[False, 0, 5][2] == (1, 6) and n[False, 5, 0][3] == n[False, 5, 0][4] == (1, 6)
        assert [n[False, ALL, ALL][i] for i in (0, 5, 6, 7)] == [(2, 20), (0, 0), (9, 9), (0, 0)]
        assert [n[True, 0, 0][i] for i in (5, 6, 7, 8, 9)] == [(9, 9), (0, 0), (0, 0), (1, 1), (3, 3)]
        assert n[True, 1, 1][10] == (5, 7) and n[True, 1, 1][6] == (0, 0)             # INVERT with context
        assert [n[True, 0, 0][i] for i in (11, 12, 13)] == [(0, 0), (0, 0), (1, 1)]


def check_newlines_only(engine, compress=True):
    """one slice that is 64 KiB of 0x0A: 65 536 empty lines, every one a hit under INVERT; and the same frame one byte and one slice longer"""
    raws = [b"\n" * S, b"\n" * (S + 1), b"\n" * (S - 1) + b"x", b"\n" * (2 * S)]
    packed = sc.pack(engine, raws, compress=compress)
    res, recs, _ = check_select(engine, packed, raws, FIXED, NEEDLE, invert=True, max_line=1, tag="newlines")
    assert [r[-1] for r in res] == [S, S + 1, S, 2 * S] and len(recs) == 5 * S + 1
    res, recs, _ = check_select(engine, packed, raws, REGEX, b"x", invert=True, after=1, max_line=1, max_lines=S - 2, tag="newlines, context")
    assert res[2][-2:] == (S - 1, S) and len(recs) == 4 * (S - 2)        # the line "x" is context
    res, _, _ = check_select(engine, packed, raws, SET, [b"x"], before=ALL, rec_cap=0, tag="newlines, counting")
    assert [r[-2:] for r in res] == [(0, 0), (0, 0), (1, S), (0, 0)]


# ---- 7. equivalence ------------------------------------------------------------------------------------------------------------------
def check_equivalence(engine, corpus, compress=True):
    raws = lc.boundary_frames(corpus) + [b"", b"\n", NEEDLE, numbered({2, 3}, 5)]
    frames, raw_lens, digests = packed = sc.pack(engine, raws, compress=compress)
    # the selection off: the matcher's own lines call, byte for byte (raw records: match is a number in both)
    raw = lambda recs: [(r[0], r[1], r[2], r[3], _lib.SEARCH_NONE if r[4] is None else r[4], r[5]) for r in recs]
    for max_lines, rec_cap in ((0, 1000), (1, 1000), (0, 7)):
        kw = dict(expect=digests, max_lines=max_lines, rec_cap=rec_cap)
        res, recs, _ = engine.select_lines(frames, raw_lens, FIXED, NEEDLE, **kw)
        own = engine.search_lines(frames, raw_lens, NEEDLE, **kw)
        assert ([r[:-1] for r in res], raw(recs)) == own and all(r[-1] == r[-2] for r in res) and len(recs) > 3
        res, recs, hits = engine.select_lines(frames, raw_lens, SET, [NEEDLE, b"row 2"], **kw)
        own = engine.search_set_lines(frames, raw_lens, [NEEDLE, b"row 2"], **kw)
        assert ([r[:-1] for r in res], raw(recs), hits) == own and all(r[-1] == r[-2] for r in res)
        res, recs, _ = engine.select_lines(frames, raw_lens, REGEX, RX + b"|row 2", **kw)
        own = engine.search_regex_lines(frames, raw_lens, RX + b"|row 2", **kw)
        assert ([r[:-1] for r in res], raw(recs)) == own and all(r[-1] == r[-2] for r in res)
    # ... and the keyword arguments of the three lines calls lead to the same entry point
    a = engine.select_lines(frames, raw_lens, FIXED, NEEDLE, expect=digests, invert=True, before=2, after=2, rec_cap=20000)
    assert engine.search_lines(frames, raw_lens, NEEDLE, expect=digests, invert=True, before=2, after=2, rec_cap=20000) == a[:2]
    assert engine.search_regex_lines(frames, raw_lens, RX, expect=digests, invert=True, before=2, after=2, rec_cap=20000) == a[:2]
    b = engine.search_set_lines(frames, raw_lens, [NEEDLE], expect=digests, invert=True, before=2, after=2, rec_cap=20000)
    # the same literal as a fixed string, a set of one and an expression: identical lines, selected and records
    assert [r[-2:] for r in b[0]] == [r[-2:] for r in a[0]] and b[1] == a[1] and len(a[1]) > 1000
    assert [r[:4] for r in b[0]] == [r[:4] for r in a[0]]
    check_select(engine, packed, raws, FIXED, NEEDLE, invert=True, before=2, after=2, tag="-v -C 2")


# ---- 8. the carry's 64-slice step ----------------------------------------------------------------------------------------------------
def check_66_slices(engine, compress=True):
    """one frame of 66 slices; hits placed so that context crosses the boundary between slices 63 and 64 in both directions, and a line
    without a 0x0A in slices 62 .. 64 in a second frame"""
    B = 64 * S
    b = text_frame(66 * S, seed=8)
    blank(b, B - 300, B + 300)
    for p in (B - 250, B - 180, B - 100, B - 1, B + 90, B + 170, B + 260): b[p] = 10
    b[B - 170:B - 163] = NEEDLE            # a hit in slice 63: after-context reaches slice 64
    c = bytearray(b)
    c[B - 170:B - 163] = b"-" * 7
    c[B + 100:B + 107] = NEEDLE            # a hit in slice 64: before-context reaches slice 63
    d = text_frame(66 * S, seed=9)
    blank(d, 62 * S - 100, 65 * S + 300)
    d[65 * S + 110] = 10; d[65 * S + 190] = 10
    d[62 * S + 10:62 * S + 17] = NEEDLE    # one line over slices 61 .. 65, its match in slice 62
    e = bytearray(d)
    e[65 * S + 120:65 * S + 127] = NEEDLE  # a hit in slice 65 right behind it
    e[62 * S + 10:62 * S + 17] = b"-" * 7
    raws = [bytes(b), bytes(c), bytes(d), bytes(e)]
    packed = sc.pack(engine, raws, compress=compress)
    for kind, what in kinds()[:1] + kinds()[2:]:
        _, recs, want = check_select(engine, packed, raws, kind, what, before=3, after=3, tag="66 slices %d" % kind)
        assert any(x[0] >= B for x in want[0]) and want[0][3][0] < B and any(x[0] < B - 1 for x in want[1]) and want[1][3][0] >= B
        assert any(x[1] > 3 * S and x[3] == 62 * S + 10 for x in want[2]) and any(x[1] > 3 * S and x[3] is None for x in want[3])
    res, recs, want = check_select(engine, packed, raws, SET, [NEEDLE], invert=True, before=1, after=1, max_lines=5, tag="66 slices, inverted")
    assert all(r[-1] == len(all_lines(raw)) for r, raw in zip(res, raws)) and len(recs) == 20


# ---- 9. many small frames, undecodable ones among them --------------------------------------------------------------------------------
def check_many_small(engine, oracle, corpus, golden_frames):
    raws = [corpus.entry(4400 + i, (i * 7919) % 2049, i % 4) for i in range(300)]
    assert max(len(r) for r in raws) > 2000
    raws[7] = b""; raws[8] = b"\n"; raws[150] = b""
    needle = lc.small_needle(raws)
    for compress in (True, False):
        packed = sc.pack(engine, raws, compress=compress)
        for kind, what in ((FIXED, needle), (SET, [needle, b"qqqq"]), (REGEX, rc.re.escape(needle))):
            res, recs, _ = check_select(engine, packed, raws, kind, what, before=1, after=2, tag="small frames %d" % kind)
            assert sum(r[-2] == 0 for r in res) > 10 and sum(r[-1] > r[-2] > 0 for r in res) > 10
        res, _, _ = check_select(engine, packed, raws, FIXED, needle, invert=True, after=1, tag="small frames, inverted")
        assert res[7][-2:] == (0, 0) and res[8][-2:] == (1, 1)
    # frames that do not decode: status as verify's, 0 and 0, no record; a DIGEST frame is delivered
    frames, raw_lens, expect, eraws = vc.error_list(oracle, corpus, golden_frames)
    good = [numbered({2}, 6), numbered({5}, 6)]
    gf, gl, gd = sc.pack(engine, good)
    frames, raw_lens, expect, eraws = [gf[0]] + frames + [gf[1]], [gl[0]] + raw_lens + [gl[1]], [gd[0]] + expect + [gd[1]], [good[0]] + eraws + [good[1]]
    verdict = engine.verify(frames, raw_lens, expect)
    res, recs, _ = engine.select_lines(frames, raw_lens, FIXED, NEEDLE, expect=expect, invert=True, after=1, rec_cap=100000)
    assert [(r[1], r[0]) for r in res] == verdict
    decoded = [i for i, r in enumerate(res) if r[0] in DECODED]
    assert 0 in decoded and len(frames) - 1 in decoded and len(decoded) < len(frames) and any(res[i][0] == _lib.FRAME_DIGEST for i in decoded)
    want = [ref_select(eraws[i], FIXED, NEEDLE, invert=True, after=1) if i in decoded else (0, [], None) for i in range(len(frames))]
    assert [r[-2:] for r in res] == [(w[0], len(w[1])) for w in want]
    assert recs == lc.deliver(eraws, [w[1] for w in want])


# ---- 10. caps ------------------------------------------------------------------------------------------------------------------------
def check_caps(engine, compress=True):
    raws = [numbered({4, 30}, 40), numbered({2, 3, 20}, 25, final_newline=False), b"", numbered(set(), 5), numbered({1, 5}, 5)]
    packed = sc.pack(engine, raws, compress=compress)
    full = [len(ref_select(r, FIXED, NEEDLE, before=2, after=2)[1]) for r in raws]
    assert full == [10, 10, 0, 0, 5]
    for kind, what in kinds():
        for max_lines in (0, 1, 4, 7):                                      # 4 and 7 cut inside a context group
            total = sum(min(f, max_lines or f) for f in full)
            for rec_cap in (0, 1, 12, total, total - 1):                    # 12 cuts inside a group of the second frame when nothing else cuts
                res, recs, _ = check_select(engine, packed, raws, kind, what, before=2, after=2, max_lines=max_lines, rec_cap=rec_cap,
                                            tag="caps %d %d %d" % (kind, max_lines, rec_cap))
                assert [r[-1] for r in res] == full and len(recs) == min(total, rec_cap)     # truncation shows as selected[i] above the delivered count
    for max_line in (1, 3, 4096):
        _, recs, _ = check_select(engine, packed, raws, FIXED, NEEDLE, invert=True, before=1, max_line=max_line, tag="max_line %d" % max_line)
        assert all(len(r[5]) == min(r[2], max_line) for r in recs) and len(recs) > 60


# ---- 11. chunking and forms ----------------------------------------------------------------------------------------------------------
def check_bounded_scratch(engine, corpus, compress=True):
    """in the manner of lines_cases.check_bounded_scratch: the remainder of rec_cap crosses the boundaries of the parts"""
    raws = sc.small_entries(corpus, 600) + [corpus.entry(4700 + i, 1 << 20, i) for i in range(3)]
    needle = lc.small_needle(raws)
    packed = sc.pack(engine, raws, compress=compress)
    sel = [len(ref_select(r, FIXED, needle, before=1, after=1)[1]) for r in raws]
    assert sum(sel) > 300 and sel[-3] > 40
    rec_cap = sum(sel[:-3]) + sel[-3] // 2                                  # runs out inside the first large frame
    free = check_select(engine, packed, raws, FIXED, needle, before=1, after=1, rec_cap=rec_cap, tag="budget 0")[:2]
    assert len(free[1]) == rec_cap and free[1][-1][0] == len(raws) - 3
    for mb in (2, 1):
        engine.set_parameter(_lib.PX_SCRATCH_MB, mb)
        try:
            assert check_select(engine, packed, raws, FIXED, needle, before=1, after=1, rec_cap=rec_cap, tag="budget %d" % mb)[:2] == free
            assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in packed[0]), sum(len(r[5]) for r in free[1]))
            assert engine.kernel_ms(_lib.T_LINES) > 0
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
    engine.set_parameter(_lib.PX_STAGE_CHUNK, 1 << 20)                      # the host form in staging chunks of 1 MiB of content
    try:
        assert check_select(engine, packed, raws, FIXED, needle, before=1, after=1, rec_cap=rec_cap, tag="chunked")[:2] == free
    finally:
        engine.set_parameter(_lib.PX_STAGE_CHUNK, 0)


def check_pieces(engine, oracle, corpus, golden_frames):
    """another encoder's frames and a frame of several MiB: frames the decoder cuts in pieces"""
    import os
    import make_golden
    d, m = golden_frames
    raws, frames = [corpus.entry(4500, (2 << 20) + 17, 0)], []
    frames.append(sc.pack(engine, raws)[0][0])
    for name in ("text300", "records200k"):
        fr = next(f for f in m["frames"] if f["recipe"] == name and f["level"] == 3 and f["checksum"] == 1 and f["libzstd"].startswith("1.5"))
        frames.append(open(os.path.join(d, fr["file"]), "rb").read())
        raws.append(make_golden.recipe_bytes(m["recipes"][name], corpus))
    packed = (frames, [len(r) for r in raws], [oracle.blake3(r) for r in raws])
    for i, r in enumerate(raws):
        at = next(k for k in range(len(r) // 2, len(r)) if b"\n" not in r[k:k + 9])
        needle = r[at:at + (9, 3, 6)[i]]
        res, _, _ = check_select(engine, packed, raws, FIXED, needle, before=2, after=1, max_lines=50, max_line=256, rec_cap=120, tag="pieces %d" % i)
        assert res[i][-2] >= 1


def check_device_form(engine, compress=True):
    raws = boundary_frames()[:2] + [numbered({3}, 9), b"", NEEDLE, b"\n" * 300]
    frames, raw_lens, digests = packed = sc.pack(engine, raws, compress=compress)
    host = check_select(engine, packed, raws, FIXED, NEEDLE, invert=True, after=1, max_lines=40, tag="host form")
    h2d, d2h, ring, direct = vc.copy_counters(engine)
    assert (h2d, d2h) == (sum(len(f) for f in frames), sum(len(r[5]) for r in host[1])) and d2h > 0       # D2H == text_used
    assert engine.kernel_ms(_lib.T_LINES) > 0 and engine.kernel_ms(_lib.T_TOTAL) >= engine.kernel_ms(_lib.T_LINES)
    d_frames, foff, _ = vc._arena(engine, frames)
    try:
        exp = np.frombuffer(b"".join(digests), dtype=np.uint8)
        for kind, what in kinds():
            dev_call = lambda **kw: engine.select_lines_device(d_frames, foff, [len(f) for f in frames], raw_lens, kind, what, expect=exp, **kw)
            for kw in (dict(invert=True, after=1, max_lines=40), dict(before=2, after=2), dict(invert=True, rec_cap=5), dict(after=ALL, max_line=9, icase=True)):
                dev = check_select(engine, packed, raws, kind, what, tag="device form %d %r" % (kind, kw), call=dev_call, **kw)
                assert vc.copy_counters(engine) == (0, 0, 0, 0) and engine.kernel_ms(_lib.T_LINES) > 0
                assert dev[:2] == check_select(engine, packed, raws, kind, what, tag="host form %d %r" % (kind, kw), **kw)[:2]
        a = engine.search_lines_device(d_frames, foff, [len(f) for f in frames], raw_lens, NEEDLE, expect=exp, invert=True, after=1, max_lines=40, rec_cap=len(host[1]) + 1)
        assert a == host[:2]
    finally:
        engine.free(d_frames)
    engine.search_lines(frames, raw_lens, NEEDLE, expect=digests)
    assert engine.kernel_ms(_lib.T_LINES) > 0
    engine.search(frames, raw_lens, NEEDLE, expect=digests)
    assert engine.kernel_ms(_lib.T_LINES) in (0.0, -1.0)


def raw_call(engine, packed, matcher, select, max_lines=0, max_line=4096, rec_cap=4, text_cap=None, with_set=False, n=None, frame_len=None, **null):
    """zarc_gpu_select_lines_batch through ctypes; matcher / select: the structures or None; null: names of arguments to pass as NULL.
    -> (rc, rec_used, text_used, lines, selected)"""
    c = ctypes
    frames, raw_lens, _ = packed
    ptrs, lens = vc._ptrs(frames)
    if frame_len is not None: lens = (c.c_size_t * len(frames))(*frame_len)
    rl = (c.c_size_t * len(frames))(*raw_lens)
    dig = np.zeros((len(frames), 32), dtype=np.uint8)
    k = len(frames)
    st, cnt, fst, which, hits, lines, sel = (c.c_int * k)(), (c.c_uint64 * k)(), (c.c_uint64 * k)(), (c.c_uint64 * k)(), (c.c_uint64 * 8)(), (c.c_uint64 * k)(), (c.c_uint64 * k)()
    rec = (_lib.Line * max(rec_cap, 1))()
    text = np.zeros(max(rec_cap * min(max_line, 65536), 1), dtype=np.uint8)
    ru, tu = c.c_size_t(77), c.c_size_t(77)
    a = dict(ptrs=ptrs, lens=lens, rl=rl, dig=dig.ctypes.data_as(c.c_void_p), st=st, cnt=cnt, fst=fst, which=which if with_set else None, hits=hits if with_set else None,
             lines=lines, sel=sel, rec=rec, ru=c.byref(ru), text=text.ctypes.data_as(c.c_void_p), tu=c.byref(tu))
    for key in null: a[key] = None
    rc_ = engine.lib.zarc_gpu_select_lines_batch(engine.h, len(frames) if n is None else n, a["ptrs"], a["lens"], a["rl"], None,
                                                 c.byref(matcher) if matcher is not None else None, c.byref(select) if select is not None else None, max_lines, max_line,
                                                 a["dig"], a["st"], a["cnt"], a["fst"], a["which"], a["hits"], a["lines"], a["sel"], a["rec"], rec_cap, a["ru"], a["text"],
                                                 rec_cap * max_line if text_cap is None else text_cap, a["tu"])
    return rc_, ru.value, tu.value, list(lines), list(sel)


def check_arguments(engine):
    raw = numbered({3}, 9)
    packed = sc.pack(engine, [raw])
    M, Q, P = _lib.MatcherDesc.of, _lib.LineSelect, _lib.E_PARAM
    fixed, q = M(FIXED, NEEDLE), Q(0, 1, 1, 0)
    ok = raw_call(engine, packed, fixed, q)
    assert ok == (_lib.OK, 3, sum(x[1] for x in ref_select(raw, FIXED, NEEDLE, before=1, after=1)[1]), [1], [3])
    # the selection's own checks
    assert [raw_call(engine, packed, fixed, s)[0] for s in (Q(2, 0, 0, 0), Q(0x80000001, 0, 0, 0), Q(0, 0, 0, 1), None)] == [P] * 4
    assert raw_call(engine, packed, fixed, q, sel=None)[0] == P and raw_call(engine, packed, None, q)[0] == P
    assert raw_call(engine, packed, M(3, NEEDLE), q)[0] == P
    assert b"select" in engine.lib.zarc_gpu_last_error(engine.h)
    assert raw_call(engine, packed, fixed, Q(1, ALL, ALL, 0), rec_cap=16)[:2] == (_lib.OK, 9)
    # which and hits: a set's, NULL or not; nobody else's
    assert raw_call(engine, packed, M(SET, [NEEDLE, b"row"]), q, with_set=True)[0] == raw_call(engine, packed, M(SET, [NEEDLE]), q)[0] == _lib.OK
    assert raw_call(engine, packed, fixed, q, with_set=True)[0] == raw_call(engine, packed, M(REGEX, RX), q, with_set=True)[0] == P
    # the matcher's own lines call refuses first, with its code and message
    assert [raw_call(engine, packed, m, q)[0] for m in (M(FIXED, b""), M(FIXED, b"p" * 257), M(FIXED, b"a\nb"), M(FIXED, NEEDLE, 2), M(SET, []), M(SET, [b"a\n"]),
                                                       M(REGEX, b"a*"), M(REGEX, b"("), M(REGEX, b"x\\n"))] == [P] * 9
    assert raw_call(engine, packed, M(REGEX, b"("), q)[0] == P and b"regex: offset" in engine.lib.zarc_gpu_last_error(engine.h)
    assert raw_call(engine, packed, M(REGEX, b".{7}a"), q)[0] == _lib.E_UNSUPPORTED
    assert raw_call(engine, packed, M(FIXED, b"a\nb"), Q(2, 0, 0, 0))[0] == P and b"newline" in engine.lib.zarc_gpu_last_error(engine.h)   # in the matcher's order
    assert [raw_call(engine, packed, fixed, q, **{k: None})[0] for k in ("lines", "ru", "tu", "rec", "text", "st", "cnt", "fst", "dig", "ptrs", "lens", "rl")] == [P] * 12
    assert [raw_call(engine, packed, fixed, q, max_line=v)[0] for v in (0, 65537)] == [P] * 2
    assert raw_call(engine, packed, fixed, q, rec_cap=5, max_line=16, text_cap=79)[0] == _lib.E_DSTSIZE
    assert raw_call(engine, packed, fixed, Q(1, 0, 0, 0), rec_cap=0, rec=None, text=None) == (_lib.OK, 0, 0, [8], [8])       # a counting call
    assert raw_call(engine, packed, fixed, q, n=0, ptrs=None, lens=None, rl=None)[:3] == (_lib.OK, 0, 0)
    assert raw_call(engine, packed, fixed, q, frame_len=[0xFFFFFFF0])[0] == _lib.E_UNSUPPORTED
    # the device form refuses the same
    c = ctypes
    u64 = lambda v: (c.c_uint64 * 1)(v)
    dig = np.zeros((1, 32), dtype=np.uint8)
    st, cnt, fst, lines, sel = (c.c_int * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)()
    rec, ru, tu = (_lib.Line * 4)(), c.c_size_t(), c.c_size_t()
    dummy = c.c_void_p(16)  # never dereferenced: the call is refused before

    def dev(n=1, base=dummy, m=fixed, s=q, sel=sel, which=None, text_cap=64, rl=u64(0)):
        return engine.lib.zarc_gpu_select_lines_batch_device(engine.h, n, base, u64(0), u64(9), rl, None, c.byref(m) if m is not None else None,
                                                             c.byref(s) if s is not None else None, 0, 16, dig.ctypes.data_as(c.c_void_p), st, cnt, fst, which, None,
                                                             lines, sel, rec, 4, c.byref(ru), dummy, text_cap, c.byref(tu))
    assert dev(n=0, base=None) == _lib.OK
    assert dev(base=None) == dev(m=None) == dev(s=None) == dev(sel=None) == dev(s=Q(4, 0, 0, 0)) == dev(s=Q(0, 0, 0, 7)) == dev(which=cnt) == dev(m=M(9, b"x")) == P
    assert dev(text_cap=63) == _lib.E_DSTSIZE and dev(rl=u64(0xFFFFFFF0)) == _lib.E_UNSUPPORTED
    # ... and the handle still works
    assert raw_call(engine, packed, fixed, q) == ok
