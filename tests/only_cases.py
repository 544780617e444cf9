"""Checks of zarc_gpu_search_matches_batch* (grep -o: every match of a matching line, cut out on the device), shared by the emulator tests
(test_only.py) and the GPU tests (test_gpu_only.py).

The reference of every expected value is Python on the bytes the frames were packed from -- never the engine.  Per line, S = the matching
start positions (FIXED / SET: compared bytes; REGEX: regex_cases.positions), E(s) = the match's end, and the matches are grep -o's loop:
c = the line's start; p = the lowest s in S with s >= c; the match is (p, E(p) - p); c = E(p).  For a regex, E(s) is the largest j for which
    re.compile(b"(?:" + R + b")(?=[^\\n]{%d}\\Z)" % (len(line) - j)).match(line, s)
succeeds: the whole line is passed and pos = s, so `^` and `$` keep their real meaning (compared with GNU grep 3.7 -o -b -a -E: no
difference).  Every comparison is equality, and every scenario asserts on the reference side that it is not vacuous."""
import ctypes
import functools
import re

import numpy as np

import lines_cases as lc
import regex_cases as rc
import search_cases as sc
import select_cases as sel
import set_cut_cases as cut
import verify_cases as vc
from zarc_amd import _lib

S = sc.SLICE
NEEDLE = sc.NEEDLE7
LEN1 = 3 * S + 1000
FIXED, SET, REGEX = _lib.MATCH_FIXED, _lib.MATCH_SET, _lib.MATCH_REGEX
RX = re.escape(NEEDLE)
DECODED = (_lib.FRAME_OK, _lib.FRAME_DIGEST)


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def fold(b):
    return bytes(c | 0x20 if 0x41 <= c <= 0x5A else c for c in b)


@functools.lru_cache(maxsize=None)
def _end_prog(rx, icase, behind):
    return re.compile(b"(?:" + rx + b")(?=[^\n]{%d}\\Z)" % behind, re.I if icase else 0)


def regex_end(line, s, rx, icase=False, ends=None):
    """E(s) in the line, or None.  ends: the candidate ends, descending (default: every j in (s, len(line)]) -- a case may narrow them where
    it says why; each candidate is still tried with the expression above"""
    for j in (ends(line, s) if ends else range(len(line), s, -1)):
        if _end_prog(rx, icase, len(line) - j).match(line, s): return j
    return None


def line_matches(line, kind, what, icase=False, starts=None, ends=None):
    """-> [(start, length, which)] of one line, positions from the line's first byte"""
    text = fold(line) if icase and kind != REGEX else line
    if kind == REGEX:
        S_ = rc.positions(line, what, icase) if starts is None else starts(line)
        end_of = lambda s: (regex_end(line, s, what, icase, ends), None)
    else:
        pats = [fold(p) if icase else bytes(p) for p in ([what] if kind == FIXED else what)]
        at = lambda s: [k for k, p in enumerate(pats) if text.startswith(p, s)]
        S_ = [m.start() for m in re.finditer(b"(?=" + b"|".join(re.escape(p) for p in pats if p) + b")", text)] if any(pats) else []

        def end_of(s):
            longest = max(len(pats[k]) for k in at(s))
            return s + longest, (min(k for k in at(s) if len(pats[k]) == longest) if kind == SET else None)
    out, c = [], 0
    for s in S_:
        if s < c: continue
        e, which = end_of(s)
        assert e is not None and e > s, (line[:40], s)          # a matching start position has an end behind it
        out.append((s, e - s, which))
        c = e
    return out


def ref_frame(d, kind, what, icase=False, **how):
    """-> the matching lines of a frame: [(line start, line length, number, [(start, length, which)])], positions in the frame"""
    out = []
    for ls, ll, no in sel.all_lines(d):
        m = line_matches(d[ls:ls + ll], kind, what, icase, **how)
        if m: out.append((ls, ll, no, [(ls + s, l, w) for s, l, w in m]))
    return out


def deliver(raws, want, max_lines=0, max_line=4096, line_cap=None, rec_cap=None):
    """the two delivery rules -> (matches[i], records)"""
    lines_left = sum(len(w) for w in want) if line_cap is None else line_cap
    matches, recs = [], []
    for i, w in enumerate(want):
        d = min(len(w), max_lines or len(w), lines_left)
        lines_left -= d
        mine = [(i, s, l, no, ls, which, raws[i][s:s + min(l, max_line)]) for ls, _, no, ms in w[:d] for s, l, which in ms]
        matches.append(len(mine))
        recs += mine
    return matches, (recs if rec_cap is None else recs[:rec_cap])


def call_host(engine, packed, kind, what):
    frames, raw_lens, digests = packed
    return lambda **kw: engine.search_matches(frames, raw_lens, kind, what, expect=digests, **kw)


def check_only(engine, packed, raws, kind, what, icase=False, max_lines=0, max_line=4096, line_cap=None, rec_cap=None, tag="", call=None, plain=True, **how):
    """one search_matches call over a packed batch of good frames against the reference.  line_cap / rec_cap None: room for everything.
    -> (results, records, the reference's matching lines per frame)"""
    digests = packed[2]
    want = [ref_frame(r, kind, what, icase, **how) for r in raws]
    lcap = sum(len(w) for w in want) + 1 if line_cap is None else line_cap
    rcap = sum(len(ms) for w in want for _, _, _, ms in w) + 1 if rec_cap is None else rec_cap
    call = call or call_host(engine, packed, kind, what)
    results, records, _ = call(icase=icase, max_lines=max_lines, max_line=max_line, line_cap=lcap, rec_cap=rcap)
    matches, exp = deliver(raws, want, max_lines, max_line, lcap, rcap)
    assert len(results) == len(raws)
    for i, res in enumerate(results):
        assert res[0] == _lib.FRAME_OK and res[1] == digests[i], (tag, i, res[0])
        if plain: assert tuple(res[2:-2]) == tuple(sel.matching(raws[i], kind, what, icase)[1]), (tag, i, res[2:-2])      # count, first[, which]: the plain search's
        assert (res[-2], res[-1]) == (len(want[i]), matches[i]), (tag, i, res[-2:], len(want[i]), matches[i])
    assert len(records) == len(exp), (tag, len(records), len(exp))
    for g, e in zip(records, exp):
        assert g == e, (tag, g, e)
    return results, records, want


def kinds():
    return ((FIXED, NEEDLE), (SET, [NEEDLE]), (REGEX, RX))


def n_matches(want):
    return sum(len(ms) for w in want for _, _, _, ms in w)


# ---- 1. leftmost-longest -------------------------------------------------------------------------------------------------------------
SMALL = (b"ab a abab xabcd abcdc\naaa\nab\r\ntook 15 ms\ntook 7 ms and 12 ms\nxAbaB\nabab aab\naaaaa\na--b--a--b\n\nzab\r\nb\n"
         b"ababab ab abab\ncabcd\nno digits ms\n9 ms")
REGEXES = (b"a|ab", b"abcd|c", b"b|abcd|ab", b"(ab)+", b"a.*b", b"[0-9]+ ms$", b"^a", b"b.$")


def check_leftmost_longest(engine, compress=True):
    raws = [SMALL, b"aaa", b"ab\r\n"]
    packed = sc.pack(engine, raws, compress=compress)
    texts = {}
    for rx in REGEXES:
        _, recs, want = check_only(engine, packed, raws, REGEX, rx, tag="longest %r" % rx)
        assert n_matches(want) >= 2, rx
        texts[rx] = [r[6] for r in recs if r[0] == 0]
    assert b"ab" in texts[b"a|ab"] and b"abcd" in texts[b"abcd|c"] and b"abcd" in texts[b"b|abcd|ab"]      # the longer alternative wins, wherever it stands
    assert b"ababab" in texts[b"(ab)+"] and b"a--b--a--b" in texts[b"a.*b"] and texts[b"[0-9]+ ms$"] == [b"15 ms", b"12 ms", b"9 ms"]
    assert [m for _, _, _, ms in ref_frame(b"aaa", REGEX, b"^a") for m in ms] == [(0, 1, None)]            # ^ holds at the line's first byte only: one match
    assert [m for _, _, _, ms in ref_frame(b"ab\r\n", REGEX, b"b.$") for m in ms] == [(1, 2, None)]        # the 0x0D is the line's last byte
    _, recs, want = check_only(engine, packed, raws, FIXED, b"aa", tag="fixed aa")
    assert [(s - ls, l) for ls, ll, _, ms in want[0] if SMALL[ls:ls + ll] == b"aaaaa" for s, l, _ in ms] == [(0, 2), (2, 2)]
    _, recs, want = check_only(engine, packed, raws, SET, [b"a", b"ab", b"aab"], tag="set")
    assert [(s - ls, l, w) for ls, _, no, ms in want[0] if no == 7 for s, l, w in ms] == [(0, 2, 1), (2, 2, 1), (5, 3, 2)]
    _, recs, want = check_only(engine, packed, raws, SET, [b"ab", b"a", b"ab", b"abab"], tag="set, duplicates")       # the lowest index of the longest
    assert {w for _, _, _, ms in want[0] for _, _, w in ms} == {0, 1, 3}
    _, recs, want = check_only(engine, packed, raws, FIXED, b"ab", icase=True, tag="icase")
    assert [r[6] for r in recs if r[3] == 6 and r[0] == 0] == [b"Ab", b"aB"]
    check_only(engine, packed, raws, REGEX, b"a[b-c]", icase=True, tag="icase regex")
    check_only(engine, packed, raws, SET, [b"AB", b"b"], icase=True, tag="icase set")


# ---- 2. the slice boundary -----------------------------------------------------------------------------------------------------------
def boundary_frames():
    """per frame one planted token: straddling position S, ending at S - 1 (its last byte is S - 2), ending at S, starting at S; and all
    four forms of the variable-length token Q<digits>Q"""
    raws = []
    for token in (NEEDLE, b"Q0123456789Q"):
        for at in (S - 3, S - 1 - len(token), S - len(token), S):
            b = sel.text_frame(LEN1, seed=at % 97)
            b[at:at + len(token)] = token
            tail = 2 * S + 77                                   # a second one in another slice of the same frame
            b[tail:tail + len(token)] = token
            raws.append(bytes(b))
    return raws


def check_boundaries(engine, compress=True):
    raws = boundary_frames()
    packed = sc.pack(engine, raws, compress=compress)
    for kind, what in kinds() + ((REGEX, b"Q[0-9]+Q"), (SET, [b"Q0", NEEDLE, b"Q0123456789Q"])):
        _, recs, want = check_only(engine, packed, raws, kind, what, tag="boundary %d %r" % (kind, what))
        hit = [i for i, w in enumerate(want) if w]
        assert len(hit) == (8 if kind == SET and len(what) > 1 else 4) and all(n_matches([want[i]]) == 2 for i in hit)
        first = [want[i][0][3][0] for i in hit]
        assert [(s < S < s + l, s + l == S - 1, s + l == S, s == S) for s, l, _ in first] == [(True, False, False, False), (False, True, False, False),
                                                                                             (False, False, True, False), (False, False, False, True)] * (len(hit) // 4)


# ---- 3. the frame's end ---------------------------------------------------------------------------------------------------------------
def check_frame_end(engine, compress=True):
    raws = [b"one\nfoo bar", b"tail " + NEEDLE[:4], NEEDLE[4:] + b" head\n", b"xabcd\nxab", b"xabc", NEEDLE]
    packed = sc.pack(engine, raws, compress=compress)
    for kind, what in ((REGEX, b"bar$"), (REGEX, b"ba.$|o+"), (FIXED, b"bar")):
        _, _, want = check_only(engine, packed, raws, kind, what, tag="last line %r" % what)
        s, l, _ = want[0][-1][3][-1]
        assert s + l == len(raws[0]) and not raws[0].endswith(b"\n")            # the match ends at the frame's last byte
    for kind, what in kinds():                                                    # the pattern cut off by the frame's end, its rest in the next frame
        res, _, want = check_only(engine, packed, raws, kind, what, tag="cut off %d" % kind)
        assert (raws[1] + raws[2]).count(NEEDLE) == 1 and [r[-1] for r in res] == [0, 0, 0, 0, 0, 1]
    _, _, want = check_only(engine, packed, raws, SET, [b"abcd", b"ab"], tag="only the shorter fits")
    assert [[(s, l, w) for _, _, _, ms in w for s, l, w in ms] for w in want[3:5]] == [[(1, 4, 0), (7, 2, 1)], [(1, 2, 1)]]


# ---- 4. a line over three slices ------------------------------------------------------------------------------------------------------
def check_long_line(engine, compress=True):
    n = 1100
    body = b"".join(b"id=%04d " % k + b"abcdefghijklmnopqrstuvwxy"[:(k * 7) % 25] * 14 + b"." * 14 for k in range(n))
    body = body[:LEN1]
    raws = [b"short id=1 line\n" + body + b"\nend id=7 id=88\n"]
    packed = sc.pack(engine, raws, compress=compress)
    near = lambda line, s: range(min(len(line), s + 16), s, -1)                  # id=[0-9]+ reads at most 3 + 4 digits here
    for kind, what, how in ((REGEX, b"id=[0-9]+", dict(ends=near)), (FIXED, b"id=", {}), (SET, [b"id=", b"id=0", b"id=01"], {})):
        _, recs, want = check_only(engine, packed, raws, kind, what, tag="long line %d" % kind, **how)
        long_ = next(w for w in want[0] if w[1] == len(body))
        assert len(long_[3]) > 950 and len(body) == LEN1 and len(want[0]) == 3
        assert long_[3][0][0] < S and long_[3][-1][0] > 3 * S
    # the adversarial line: behind its one match no position starts a match, and a walk from any of them would reach the line's end
    line = b"az" + b"a" * (3 * S)
    raws = [line, b"x\n" + line + b"\naz\n"]
    packed = sc.pack(engine, raws, compress=compress)
    # every word of L(a[^z]*z) ends in z: starts lie in front of the line's last z, ends behind a z
    starts = lambda ln: rc.positions(ln[:ln.rfind(b"z") + 1], b"a[^z]*z")
    ends = lambda ln, s: [j for j in range(len(ln), s, -1) if ln[j - 1:j] == b"z"]
    plain = [(1, 0), (2, 2)]
    res, recs, want = check_only(engine, packed, raws, REGEX, b"a[^z]*z", tag="adversarial", plain=False, starts=starts, ends=ends)
    assert [tuple(r[2:4]) for r in res] == plain and [r[-2:] for r in res] == [(1, 1), (2, 2)]
    assert [(r[0], r[1], r[2]) for r in recs] == [(0, 0, 2), (1, 2, 2), (1, len(line) + 3, 2)]


# ---- 5. equivalences ------------------------------------------------------------------------------------------------------------------
def check_equivalences(engine, corpus, compress=True):
    raws = lc.boundary_frames(corpus) + [b"", b"\n", NEEDLE, sel.numbered({2, 3}, 5), NEEDLE * 3 + b" " + NEEDLE + b"\n" + NEEDLE]
    frames, raw_lens, digests = packed = sc.pack(engine, raws, compress=compress)
    fixed = check_only(engine, packed, raws, FIXED, NEEDLE, tag="fixed")
    as_rx = check_only(engine, packed, raws, REGEX, RX, tag="a literal as an expression")
    as_set = check_only(engine, packed, raws, SET, [NEEDLE], tag="a set of one")
    assert n_matches(fixed[2]) > 20 and as_rx[:2] == fixed[:2]
    assert [r[:4] + r[5:] for r in as_set[0]] == fixed[0] and [r[:5] + (None,) + r[6:] for r in as_set[1]] == fixed[1] and all(r[5] == 0 for r in as_set[1])
    # lines, count, first are the plain lines call's; every delivered line's first match starts at the line's `match`
    for kind, what, own in ((FIXED, NEEDLE, engine.search_lines(frames, raw_lens, NEEDLE, expect=digests, rec_cap=10000)),
                            (REGEX, RX + b"|row [0-9]", engine.search_regex_lines(frames, raw_lens, RX + b"|row [0-9]", expect=digests, rec_cap=10000)),
                            (SET, [NEEDLE, b"row"], engine.search_set_lines(frames, raw_lens, [NEEDLE, b"row"], expect=digests, rec_cap=10000)[:2])):
        res, recs, _ = engine.search_matches(frames, raw_lens, kind, what, expect=digests, line_cap=10000, rec_cap=100000)
        assert [r[:-1] for r in res] == own[0] and len(own[1]) > 10
        firsts = {}
        for r in recs: firsts.setdefault((r[0], r[4]), r[1])
        assert firsts == {(l[0], l[1]): l[4] for l in own[1]}
    # everything delivered, a pattern that cannot overlap itself: as many matches as matching start positions
    assert sum(r[-1] for r in fixed[0]) == sum(r[2] for r in fixed[0]) > 20


# ---- 6. caps --------------------------------------------------------------------------------------------------------------------------
def caps_frames():
    row = lambda k, hits: b"row %d " % k + b" ".join([NEEDLE] * hits) + b" end"
    mk = lambda spec: b"\n".join(row(k, h) for k, h in enumerate(spec, 1)) + b"\n"
    return [mk((0, 2, 0, 3, 1, 0, 4)), mk((1, 1, 1)), b"", mk((0, 0)), mk((5, 0, 2))]       # matching lines 4, 3, 0, 0, 2; matches 10, 3, 0, 0, 7


def check_caps(engine, compress=True):
    raws = caps_frames()
    packed = sc.pack(engine, raws, compress=compress)
    full = [(len(w), n_matches([w])) for w in (ref_frame(r, FIXED, NEEDLE) for r in raws)]
    assert full == [(4, 10), (3, 3), (0, 0), (0, 0), (2, 7)]
    for kind, what in kinds():
        for max_lines in (0, 1, 3):
            for line_cap in (None, 0, 5, 6):                                  # 5 and 6 run out inside the second frame
                for rec_cap in (None, 0, 1, 4, 11, 12):                       # 1 and 4 cut inside a line of the first frame, 11 and 12 inside the second frame
                    res, recs, _ = check_only(engine, packed, raws, kind, what, max_lines=max_lines, line_cap=line_cap, rec_cap=rec_cap,
                                              tag="caps %d %r %r %r" % (kind, max_lines, line_cap, rec_cap))
                    assert [r[-2] for r in res] == [f[0] for f in full]            # lines[i]: all of them whatever the caps
                    if line_cap == 0: assert [r[-1] for r in res] == [0] * 5 and recs == []
    res, recs, _ = check_only(engine, packed, raws, FIXED, NEEDLE, rec_cap=4, tag="a cut inside a line")
    assert [r[3] for r in recs] == [2, 2, 4, 4] and res[0][-1] == 10           # line 4 holds three matches: two of them delivered; matches[i] whatever rec_cap
    for max_line in (1, 3, 7, 4096):
        _, recs, _ = check_only(engine, packed, raws, REGEX, RX + b"( " + RX + b")*", max_line=max_line, tag="max_line %d" % max_line)
        assert all(len(r[6]) == min(r[2], max_line) for r in recs) and max(r[2] for r in recs) == 39 and len(recs) == 9     # length whole, text cut
    # counting calls: rec and text may be NULL
    assert raw_call(engine, packed, _lib.MatcherDesc.of(FIXED, NEEDLE), line_cap=100, rec_cap=0, rec=None, text=None) == (_lib.OK, 0, 0, [4, 3, 0, 0, 2], [10, 3, 0, 0, 7])
    assert raw_call(engine, packed, _lib.MatcherDesc.of(FIXED, NEEDLE), line_cap=0, rec=None, text=None) == (_lib.OK, 0, 0, [4, 3, 0, 0, 2], [0] * 5)
    # both E_DSTSIZE rules
    assert raw_call(engine, packed, _lib.MatcherDesc.of(FIXED, NEEDLE), rec_cap=5, max_line=16, text_cap=79)[0] == _lib.E_DSTSIZE
    assert raw_call(engine, packed, _lib.MatcherDesc.of(FIXED, NEEDLE), rec_cap=2 ** 62, max_line=16, text_cap=2 ** 63, rec=None, text=None)[0] == _lib.E_DSTSIZE
    assert raw_call(engine, packed, _lib.MatcherDesc.of(FIXED, NEEDLE), rec_cap=5, max_line=16, text_cap=80)[:2] == (_lib.OK, 5)


# ---- 7. cuts --------------------------------------------------------------------------------------------------------------------------
def check_cut_invariance(engine, corpus, compress=True):
    """the batch of set_cut_cases: max_lines is 40 and every frame has more matching lines, so line_cap = 255 runs out in the seventh frame
    and rec_cap cuts inside it as well: the remainders of both caps and the text offset cross every cut"""
    raws = [corpus.entry(6600 + i, k * 1024, 0) for i, k in enumerate(cut.KIB)]
    packed = frames, raw_lens, digests = sc.pack(engine, raws, compress=compress)
    d_frames, foff, _ = vc._arena(engine, frames)
    try:
        exp = np.frombuffer(b"".join(digests), dtype=np.uint8)
        word = lambda ln, s: range(min(len(ln), s + 41), s, -1)               # [a-z]+cr and its blank lie inside 41 bytes: no word of the text has 40
        assert all(len(w) < 40 for r in raws for w in re.findall(rb"[a-z]+", r))
        for kind, what, cuts in ((SET, cut.PATTERNS, ((1, 0), (0, 650000), (1, 1300000))), (REGEX, b"[a-z]+cr ", ((1, 650000),)), (FIXED, b"e ", ((1, 1300000),))):
            how = dict(ends=word) if kind == REGEX else {}
            want = [ref_frame(r, kind, what, **how) for r in raws]
            total = deliver(raws, want, 40, 4096, 255, None)[0]
            kw = dict(max_lines=40, line_cap=255, rec_cap=sum(total) - total[6] // 2)
            free = check_only(engine, packed, raws, kind, what, tag="uncut %d" % kind, **kw, **how)[:2]
            assert all(len(w) > 40 for w in want) and total[6] > 2 and total[7] == 0 and free[1][-1][0] == 6 and len(free[1]) == kw["rec_cap"]
            assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in frames), sum(len(r[6]) for r in free[1]))       # D2H == text_used
            assert engine.kernel_ms(_lib.T_LINES) > 0
            for mb, chunk in cuts:
                engine.set_parameter(_lib.PX_SCRATCH_MB, mb)
                engine.set_parameter(_lib.PX_STAGE_CHUNK, chunk)
                try:
                    assert engine.search_matches(frames, raw_lens, kind, what, expect=digests, **kw)[:2] == free, ("host form", kind, mb, chunk)
                    assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in frames), sum(len(r[6]) for r in free[1]))
                    dev = engine.search_matches_device(d_frames, foff, [len(f) for f in frames], raw_lens, kind, what, expect=exp, **kw)
                    assert dev[:2] == free, ("device form", kind, mb)
                    assert vc.copy_counters(engine) == (0, 0, 0, 0)
                finally:
                    engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
                    engine.set_parameter(_lib.PX_STAGE_CHUNK, 0)
    finally:
        engine.free(d_frames)


# ---- 8. many small frames, undecodable ones among them --------------------------------------------------------------------------------
def check_many_small(engine, oracle, corpus, golden_frames):
    raws = [corpus.entry(4400 + i, (i * 7919) % 2049, i % 4) for i in range(300)]
    raws[7] = b""; raws[8] = b"\n"; raws[150] = b""
    needle = lc.small_needle(raws)
    packed = sc.pack(engine, raws)
    for kind, what in ((FIXED, needle), (SET, [needle, needle[:2], b"qqqq"]), (REGEX, re.escape(needle) + b"+")):
        res, recs, want = check_only(engine, packed, raws, kind, what, tag="small frames %d" % kind)
        assert sum(r[-1] == 0 for r in res) > 10 and sum(r[-1] > r[-2] > 0 for r in res) > 10
    # frames that do not decode: status as verify's, 0 matches, no record; a DIGEST frame is delivered
    frames, raw_lens, expect, eraws = vc.error_list(oracle, corpus, golden_frames)
    good = [sel.numbered({2}, 6), sel.numbered({5}, 6)]
    gf, gl, gd = sc.pack(engine, good)
    frames, raw_lens, expect, eraws = [gf[0]] + frames + [gf[1]], [gl[0]] + raw_lens + [gl[1]], [gd[0]] + expect + [gd[1]], [good[0]] + eraws + [good[1]]
    at = next(k for k in range(100, len(eraws[1])) if b"\n" not in eraws[1][k:k + 3])
    word = b"row|" + re.escape(eraws[1][at:at + 3])
    short = lambda ln, s: range(min(len(ln), s + 3), s, -1)          # either alternative has three bytes
    verdict = engine.verify(frames, raw_lens, expect)
    res, recs, _ = engine.search_matches(frames, raw_lens, REGEX, word, expect=expect, line_cap=100000, rec_cap=400000)
    assert [(r[1], r[0]) for r in res] == verdict
    decoded = [i for i, r in enumerate(res) if r[0] in DECODED]
    assert 0 in decoded and len(frames) - 1 in decoded and len(decoded) < len(frames) and any(res[i][0] == _lib.FRAME_DIGEST for i in decoded)
    want = [ref_frame(eraws[i], REGEX, word, ends=short) if i in decoded else [] for i in range(len(frames))]
    matches, exp = deliver(eraws, want)
    assert [r[-2:] for r in res] == [(len(w), m) for w, m in zip(want, matches)] and matches[0] == 6 and matches[1] > 6
    assert all(res[i][2:] == (0, None, 0, 0) for i in range(len(frames)) if i not in decoded)
    assert recs == exp


# ---- 9. arguments ---------------------------------------------------------------------------------------------------------------------
def raw_call(engine, packed, matcher, max_lines=0, max_line=4096, line_cap=4, rec_cap=4, text_cap=None, with_set=False, n=None, frame_len=None, **null):
    """zarc_gpu_search_matches_batch through ctypes; matcher: the structure or None; null: names of arguments to pass as NULL.
    -> (rc, rec_used, text_used, lines, matches)"""
    c = ctypes
    frames, raw_lens, _ = packed
    ptrs, lens = vc._ptrs(frames)
    if frame_len is not None: lens = (c.c_size_t * len(frames))(*frame_len)
    rl = (c.c_size_t * len(frames))(*raw_lens)
    k = len(frames)
    dig = np.zeros((k, 32), dtype=np.uint8)
    st, cnt, fst, which, hits, lines, mts = (c.c_int * k)(), (c.c_uint64 * k)(), (c.c_uint64 * k)(), (c.c_uint64 * k)(), (c.c_uint64 * 8)(), (c.c_uint64 * k)(), (c.c_uint64 * k)()
    small = min(rec_cap, 64)
    rec = (_lib.Match * max(small, 1))()
    text = np.zeros(max(small * min(max_line, 65536), 1), dtype=np.uint8)
    ru, tu = c.c_size_t(77), c.c_size_t(77)
    a = dict(ptrs=ptrs, lens=lens, rl=rl, dig=dig.ctypes.data_as(c.c_void_p), st=st, cnt=cnt, fst=fst, which=which if with_set else None, hits=hits if with_set else None,
             lines=lines, mts=mts, rec=rec, ru=c.byref(ru), text=text.ctypes.data_as(c.c_void_p), tu=c.byref(tu))
    for key in null: a[key] = None
    rc_ = engine.lib.zarc_gpu_search_matches_batch(engine.h, k if n is None else n, a["ptrs"], a["lens"], a["rl"], None, c.byref(matcher) if matcher is not None else None,
                                                   max_lines, max_line, line_cap, a["dig"], a["st"], a["cnt"], a["fst"], a["which"], a["hits"], a["lines"], a["mts"], a["rec"],
                                                   rec_cap, a["ru"], a["text"], rec_cap * max_line if text_cap is None else text_cap, a["tu"])
    return rc_, ru.value, tu.value, list(lines), list(mts)


def check_arguments(engine):
    raw = sel.numbered({3, 5}, 9)
    packed = sc.pack(engine, [raw])
    M, P = _lib.MatcherDesc.of, _lib.E_PARAM
    fixed = M(FIXED, NEEDLE)
    ok = raw_call(engine, packed, fixed)
    assert ok == (_lib.OK, 2, 14, [2], [2])
    # the matches call's own checks
    assert [raw_call(engine, packed, fixed, **{k: None})[0] for k in ("mts", "ru", "tu", "rec", "text")] == [P] * 5
    assert raw_call(engine, packed, None)[0] == P and raw_call(engine, packed, M(3, NEEDLE))[0] == P
    assert b"search_matches" in engine.lib.zarc_gpu_last_error(engine.h)
    assert raw_call(engine, packed, fixed, rec=None, line_cap=0)[0] == raw_call(engine, packed, fixed, text=None, rec_cap=0)[0] == _lib.OK
    # which and hits: a set's, NULL or not; nobody else's
    assert raw_call(engine, packed, M(SET, [NEEDLE, b"row"]), with_set=True)[0] == raw_call(engine, packed, M(SET, [NEEDLE]))[0] == _lib.OK
    assert raw_call(engine, packed, fixed, with_set=True)[0] == raw_call(engine, packed, M(REGEX, RX), with_set=True)[0] == P
    # the matcher's own lines call refuses first, with its code and message
    assert [raw_call(engine, packed, m)[0] for m in (M(FIXED, b""), M(FIXED, b"p" * 257), M(FIXED, b"a\nb"), M(FIXED, NEEDLE, 2), M(SET, []), M(SET, [b"a\n"]),
                                                    M(REGEX, b"a*"), M(REGEX, b"("), M(REGEX, b"x\\n"))] == [P] * 9
    assert raw_call(engine, packed, M(REGEX, b"("))[0] == P and b"regex: offset" in engine.lib.zarc_gpu_last_error(engine.h)
    assert raw_call(engine, packed, M(REGEX, b".{7}a"))[0] == _lib.E_UNSUPPORTED
    # an expression the lines call accepts and the forward table refuses: the message gives the states needed
    assert engine.search_regex_lines(packed[0], packed[1], b"(a|b)*a(a|b){6}")[0][0][0] == _lib.FRAME_OK
    assert raw_call(engine, packed, M(REGEX, b"(a|b)*a(a|b){6}"))[0] == _lib.E_UNSUPPORTED
    assert re.search(rb"needs \d+ states; the limit is 64", engine.lib.zarc_gpu_last_error(engine.h))
    assert raw_call(engine, packed, M(FIXED, b"a\nb"), mts=None)[0] == P and b"newline" in engine.lib.zarc_gpu_last_error(engine.h)        # in the matcher's order
    assert [raw_call(engine, packed, fixed, **{k: None})[0] for k in ("lines", "st", "cnt", "fst", "dig", "ptrs", "lens", "rl")] == [P] * 8
    assert [raw_call(engine, packed, fixed, max_line=v)[0] for v in (0, 65537)] == [P] * 2
    assert raw_call(engine, packed, fixed, n=0, ptrs=None, lens=None, rl=None)[:3] == (_lib.OK, 0, 0)
    assert raw_call(engine, packed, M(REGEX, b"("), n=0, ptrs=None, lens=None, rl=None)[0] == P
    assert raw_call(engine, packed, fixed, frame_len=[0xFFFFFFF0])[0] == _lib.E_UNSUPPORTED
    # the device form refuses the same
    c = ctypes
    u64 = lambda v: (c.c_uint64 * 1)(v)
    dig = np.zeros((1, 32), dtype=np.uint8)
    st, cnt, fst, lines, mts = (c.c_int * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)(), (c.c_uint64 * 1)()
    rec, ru, tu = (_lib.Match * 4)(), c.c_size_t(), c.c_size_t()
    dummy = c.c_void_p(16)  # never dereferenced: the call is refused before

    def dev(n=1, base=dummy, m=fixed, mts=mts, which=None, text_cap=64, rl=u64(0), rec=rec):
        return engine.lib.zarc_gpu_search_matches_batch_device(engine.h, n, base, u64(0), u64(9), rl, None, c.byref(m) if m is not None else None, 0, 16, 4,
                                                               dig.ctypes.data_as(c.c_void_p), st, cnt, fst, which, None, lines, mts, rec, 4, c.byref(ru), dummy, text_cap,
                                                               c.byref(tu))
    assert dev(n=0, base=None) == _lib.OK
    assert dev(base=None) == dev(m=None) == dev(mts=None) == dev(rec=None) == dev(which=cnt) == dev(m=M(9, b"x")) == P
    assert dev(text_cap=63) == _lib.E_DSTSIZE and dev(rl=u64(0xFFFFFFF0)) == _lib.E_UNSUPPORTED
    assert dev(m=M(REGEX, b"(a|b)*a(a|b){6}")) == _lib.E_UNSUPPORTED
    # ... and the handle still works
    assert raw_call(engine, packed, fixed) == ok
