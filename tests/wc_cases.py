"""Checks of zarc_gpu_count_batch*, shared by the emulator tests (test_wc.py) and the GPU tests (test_gpu_wc.py).

The reference for every expected value is Python on the bytes the frames were packed from -- never the engine: ref_wc() is the contract of
include/zarc_gpu.h, written out literally.  Every comparison is equality."""
import ctypes

import numpy as np

import search_cases as sc
import verify_cases as vc
from zarc_amd import _lib

S = sc.SLICE
LEN1 = 3 * S + 1000
DECODED = (_lib.FRAME_OK, _lib.FRAME_DIGEST)
ZERO = (0,) * 6


def ref_wc(d):
    """-> (lines, words, chars, max_line, max_line_start, max_line_no) of the content d"""
    if not d: return ZERO
    pieces = d.split(b"\n")
    longest = max(len(p) for p in pieces)
    k = next(i for i, p in enumerate(pieces) if len(p) == longest)              # the lowest such piece
    start = sum(len(p) + 1 for p in pieces[:k])
    chars = int(np.count_nonzero((np.frombuffer(d, dtype=np.uint8) & 0xC0) != 0x80))
    return d.count(b"\n"), len(d.split()), chars, longest, start, k + 1


def dirty_scratch(engine, nbytes):
    """a verify pass over content in which every 16-byte step holds line feeds, word starts and characters: it is what lies in the handle's
    scratch behind the content of the frames counted next, where a wrong mask of a frame's last step would count it"""
    junk = (b"\n x" * (nbytes // 3 + 8))[:nbytes]
    frames, raw_lens, digests = sc.pack(engine, [junk], compress=False)
    assert engine.verify(frames, raw_lens, digests) == [(digests[0], _lib.FRAME_OK)]


def check_counts(engine, raws, compress=True, tag="", call=None):
    """one count call over the packed raws (all good frames) against the reference -> counts"""
    frames, raw_lens, digests = sc.pack(engine, raws, compress=compress)
    verdicts, counts = call(frames, raw_lens, digests) if call else engine.count(frames, raw_lens, expect=digests)
    assert verdicts == [(d, _lib.FRAME_OK) for d in digests], tag
    assert len(counts) == len(raws)
    for i, (g, d) in enumerate(zip(counts, raws)):
        assert g == ref_wc(d), (tag, i, len(d), g, ref_wc(d))
    return counts


def put(raw, edits):
    """raw with bytes written over: edits = [(offset, bytes)]"""
    b = bytearray(raw)
    for at, v in edits: b[at:at + len(v)] = v
    assert len(b) == len(raw)
    return bytes(b)


# ---- 1. seams ------------------------------------------------------------------------------------------------------------------------
def seam_frames(corpus):
    text = corpus.entry(7000, LEN1, 0)
    assert text.count(b"\n") > 100 and len(text.split()) > 1000
    word = (S - 8, b"abcdefghijklmnop")                                         # one word across the slice seam
    flat = (S - 300, text[S - 300:S + 300].replace(b"\n", b" "))                # no line feed near the seam but the planted ones
    names, raws = [], []

    def add(name, edits): names.append(name); raws.append(put(text, edits))
    add("word across the seam", [word])
    add("space at S - 1", [word, (S - 1, b" ")])
    add("space at S", [word, (S, b" ")])
    add("line feed at S - 1", [flat, (S - 1, b"\n")])
    add("line feed at S", [flat, (S, b"\n")])
    add("line feeds at S - 1 and S", [flat, (S - 1, b"\n\n")])
    for ch in ("é", "€", "\U0001F600"):                               # 2, 3 and 4 bytes
        u = ch.encode()
        for back in range(1, len(u)):
            add("%d-byte character, %d in front of S" % (len(u), back), [(S - back, u)])
            add("%d-byte character, %d in front of a step" % (len(u), back), [(16 * 1000 - back, u), (S + 256 * 9 - back, u)])
    # a word start at the first byte of a wave's first step (1024 w + 4096 r), behind white space of every kind -- and none behind a letter
    firsts = [1024, 2048, 3072, 4096, 5120, S + 1024, 2 * S + 4096 + 3072]
    add("word starts at a wave's first step", [(p - 2, b"q" + bytes([(9, 10, 11, 12, 13, 32, 32)[i]]) + b"Wq") for i, p in enumerate(firsts)])
    add("no word start at a wave's first step", [(p - 2, b"qqWq") for p in firsts])
    return names, raws


def check_seams(engine, corpus, compress=True):
    names, raws = seam_frames(corpus)
    want = [ref_wc(d) for d in raws]
    w = dict(zip(names, want))
    base = w["word across the seam"]
    assert w["space at S - 1"][1] == w["space at S"][1] == base[1] + 1 and raws[1] != raws[2]       # a cut word is two words
    assert w["line feeds at S - 1 and S"][0] == w["line feed at S"][0] + 1 == w["line feed at S - 1"][0] + 1
    assert w["word starts at a wave's first step"][1] > w["no word start at a wave's first step"][1]
    assert len({x[2] for x in want}) >= 4                                                          # the characters differ from case to case
    got = check_counts(engine, raws, compress, "seams")
    assert got == want


# ---- 2. the longest line -------------------------------------------------------------------------------------------------------------
def ruled(n, longs, final_nl=True):
    """n bytes of 9-byte lines; longs = [(a, b)]: [a, b) becomes one line of b - a bytes 'y' with a line feed on either side (where there is one)"""
    b = bytearray((b"xxxxxxxxx\n" * (n // 10 + 1))[:n])
    if not final_nl and b[-1] == 10: b[-1] = ord("x")
    for a, e in longs:
        b[a:e] = b"y" * (e - a)
        if a > 0: b[a - 1] = 10
        if e < n: b[e] = 10
    return bytes(b)


def longest_frames():
    n = LEN1
    cases = [
        ("inside one chunk", ruled(n, [(256 * 5 + 20, 256 * 5 + 120)]), (100, 256 * 5 + 20)),
        ("across a chunk", ruled(n, [(256 * 7 + 200, 256 * 7 + 350)]), (150, 256 * 7 + 200)),
        ("across a slice", ruled(n, [(S - 300, S + 400)]), (700, S - 300)),
        ("over three whole slices", ruled(4 * S + 100, [(S // 2, 3 * S + S // 2)]), (3 * S, S // 2)),
        ("the head", ruled(n, [(0, 500)]), (500, 0)),
        ("the head, to the seam", ruled(n, [(0, S)]), (S, 0)),
        ("the tail", ruled(n, [(n - 500, n)]), (500, n - 500)),
        ("the tail, from the seam", ruled(n, [(3 * S, n)]), (1000, 3 * S)),
        ("two equal lines in a slice", ruled(n, [(3000, 3100), (40000, 40100)]), (100, 3000)),
        ("a seam line, then an equal inner line", ruled(n, [(S - 50, S + 50), (2 * S + 1000, 2 * S + 1100)]), (100, S - 50)),
        ("an inner line, then an equal seam line", ruled(n, [(1000, 1100), (2 * S - 50, 2 * S + 50)]), (100, 1000)),
        ("equal head, inner line and tail", ruled(n, [(0, 100), (S + 700, S + 800), (n - 100, n)]), (100, 0)),
        ("only line feeds", b"\n" * 5000, (0, 0)),
        ("only line feeds, two slices", b"\n" * (S + 5), (0, 0)),
        ("no line feed", b"y z" * (2 * S // 3 + 25), (3 * (2 * S // 3 + 25), 0)),
        ("no line feed, one byte", b"y", (1, 0)),
    ]
    return cases


def check_longest(engine, compress=True):
    cases = longest_frames()
    for name, d, (length, start) in cases:                                      # the reference agrees with what was planted
        r = ref_wc(d)
        assert r[3:5] == (length, start) and r[5] == d[:start].count(b"\n") + 1, (name, r)
    assert ref_wc(cases[12][1]) == (5000, 0, 5000, 0, 0, 1)
    raws = [d for _, d, _ in cases]
    mid = raws[3]
    assert mid[S:3 * S].count(b"\n") == 0
    check_counts(engine, raws, compress, "longest line")


# ---- 3. ends of content --------------------------------------------------------------------------------------------------------------
END_LENS = (0, 1, 15, 16, 17, 255, 256, 257, S - 1, S, S + 1)


def check_ends(engine, corpus, compress=True):
    text = corpus.entry(7100, S + 1, 0)
    raws = []
    for n in END_LENS:
        for last in (b"\n", b"z"):
            d = put(text[:n], [(n - 1, last)]) if n else b""
            neighbour = (b"\n q" * (n // 3 + 1))[:n]                             # lies in front of or behind d in the scratch: frames go by size
            raws += [neighbour, d, neighbour]
    raws += [b"ends in a word", b"ends in spaces \t \r ", b" ", b"\n", b"\x80", b"\xc3\xa9"]
    assert ref_wc(b" ") == (0, 0, 1, 1, 0, 1) and ref_wc(b"\n") == (1, 0, 1, 0, 0, 1) and ref_wc(b"") == ZERO
    assert ref_wc(b"ends in spaces \t \r ")[1] == 3 and ref_wc(b"\x80")[2] == 0 and ref_wc(b"\xc3\xa9")[1:3] == (1, 1)
    dirty_scratch(engine, sum(len(d) + 16 for d in raws) + 4096)
    check_counts(engine, raws, compress, "ends")


# ---- 4. carry paths ------------------------------------------------------------------------------------------------------------------
def carry_frames(corpus):
    """32 slices (the lane folds them), 33 (the wave does, one slice a lane) and 133 = 64 * 2 + 5 (three slices a lane, the last lanes
    none): the longest line crosses the boundary between two lanes' shares"""
    sizes = (32 * S, 32 * S + 1, 133 * S - 1234)
    raws = []
    for i, n in enumerate(sizes):
        text = corpus.entry(7200 + i, n, 0)
        slices = (n + S - 1) // S
        per = (slices + 63) // 64
        seam = (11 * per) * S if slices > 32 else 20 * S                          # lanes 10 and 11 meet here
        lo, hi = seam - 5000 - i, seam + 7000 + i
        d = put(text, [(lo, text[lo:hi].replace(b"\n", b" "))])
        r = ref_wc(d)
        assert r[4] < seam < r[4] + r[3] and r[3] >= 12000 and r[0] > 1000, (n, r)
        raws.append(d)
    return raws


def check_carry(engine, corpus, compress=True):
    big = carry_frames(corpus)
    # the winner in the last slice, which only the last lane with a share holds; and in the first
    last = put(big[2], [(len(big[2]) - 30000, b"L" * 20000)])
    first = put(big[1], [(100, b"F" * 20000)])
    assert ref_wc(last)[3] >= 20000 and ref_wc(last)[4] > 132 * S - 40000 and ref_wc(first)[4] <= 100 and ref_wc(first)[3] >= 20000
    small = [corpus.entry(7300 + i, n, 0) for i, n in enumerate((5000, S + 17, 3 * S))]
    check_counts(engine, [big[0], big[1]], compress, "32 and 33 slices")
    check_counts(engine, [small[0], big[2], small[1], first, small[2], last[:70 * S + 5]], compress, "wave-path frames among lane-path ones")
    check_counts(engine, [last], compress, "the last slice wins")


def check_random(engine, compress=True):
    """contents made of lines whose lengths come from a handful of values, so that equal longest lines are the rule: in one chunk, across
    chunks, slices and the shares of the carry's lanes, with slices that hold no line feed at all; bytes of every class among them"""
    import random
    rnd = random.Random(20)
    alphabet = [b"a", b"b", b" ", b"\t", b"\r", b"\x80", b"\xc3", b"\xe2", b"\xf0", b"\x0b", b"z "]
    raws = []
    for total, lengths in [(n, ls) for n in (700, 5000, S - 3, S + 9, 2 * S + 100, 3 * S) for ls in ((0, 1, 7), (15, 16, 17, 40), (255, 256, 300, 1000))] + \
                          [(34 * S + 11, (S // 2, S, 2 * S + 5, 3000)), (70 * S - 7, (S - 1, S, S + 1, 3 * S, 100)), (40 * S, (5 * S, 7, 5 * S))]:
        out = bytearray()
        while len(out) < total:
            n = rnd.choice(lengths)
            fill = rnd.choice(alphabet)
            out += (fill * (n // len(fill) + 1))[:n] + b"\n"
        if rnd.random() < 0.5: out += b"tail"
        raws.append(bytes(out[:total]) if rnd.random() < 0.5 else bytes(out))
    want = [ref_wc(d) for d in raws]
    ties = sum(1 for d, w in zip(raws, want) if sum(1 for piece in d.split(b"\n") if len(piece) == w[3]) > 1)
    assert ties >= len(raws) // 2 and any(w[5] > 1 for w in want)
    check_counts(engine, raws, compress, "random lines")


# ---- 5. many small and bad frames ----------------------------------------------------------------------------------------------------
def check_many_small(engine, oracle, corpus, golden_frames, compress=True):
    raws = sc.small_entries(corpus)
    frames, raw_lens, digests = sc.pack(engine, raws, compress=compress)
    ef, el, ee, er = vc.error_list(oracle, corpus, golden_frames)                  # committed libzstd frames: good, wrong checksum, bad magic, cut short,
    for j, at in enumerate((5, 400, 401, 999, 1500, 2222, 2999)):                  # corrupt, wrong digest, wrong size
        frames.insert(at, ef[j]); raw_lens.insert(at, el[j]); digests.insert(at, ee[j]); raws.insert(at, er[j])
    want_v = engine.verify(frames, raw_lens, digests)
    status = [st for _, st in want_v]
    assert [status[at] for at in (5, 400, 2222)] == [_lib.FRAME_OK, _lib.FRAME_CHECKSUM, _lib.FRAME_DIGEST] and status[1500] not in DECODED
    assert sum(st in DECODED for st in status) == len(raws) - 5
    want = [ref_wc(d) if st in DECODED else ZERO for d, st in zip(raws, status)]
    assert want[2222] == want[5] != ZERO and want[400] == want[1500] == ZERO and sum(w == ZERO for w in want) > 5
    verdicts, counts = engine.count(frames, raw_lens, expect=digests)
    assert verdicts == want_v                                                      # status and digest are verify's
    for i, (g, w) in enumerate(zip(counts, want)):
        assert g == w, (i, status[i], g, w)


# ---- 6. cut invariance, forms and counters -------------------------------------------------------------------------------------------
def check_cut_invariance(engine, corpus, compress=True):
    raws = sc.small_entries(corpus, 600) + [corpus.entry(7400 + i, 1 << 20, 0) for i in range(3)] + [corpus.entry(7410, 70000, 0), corpus.entry(7411, 40 * S + 9, 0)]
    frames, raw_lens, digests = sc.pack(engine, raws, compress=compress)
    want = [ref_wc(d) for d in raws]
    up = sum(len(f) for f in frames)
    verdicts = [(d, _lib.FRAME_OK) for d in digests]
    assert engine.count(frames, raw_lens, expect=digests) == (verdicts, want)
    assert vc.copy_counters(engine)[:2] == (up, 0)
    assert 0 < engine.kernel_ms(_lib.T_WC) <= engine.kernel_ms(_lib.T_TOTAL)
    assert engine.kernel_ms(_lib.T_RANGE) in (0.0, -1.0)
    for mb in (2, 1):                                                              # two parts and more
        engine.set_parameter(_lib.PX_SCRATCH_MB, mb)
        try:
            assert engine.count(frames, raw_lens, expect=digests) == (verdicts, want), mb
            assert vc.copy_counters(engine)[:2] == (up, 0)
            assert 0 < engine.kernel_ms(_lib.T_WC) <= engine.kernel_ms(_lib.T_TOTAL)
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
    engine.set_parameter(_lib.PX_STAGE_CHUNK, 65536)                               # many staged chunks
    try:
        assert engine.count(frames, raw_lens, expect=digests) == (verdicts, want)
        assert vc.copy_counters(engine)[:2] == (up, 0)
    finally:
        engine.set_parameter(_lib.PX_STAGE_CHUNK, 0)
    d_frames, foff, _ = vc._arena(engine, frames)
    try:
        exp = np.frombuffer(b"".join(digests), dtype=np.uint8)
        flen = [len(f) for f in frames]
        assert engine.count_device(d_frames, foff, flen, raw_lens, exp) == (verdicts, want)
        assert vc.copy_counters(engine) == (0, 0, 0, 0)
        assert 0 < engine.kernel_ms(_lib.T_WC) <= engine.kernel_ms(_lib.T_TOTAL)
        engine.set_parameter(_lib.PX_SCRATCH_MB, 1)
        try:
            assert engine.count_device(d_frames, foff, flen, raw_lens, exp) == (verdicts, want)
            assert vc.copy_counters(engine) == (0, 0, 0, 0)
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
        engine.verify_device(d_frames, foff, flen, raw_lens, exp)
        assert engine.kernel_ms(_lib.T_WC) in (0.0, -1.0)
    finally:
        engine.free(d_frames)
    engine.verify(frames, raw_lens, digests)
    assert engine.kernel_ms(_lib.T_WC) in (0.0, -1.0)                              # an unused timer after any other call
    engine.count(frames[:3], raw_lens[:3])
    assert engine.kernel_ms(_lib.T_RANGE) in (0.0, -1.0) and engine.kernel_ms(_lib.T_WC) > 0


# ---- 7. arguments --------------------------------------------------------------------------------------------------------------------
def raw_call(engine, packed, n=None, frame_len=None, **null):
    """zarc_gpu_count_batch through ctypes; null: names of arguments to pass as NULL -> (rc, counts)"""
    c = ctypes
    frames, raw_lens, _ = packed
    m = len(frames)
    ptrs, lens = vc._ptrs(frames)
    if frame_len is not None: lens = (c.c_size_t * m)(*frame_len)
    rl = (c.c_size_t * m)(*raw_lens)
    dig = np.zeros((m, 32), dtype=np.uint8)
    st = (c.c_int * m)()
    res = (_lib.Wc * m)()
    a = dict(ptrs=ptrs, lens=lens, rl=rl, dig=dig.ctypes.data_as(c.c_void_p), st=st, res=res)
    for k in null: a[k] = None
    rc = engine.lib.zarc_gpu_count_batch(engine.h, m if n is None else n, a["ptrs"], a["lens"], a["rl"], None, a["dig"], a["st"], a["res"])
    assert all(tuple(r.reserved) == (0, 0) for r in res)
    return rc, [(r.lines, r.words, r.chars, r.max_line, r.max_line_start, r.max_line_no) for r in res]


def check_arguments(engine, corpus):
    c = ctypes
    raw = corpus.entry(7500, 5000, 0)
    packed = sc.pack(engine, [raw])
    ok = raw_call(engine, packed)
    assert ok == (_lib.OK, [ref_wc(raw)]) and ok[1][0][0] > 0
    P = _lib.E_PARAM
    assert [raw_call(engine, packed, **{k: None})[0] for k in ("ptrs", "lens", "rl", "dig", "st")] == [P] * 5        # verify's checks
    assert raw_call(engine, packed, res=None)[0] == P
    assert raw_call(engine, packed, n=0)[0] == _lib.OK
    assert raw_call(engine, packed, n=0, ptrs=None, lens=None, rl=None, dig=None, st=None, res=None)[0] == _lib.OK
    assert raw_call(engine, (packed[0], [0xFFFFFFF0], packed[2]))[0] == raw_call(engine, packed, frame_len=[0xFFFFFFF0])[0] == _lib.E_UNSUPPORTED
    # the device form
    lib, h = engine.lib, engine.h
    u64 = lambda v: (c.c_uint64 * 1)(v)
    dig = np.zeros((1, 32), dtype=np.uint8)
    pdig = dig.ctypes.data_as(c.c_void_p)
    st, res = (c.c_int * 1)(), (_lib.Wc * 1)()
    dummy = c.c_void_p(16)  # never dereferenced: the call is refused before

    def dev(n=1, base=dummy, off=u64(0), fl=u64(9), rl=u64(0), pdig=pdig, st=st, res=res):
        return lib.zarc_gpu_count_batch_device(h, n, base, off, fl, rl, None, pdig, st, res)
    assert dev(n=0, base=None, off=None, fl=None, rl=None, pdig=None, st=None, res=None) == _lib.OK
    assert dev(base=None) == dev(off=None) == dev(fl=None) == dev(rl=None) == dev(pdig=None) == dev(st=None) == dev(res=None) == P
    assert dev(rl=u64(0xFFFFFFF0)) == dev(fl=u64(1 << 32)) == _lib.E_UNSUPPORTED
    assert lib.zarc_gpu_abi_version() == 2
    # ... and the handle still works
    assert raw_call(engine, packed) == ok
    assert engine.count(packed[0], packed[1], expect=packed[2]) == ([(packed[2][0], _lib.FRAME_OK)], [ref_wc(raw)])
