"""Checks of zarc_gpu_read_ranges_batch*, shared by the emulator tests (test_range.py) and the GPU tests (test_gpu_range.py).

The reference for every expected value is Python on the bytes the frames were packed from -- never the engine: ref_range() computes T, a and
b literally from the definition in include/zarc_gpu.h, deliver() applies the delivery rule.  Every comparison is equality."""
import ctypes

import numpy as np

import search_cases as sc
import verify_cases as vc
from zarc_amd import _lib

S = sc.SLICE
LEN1 = 3 * S + 1000
B, L, END, ALL = _lib.RANGE_BYTES, _lib.RANGE_LINES, _lib.RANGE_FROM_END, _lib.RANGE_ALL
U64 = 2 ** 64 - 1
DECODED = (_lib.FRAME_OK, _lib.FRAME_DIGEST)


# the usual tools as ranges (include/zarc_gpu.h)
def head(n, unit=L): return (unit, 0, 0, n)
def head_minus(n, unit=L): return (unit, END, n, ALL)
def tail(n, unit=L): return (unit, END, 0, n)
def tail_plus(k, unit=L): return (unit, 0, max(k, 1) - 1, ALL)
def span(a, b, unit=L): return (unit, 0, a - 1, b - a + 1)      # sed -n 'a,bp'


def units_of(d):
    """the LINES units of d, by the definition: every line with its 0x0A, and an unterminated last line"""
    pieces = d.split(b"\n")
    units = [p + b"\n" for p in pieces[:-1]] + ([pieces[-1]] if pieces[-1] else [])
    assert b"".join(units) == d and len(units) == d.count(b"\n") + (1 if d and d[-1] != 10 else 0)
    return units


def ref_range(d, rng):
    """-> (units, first, taken, start, length) of range rng = (unit, flags, skip, take) over the content d"""
    unit, flags, skip, take = rng
    if unit == B:
        T, pos = len(d), (lambda k: k)
    else:
        nl = np.flatnonzero(np.frombuffer(d, dtype=np.uint8) == 10)
        T = len(nl) + (1 if d and d[-1] != 10 else 0)
        pos = lambda k: 0 if k == 0 else (len(d) if k == T else int(nl[k - 1]) + 1)
    if flags & END:
        b = T - min(skip, T)
        a = b - min(take, b)
    else:
        a = min(skip, T)
        b = min(min(a + take, U64), T)
    return T, a, b - a, pos(a), pos(b) - pos(a)


def deliver(raws, ranges, decoded=None, max_bytes=0, text_cap=None):
    """the delivery rule -> (res, text): frames in batch order, per frame the first min(length, max_bytes or all, what text_cap leaves) bytes"""
    res, text = [], []
    used = 0
    for i, (d, r) in enumerate(zip(raws, ranges)):
        if decoded is not None and not decoded[i]:
            res.append((0,) * 7)
            continue
        T, a, n, start, length = ref_range(d, r)
        e = min(length, max_bytes or length, (U64 if text_cap is None else text_cap) - used)
        res.append((T, a, n, start, length, used, e))
        text.append(d[start:start + e])
        used += e
    return res, b"".join(text)


def check_ranges(engine, packed, raws, ranges, max_bytes=0, text_cap=None, tag="", call=None):
    """one read_ranges call over a packed batch of good frames against the reference.  text_cap None: room for everything.  -> (res, text)"""
    frames, raw_lens, digests = packed
    cap = sum(ref_range(d, r)[4] for d, r in zip(raws, ranges)) + 1 if text_cap is None else text_cap
    call = call or (lambda **kw: engine.read_ranges(frames, raw_lens, ranges, expect=digests, **kw))
    verdicts, res, text = call(max_bytes=max_bytes, text_cap=cap)
    assert verdicts == [(d, _lib.FRAME_OK) for d in digests], tag
    want_res, want_text = deliver(raws, ranges, None, max_bytes, cap)
    for i, (g, w) in enumerate(zip(res, want_res)):
        assert g == w, (tag, i, ranges[i], g, w)
    assert len(res) == len(want_res) and text == want_text, (tag, len(text), len(want_text))
    return res, text


def repeat(packed, raws, picks):
    """the batch that holds frame k once per entry (k, range) of picks -> (packed, raws, ranges)"""
    frames, raw_lens, digests = packed
    ks = [k for k, _ in picks]
    return ([frames[k] for k in ks], [raw_lens[k] for k in ks], [digests[k] for k in ks]), [raws[k] for k in ks], [r for _, r in picks]


# ---- 1. boundaries -------------------------------------------------------------------------------------------------------------------
def boundary_frames(corpus):
    text = corpus.entry(6000, LEN1, 0)
    assert text.count(b"\n") > 100

    def frame(put, lo=S - 300, hi=S + 300):
        b = bytearray(text)
        b[lo:hi] = bytes(b[lo:hi]).replace(b"\n", b" ")
        for p in put: b[p] = 10
        assert len(b) == LEN1
        return bytes(b)
    return [frame([S - 1]), frame([S]), frame([S - 1, S]), frame([], S - 100, 3 * S + 100)]


def check_boundaries(engine, corpus, compress=True):
    raws = boundary_frames(corpus)
    packed = sc.pack(engine, raws, compress=compress)
    picks = []
    for k, planted in ((0, [S - 1]), (1, [S]), (2, [S - 1, S])):
        d = raws[k]
        for p in planted:
            n = d[:p + 1].count(b"\n")                     # the line that ends at p is unit n - 1
            T = ref_range(d, head(0))[0]
            assert ref_range(d, span(n, n))[3] + ref_range(d, span(n, n))[4] == p + 1 and ref_range(d, tail_plus(n + 1))[3] == p + 1
            picks += [(k, span(n, n)), (k, head(n)), (k, tail_plus(n + 1)), (k, tail(T - n)), (k, head_minus(T - n)), (k, span(n + 1, n + 1))]
    assert ref_range(raws[2], span(raws[2][:S + 1].count(b"\n"), raws[2][:S + 1].count(b"\n")))[3:] == (S, 1)   # the empty line between both line feeds
    # one line over three slices: it is the line behind the last 0x0A in front of S - 100
    d = raws[3]
    n = d[:S - 100].count(b"\n") + 1
    r = ref_range(d, span(n, n))
    assert r[3] < S - 100 and r[3] + r[4] > 3 * S + 100 and r[3] // S == 0 and (r[3] + r[4] - 1) // S == 3
    picks += [(3, span(n, n)), (3, head(n)), (3, tail_plus(n)), (3, tail_plus(n + 1)), (3, head(n - 1))]
    # a range inside one 256-byte chunk, one across a chunk, one across a slice, the whole frame
    d = raws[0]
    nl = [i for i in range(2000, 40000) if d[i] == 10]
    inside = next(j for j in range(len(nl) - 1) if nl[j] // 256 == nl[j + 1] // 256)
    across = next(j for j in range(len(nl) - 1) if nl[j] // 256 != nl[j + 1] // 256)
    for j in (inside, across):
        n = d[:nl[j] + 1].count(b"\n") + 1                 # the line between nl[j] and nl[j + 1]
        assert ref_range(d, span(n, n))[3:] == (nl[j] + 1, nl[j + 1] - nl[j])
        picks.append((0, span(n, n)))
    n1, n2 = d[:S // 2].count(b"\n"), d[:2 * S + S // 2].count(b"\n")
    r = ref_range(d, span(n1, n2))
    assert r[3] // S == 0 and (r[3] + r[4]) // S == 2
    picks += [(0, span(n1, n2)), (0, head(ALL)), (0, head(ALL, B)), (0, tail(ALL)), (3, tail(ALL, B))]
    res, text = check_ranges(engine, *repeat(packed, raws, picks), tag="boundaries")
    assert res[-4][4] == res[-3][4] == LEN1


def check_large(engine, corpus, compress=True):
    """frames on both sides of the size at which zarc_range_carry hands a frame from its lane to the whole wave (32 slices), and one whose
    lanes sum two slices each (65 slices): boundaries in the first, a middle and the last slice"""
    raws = [corpus.entry(6050 + i, n, 0) for i, n in enumerate((32 * S, 32 * S + 1, (4 << 20) + 17))]
    packed = sc.pack(engine, raws, compress=compress)
    picks = []
    for k, d in enumerate(raws):
        T = ref_range(d, head(0))[0]
        n1, n2 = d[:len(d) // 2 + 777].count(b"\n"), d[:len(d) - 100].count(b"\n")
        r = ref_range(d, span(n1, n2))
        assert 10 < n1 < n2 - 10 < T and 0 < r[3] // S < (r[3] + r[4]) // S == (len(d) - 1000) // S and ref_range(d, span(5, n1))[3] < S
        picks += [(k, span(n1, n2)), (k, span(5, n1 + 1)), (k, tail(T - n2))]
    res, _ = check_ranges(engine, *repeat(packed, raws, picks), tag="large")
    assert all(r[4] > 1000 for r in res[0::3] + res[1::3]) and all(r[2] >= 1 and r[3] + r[4] == len(d) for r, d in zip(res[2::3], raws))


# ---- 2. ends of content --------------------------------------------------------------------------------------------------------------
ENDS = [b"a\nbb\nccc\n", b"a\nbb\nccc", b"\n", b"", b"no line feed at all", b"x\r\ny\r\n\r\nz\r\n"]


def check_ends(engine, compress=True):
    raws = ENDS
    packed = sc.pack(engine, raws, compress=compress)
    assert [ref_range(d, head(0))[0] for d in raws] == [3, 3, 1, 0, 1, 4]
    r = ref_range(raws[5], span(2, 3))
    assert raws[5][r[3]:r[3] + r[4]] == b"y\r\n\r\n" and [len(units_of(d)) for d in raws] == [3, 3, 1, 0, 1, 4]   # the 0x0D stays in its line
    picks = []
    for k, d in enumerate(raws):
        for unit in (L, B):
            T = ref_range(d, (unit, 0, 0, 0))[0]
            for N in sorted({0, max(T - 1, 0), T, T + 1, T + 5}):
                picks += [(k, head(N, unit)), (k, head_minus(N, unit)), (k, tail(N, unit)), (k, tail_plus(N, unit)), (k, span(1, max(N, 1), unit)),
                          (k, span(max(N, 1), N + 2, unit)), (k, span(2, max(T, 2), unit))]
    res, text = check_ranges(engine, *repeat(packed, raws, picks), tag="ends")
    assert len(text) > 100 and any(r[4] == 0 for r in res)


# ---- 3. arithmetic -------------------------------------------------------------------------------------------------------------------
def check_arithmetic(engine, corpus, compress=True):
    raws = [corpus.entry(6100, 5000, 0), corpus.entry(6101, S + 7, 0)]
    packed = sc.pack(engine, raws, compress=compress)
    T = [ref_range(d, head(0))[0] for d in raws]
    assert min(T) > 20
    picks = []
    for k in (0, 1):
        for unit, t in ((L, T[k]), (B, len(raws[k]))):
            for flags in (0, END):
                picks += [(k, (unit, flags, t, 5)), (k, (unit, flags, t + 1, ALL)), (k, (unit, flags, U64, U64)),       # skip >= T
                          (k, (unit, flags, 3, 0)), (k, (unit, flags, 3, ALL)), (k, (unit, flags, 0, ALL)),             # take 0, take ALL
                          (k, (unit, flags, U64 - 1, 5)), (k, (unit, flags, 3, U64 - 1)), (k, (unit, flags, 2 ** 63, 2 ** 63)),  # sums that overflow
                          (k, (unit, flags, 7, 9)), (k, (unit, flags, t - 1, 1)), (k, (unit, flags, t - 1, 2))]
    want = [ref_range(raws[k], r) for k, r in picks]
    assert any(w[2] == 0 and w[3] == len(raws[0]) for w in want) and any(w[4] == len(raws[1]) for w in want)
    assert ref_range(raws[0], (L, END, T[0] + 3, 2))[:3] == (T[0], 0, 0)                                                 # FROM_END with skip > T
    check_ranges(engine, *repeat(packed, raws, picks), tag="arithmetic")


# ---- 4. gather alignment -------------------------------------------------------------------------------------------------------------
ALIGN_LENS = (0, 1, 15, 16, 17, S - 1, S, S + 1, 3 * S + 7)
CANARY = 0xA5


def check_alignment(engine, corpus, compress=True):
    """BYTES ranges whose start and whose place in the text are 0, 1 and 15 bytes behind a multiple of 16, of every length of the list.
    Host form: one batch, a filler range in front of every case moves the running text offset where it is wanted.  Device form: every case
    alone, its text pointer at the wanted offset inside a buffer of canary bytes -- the bytes on both sides of the run keep the canary."""
    big, tiny = corpus.entry(6200, 3 * S + 7 + 64, 3), corpus.entry(6201, 64, 3)
    raws = [big, tiny]
    frames, raw_lens, digests = packed = sc.pack(engine, raws, compress=compress)
    cases = [(smod, tmod, n) for smod in (0, 1, 15) for tmod in (0, 1, 15) for n in ALIGN_LENS]
    picks, used = [], 0
    for smod, tmod, n in cases:
        pad = (tmod - used) % 16
        picks += [(1, (B, 0, 5, pad)), (0 if n > 17 else 1, (B, 0, 32 + smod, n))]
        used += pad + n
    res, text = check_ranges(engine, *repeat(packed, raws, picks), tag="alignment, host form")
    assert [(r[3] % 16, r[5] % 16, r[6]) for r in res[1::2]] == cases
    cap = 3 * S + 7 + 64
    d_frames, foff, _ = vc._arena(engine, frames)
    d_buf = engine.malloc(cap + 64)
    try:
        c = ctypes
        for smod, tmod, n in cases:
            k = 0 if n > 17 else 1
            engine.h2d(d_buf, bytes([CANARY]) * (cap + 64))
            rng, res1 = (_lib.Range * 1)(), (_lib.RangeResult * 1)()
            rng[0].unit, rng[0].flags, rng[0].skip, rng[0].take = B, 0, 32 + smod, n
            dig, st, tu = np.zeros((1, 32), dtype=np.uint8), (c.c_int * 1)(), c.c_size_t()
            u64 = lambda v: (c.c_uint64 * 1)(v)
            rc = engine.lib.zarc_gpu_read_ranges_batch_device(engine.h, 1, c.c_void_p(d_frames), u64(foff[k]), u64(len(frames[k])), u64(raw_lens[k]), None, rng, 0,
                                                              dig.ctypes.data_as(c.c_void_p), st, res1, c.c_void_p(d_buf + 16 + tmod), n, c.byref(tu))
            assert (rc, st[0], tu.value, res1[0].text_len) == (_lib.OK, _lib.FRAME_OK, n, n), (smod, tmod, n)
            got = bytes(engine.d2h(d_buf, cap + 64))
            lo = 16 + tmod
            assert got[lo:lo + n] == raws[k][32 + smod:32 + smod + n], (smod, tmod, n)
            assert got[:lo] == bytes([CANARY]) * lo and got[lo + n:] == bytes([CANARY]) * (cap + 64 - lo - n), (smod, tmod, n)
    finally:
        engine.free(d_buf)
        engine.free(d_frames)


# ---- 5. caps -------------------------------------------------------------------------------------------------------------------------
def check_caps(engine, corpus, compress=True):
    raws = [corpus.entry(6300 + i, n, 0) for i, n in enumerate((3000, 100000, 0, 2000, 50000))]
    packed = sc.pack(engine, raws, compress=compress)
    ranges = [head(10), span(100, 600), head(3), (B, 0, 100, 1500), tail(200)]
    lens = [ref_range(d, r)[4] for d, r in zip(raws, ranges)]
    assert lens[1] > 20000 and lens[4] > 5000 and lens[2] == 0 and lens[3] == 1500
    total = sum(lens)
    for max_bytes in (0, 1, 700, 1500, lens[1] - 1):                                # cuts inside the ranges of some frames, of all, of none
        check_ranges(engine, packed, raws, ranges, max_bytes=max_bytes, tag="max_bytes %d" % max_bytes)
    for cap in (0, 1, lens[0], lens[0] + 1, lens[0] + lens[1] - 1, lens[0] + lens[1], total - 1, total, total + 100):   # in a frame's middle, at its edge
        res, text = check_ranges(engine, packed, raws, ranges, text_cap=cap, tag="text_cap %d" % cap)
        assert len(text) == min(cap, total) and [r[:5] for r in res] == [ref_range(d, r) for d, r in zip(raws, ranges)]   # the truth whatever the caps
    res, text = check_ranges(engine, packed, raws, ranges, max_bytes=700, text_cap=min(lens[0], 700) + 300, tag="both caps")   # frame 1 gets 300 bytes, 3 and 4 none
    # the continuation rule: what a call cut off is exactly what the BYTES range {start + text_len, length - text_len} delivers
    cut = [(i, r) for i, r in enumerate(res) if r[6] < r[4]]
    assert len(cut) >= 3 and any(0 < r[6] for _, r in cut) and any(r[6] == 0 for _, r in cut)
    rest = [(B, 0, r[3] + r[6], r[4] - r[6]) for _, r in cut]
    sub = ([packed[0][i] for i, _ in cut], [packed[1][i] for i, _ in cut], [packed[2][i] for i, _ in cut])
    res2, text2 = check_ranges(engine, sub, [raws[i] for i, _ in cut], rest, tag="continuation")
    for (i, r), r2 in zip(cut, res2):
        whole = raws[i][r[3]:r[3] + r[4]]
        assert text[r[5]:r[5] + r[6]] + text2[r2[5]:r2[5] + r2[6]] == whole and r2[6] == r[4] - r[6]
    # a counting call: no text buffer at all
    rc, res3, used = raw_call(engine, packed, ranges, text_cap=0, text=None)
    assert rc == _lib.OK and used == 0 and [r[:5] for r in res3] == [r[:5] for r in res] and all(r[5:] == (0, 0) for r in res3)


def raw_call(engine, packed, ranges, max_bytes=0, text_cap=4096, n=None, frame_len=None, **null):
    """zarc_gpu_read_ranges_batch through ctypes; null: names of arguments to pass as NULL -> (rc, res, text_used)"""
    c = ctypes
    frames, raw_lens, _ = packed
    m = len(frames)
    ptrs, lens = vc._ptrs(frames)
    if frame_len is not None: lens = (c.c_size_t * m)(*frame_len)
    rl = (c.c_size_t * m)(*raw_lens)
    dig = np.zeros((m, 32), dtype=np.uint8)
    st = (c.c_int * m)()
    rng = (_lib.Range * m)()
    for i, r in enumerate(ranges): rng[i].unit, rng[i].flags, rng[i].skip, rng[i].take = r
    res = (_lib.RangeResult * m)()
    text = np.zeros(max(text_cap, 1), dtype=np.uint8)
    tu = c.c_size_t(77)
    a = dict(ptrs=ptrs, lens=lens, rl=rl, dig=dig.ctypes.data_as(c.c_void_p), st=st, rng=rng, res=res, text=text.ctypes.data_as(c.c_void_p), tu=c.byref(tu))
    for k in null: a[k] = None
    rc = engine.lib.zarc_gpu_read_ranges_batch(engine.h, m if n is None else n, a["ptrs"], a["lens"], a["rl"], None, a["rng"], max_bytes, a["dig"], a["st"],
                                               a["res"], a["text"], text_cap, a["tu"])
    return rc, [(r.units, r.first, r.taken, r.start, r.length, r.text_off, r.text_len) for r in res], tu.value


# ---- 6. cut invariance ---------------------------------------------------------------------------------------------------------------
def check_cut_invariance(engine, corpus, compress=True):
    raws = sc.small_entries(corpus, 600) + [corpus.entry(6400 + i, 1 << 20, 0) for i in range(3)] + [corpus.entry(6410, 70000, 0)]
    forms = [head(3), tail(2), span(2, 4), head(40, B), tail(33, B), head_minus(1), tail_plus(3), (B, 0, 7, 100)]
    ranges = [forms[i % len(forms)] for i in range(len(raws))]
    ranges[-4:] = [span(1000, 3000), tail(500), head(ALL, B), span(5, 400)]
    frames, raw_lens, digests = packed = sc.pack(engine, raws, compress=compress)
    lens = [ref_range(d, r)[4] for d, r in zip(raws, ranges)]
    assert lens[-2] == 1 << 20 and lens[-4] > 50000 and lens[-3] > 10000 and sum(lens[:-4]) > 10000
    cap = sum(lens) - lens[-1] - lens[-2] // 2                                     # runs out inside the last large frame
    free = check_ranges(engine, packed, raws, ranges, text_cap=cap, tag="budget 0")
    assert len(free[1]) == cap
    assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in frames), cap)
    assert engine.kernel_ms(_lib.T_RANGE) > 0 and engine.kernel_ms(_lib.T_TOTAL) >= engine.kernel_ms(_lib.T_RANGE)
    for mb in (2, 1):                                                              # two parts and more: the remainder of text_cap crosses their boundaries
        engine.set_parameter(_lib.PX_SCRATCH_MB, mb)
        try:
            assert check_ranges(engine, packed, raws, ranges, text_cap=cap, tag="budget %d" % mb) == free
            assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in frames), cap)
            assert engine.kernel_ms(_lib.T_RANGE) > 0
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
    engine.set_parameter(_lib.PX_STAGE_CHUNK, 65536)                               # many staged chunks
    try:
        assert check_ranges(engine, packed, raws, ranges, text_cap=cap, tag="small chunks") == free
        assert vc.copy_counters(engine)[:2] == (sum(len(f) for f in frames), cap)
    finally:
        engine.set_parameter(_lib.PX_STAGE_CHUNK, 0)
    d_frames, foff, _ = vc._arena(engine, frames)
    try:
        exp = np.frombuffer(b"".join(digests), dtype=np.uint8)
        dev_call = lambda **kw: engine.read_ranges_device(d_frames, foff, [len(f) for f in frames], raw_lens, ranges, expect=exp, **kw)
        assert check_ranges(engine, packed, raws, ranges, text_cap=cap, tag="device form", call=dev_call) == free
        assert vc.copy_counters(engine) == (0, 0, 0, 0) and engine.kernel_ms(_lib.T_RANGE) > 0
        engine.set_parameter(_lib.PX_SCRATCH_MB, 1)
        try:
            assert check_ranges(engine, packed, raws, ranges, text_cap=cap, tag="device form, budget 1", call=dev_call) == free
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
        engine.verify_device(d_frames, foff, [len(f) for f in frames], raw_lens, exp)
        assert engine.kernel_ms(_lib.T_RANGE) in (0.0, -1.0)
    finally:
        engine.free(d_frames)
    engine.verify(frames, raw_lens, digests)
    assert engine.kernel_ms(_lib.T_RANGE) in (0.0, -1.0)                           # an unused timer after any other call


# ---- 7. many small and bad frames ----------------------------------------------------------------------------------------------------
def check_many_small(engine, oracle, corpus, golden_frames, compress=True):
    raws = [corpus.entry(6500 + i, (i * 7919) % 2001, i % 4) for i in range(3000)]
    frames, raw_lens, digests = sc.pack(engine, raws, compress=compress)
    ef, el, ee, er = vc.error_list(oracle, corpus, golden_frames)                  # committed libzstd frames: good, wrong checksum, bad magic, cut short,
    for j, at in enumerate((5, 400, 401, 999, 1500, 2222, 2999)):                  # corrupt, wrong digest, wrong size
        frames.insert(at, ef[j]); raw_lens.insert(at, el[j]); digests.insert(at, ee[j]); raws.insert(at, er[j])
    forms = [head(3), tail(2), span(2, 4), head(40, B), tail(33, B), head_minus(1), tail_plus(3), (B, 0, 7, 100), head(0), tail(ALL), (L, END, 1, 1)]
    ranges = [forms[(i * 5) % len(forms)] for i in range(len(raws))]
    want_v = engine.verify(frames, raw_lens, digests)
    status = [st for _, st in want_v]
    assert [status[at] for at in (5, 400, 2222)] == [_lib.FRAME_OK, _lib.FRAME_CHECKSUM, _lib.FRAME_DIGEST] and status[1500] not in DECODED
    decoded = [st in DECODED for st in status]
    assert sum(decoded) == len(raws) - 5
    want_res, want_text = deliver(raws, ranges, decoded, 0, 1 << 22)
    assert want_res[2222][6] > 0 and want_res[400] == want_res[1500] == (0,) * 7 and sum(r[6] == 0 for r in want_res) > 100
    verdicts, res, text = engine.read_ranges(frames, raw_lens, ranges, expect=digests, text_cap=1 << 22)
    assert verdicts == want_v                                                      # status and digest are verify's
    for i, (g, w) in enumerate(zip(res, want_res)):
        assert g == w, (i, ranges[i], g, w)
    assert text == want_text


# ---- 8. arguments --------------------------------------------------------------------------------------------------------------------
def check_arguments(engine, corpus):
    c = ctypes
    raw = corpus.entry(6600, 5000, 0)
    packed = sc.pack(engine, [raw])
    want = deliver([raw], [head(3)], None, 0, 4096)
    ok = raw_call(engine, packed, [head(3)])
    assert ok == (_lib.OK, want[0], len(want[1])) and len(want[1]) > 0
    P = _lib.E_PARAM
    assert [raw_call(engine, packed, [head(3)], **{k: None})[0] for k in ("ptrs", "lens", "rl", "dig", "st")] == [P] * 5        # verify's checks
    assert [raw_call(engine, packed, [head(3)], **{k: None})[0] for k in ("rng", "res", "tu", "text")] == [P] * 4
    assert raw_call(engine, packed, [head(3)], text_cap=0, text=None)[::2] == (_lib.OK, 0)
    assert [raw_call(engine, packed, [(u, 0, 0, 1)])[0] for u in (2, 3, 0xFFFFFFFF)] == [P] * 3                              # an unknown unit
    assert [raw_call(engine, packed, [(L, f, 0, 1)])[0] for f in (2, 3, 0x80000000)] == [P] * 3                              # an unknown flag bit
    assert raw_call(engine, packed, [head(3)], n=0)[::2] == (_lib.OK, 0)
    assert raw_call(engine, packed, [head(3)], n=0, ptrs=None, lens=None, rl=None, rng=None, res=None, text=None)[::2] == (_lib.OK, 0)
    assert raw_call(engine, (packed[0], [0xFFFFFFF0], packed[2]), [head(3)])[0] == raw_call(engine, packed, [head(3)], frame_len=[0xFFFFFFF0])[0] == _lib.E_UNSUPPORTED
    # the device form
    lib, h = engine.lib, engine.h
    u64 = lambda v: (c.c_uint64 * 1)(v)
    dig = np.zeros((1, 32), dtype=np.uint8)
    pdig = dig.ctypes.data_as(c.c_void_p)
    st, tu = (c.c_int * 1)(), c.c_size_t(77)
    rng, res = (_lib.Range * 1)(), (_lib.RangeResult * 1)()
    rng[0].unit, rng[0].take = L, 3
    bad_unit, bad_flag = (_lib.Range * 1)(), (_lib.Range * 1)()
    bad_unit[0].unit, bad_flag[0].flags = 2, 2
    dummy = c.c_void_p(16)  # never dereferenced: the call is refused before

    def dev(n=1, base=dummy, off=u64(0), fl=u64(9), rl=u64(0), rng=rng, pdig=pdig, st=st, res=res, text=dummy, text_cap=64, tu=c.byref(tu)):
        return lib.zarc_gpu_read_ranges_batch_device(h, n, base, off, fl, rl, None, rng, 0, pdig, st, res, text, text_cap, tu)
    assert dev(n=0, base=None, off=None, fl=None, rl=None) == _lib.OK and tu.value == 0
    assert dev(base=None) == dev(off=None) == dev(fl=None) == dev(rl=None) == dev(pdig=None) == dev(st=None) == P
    assert dev(rng=None) == dev(res=None) == dev(tu=None) == dev(text=None) == dev(rng=bad_unit) == dev(rng=bad_flag) == P
    assert dev(rl=u64(0xFFFFFFF0)) == dev(fl=u64(1 << 32)) == _lib.E_UNSUPPORTED
    assert lib.zarc_gpu_abi_version() == 2
    # ... and the handle still works
    assert raw_call(engine, packed, [head(3)]) == ok
    assert engine.read_ranges(packed[0], packed[1], [head(3)], expect=packed[2]) == ([(packed[2][0], _lib.FRAME_OK)], want[0], want[1])
