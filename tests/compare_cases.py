"""Checks of zarc_gpu_compare_batch*, shared by the emulator tests (test_compare.py) and the GPU tests (test_gpu_compare.py).

The reference for every expected value is Python on the bytes the frames were packed from and on the other side's bytes -- never the
engine: ref_cmp() is the table of include/zarc_gpu.h, written out literally.  Every comparison is equality."""
import ctypes
import random

import numpy as np

import search_cases as sc
import verify_cases as vc
from zarc_amd import Engine, _lib

S = sc.SLICE
LEN1 = 3 * S + 1000
DECODED = (_lib.FRAME_OK, _lib.FRAME_DIGEST)
ZERO = (0,) * 7
EOF = _lib.CMP_EOF
EQUAL, DIFFER, FRAME_IS_PREFIX, OTHER_IS_PREFIX = _lib.CMP_EQUAL, _lib.CMP_DIFFER, _lib.CMP_FRAME_IS_PREFIX, _lib.CMP_OTHER_IS_PREFIX


def ref_cmp(a, b):
    """-> (relation, prefix, line, differing, suffix, byte_a, byte_b) of the content a against the other side b"""
    la, lb = len(a), len(b)
    common = min(la, lb)
    ne = np.frombuffer(a[:common], dtype=np.uint8) != np.frombuffer(b[:common], dtype=np.uint8)
    differing = int(np.count_nonzero(ne))
    prefix = int(np.argmax(ne)) if differing else common
    if differing: relation = DIFFER
    elif la == lb: relation = EQUAL
    else: relation = FRAME_IS_PREFIX if la < lb else OTHER_IS_PREFIX
    line = 1 + a[:prefix].count(b"\n")
    byte_a = a[prefix] if prefix < la else EOF
    byte_b = b[prefix] if prefix < lb else EOF
    limit = common - prefix                                                     # the tail never overlaps the head
    suffix = 0
    if limit:
        tail_ne = np.frombuffer(a[la - limit:], dtype=np.uint8) != np.frombuffer(b[lb - limit:], dtype=np.uint8)
        suffix = limit - 1 - int(np.flatnonzero(tail_ne)[-1]) if tail_ne.any() else limit
    return relation, prefix, line, differing, suffix, byte_a, byte_b


def junk(n, seed=0):
    """bytes with line feeds in every few of them, and no period: whatever they lie next to, most of them differ from it"""
    return np.random.default_rng(1000 + seed).choice(np.frombuffer(b"\nxyz", dtype=np.uint8), size=n).tobytes()


def dirty_scratch(engine, nbytes):
    """a verify pass over junk: it is what lies in the handle's scratch and in its staging arena behind the content of the pairs compared
    next, where a wrong mask of a last step would count it"""
    frames, raw_lens, digests = sc.pack(engine, [junk(nbytes)], compress=False)
    assert engine.verify(frames, raw_lens, digests) == [(digests[0], _lib.FRAME_OK)]


def other_arena(engine, raws, others):
    """the other sides on the device, 16-byte aligned, and behind every one bytes that differ from what the content has there (or junk)
    -> (pointer, offsets)"""
    buf, off = bytearray(), []
    for k, (a, b) in enumerate(zip(raws, others)):
        off.append(len(buf))
        room = (len(b) + 15) // 16 * 16 - len(b)
        behind = bytes(c ^ 0xFF for c in a[len(b):len(b) + room])
        buf += b + behind + junk(room - len(behind), k)
    buf += junk(_lib.PAD + 256, 77)
    d = engine.malloc(len(buf))
    engine.h2d(d, bytes(buf))
    return d, off


def compare_device(engine, frames, raw_lens, digests, raws, others):
    d_frames, foff, _ = vc._arena(engine, frames)
    d_other, ooff = other_arena(engine, raws, others)
    try:
        exp = np.frombuffer(b"".join(digests), dtype=np.uint8)
        return engine.compare_device(d_frames, foff, [len(f) for f in frames], raw_lens, d_other, ooff, [len(o) for o in others], exp)
    finally:
        engine.free(d_frames)
        engine.free(d_other)


def check_pairs(engine, raws, others, compress=True, tag="", device=False, dirty=False):
    """one compare call over the packed raws (all good frames) against the reference -> results; device: the device form as well"""
    assert len(raws) == len(others)
    frames, raw_lens, digests = sc.pack(engine, raws, compress=compress)
    want = [ref_cmp(a, b) for a, b in zip(raws, others)]
    if dirty: dirty_scratch(engine, sum(max(len(a), len(b)) + 16 for a, b in zip(raws, others)) + 4096)
    verdicts, got = engine.compare(frames, raw_lens, others, expect=digests)
    assert verdicts == [(d, _lib.FRAME_OK) for d in digests], tag
    assert len(got) == len(raws)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (tag, i, len(raws[i]), len(others[i]), g, w)
    if device:
        if dirty: dirty_scratch(engine, sum(len(a) + 16 for a in raws) + 4096)
        verdicts, got = compare_device(engine, frames, raw_lens, digests, raws, others)
        assert verdicts == [(d, _lib.FRAME_OK) for d in digests], tag
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (tag, "device form", i, len(raws[i]), len(others[i]), g, w)
    return want


def put(raw, edits):
    """raw with bytes written over: edits = [(offset, bytes)]"""
    b = bytearray(raw)
    for at, v in edits: b[at:at + len(v)] = v
    assert len(b) == len(raw)
    return bytes(b)


def flip(raw, *positions):
    """raw with the bytes at the positions changed, to and from nothing that is a line feed"""
    b = bytearray(raw)
    for p in positions:
        b[p] ^= 0x40
        assert b[p] != 10 and raw[p] != 10
    return bytes(b)


# ---- 1. seams ------------------------------------------------------------------------------------------------------------------------
SEAM_POSITIONS = (0, 15, 16, 4095, 4096, S - 1, S, S + 1, 1024, 2048, 3072, S + 1024, 2 * S + 4096 + 3072, LEN1 - 1)


def check_seams(engine, corpus, compress=True):
    text = bytearray(corpus.entry(8000, LEN1, 0))
    assert text.count(b"\n") > 100
    for p in SEAM_POSITIONS + (100, 2 * S + 50):
        if text[p] == 10: text[p] = ord("q")
    text = bytes(text)
    raws, others = [], []
    for p in SEAM_POSITIONS:
        raws.append(text); others.append(flip(text, p))
        assert ref_cmp(raws[-1], others[-1]) == (DIFFER, p, 1 + text[:p].count(b"\n"), 1, LEN1 - 1 - p, text[p], text[p] ^ 0x40)
    raws.append(text); others.append(flip(text, 100, 2 * S + 50))                  # the first wins prefix, the last wins suffix
    assert ref_cmp(raws[-1], others[-1])[1:5] == (100, 1 + text[:100].count(b"\n"), 2, LEN1 - 1 - (2 * S + 50))
    raws.append(text); others.append(text)
    assert ref_cmp(text, text) == (EQUAL, LEN1, text.count(b"\n") + 1, 0, 0, EOF, EOF)
    # a line feed at prefix - 1 counts for `line`, one at prefix does not; a byte changed from and to 0x0A
    for p in (777, 4096, S):
        flat = put(text, [(p - 40, text[p - 40:p + 40].replace(b"\n", b" "))])
        before, at = put(flat, [(p - 1, b"\n")]), put(flat, [(p, b"\n")])
        base = ref_cmp(flat, flip(flat, p))[2]
        for a, b in ((before, flip(before, p)), (at, put(at, [(p, b"x")])), (flat, put(flat, [(p, b"\n")]))):
            raws.append(a); others.append(b)
        assert [ref_cmp(a, b)[1:3] for a, b in zip(raws[-3:], others[-3:])] == [(p, base + 1), (p, base), (p, base)]
        assert ref_cmp(raws[-2], others[-2])[5:] == (10, ord("x")) and ref_cmp(raws[-1], others[-1])[5:] == (flat[p], 10)
    check_pairs(engine, raws, others, compress, "seams", device=True)


# ---- 2. lengths ----------------------------------------------------------------------------------------------------------------------
LENGTH_STEPS = (1, 15, 16, 17, S, S + 5)


def check_lengths(engine, corpus, compress=True):
    base = corpus.entry(8100, LEN1, 0)
    more = corpus.entry(8101, S + 5, 0)
    raws, others = [], []
    for k in LENGTH_STEPS:
        raws += [base, base]; others += [base[:-k], base + more[:k]]
        assert ref_cmp(base, base[:-k]) == (OTHER_IS_PREFIX, LEN1 - k, 1 + base[:LEN1 - k].count(b"\n"), 0, 0, base[LEN1 - k], EOF)
        assert ref_cmp(base, base + more[:k]) == (FRAME_IS_PREFIX, LEN1, 1 + base.count(b"\n"), 0, 0, EOF, more[0])
    for n in (1, 15, 16, 17, 31, 32, 33):                                         # ends inside the first steps
        raws += [base[:n], base[:n], base[:n]]; others += [base[:n - 1], base[:n + 1], base[:n]]
    raws += [b"", base[:100], b"", base[:S], b""]; others += [base[:100], b"", b"", b"", base[:S + 1]]
    assert ref_cmp(b"", b"") == (EQUAL, 0, 1, 0, 0, EOF, EOF)
    assert ref_cmp(b"", base[:100]) == (FRAME_IS_PREFIX, 0, 1, 0, 0, EOF, base[0]) and ref_cmp(base[:100], b"") == (OTHER_IS_PREFIX, 0, 1, 0, 0, base[0], EOF)
    check_pairs(engine, raws, others, compress, "lengths", device=True, dirty=True)


# ---- 3. the shifted tail -------------------------------------------------------------------------------------------------------------
SHIFTS = (1, 7, 8, 15, 16, 17, 33, S + 3)


def check_shifted(engine, corpus, compress=True):
    base = corpus.entry(8200, LEN1, 0)
    assert max(base) < 0x80
    mid = LEN1 // 2 + 1
    raws, others = [], []
    for k in SHIFTS:
        ins = base[:mid] + sc.needle_of(k) + base[mid:]                           # bytes >= 0x80: not in the corpus text
        raws += [base, ins, base]; others += [ins, base, base[:mid] + base[mid + k:]]
        r = ref_cmp(base, ins)
        assert r[:2] == (DIFFER, mid) and r[4] == LEN1 - mid and ref_cmp(ins, base)[4] == LEN1 - mid
        assert ref_cmp(raws[-1], others[-1])[1] >= mid and ref_cmp(raws[-1], others[-1])[4] <= LEN1 - mid - k
    # the mismatch of the backward pass one byte in front of and behind a slice seam of the content
    for p in (S - 1, S, 2 * S - 1, 2 * S):
        for shift in (5, 16):
            raws.append(base); others.append(b"#" * shift + flip(base, p))
            assert ref_cmp(raws[-1], others[-1])[4] == LEN1 - 1 - p
            raws.append(base); others.append(flip(base, p)[shift:])
            assert ref_cmp(raws[-1], others[-1])[4] == LEN1 - 1 - p
    # the overlap cap
    raws += [b"a" * 1000, b"a" * 1003, b"abcabc", b"abc", b"a" * (S + 7), b"a" * S]
    others += [b"a" * 1003, b"a" * 1000, b"abc", b"abcabc", b"a" * S, b"a" * (S + 7)]
    assert ref_cmp(b"a" * 1000, b"a" * 1003) == (FRAME_IS_PREFIX, 1000, 1, 0, 0, EOF, ord("a")) and ref_cmp(b"abcabc", b"abc") == (OTHER_IS_PREFIX, 3, 1, 0, 0, ord("a"), EOF)
    raws += [b"xabcabc", b"abcabx"]; others += [b"yabc", b"abx"]
    assert ref_cmp(b"xabcabc", b"yabc")[:5] == (DIFFER, 0, 1, 1, 3) and ref_cmp(b"abcabx", b"abx")[:5] == (DIFFER, 2, 1, 1, 1)
    # the other side's index goes negative inside a slice: at a step boundary, inside a step, in the content's last slice, and all of it
    for lb in (S + 104, S + 100, 500, 3, 16):
        raws.append(base); others.append(base[-lb:])
        r = ref_cmp(raws[-1], others[-1])
        assert r[0] == DIFFER and r[4] == min(lb, lb - r[1])
    assert (LEN1 - (S + 104)) % 16 == 0 and (LEN1 - (S + 100)) % 16 != 0
    raws += [b"0123456789abcdefXYZ", b"XYZ"]; others += [b"XYZ", b"0123456789abcdefXYZ"]
    check_pairs(engine, raws, others, compress, "shifted tail", device=True, dirty=True)


# ---- 4. carry paths ------------------------------------------------------------------------------------------------------------------
def check_carry(engine, corpus, compress=True):
    n40 = 40 * S - 77
    big = corpus.entry(8300, n40, 0)
    first, last = 5, 39 * S + 11
    assert big[first] != 10 and big[last] != 10
    raws = [big, big, big, big]
    others = [flip(big, first), flip(big, last), flip(big, first, last), big[:20 * S + 3] + b"\x80\x81\x82" + big[20 * S + 3:]]
    assert [ref_cmp(a, b)[1:5:3] for a, b in zip(raws, others)] == [(first, n40 - 1 - first), (last, n40 - 1 - last), (first, n40 - 1 - last), (20 * S + 3, n40 - 20 * S - 3)]
    check_pairs(engine, raws, others, compress, "40 slices")
    b33, b32 = corpus.entry(8301, 32 * S + 1, 0), corpus.entry(8302, 32 * S, 0)   # the wave folds 33 slices, the lane 32
    raws, others = [], []
    for d in (b33, b32):
        for pos in ((3,), (len(d) - 1,), (S + 9, len(d) - 2), ()):
            raws.append(d); others.append(put(d, [(p, bytes([d[p] ^ 0x80])) for p in pos]))
        raws.append(d); others.append(d[7:])
    check_pairs(engine, raws, others, compress, "32 and 33 slices")
    # both paths in one wave: frames the wave takes among frames of their lanes
    small = [corpus.entry(8310 + i, n, 0) for i, n in enumerate((0, 1, 5000, S + 17, 3 * S, 200, 70000))] * 10
    raws = small[:31] + [big] + small[31:50] + [b33] + small[50:] + [big[:35 * S + 1]]
    others = []
    for i, d in enumerate(raws):
        if i % 3 == 0 or len(d) < 2: others.append(d)
        elif i % 3 == 1: others.append(put(d, [(len(d) // 2, bytes([d[len(d) // 2] ^ 0x20]))]))
        else: others.append(d[:len(d) // 3] + b"\xf0" + d[len(d) // 3:])
    assert len(raws) == 73
    check_pairs(engine, raws, others, compress, "wave-path frames among lane-path ones")


# ---- 5. random edits -----------------------------------------------------------------------------------------------------------------
def random_pairs(count=300):
    rnd = random.Random(21)
    alphabet = b"ab\n \nxyz\x80\xc3"
    pairs = []
    for i in range(count):
        n = rnd.choice((0, 1, 15, 16, 17)) if i % 10 == 0 else rnd.randrange(0, 5001)
        a = bytes(rnd.choice(alphabet) for _ in range(n))
        b = bytearray(a)
        kind = i % 6
        if kind == 1: b = b[:rnd.randrange(0, n + 1)]
        elif kind == 2: b += bytes(rnd.choice(alphabet) for _ in range(rnd.randrange(1, 40)))
        elif kind >= 3:
            for _ in range(rnd.randrange(1, 4)):
                op, at = rnd.randrange(3), rnd.randrange(0, len(b) + 1)
                if op == 0 and at < len(b): b[at] = rnd.choice(alphabet)
                elif op == 1: b[at:at] = bytes(rnd.choice(alphabet) for _ in range(rnd.randrange(1, 20)))
                else: del b[at:at + rnd.randrange(1, 20)]
        pairs.append((a, bytes(b)))
    return pairs


def check_random(engine, compress=True):
    pairs = random_pairs()
    want = [ref_cmp(a, b) for a, b in pairs]
    assert {w[0] for w in want} == {EQUAL, DIFFER, FRAME_IS_PREFIX, OTHER_IS_PREFIX}
    assert any(w[0] == DIFFER and w[4] > 0 and len(a) != len(b) for w, (a, b) in zip(want, pairs)) and any(w[2] > 5 for w in want)
    check_pairs(engine, [a for a, _ in pairs], [b for _, b in pairs], compress, "random edits", device=True, dirty=True)


# ---- 6. bad frames -------------------------------------------------------------------------------------------------------------------
def check_bad_frames(engine, oracle, corpus, golden_frames, compress=True):
    raws = sc.small_entries(corpus, 600)
    frames, raw_lens, digests = sc.pack(engine, raws, compress=compress)
    ef, el, ee, er = vc.error_list(oracle, corpus, golden_frames)                  # committed libzstd frames: good, wrong checksum, bad magic, cut short,
    for j, at in enumerate((5, 100, 101, 299, 400, 500, 599)):                     # corrupt, wrong digest, wrong size
        frames.insert(at, ef[j]); raw_lens.insert(at, el[j]); digests.insert(at, ee[j]); raws.insert(at, er[j])
    others = []
    for i, d in enumerate(raws):
        if i % 4 == 0 or not d: others.append(d)
        elif i % 4 == 1: others.append(put(d, [(len(d) - 1, bytes([d[-1] ^ 1]))]))
        elif i % 4 == 2: others.append(d[:len(d) // 2])
        else: others.append(d + b"more\n")
    want_v = engine.verify(frames, raw_lens, digests)
    status = [st for _, st in want_v]
    assert [status[at] for at in (5, 100, 500)] == [_lib.FRAME_OK, _lib.FRAME_CHECKSUM, _lib.FRAME_DIGEST] and status[400] not in DECODED
    assert sum(st in DECODED for st in status) == len(raws) - 5
    want = [ref_cmp(d, o) if st in DECODED else ZERO for d, o, st in zip(raws, others, status)]
    assert want[500] != ZERO and want[100] == want[400] == ZERO and _lib.CMP_NONE == 0
    verdicts, got = engine.compare(frames, raw_lens, others, expect=digests)
    assert verdicts == want_v                                                      # status and digest are verify's
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, status[i], g, w)


# ---- 7. cut invariance, forms, handles and counters ----------------------------------------------------------------------------------
def check_cut_invariance(engine, corpus, compress=True):
    raws = sc.small_entries(corpus, 600) + [corpus.entry(8400 + i, 1 << 20, 0) for i in range(3)] + [corpus.entry(8410, 70000, 0), corpus.entry(8411, 40 * S + 9, 0)]
    others = []
    for i, d in enumerate(raws):
        if i % 3 == 0 or len(d) < 3: others.append(d)
        elif i % 3 == 1: others.append(put(d, [(len(d) * 2 // 3, bytes([d[len(d) * 2 // 3] ^ 2]))]))
        else: others.append(d[:len(d) // 2] + b"\xee" * 5 + d[len(d) // 2:])
    frames, raw_lens, digests = sc.pack(engine, raws, compress=compress)
    want = [ref_cmp(a, b) for a, b in zip(raws, others)]
    up = sum(len(f) for f in frames) + sum(len(o) for o in others)
    verdicts = [(d, _lib.FRAME_OK) for d in digests]
    assert engine.compare(frames, raw_lens, others, expect=digests) == (verdicts, want)
    assert vc.copy_counters(engine)[:2] == (up, 0)
    assert 0 < engine.compare_ms() <= engine.kernel_ms(_lib.T_TOTAL)
    assert engine.kernel_ms(_lib.T_WC) in (0.0, -1.0) and engine.kernel_ms(_lib.T_RANGE) in (0.0, -1.0)
    for mb in (2, 1):                                                              # two parts and more
        engine.set_parameter(_lib.PX_SCRATCH_MB, mb)
        try:
            assert engine.compare(frames, raw_lens, others, expect=digests) == (verdicts, want), mb
            assert vc.copy_counters(engine)[:2] == (up, 0)
            assert 0 < engine.compare_ms() <= engine.kernel_ms(_lib.T_TOTAL)
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
    engine.set_parameter(_lib.PX_STAGE_CHUNK, 65536)                               # many staged chunks
    try:
        assert engine.compare(frames, raw_lens, others, expect=digests) == (verdicts, want)
        assert vc.copy_counters(engine)[:2] == (up, 0)
        assert engine.compare_ms() > 0
    finally:
        engine.set_parameter(_lib.PX_STAGE_CHUNK, 0)
    d_frames, foff, _ = vc._arena(engine, frames)
    d_other, ooff = other_arena(engine, raws, others)
    try:
        exp = np.frombuffer(b"".join(digests), dtype=np.uint8)
        flen, olen = [len(f) for f in frames], [len(o) for o in others]
        assert engine.compare_device(d_frames, foff, flen, raw_lens, d_other, ooff, olen, exp) == (verdicts, want)
        assert vc.copy_counters(engine) == (0, 0, 0, 0)
        assert 0 < engine.compare_ms() <= engine.kernel_ms(_lib.T_TOTAL)
        engine.set_parameter(_lib.PX_SCRATCH_MB, 1)
        try:
            assert engine.compare_device(d_frames, foff, flen, raw_lens, d_other, ooff, olen, exp) == (verdicts, want)
            assert vc.copy_counters(engine) == (0, 0, 0, 0)
        finally:
            engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
        engine.verify_device(d_frames, foff, flen, raw_lens, exp)
        assert engine.compare_ms() <= 0
    finally:
        engine.free(d_frames)
        engine.free(d_other)
    # two handles, the batch dealt by index
    second = Engine(0, engine.lib_path)
    try:
        got = [None] * len(raws)
        for g, e in enumerate((engine, second)):
            v, r = e.compare(frames[g::2], raw_lens[g::2], others[g::2], expect=digests[g::2])
            assert v == verdicts[g::2]
            got[g::2] = r
        assert got == want
    finally:
        second.close()
    engine.verify(frames, raw_lens, digests)
    assert engine.compare_ms() <= 0                                                # nothing to report after any other call
    engine.count(frames[:3], raw_lens[:3])
    assert engine.compare_ms() <= 0 and engine.kernel_ms(_lib.T_WC) > 0
    engine.compare(frames[:3], raw_lens[:3], others[:3])
    assert engine.kernel_ms(_lib.T_WC) in (0.0, -1.0) and engine.compare_ms() > 0


# ---- 8. arguments --------------------------------------------------------------------------------------------------------------------
def raw_call(engine, packed, others, n=None, frame_len=None, other_len=None, **null):
    """zarc_gpu_compare_batch through ctypes; null: arguments to replace (None: NULL) -> (rc, results)"""
    c = ctypes
    frames, raw_lens, _ = packed
    m = len(frames)
    ptrs, lens = vc._ptrs(frames)
    optrs, olens = vc._ptrs(others)
    if frame_len is not None: lens = (c.c_size_t * m)(*frame_len)
    if other_len is not None: olens = (c.c_size_t * m)(*other_len)
    rl = (c.c_size_t * m)(*raw_lens)
    dig = np.zeros((m, 32), dtype=np.uint8)
    st = (c.c_int * m)()
    res = (_lib.Cmp * m)()
    a = dict(ptrs=ptrs, lens=lens, rl=rl, dig=dig.ctypes.data_as(c.c_void_p), st=st, res=res, optrs=optrs, olens=olens)
    a.update(null)
    rc = engine.lib.zarc_gpu_compare_batch(engine.h, m if n is None else n, a["ptrs"], a["lens"], a["rl"], None, a["optrs"], a["olens"], a["dig"], a["st"], a["res"])
    assert all(tuple(r.reserved) == (0, 0) and r.reserved0 == 0 for r in res)
    return rc, [(r.relation, r.prefix, r.line, r.differing, r.suffix, r.byte_a, r.byte_b) for r in res]


def check_arguments(engine, corpus):
    c = ctypes
    raw = corpus.entry(8500, 5000, 0)
    other = put(raw, [(3000, bytes([raw[3000] ^ 4]))])
    packed = sc.pack(engine, [raw])
    ok = raw_call(engine, packed, [other])
    assert ok == (_lib.OK, [ref_cmp(raw, other)]) and ok[1][0][:2] == (DIFFER, 3000)
    P, U = _lib.E_PARAM, _lib.E_UNSUPPORTED
    assert [raw_call(engine, packed, [other], **{k: None})[0] for k in ("ptrs", "lens", "rl", "dig", "st")] == [P] * 5   # verify's checks
    assert [raw_call(engine, packed, [other], **{k: None})[0] for k in ("res", "optrs", "olens")] == [P] * 3
    assert raw_call(engine, packed, [other], n=0)[0] == _lib.OK
    assert raw_call(engine, packed, [other], n=0, ptrs=None, lens=None, rl=None, dig=None, st=None, res=None, optrs=None, olens=None)[0] == _lib.OK
    assert raw_call(engine, (packed[0], [0xFFFFFFF0], packed[2]), [other])[0] == raw_call(engine, packed, [other], frame_len=[0xFFFFFFF0])[0] == U
    assert raw_call(engine, packed, [other], other_len=[1 << 32])[0] == raw_call(engine, packed, [other], other_len=[0xFFFFFFF0])[0] == U
    # other[i] may be NULL only where other_len[i] == 0
    null1 = (c.c_void_p * 1)(None)
    assert raw_call(engine, packed, [other], optrs=null1)[0] == P
    assert raw_call(engine, packed, [other], optrs=null1, other_len=[0]) == (_lib.OK, [ref_cmp(raw, b"")])
    # the device form
    lib, h = engine.lib, engine.h
    u64 = lambda v: (c.c_uint64 * 1)(v)
    dig = np.zeros((1, 32), dtype=np.uint8)
    pdig = dig.ctypes.data_as(c.c_void_p)
    st, res = (c.c_int * 1)(), (_lib.Cmp * 1)()
    dummy = c.c_void_p(16)  # never dereferenced: the call is refused before

    def dev(n=1, base=dummy, off=u64(0), fl=u64(9), rl=u64(0), obase=dummy, ooff=u64(0), olen=u64(0), pdig=pdig, st=st, res=res):
        return lib.zarc_gpu_compare_batch_device(h, n, base, off, fl, rl, None, obase, ooff, olen, pdig, st, res)
    assert dev(n=0, base=None, off=None, fl=None, rl=None, obase=None, ooff=None, olen=None, pdig=None, st=None, res=None) == _lib.OK
    assert dev(base=None) == dev(off=None) == dev(fl=None) == dev(rl=None) == dev(pdig=None) == dev(st=None) == P
    assert dev(res=None) == dev(obase=None) == dev(ooff=None) == dev(olen=None) == P
    assert dev(ooff=u64(8)) == dev(ooff=u64(17)) == P                              # pack's rule for device-resident sources
    assert dev(rl=u64(0xFFFFFFF0)) == dev(fl=u64(1 << 32)) == dev(olen=u64(1 << 32)) == U
    assert lib.zarc_gpu_abi_version() == 2
    # ... and the handle still works
    assert raw_call(engine, packed, [other]) == ok
    assert engine.compare(packed[0], packed[1], [other], expect=packed[2]) == ([(packed[2][0], _lib.FRAME_OK)], [ref_cmp(raw, other)])
