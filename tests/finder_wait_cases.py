"""Cases for the places where the match finder issues and waits for its memory requests (zge_match.hip: the window of tile T+2 is
requested behind tile T's S4 barrier and parked in a register, the far entries of tile T+1 in S3 of tile T).  Every case is the
smallest shape at which one of the paths that carry such a request across a tile, block, segment or frame boundary can go wrong.
Used twice: on the emulator build (which guards the bookkeeping -- which tile a parked word belongs to) and on the MI355X (where a
request consumed before it has arrived shows up as a frame that differs from the model's).

Every frame must be bit-identical to the model (oracle.zge_encode), decode with the oracle decoder and with every libzstd on the box:
the same triple as parity_cases.check_pack."""
from zarc_amd import _lib

TILE = 1024
BLOCK = 65536
TEXT, LZ, RANDOM = 0, 2, 3   # corpus kinds (corpus.h)

# first tile loaded on the spot, no tile T+1, no tile T+2, the far table off / on at 64 KiB, the first tile of a second block
THRESHOLD_SIZES = (0, 1, 7, 8, 11, 12, 1023, 1024, 1025, 2047, 2048, 2049, 65535, 65536, 65537, 66560, 131073)


def thresholds(corpus):
    c = {}
    for i, n in enumerate(THRESHOLD_SIZES):
        c["text_%d" % n] = corpus.entry(900 + i, n, TEXT)
        c["lz_%d" % n] = corpus.entry(940 + i, n, LZ)
    return c


def passed_tile(corpus):
    """A long match carries the cursor over tile boundaries while the next windows are staged / parked."""
    a = corpus.entry(980, 5000, TEXT)
    c = {"text_copy3000_text": a + a[700:3700] + corpus.entry(981, 4000, TEXT)}
    # the same cut inside the copy: the frame's last tile (200 bytes at 5120) lies inside the match that starts in the tile before it, so
    # the cursor is at or behind its end when the tile begins (pos >= tend: the tile leaves before S0, with a window parked for it)
    b = corpus.entry(982, 4696, TEXT)
    c["cut_inside_copy"] = (b + b[100:3100])[:5 * TILE + 200]
    return c


def cold(corpus):
    """Unsearched tiles (after two searched tiles in a row without a match the next 1, 3, then 7 tiles are skipped) and the way back:
    the first searched tile behind a stretch finds neither its window nor its far entries requested ahead."""
    c = {"rand_text_rand_text": corpus.entry(983, 40000, RANDOM) + corpus.entry(984, 5000, TEXT) + corpus.entry(985, 20000, RANDOM) + corpus.entry(986, 8000, TEXT)}
    # Tile 0 is text (a match: the count starts at 0), tiles 1 .. 63 are random: searched 1, 2 | skipped 3 | searched 4 | skipped 5 - 7 |
    # searched 8 | skipped 9 - 15 | searched 16, 24 .. 56 | skipped 57 - 63.  So tile 64, the FIRST TILE OF THE SECOND BLOCK, is the first
    # searched tile behind unsearched ones; it is text and ends the stretch.  Tiles 65 .. 71 are random again: searched 65, 66 | skipped 67 |
    # searched 68 | skipped 69 - 71, and tile 72 -- 500 bytes of text, THE LAST TILE OF THE FRAME -- is once more the first searched tile behind
    # a stretch: it asks for its far entries late (the frame is larger than 64 KiB: the far table is on) and nothing follows it.
    t0 = corpus.entry(987, TILE, TEXT)
    c["cut_at_block_and_frame_end"] = t0 + corpus.entry(988, 63 * TILE, RANDOM) + corpus.entry(989, TILE, TEXT) + corpus.entry(990, 7 * TILE, RANDOM) + corpus.entry(991, 500, TEXT)
    assert len(c["cut_at_block_and_frame_end"]) == 72 * TILE + 500 and 64 * TILE == BLOCK
    return c


def rle_between(corpus):
    """Prefetch registers are carried across a block that is skipped as a whole, and a far repeat lies behind it."""
    t = corpus.entry(992, BLOCK, TEXT)
    return {"text_zeros_text": t + bytes(BLOCK) + t}


def segment(corpus):
    """2 MiB + 5000 bytes in one frame with a repeat 1 MiB back: the tables restart at 2 MiB (the slab is cleared with requests of the
    old segment in flight), and the last tiles repeat bytes that lie in the old segment."""
    a = corpus.entry(993, 1 << 20, TEXT)
    return {"seg_2m_5000": a + a + a[:5000]}


def many_entries(corpus, n):
    """n entries whose sizes cycle through what makes a workgroup change its path from one frame to the next (kinds round-robin)."""
    sizes = (3000, 1024, 70000, 1, 2049, 0, 66000)
    return [corpus.entry(2000 + i, sizes[i % len(sizes)], -1) for i in range(n)]


def check_frames(engine, oracle, libzstds, cases, level=3):
    """cases: name -> bytes.  Packs them in one batch at `level` and checks every frame three ways."""
    assert libzstds, "no libzstd on this box: the cross-decoding half of this check would be vacuous"
    names = list(cases)
    params = oracle.params(level=level)
    engine.set_parameter(_lib.P_COMPRESSION_LEVEL, level)
    try:
        res = engine.pack([cases[k] for k in names])
    finally:
        engine.set_parameter(_lib.P_COMPRESSION_LEVEL, 3)
    for k, (frame, dig) in zip(names, res):
        raw = cases[k]
        assert dig == oracle.blake3(raw), (k, level)
        assert frame == oracle.zge_encode(raw, params), (k, level)          # bit-exact vs the CPU model
        rc, out, used = oracle.zstd_decode(frame, len(raw))
        assert rc == 0 and used == len(frame) and out == raw, (k, level)    # valid Zstandard
        for z in libzstds:
            got, err = z.decompress(frame, len(raw))
            assert got == raw, (k, level, z.version, err)


def check_many(engine, oracle, libzstds, corpus, n):
    """The batch once in order and once reversed: state that a workgroup carries from one frame to the next in registers (a parked
    window word, far entries asked for ahead) would make a frame depend on its neighbours.  Every frame equals the model's both times."""
    assert libzstds
    ents = many_entries(corpus, n)
    want = [oracle.zge_encode(e) for e in ents]
    fwd = engine.pack(ents)
    rev = engine.pack(ents[::-1])[::-1]
    for i, raw in enumerate(ents):
        assert fwd[i][0] == want[i], ("forward", i, len(raw))
        assert rev[i][0] == want[i], ("reversed", i, len(raw))
        assert fwd[i][1] == rev[i][1] == oracle.blake3(raw), i
        rc, out, used = oracle.zstd_decode(want[i], len(raw))
        assert rc == 0 and used == len(want[i]) and out == raw, i
        for z in libzstds:
            got, err = z.decompress(want[i], len(raw))
            assert got == raw, (i, z.version, err)


GROUPS = {"thresholds": thresholds, "passed_tile": passed_tile, "cold": cold, "rle_between": rle_between, "segment": segment}
LEVEL_GROUPS = ("thresholds", "passed_tile", "cold")   # these run at levels 1 and 9 as well: the fast and the deep instantiation


def plan():
    """What check() runs, as (group, level) pairs: every group at level 3, the first three at levels 1 and 9 as well.  The test files
    parametrise over this list, so a group added to GROUPS / LEVEL_GROUPS runs in check() and in the suites alike."""
    return [(g, 3) for g in GROUPS] + [(g, level) for level in (1, 9) for g in LEVEL_GROUPS]


def check(engine, oracle, corpus, libzstds, many):
    """Everything: the pairs of plan(), then `many` entries in both orders."""
    made = {}
    for g, level in plan():
        if g not in made:
            made[g] = GROUPS[g](corpus)
        check_frames(engine, oracle, libzstds, made[g], level=level)
    check_many(engine, oracle, libzstds, corpus, many)


def check_positions_past_2g(engine):
    """One entry of 2 GiB + 3 MiB + 5000 bytes, device-resident (2052 corpus entries of 1 MiB, kinds round-robin, laid end to end and
    packed as ONE entry): frame positions are unsigned 32-bit, and the window of a tile is fetched at `frame base + position` -- an
    offset that is sign-extended on the way reads 4 GiB in front of the entry for every tile past 2^31.  The model cannot encode 2 GiB in
    a test's time, so the check is the round trip: the frame decodes on the device to bytes with the source's BLAKE3 (literals are
    copied out of the staged windows: a window from elsewhere gives other bytes)."""
    mib = 1 << 20
    n = (1 << 31) + 3 * mib + 5000
    parts = (n + mib - 1) // mib
    off = [i * mib for i in range(parts)]
    lens = [min(mib, n - o) for o in off]
    cap = engine.bound(n)
    ptrs = [engine.malloc(n + _lib.PAD), engine.malloc(cap + _lib.PAD), engine.malloc(n + _lib.PAD)]
    d_src, d_dst, d_out = ptrs
    try:
        engine.corpus_fill(d_src, off, lens, first_index=9100, kind=-1)
        want = engine.blake3_device(d_src, [0], [n])
        doff, dlen, dig, st = engine.pack_device(d_src, [0], [n], d_dst, cap)
        assert int(st[0]) == 0 and 0 < int(dlen[0]) <= cap
        assert bytes(dig[0]) == bytes(want[0])
        dig2, st2 = engine.unpack_device(d_dst, doff, dlen, d_out, [0], [n], expect=dig)
        assert int(st2[0]) == _lib.FRAME_OK
        assert bytes(dig2[0]) == bytes(want[0])
        assert bytes(engine.blake3_device(d_out, [0], [n])[0]) == bytes(want[0])
    finally:
        for q in ptrs:
            engine.free(q)
