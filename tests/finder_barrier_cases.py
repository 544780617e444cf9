"""Cases for the barriers of the match finder's tile loop (zge_match.hip, zge_parse_round.h).  The level-3 and the fast finder have none
between adoption and the lazy rule: the rule takes the next position's final score from the next lane, for the last position of a
wave's 128 it works the score of another wave's position out by itself, and the chunk exits of the parse walk live in a1[] so that
ex[] keeps the offers for a wave that is still adopting.  The barrier at the top of the tile publishes the cursor and the two recent
offsets for the next tile; the hand-over cases are the net for it.  Every case is the smallest shape at which one of these can go
wrong.  Used twice: on the emulator build, whose fibres run a wave ahead of where no barrier holds it, and on the MI355X.

Every frame must be bit-identical to the model (oracle.zge_encode) and decode with the oracle decoder, at levels 1, 3 and 9 (the fast,
the level-3 and the deep instantiation); the deep case runs at level 15 as well."""
from zarc_amd import _lib

TILE = 1024
BLOCK = 65536
WAVE_SPAN = 128               # positions of one wave: two adjacent 64-position chunks
TEXT, RECORDS, LZ, RANDOM = 0, 1, 2, 3   # corpus kinds (corpus.h)
LEVELS = (1, 3, 9)


def wave_edge_sweep(corpus):
    """One text-like block of 3 KiB behind 0 .. 129 filler bytes, 130 entries: every alignment of its matches against the wave edges
    (positions 127 / 128, 255 / 256, ...) and the tile edges (1023 / 1024, 2047 / 2048) occurs, so the lazy rule reads a neighbour in
    the next lane, in the wave's second chunk and in another wave at every match boundary of the text."""
    text = corpus.entry(3000, 3 * TILE, TEXT)
    filler = corpus.entry(3001, 129, RANDOM)
    return {"shift_%d" % k: filler[:k] + text for k in range(130)}


def _adopted_at(corpus, seed, edge, far):
    """A frame in which position `edge` adopts the backward extension of the match found at edge + 1, and position edge - 1 has a short
    match of its own: whether edge - 1 is taken depends on the FINAL score of `edge` (the adopted one; its own would let it stand).
    S (64 bytes) lies early in the frame; a decoy x + S[:5] + junk lies between S and the copy: at the copy's first byte the 5-byte hash
    leads to the decoy (the most recent position with that hash, a 5-byte match), one byte on it leads to S + 1, whose match extends one
    byte backwards.  far: S lies more than 64 KiB in front of the copy, out of the near table's reach, so the match comes from a
    sampled far position some bytes into the copy and reaches back over all of them (more than 8)."""
    rnd = corpus.entry(seed, 4096 + (BLOCK + 4096 if far else 0), RANDOM)
    s, x, junk = rnd[:64] if not far else rnd[:160], rnd[200:201], rnd[300:320]
    decoy = x + s[:5] + junk
    if far:
        head = corpus.entry(seed + 1, 200, TEXT) + s + corpus.entry(seed + 2, BLOCK + 1500, TEXT)   # text: the tiles in between are searched
        head = head[:len(head) - (len(head) % TILE)]
    else:
        head = corpus.entry(seed + 1, 300, TEXT) + s + corpus.entry(seed + 2, 200, TEXT)
        head = head + rnd[400:400 + (-len(head)) % TILE]
    assert len(head) % TILE == 0
    body = rnd[1000:1000 + 40] + decoy
    body = body + rnd[1100:1100 + edge - 1 - len(body)]
    assert len(body) == edge - 1
    return head + body + x + s + rnd[2000:2300]


def adopted_edge(corpus):
    """The adopting position at 128 k, k = 1 .. 7 (the first position of wave k: the last position of wave k - 1 reads its final score),
    near and far."""
    c = {}
    for k in range(1, 8):
        c["near_%d" % k] = _adopted_at(corpus, 3100 + 4 * k, WAVE_SPAN * k, False)
    for k in (1, 4, 7):
        c["far_%d" % k] = _adopted_at(corpus, 3200 + 4 * k, WAVE_SPAN * k, True)
    return c


DISTANCES = (210, 333, 419, 505)   # of the copies: near enough for a recent-offset guess of the next tile (offset <= position in the tile + 256)


class _Frame:
    """A frame built tile by tile.  A tile of kind 0 is random bytes; kinds 1 and 2 carry that many copies of 40 bytes in their second
    half, each at its own distance; "many" is text with five.  In front of its copies every such tile repeats 4 bytes at the distance of
    the second-to-last and of the last copy placed so far: too short for the hash table (5 bytes), so only the recent offsets handed
    over by the tile before find them -- a wrong hand-over loses a match and the frame differs from the model's."""

    def __init__(self, corpus, seed):
        self.corpus, self.seed, self.data, self.placed = corpus, seed, bytearray(), []

    def repeat(self, at, dist, n):
        if at - dist >= 0 and at + n <= len(self.data):
            self.data[at:at + n] = self.data[at - dist:at - dist + n]
            return True
        return False

    def raw(self, data):
        self.data += data
        return self

    def tile(self, kind, n=TILE):
        base = len(self.data)
        self.seed += 1
        self.data += self.corpus.entry(self.seed, n, TEXT if kind == "many" else RANDOM)
        if kind == 0:
            return self
        for j, d in enumerate(self.placed[-2:]):
            self.repeat(base + 300 + 100 * j, d, 4)
        for j in range(5 if kind == "many" else kind):
            d = DISTANCES[(self.seed + j) % len(DISTANCES)]
            if self.repeat(base + 520 + 90 * j, d, 40):
                self.placed.append(d)
        return self

    def bytes(self):
        return bytes(self.data)


def rep_handover(corpus):
    """The recent offsets one tile hands to the next: tiles with 0, 1, 2 and many selected matches in every order of two, behind a cold
    stretch, behind tiles the cursor passed, across the first tile of a second block and into the last short tile of a frame."""
    kinds = (0, 1, 2, "many")
    c = {}
    f = _Frame(corpus, 3300).tile(2)
    for a in kinds:
        for b in kinds:
            f.tile(a).tile(b)
    c["pairs"] = f.bytes()
    # searched without a match: tiles 1, 2 | skipped 3 | searched 4 | skipped 5 - 7 | then two matches, one, many, and a short last tile
    f = _Frame(corpus, 3340).tile(2)
    for k in [0] * 7 + [2, 1, "many", 1]:
        f.tile(k)
    c["behind_cold"] = f.tile(2, 450).bytes()
    # a copy of 2500 bytes carries the cursor over tiles; then one match, none, two
    a = corpus.entry(3360, 3 * TILE, TEXT)
    f = _Frame(corpus, 3361).tile(2).raw(a + a[100:2600]).tile(1, 3 * TILE - 2500).tile(1).tile(0).tile(2).tile(1)
    assert len(f.data) == 11 * TILE
    c["behind_passed"] = f.bytes()
    # the last tiles of a block and the first of the next: 2 -> 1 | 1 -> many -> 0 -> 2, and a last tile of 450 bytes
    f = _Frame(corpus, 3370).raw(corpus.entry(3370, BLOCK - 3 * TILE, LZ)).tile(1).tile(2).tile(1)
    assert len(f.data) == BLOCK
    c["second_block"] = f.tile(1).tile("many").tile(0).tile(2).tile(1, 450).bytes()
    return c


def ext_latch(corpus):
    """A repeat of 900 bytes found through the far table (it lies 66 KiB back): its tile sets K_LONG and re-parses, the tiles behind
    it do not.  A second one further on sets it again."""
    a = corpus.entry(3400, BLOCK + 2 * TILE, TEXT)
    return {"long_far_repeat": a + a[500:1400] + corpus.entry(3401, 3 * TILE, TEXT) + a[4000:4700] + corpus.entry(3402, 2 * TILE + 100, TEXT)}


def deep_rounds(corpus):
    """Records and LZ-like data: at level >= 9 the live recent-offset rounds change matches (checked against the model without
    them in check_cases_bite), so the included parse runs more than once per tile."""
    return {"records": corpus.entry(3500, 20 * TILE + 300, RECORDS), "lz": corpus.entry(3501, 12 * TILE + 5, LZ)}


GROUPS = {"wave_edge_sweep": wave_edge_sweep, "adopted_edge": adopted_edge, "rep_handover": rep_handover, "ext_latch": ext_latch,
          "deep_rounds": deep_rounds}


def plan():
    """(group, level) pairs: every group at levels 1, 3 and 9, the deep case at 15 as well."""
    return [(g, level) for g in GROUPS for level in LEVELS] + [("deep_rounds", 15)]


def check_frames(engine, oracle, cases, level):
    """cases: name -> bytes.  One batch at `level`; every frame equals the model's and decodes to its source."""
    names = list(cases)
    params = oracle.params(level=level)
    engine.set_parameter(_lib.P_COMPRESSION_LEVEL, level)
    try:
        res = engine.pack([cases[k] for k in names])
    finally:
        engine.set_parameter(_lib.P_COMPRESSION_LEVEL, 3)
    for k, (frame, dig) in zip(names, res):
        raw = cases[k]
        assert len(raw) <= 80 * 1024, (k, len(raw))
        assert dig == oracle.blake3(raw), (k, level)
        assert frame == oracle.zge_encode(raw, params), (k, level)          # bit-exact vs the CPU model
        rc, out, used = oracle.zstd_decode(frame, len(raw))
        assert rc == 0 and used == len(frame) and out == raw, (k, level)    # valid Zstandard


def check_cases_bite(oracle, made):
    """The cases do what their names say, judged by the model alone: without backward propagation the adopted-edge frames differ,
    without the extension round the long repeat's frame differs, without the live rounds the deep frames differ."""
    for k, raw in made["adopted_edge"].items():
        assert oracle.zge_encode(raw, oracle.params(level=3, back_cap=0)) != oracle.zge_encode(raw, oracle.params(level=3)), k
    for k, raw in made["ext_latch"].items():
        assert oracle.zge_encode(raw, oracle.params(level=3, ext_cap=0)) != oracle.zge_encode(raw, oracle.params(level=3)), k
    for level in (9, 15):
        for k, raw in made["deep_rounds"].items():
            assert oracle.zge_encode(raw, oracle.params(level=level, rep_pass=0)) != oracle.zge_encode(raw, oracle.params(level=level)), (k, level)
