"""Cases for zarc_zge_seq_states (zge_entropy.hip): the FSE state chains of the blocks of a 1 MiB group that code with the same tables
run side by side on one wave, and pass 2 takes the states from the blocks' literal slots.  ZARC_GPU_PX_SEQ_STATES switches it: 0 = every
block's wave runs its own chains, 1 = on, N > 1 = on for blocks of fewer than N sequences.  No value may change a byte: every frame
must be bit-identical to the model (oracle.zge_encode) and decode with the oracle decoder, for every value.  Used twice: on the
emulator build and on the MI355X.

What the state kernel does with a frame follows from the table plan, and the plan can be read off the model's frame: each compressed
block's Symbol_Compression_Modes byte says per type (LL, OF, ML) 0 predefined, 1 RLE, 2 described here, 3 Repeat_Mode.  runs_of()
applies the kernel's rule to those: a block continues the run of the block in front of it if both have sequences to code and it
says 1 or 3 for every type; runs of at least MIN_RUN blocks whose sequence counts fit the capacity are taken.  (A block that pass 2
codes and that then ends up raw shows as a raw block here and counts as a break; for the kernel it ends a run one block later, which
no case relies on.)  check_cases_bite reads from this, on the CPU, that every case does what its name says.

The synthetic blocks are random bytes (raw literals) with planted repeats: a repeat is a copy of `length` bytes from `dist` back, so
a block's sequence count is the number of repeats planted, by construction; lengths, distances and the gaps between them cycle
through values with different codes, so that no type has a single code (which would be RLE mode) unless the case wants that."""
from zarc_amd import _lib

BLOCK = 65536
GROUP = 16                    # ZGE_TABLE_GROUP
MIN_RUN = 4                   # ZGE_STATE_MIN_RUN
TEXT, RANDOM = 0, 3           # corpus kinds (corpus.h)
LEVELS = (3, 9)


# ---- reading the plan off a frame ------------------------------------------------------------------------------------------------

def parse_blocks(frame):
    """-> one dict per block of a Zstandard frame: type ('raw', 'rle', 'comp'), nseq and modes (ll, of, ml) of a compressed block."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    single, fcs = (fhd >> 5) & 1, fhd >> 6
    at = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0), 2, 4, 8)[fcs]
    out = []
    while True:
        h = frame[at] | frame[at + 1] << 8 | frame[at + 2] << 16
        last, btype, size = h & 1, (h >> 1) & 3, h >> 3
        at += 3
        blk = {"type": ("raw", "rle", "comp")[btype], "nseq": 0, "modes": None}
        if btype == 2:
            p = at
            lt, sf = frame[p] & 3, (frame[p] >> 2) & 3
            if lt < 2:
                hdr = (1, 2, 1, 3)[sf]
                v = int.from_bytes(frame[p:p + hdr], "little")
                n = v >> (3 if hdr == 1 else 4)
                p += hdr + (n if lt == 0 else 1)
            else:
                hdr = (3, 3, 4, 5)[sf]
                bits = (10, 10, 14, 18)[sf]
                v = int.from_bytes(frame[p:p + hdr], "little")
                p += hdr + ((v >> (4 + bits)) & ((1 << bits) - 1))
            b0 = frame[p]
            if b0 == 0:
                nseq, p = 0, p + 1
            elif b0 < 128:
                nseq, p = b0, p + 1
            elif b0 < 255:
                nseq, p = ((b0 - 128) << 8) + frame[p + 1], p + 2
            else:
                nseq, p = frame[p + 1] + (frame[p + 2] << 8) + 0x7F00, p + 3
            blk["nseq"] = nseq
            if nseq:
                m = frame[p]
                blk["modes"] = (m >> 6, (m >> 4) & 3, (m >> 2) & 3)
        out.append(blk)
        at += 1 if btype == 1 else size
        if last:
            return out


def runs_of(blocks, cap=None):
    """-> (runs, taken): runs = [(first, count)] over the whole frame by the kernel's rule (a run ends at a group's end); taken = the
    set of block indexes whose states the kernel computes at capacity `cap` words (None: the slot's 16 400)."""
    cap = cap or (BLOCK + 64) // 4
    runs = []
    for g0 in range(0, len(blocks), GROUP):
        grp = blocks[g0:g0 + GROUP]
        if len(blocks) < 2:
            break
        b = 0
        while b < len(grp):
            if grp[b]["modes"] is None:
                b += 1
                continue
            e = b + 1
            while e < len(grp) and grp[e]["modes"] is not None and all(m in (1, 3) for m in grp[e]["modes"]):
                e += 1
            runs.append((g0 + b, e - b))
            b = e
    taken = set()
    for first, count in runs:
        fit = [i for i in range(first, first + count) if blocks[i]["nseq"] < cap]
        if len(fit) >= MIN_RUN:
            taken.update(fit)
    return runs, taken


# ---- building blocks -------------------------------------------------------------------------------------------------------------

class _Src:
    def __init__(self, corpus, seed):
        self.rnd, self.rat = corpus.entry(seed, 40 * BLOCK, RANDOM), 0
        self.txt, self.tat = corpus.entry(seed + 1, 80 * BLOCK, TEXT), 0

    def random(self, n):
        assert self.rat + n <= len(self.rnd)
        self.rat += n
        return self.rnd[self.rat - n:self.rat]

    def text(self, n=BLOCK):
        assert self.tat + n <= len(self.txt)
        self.tat += n
        return self.txt[self.tat - n:self.tat]


LENGTHS = (200, 48, 400, 100, 27, 300)        # match-length codes 43, 37, 44, 42, 24, 44
GAPS = (40, 9, 150, 20, 700, 3)               # literal-length codes 23, 9, 26, 18, 28, 3
DISTS = (900, 1900, 300, 1500, 600, 70)       # offset codes 9, 10, 8, 10, 9, 6
HEAD = 2000                                   # random bytes a block starts with: every distance above reaches into them at the least


def planted(src, k, lengths=LENGTHS, gaps=GAPS, dists=DISTS, fill=None, tail=True):
    """One block of k sequences, by construction: HEAD random bytes, then k - 1 times a gap of random bytes and a copy of `length`
    bytes from `dist` back, then one more gap and (tail) one byte value to the end of the block, which is ONE match at distance 1
    whatever its length (the pieces the finder cuts it into are joined again).  The finder leaves tiles out behind tiles in which it
    found nothing, so no stretch of random bytes here is longer than a tile (but with tail=False: plain random bytes to the end,
    k - 1 sequences at the most; what follows such a block must not rely on being searched at once)."""
    out = bytearray(src.random(HEAD))
    for i in range(k - 1):
        out += src.random(gaps[i % len(gaps)])
        d, n = dists[i % len(dists)], lengths[i % len(lengths)]
        for _ in range(n):           # byte by byte: a copy may overlap itself
            out.append(out[-d])
    out += src.random(gaps[(k - 1) % len(gaps)])
    assert len(out) + 64 <= BLOCK, (k, len(out))
    if not tail:
        return bytes(out + src.random(BLOCK - len(out)))
    return bytes(out) + bytes([(0x30 + k) & 0xFF if fill is None else fill]) * (BLOCK - len(out))   # (another value than the neighbours' tails)


def one_offset_code(src):
    """One block in which every match has the same offset code, 10: random gaps of 120 .. 190 bytes, each followed by a copy of 40 ..
    100 bytes FROM THE START OF AN EARLIER GAP between 1024 and 2044 bytes back (fresh random bytes that occur nowhere else, so the
    finder has one candidate), no two distances of four in a row equal (a repeated offset has another code), random bytes at the
    end for less than a tile."""
    out = bytearray(src.random(HEAD + 100))
    fresh = list(range(0, HEAD + 100, 150))       # starts of stretches of at least 100 fresh random bytes
    i = 0
    while len(out) + 400 < BLOCK:
        fresh.append(len(out))
        out += src.random(120 + 10 * (i % 8))
        n = 40 + 12 * (i % 6)
        f = [f for f in fresh if 1024 <= len(out) - f < 2045][0]      # the oldest; each start is used once (a second copy would find the first)
        fresh.remove(f)
        out += out[f:f + n]
        i += 1
    return bytes(out + src.random(BLOCK - len(out)))


# ---- the cases -------------------------------------------------------------------------------------------------------------------

GROUP_SIZES = (2, 3, 4, 5, 16, 17, 33)


def group_sizes(corpus):
    """Corpus text of 2 .. 33 blocks: runs below, at and above the minimum, a group of one block behind a full one, three groups."""
    return {"b%d" % n: _Src(corpus, 7000 + n).text(n * BLOCK) for n in GROUP_SIZES}


EDGE_COUNTS = (2, 63, 64, 65, 128, 3, 1)      # in frame order, behind one block of 100; the 1-sequence block codes every type in RLE mode
EDGE_ZERO_AT = 12                             # ... and a block without sequences further on


def round_edges(corpus):
    s = _Src(corpus, 7100)
    # (planted blocks throughout: next to text blocks the plan would not give them the group's tables)
    blocks = [planted(s, 100)] + [planted(s, k) for k in EDGE_COUNTS] + [planted(s, 100 + j) for j in range(4)] + [s.random(BLOCK)] + [planted(s, 90 + j) for j in range(3)]
    assert len(blocks) == GROUP and EDGE_ZERO_AT == 1 + len(EDGE_COUNTS) + 4
    return {"edges": b"".join(blocks)}


UNEVEN = (0, 30, 0, 0, 45, 0, 24, 0)          # 0 = a text block (thousands of sequences), k = k planted repeats


def uneven_run(corpus):
    s = _Src(corpus, 7200)
    return {"uneven": b"".join(s.text() if k == 0 else planted(s, k) for k in UNEVEN)}


BROKEN_AT = 5                                 # the odd block: five text blocks in front of it, five behind
BROKEN_KINDS = ("raw", "rle", "noseq", "unproven")


def _odd_block(s, kind):
    if kind == "raw":
        return s.random(BLOCK)                                  # nothing to find, literals stay raw: a raw block
    if kind == "rle":
        return b"\x5a" * BLOCK                                  # an RLE block
    if kind == "noseq":
        return bytes(b & 0x7F for b in s.random(BLOCK))         # 7-bit random bytes: Huffman literals, no match of 5 bytes
    # five repeats of 8 bytes behind gaps whose lengths take many extra bits: the block saves a few bytes, too few to prove it
    return planted(s, 6, lengths=(8, 8, 8), gaps=(700, 150, 40, 300), tail=False)


def broken_chain(corpus):
    out = {}
    for j, kind in enumerate(BROKEN_KINDS):
        s = _Src(corpus, 7300 + 10 * j)
        out[kind] = b"".join([s.text() for _ in range(BROKEN_AT)] + [_odd_block(s, kind)] + [s.text() for _ in range(5)])
    return out


RLE_BLOCKS = 6


def rle_modes(corpus):
    """of_rle: blocks whose offsets all have one code.  predefined: blocks of five sequences each, of two kinds in turn (short
    matches behind short gaps, long ones behind long gaps), so that for the literal lengths a table of the group's costs more than
    the blocks' own choices, which are the predefined table (a description would cost more than it saves): every block says
    Predefined_Mode for them and none continues a run."""
    s = _Src(corpus, 7400)
    of_rle = b"".join(one_offset_code(s) for _ in range(RLE_BLOCKS))
    pre = b"".join(planted(s, 5, lengths=(6, 7, 9, 11), gaps=(2, 5, 1, 7, 3), fill=j) if j & 1 else planted(s, 5, lengths=(300, 600, 150, 1000), gaps=(700, 300, 150, 90, 500), fill=j)
                   for j in range(RLE_BLOCKS))
    # ml_own: the same gaps and distances in every block but short matches in one and long ones in the next: the group's table serves
    # the literal lengths and the offsets (Repeat_Mode) and not the match lengths, which every block describes itself -- no run
    ml_own = b"".join(planted(s, 100 + j, lengths=(6, 7, 9, 11, 8, 10) if j & 1 else (300, 600, 150, 1000, 200, 400), gaps=(40, 9, 150, 20, 200, 3))
                      for j in range(RLE_BLOCKS))
    return {"of_rle": of_rle, "predefined": pre, "ml_own": ml_own}


CAPACITIES = (2, 64, 65, 1000)


def capacity(corpus):
    """The frame of round_edges, not corpus text: every block of text has thousands of sequences, so each of the capacities 2, 64,
    65 and 1000 would turn all of them down alike.  This frame's run holds blocks of 1, 2, 3, 63, 64, 65, 100 and 128 sequences:
    each capacity turns down some blocks of a group whose other blocks are taken, and 64 / 65 fall on both sides of a full round."""
    return round_edges(corpus)


def mixed_batch(corpus):
    """Everything above in one call, plus one-block frames (the one-pass kernel) and a frame of 4 MiB + 1 byte (searched in 2 MiB
    segments): one sub-batch with every kernel of the stage in it."""
    out = {}
    for g in ("group_sizes", "round_edges", "uneven_run", "broken_chain", "rle_modes"):
        out.update({"%s.%s" % (g, k): v for k, v in GROUPS[g](corpus).items()})
    s = _Src(corpus, 7500)
    out["one_text"] = s.text(50000)
    out["one_planted"] = planted(s, 64)
    out["empty"] = b""
    out["seg"] = s.text(32 * BLOCK) + s.text(32 * BLOCK) + b"!"
    return out


GROUPS = {"group_sizes": group_sizes, "round_edges": round_edges, "uneven_run": uneven_run, "broken_chain": broken_chain, "rle_modes": rle_modes}
LEVEL9 = ("round_edges", "uneven_run", "rle_modes")   # the cheap ones: one frame of at most 16 blocks, or synthetic blocks only


def group_sizes_small(corpus):
    """The frames of group_sizes up to five blocks (the emulator's share: the runs around the minimum)."""
    return {k: v for k, v in made(corpus, "group_sizes").items() if int(k[1:]) <= 5}


def plan(emu=False):
    """(group, level, PX_SEQ_STATES): every group at level 3 with the switch at 0 and 1, the cheap ones at level 9 as well, capacity
    at its four values, the mixed batch at level 3.  emu: what the emulator build runs -- the synthetic groups and the text frames
    of up to five blocks; the frames of 16, 17 and 33 blocks and the mixed batch with its 4 MiB frame take the emulator minutes and
    the device a second, so they are left to the device."""
    if emu:
        out = [(g, 3, px) for g in ("group_sizes_small", "round_edges", "uneven_run", "rle_modes") for px in (0, 1)] + [("broken_chain", 3, 1)]
        out += [(g, 9, 1) for g in LEVEL9]
        return out + [("capacity", 3, n) for n in CAPACITIES]
    out = [(g, 3, px) for g in GROUPS for px in (0, 1)]
    out += [(g, 9, px) for g in LEVEL9 for px in (0, 1)]
    out += [("capacity", 3, n) for n in CAPACITIES]
    out += [("mixed_batch", 3, px) for px in (0, 1)]
    return out


ALL = dict(GROUPS, capacity=capacity, mixed_batch=mixed_batch, group_sizes_small=group_sizes_small)
_made, _model = {}, {}


def made(corpus, group):
    if group not in _made:
        _made[group] = ALL[group](corpus)
    return _made[group]


def model(oracle, corpus, group, level):
    """The model's frames of a group, computed once and shared."""
    if (group, level) not in _model:
        p = oracle.params(level=level)
        _model[(group, level)] = {k: oracle.zge_encode(raw, p) for k, raw in made(corpus, group).items()}
    return _model[(group, level)]


def check_frames(engine, oracle, corpus, group, level, px):
    """One batch at `level` with ZARC_GPU_PX_SEQ_STATES = px: every frame equals the model's and decodes to its source."""
    cases, want = made(corpus, group), model(oracle, corpus, group, level)
    names = list(cases)
    engine.set_parameter(_lib.P_COMPRESSION_LEVEL, level)
    engine.set_parameter(_lib.PX_SEQ_STATES, px)
    try:
        res = engine.pack([cases[k] for k in names])
    finally:
        engine.set_parameter(_lib.P_COMPRESSION_LEVEL, 3)
        engine.set_parameter(_lib.PX_SEQ_STATES, 1)
    for k, (frame, dig) in zip(names, res):
        raw = cases[k]
        assert dig == oracle.blake3(raw), (group, k, level, px)
        assert frame == want[k], (group, k, level, px)                                       # bit-exact vs the CPU model
        rc, out, used = oracle.zstd_decode(frame, len(raw))
        assert rc == 0 and used == len(frame) and out == raw, (group, k, level, px)          # valid Zstandard


TAKEN_CASES = (("group_sizes_small", "b3", 1), ("group_sizes_small", "b4", 1), ("round_edges", "edges", 1), ("round_edges", "edges", 2),
               ("round_edges", "edges", 64), ("uneven_run", "uneven", 1), ("broken_chain", "unproven", 1),
               ("broken_chain", "rle", 1), ("rle_modes", "of_rle", 1), ("rle_modes", "predefined", 1), ("rle_modes", "ml_own", 1))


def taken_expected(oracle, corpus, group, k, px):
    """Blocks whose states the state kernel computes for one frame at ZARC_GPU_PX_SEQ_STATES = px, by runs_of() on the model's frame:
    what the diagnostic build's count of taken blocks must equal (none of these frames has a block that pass 2 codes and that ends
    up raw, where runs_of() and the kernel differ)."""
    blocks = parse_blocks(model(oracle, corpus, group, 3)[k])
    return len(runs_of(blocks, px if px > 1 else None)[1])


def check_cases_bite(oracle, corpus):
    """The cases do what their names say, judged by the model's frames alone (level 3)."""
    def look(group, k):
        blocks = parse_blocks(model(oracle, corpus, group, 3)[k])
        return (blocks,) + runs_of(blocks)

    # group_sizes: nothing taken below four blocks, everything from four on; at 16 blocks at least 12 lie in a taken run; the group of
    # one block behind a full one (17) is not taken; three groups (33) have taken runs in the first two
    for n in GROUP_SIZES:
        blocks, runs, taken = look("group_sizes", "b%d" % n)
        assert len(blocks) == n and all(b["type"] == "comp" and b["nseq"] > 1000 for b in blocks), n
        if n < MIN_RUN:
            assert not taken, (n, runs)
        else:
            assert len([i for i in taken if i < GROUP]) >= min(n, GROUP) * 3 // 4, (n, runs)
    blocks, runs, taken = look("group_sizes", "b4")
    assert runs == [(0, 4)], runs                                      # a run of exactly the minimum
    blocks, runs, taken = look("group_sizes", "b17")
    assert 16 not in taken and (16, 1) in runs, runs
    blocks, runs, taken = look("group_sizes", "b33")
    assert any(i in taken for i in range(16, 32)) and 32 not in taken, runs
    # round_edges: the planted blocks have the sequence counts planted, all of them lie in ONE taken run with coded (not RLE) types
    # but the 1-sequence block, which codes nothing with a table and ends the run; the block without sequences is a break
    blocks, runs, taken = look("round_edges", "edges")
    assert [b["nseq"] for b in blocks[1:1 + len(EDGE_COUNTS)]] == list(EDGE_COUNTS), [b["nseq"] for b in blocks]
    assert (0, 2 + len(EDGE_COUNTS)) not in runs and runs[0] == (0, 1 + len(EDGE_COUNTS)) and all(i in taken for i in range(1 + len(EDGE_COUNTS))), runs
    for i, k in enumerate(EDGE_COUNTS):
        if k > 1:
            assert all(m == 3 for m in blocks[1 + i]["modes"]), (k, blocks[1 + i])
    assert blocks[len(EDGE_COUNTS)]["modes"] == (1, 1, 1), blocks[len(EDGE_COUNTS)]
    assert blocks[EDGE_ZERO_AT]["modes"] is None and EDGE_ZERO_AT not in taken and not any(r[0] <= EDGE_ZERO_AT < r[0] + r[1] for r in runs)
    # uneven_run: one taken run with a few dozen sequences next to thousands
    blocks, runs, taken = look("uneven_run", "uneven")
    run = max(runs, key=lambda r: r[1])
    inside = [blocks[i]["nseq"] for i in range(run[0], run[0] + run[1])]
    assert run[1] >= MIN_RUN and min(inside) < 50 and max(inside) > 2000 and all(i in taken for i in range(run[0], run[0] + run[1])), (runs, inside)
    # broken_chain: a taken run in front of the odd block and one that starts behind it
    for kind in BROKEN_KINDS:
        blocks, runs, taken = look("broken_chain", kind)
        odd = blocks[BROKEN_AT]
        if kind == "raw":
            assert odd["type"] == "raw"
        elif kind == "rle":
            assert odd["type"] == "rle"
        elif kind == "noseq":
            assert odd["type"] == "comp" and odd["nseq"] == 0
        else:
            assert odd["type"] == "comp" and odd["nseq"] > 0 and 2 in blocks[BROKEN_AT + 1]["modes"], (odd, blocks[BROKEN_AT + 1])  # the table is described again behind it
        assert (BROKEN_AT + 1, 5) in runs and all(i in taken for i in range(BROKEN_AT + 1, BROKEN_AT + 6)), (kind, runs)
        assert any(r[0] == 0 and r[1] >= BROKEN_AT for r in runs) and all(i in taken for i in range(BROKEN_AT)), (kind, runs)
    # rle_modes: the offsets are in RLE mode in a taken run; the predefined blocks keep mode 0 and are left to pass 2
    blocks, runs, taken = look("rle_modes", "of_rle")
    assert all(b["modes"][1] == 1 and b["modes"][0] != 1 and b["modes"][2] != 1 for b in blocks), [b["modes"] for b in blocks]
    assert len(taken) >= MIN_RUN, runs
    blocks, runs, taken = look("rle_modes", "predefined")
    assert all(b["modes"][0] == 0 for b in blocks) and not taken, [b["modes"] for b in blocks]   # the literal lengths keep theirs: no run
    blocks, runs, taken = look("rle_modes", "ml_own")
    assert all(b["modes"][:2] == (3, 3) and b["modes"][2] in (0, 2) for b in blocks[1:]) and not taken, [b["modes"] for b in blocks]
    # capacity: which blocks of the round_edges run still fit
    blocks = parse_blocks(model(oracle, corpus, "capacity", 3)["edges"])
    fit = {n: sorted(blocks[i]["nseq"] for i in runs_of(blocks, n)[1]) for n in CAPACITIES}
    assert fit[2] == [] and fit[64] == [1, 2, 3, 63] and fit[65] == [1, 2, 3, 63, 64] and fit[1000][:6] == [1, 2, 3, 63, 64, 65] and fit[1000][-1] == 128, fit
