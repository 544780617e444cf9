"""Cases for the backward offers of the match finder (S4 at the top of zge_parse_round.h).  A match whose source and target agree on
b bytes in front of it offers itself to the b positions before it: the source posts ONE word, G = (score + bias) << 6 | 63 plus
OFFER_C times its tile position, to ex[] of every target (ds_max), and a target takes OFFER_C times its own position off the winner.
What can go wrong there: the order of two offers that reach one target (score first, then the nearer source), an offer that would
land in front of the tile, the block or the frame, the targets of a wave's first positions (they belong to the wave in front), the
far candidates' longer reach (9 .. 48 bytes, the loop behind the eight straight-line distances), and a wave in which every position
offers.  Every case is the smallest shape at which one of these can go wrong.  Used twice: on the emulator build and on the MI355X.

Every frame must be bit-identical to the model (oracle.zge_encode) and decode with the oracle decoder, at levels 1, 3, 9 and 15.

How the inputs steer the finder (level 3: one near table on the 5-byte hash, the most recent position with a hash wins; a match must
score above 0, score = 5 * length - 12 - floor(log2(offset))): a DECOY is a short copy of some bytes of the text that lies between an
older occurrence and the text itself, so the positions whose five bytes it holds find the decoy instead of the older occurrence.  A
decoy more than 8 KiB back hides it without giving a match at all: five bytes at that distance score 0."""
import ctypes

import finder_barrier_cases as fb

TILE = fb.TILE
BLOCK = fb.BLOCK
WAVE_SPAN = fb.WAVE_SPAN
RANDOM = fb.RANDOM
TEXT = fb.TEXT
LEVELS = (1, 3, 9, 15)


class _Rnd:
    """Random bytes of one corpus entry, handed out piece by piece (no piece is handed out twice), and text to fill the room between
    the pieces: tiles of text are searched, while behind two tiles of random bytes the finder skips tiles (its cold stretches)."""

    def __init__(self, corpus, seed):
        self.data, self.at = corpus.entry(seed, 8192, RANDOM), 0
        self.text, self.tat = corpus.entry(seed + 50000, 1 << 17, TEXT), 0

    def take(self, n):
        assert self.at + n <= len(self.data)
        self.at += n
        return self.data[self.at - n:self.at]

    def fill(self, n):
        assert n >= 0 and self.tat + n <= len(self.text)
        self.tat += n
        return self.text[self.tat - n:self.tat]


# ---- dense_offers ----------------------------------------------------------------------------------------------------------------

DENSE_LEN = 288      # of S: at any alignment a whole wave span (128 positions) lies inside the copy
DENSE_AT = (0, 1, 63, 64, 65, 127)


def _dense(corpus, seed, at):
    """S, then a decoy for every position i >= 1 of S in DESCENDING order of i (S[i-1 : i+5] and two other bytes), then a copy of S
    whose first byte lies at tile position `at`.  Position i of the copy finds its five bytes in decoy i (the most recent place that
    holds them; decoy i + 1 holds them too but lies further back): a 5-byte match with one equal byte in front of it.  The distances
    grow by 9 from one position to the next, so no position is a follower of its neighbour: every position of the copy offers, and
    every position adopts its neighbour's match (6 bytes beat 5).  All distances stay below 4 KiB."""
    r = _Rnd(corpus, seed)
    s = r.take(DENSE_LEN)
    decoys = b"".join(s[i - 1:i + 5] + r.take(2) for i in range(DENSE_LEN - 5, 0, -1))
    head = r.take(40) + s + decoys
    head += r.take((at - len(head)) % TILE)
    return head + s + r.take(100)


def dense_offers(corpus):
    return {"at_%d" % a: _dense(corpus, 4000 + a, a) for a in DENSE_AT}


# ---- tie_and_order ---------------------------------------------------------------------------------------------------------------

TIE_AT = (200, 62, 63, 126, 127)     # tile position of the target: inside a chunk, its sources in the next chunk, in the next wave
TIE_KINDS = ("far_stronger", "near_stronger", "equal")


def _two_offers(corpus, seed, at, kind):
    """Target t (tile position `at` of the frame's sixth tile), offered to by t + 1 and by t + 2.  W is the text at t.  Three decoys:
    B = W[0 : 2 + lb] lies furthest back: position t + 2 finds it (lb bytes, two equal bytes in front);
    A = W[0 : 6] lies nearer: position t + 1 finds it (5 bytes, one equal byte in front; A does not hold the five bytes of t + 2);
    C = W[0 : 5] lies nearest: position t finds it and not A, so t has a match of its own that is no copy of an offer (5 bytes at a
    short distance: both offers beat it).
    The offer of t + 1 scores 5 * 6 - 12 - log2(dA), that of t + 2 scores 5 * (lb + 2) - 12 - log2(dB).  With dA in [64, 128):
    far_stronger: lb = 8; near_stronger: lb = 5 and dB in [4096, 8192); equal: lb = 5 and dB in [2048, 4096) -- 12 on both sides, and
    the nearer source, t + 1, must win (the model's ascending k with sc > best_score).  No seed was searched: the distances give the
    scores; check_cases_bite reads the winner off the model's sequences."""
    r = _Rnd(corpus, seed)
    lb = 8 if kind == "far_stronger" else 5
    d_b = 5000 if kind == "near_stronger" else 2600
    t = 5 * TILE + at
    w = r.take(40)
    dec_b, dec_a, dec_c = w[:2 + lb] + r.take(3), w[:6] + r.take(3), w[:5] + r.take(3)
    p_b, p_a, p_c = t - d_b, t - 100, t - 40
    out = r.fill(p_b - 4) + r.take(4) + dec_b
    out += r.fill(p_a - 4 - len(out)) + r.take(4) + dec_a
    out += r.take(p_c - len(out)) + dec_c
    out += r.take(t - len(out)) + w + r.take(60)
    return out


def tie_expect(at, kind):
    """(frame position, match length, offset) of the sequence the target must start."""
    t = 5 * TILE + at
    return (t, 10, 2600) if kind == "far_stronger" else (t, 6, 100)


def tie_and_order(corpus):
    return {"%s_%d" % (kind, at): _two_offers(corpus, 4100 + 10 * j + i, at, kind) for j, kind in enumerate(TIE_KINDS) for i, at in enumerate(TIE_AT)}


# ---- clipped ---------------------------------------------------------------------------------------------------------------------

FAR_HIDE = 8192 + 64   # a decoy this far back hides an older occurrence and gives no match itself


def _reach_back(corpus, seed, at, body=20, tail=60, last=None):
    """Z = 8 bytes and a body.  Z lies early in the frame; behind it a decoy for each of the eight 5-byte windows that start in the
    first 8 bytes of Z; more than 8 KiB further on, the copy of Z with the BODY's first byte at frame position `at`.  The body finds Z
    (its windows have no decoy) with 8 equal bytes in front of it; the 8 positions in front of the body find their decoys, which are
    too far back to be a match: they have no match of their own and take what the body offers them -- those of them that the offer
    may reach.  The room in between is zero bytes: they all share one slot of the near table, so every decoy is still in it when the
    copy comes (text would have overwritten most of them), and their tiles find matches, so the finder does not skip tiles on the
    way.  last: the frame ends `last` bytes behind the body."""
    r = _Rnd(corpus, seed)
    z = r.take(8 + body)
    out = r.take(24) + z + r.take(8)
    for j in range(8):
        out += r.take(1) + z[j:j + 5] + r.take(2)
    assert at - 8 - len(out) >= FAR_HIDE
    out += bytes(at - 16 - len(out)) + r.take(8) + z
    return out + r.take(tail if last is None else last)


# name -> (frame position of the body's first byte, reach: how many of the 8 positions in front of it the offer may reach, keywords)
CLIPPED = {}
for _i in range(1, 8):                                   # the offers further back would land in front of the tile
    CLIPPED["tile_%d" % _i] = (9 * TILE + _i, _i, {})
for _i in (1, 4, 7):                                     # the model cuts `back` at the block start
    CLIPPED["block_%d" % _i] = (BLOCK + _i, _i, {})
for _w, _i in ((1, 0), (1, 3), (4, 7), (7, 1)):          # the first positions of a wave: nothing is cut, the targets belong to the wave in front
    CLIPPED["wave_%d_%d" % (_w, _i)] = (9 * TILE + WAVE_SPAN * _w + _i, 8, {})
CLIPPED["last_tile_5"] = (9 * TILE + 5, 5, {"last": 300})                    # a short last tile
CLIPPED["last_tile_end"] = (9 * TILE + 130, 8, {"body": 12, "last": 0})     # the frame ends with the body
# position 0 of a tile and of a block: every target lies in front of it and nothing is offered
CLIPPED_NONE = {"tile_0": (9 * TILE, 0, {}), "block_0": (BLOCK, 0, {})}


def clipped(corpus):
    return {k: _reach_back(corpus, 4200 + j, at, **kw) for j, (k, (at, reach, kw)) in enumerate(CLIPPED.items())}


def clipped_none(corpus):
    return {k: _reach_back(corpus, 4270 + j, at, **kw) for j, (k, (at, reach, kw)) in enumerate(CLIPPED_NONE.items())}


def clipped_expect(spec):
    """(frame position, match length, offset) of the sequence that takes the body: it starts `reach` positions in front of it."""
    at, reach, kw = spec
    return (at - reach, kw.get("body", 20) + reach, at - 32)


# ---- far_tail --------------------------------------------------------------------------------------------------------------------

def far_tail(corpus):
    """A far candidate that reaches back more than 8 bytes offers over a wave edge (finder_barrier_cases._adopted_at with far=True):
    the adopting position at 128 k for the k that adopted_edge does not use."""
    return {"far_%d" % k: fb._adopted_at(corpus, 4300 + 4 * k, WAVE_SPAN * k, True) for k in (2, 3, 5, 6)}


GROUPS = {"dense_offers": dense_offers, "tie_and_order": tie_and_order, "clipped": clipped, "clipped_none": clipped_none, "far_tail": far_tail}


def plan():
    """(group, level) pairs: every group at levels 1, 3, 9 and 15."""
    return [(g, level) for g in GROUPS for level in LEVELS]


check_frames = fb.check_frames


def sequences(oracle, frame, n):
    """(frame position of the match, match length, offset) of every sequence of a frame, from the oracle decoder's trace."""
    seqs = []
    proto = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32)
    cb = proto(lambda ctx, pos, ll, ml, off: seqs.append((pos, ml, off)))
    hook = ctypes.c_void_p.in_dll(oracle.lib, "oracle_zstd_trace")
    hook.value = ctypes.cast(cb, ctypes.c_void_p).value
    try:
        rc, out, used = oracle.zstd_decode(frame, n)
    finally:
        hook.value = None
    assert rc == 0 and len(out) == n
    return seqs


def check_cases_bite(oracle, made):
    """The cases do what their names say, judged by the model alone (level 3).  Without backward propagation every dense_offers,
    tie_and_order and clipped frame differs; with the far candidates held to 8 bytes every far_tail frame differs.  The text that
    fills these frames adopts matches of its own, so the model's sequences are read as well.  dense_offers: the copy is parsed as
    6-byte matches, each at the distance of the position behind it (adopted).  tie_and_order: the target starts the sequence of the
    source that must win.  clipped: the sequence that takes the body starts at the first position its offer may reach (clipped_none:
    at the body itself)."""
    p3 = oracle.params(level=3)
    model = {g: {k: oracle.zge_encode(raw, p3) for k, raw in made[g].items()} for g in made}
    for g in ("dense_offers", "tie_and_order", "clipped"):
        for k, raw in made[g].items():
            assert oracle.zge_encode(raw, oracle.params(level=3, back_cap=0)) != model[g][k], (g, k)
    for k, raw in made["far_tail"].items():
        assert oracle.zge_encode(raw, oracle.params(level=3, far_back=8)) != model["far_tail"][k], k
    for k, raw in made["dense_offers"].items():
        start = len(raw) - 100 - DENSE_LEN
        # adopted: 6 bytes at the distance of the position behind.  A few positions lose their decoy to another hash in the table's
        # 2^15 slots and offer nothing; the position in front of such a one keeps its own 5 bytes.
        adopted = [s for s in sequences(oracle, model["dense_offers"][k], len(raw))
                   if start <= s[0] < start + DENSE_LEN and s[1] == 6 and s[2] == _dense_dist(start, s[0] - start + 1)]
        assert len(adopted) >= 40, (k, len(adopted))             # 240 of the copy's 288 bytes
    for kind in TIE_KINDS:
        for at in TIE_AT:
            k = "%s_%d" % (kind, at)
            seqs = sequences(oracle, model["tie_and_order"][k], len(made["tie_and_order"][k]))
            assert tie_expect(at, kind) in seqs, (k, [s for s in seqs if abs(s[0] - tie_expect(at, kind)[0]) < 12])
    for g, specs in (("clipped", CLIPPED), ("clipped_none", CLIPPED_NONE)):
        for k, spec in specs.items():
            seqs = sequences(oracle, model[g][k], len(made[g][k]))
            assert clipped_expect(spec) in seqs, (g, k, clipped_expect(spec), seqs[-3:])


def _dense_dist(start, i):
    """Distance of copy position i to its five bytes in decoy i: the decoys start 40 + DENSE_LEN into the frame, 8 bytes each, decoy
    DENSE_LEN - 5 first, and hold the five bytes from their second byte on."""
    return start + i - (40 + DENSE_LEN + 8 * (DENSE_LEN - 5 - i) + 1)
