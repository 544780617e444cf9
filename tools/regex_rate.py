#!/usr/bin/env python3
"""What a regular-expression search costs (zarc_gpu_search_regex_batch_device) against the fixed-string search of the same literal
(zarc_gpu_search_batch_device) and against verify alone (zarc_gpu_verify_batch_device), frames resident in HBM, one device.
Shapes: `c2` (BASELINE configs[1]: 10 000 x 1 MiB synthetic entries, level 3, checksum on), `small` (the million-entry log-normal shape of
bench.py --config small) and `nolf` (1 MiB entries of the corpus' printable kind, which holds no 0x0A -- the tool counts them and records the
number: every 256-byte chunk then needs its transition table).
Per shape, rounds of: verify; the fixed-string search of a literal cut from the content; the regex search of the same literal (the answers
must be equal, asserted); an expression with `.*`; an anchored one.  --runs rounds after one warm-up round, the calls alternating inside a
round; the document keeps min / median / max of the wall clock of each, the median of T_SEARCH, and the states of every expression.
  usage: regex_rate.py [--shapes c2,small,nolf] [--entries N] [--runs 5] [--out profiles/r12_regex_rate.json]"""
import argparse, ctypes, hashlib, json, math, os, random, re, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,small,nolf")
ap.add_argument("--entries", type=int, default=0, help="entries of a shape (default: 10000 for c2, 1000000 for small, 2000 for nolf)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()
c = ctypes


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def sizes_of(shape):
    if shape == "small":
        rnd = random.Random(822)
        return [max(1, min(16 << 20, int(math.exp(rnd.gauss(math.log(822.0), 1.819))))) for _ in range(a.entries or 1000000)]
    return [1 << 20] * (a.entries or (2000 if shape == "nolf" else 10000))


def shape_doc(shape):
    eng = Engine(0)
    eng.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    eng.set_parameter(_lib.P_COMPRESSION_LEVEL, 3)
    lib, h = eng.lib, eng.h
    lens = np.array(sizes_of(shape), dtype=np.uint64)
    n = len(lens)
    al = (lens + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    off = np.concatenate(([0], np.cumsum(al)[:-1])).astype(np.uint64)
    total, raw = int(al.sum()), int(lens.sum())
    blocks = np.maximum((lens + np.uint64(65535)) // np.uint64(65536), np.uint64(1))
    cap = int(((lens + np.uint64(3) * blocks + np.uint64(18 + 15)) // np.uint64(16) * np.uint64(16)).sum())   # sum of zarc_gpu_bound()
    d_src, d_dst = eng.malloc(total + _lib.PAD), eng.malloc(cap + _lib.PAD)
    eng.corpus_fill(d_src, off, lens, first_index=0, kind=2 if shape == "nolf" else -1)
    big = next(i for i in range(n) if int(lens[i]) >= 4096)
    sample = bytes(eng.d2h(d_src + int(off[big]), 4096))
    word = next((m.group() for m in re.finditer(rb"[A-Za-z]{6,8}", sample[2048:])), sample[2048:2055])   # the literal: a word of the content
    doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
    assert (st == 0).all()
    eng.free(d_src)
    print("%s: %d entries, %d bytes packed, literal %r" % (shape, n, raw, word), file=sys.stderr, flush=True)
    u64p = c.POINTER(c.c_uint64)
    digest, status = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    count, first = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    pexp, pdig, pst = dig.ctypes.data_as(c.c_void_p), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int))
    frames = (c.c_void_p(d_dst), doff.ctypes.data_as(u64p), dlen.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), pexp)
    out = (pdig, pst, count.ctypes.data_as(u64p), first.ctypes.data_as(u64p))

    def verify():
        assert lib.zarc_gpu_verify_batch_device(h, n, *frames, pdig, pst) == 0 and (status == 0).all()

    def call(fn, pat):   # (the raw calls: Engine's wrappers build a tuple per frame, a million of them here)
        assert fn(h, n, *frames, c.cast(c.c_char_p(pat), c.c_void_p), len(pat), 0, *out) == 0 and (status == 0).all()
        return int(count.sum()), count.copy(), first.copy()

    def clock(f, *args):
        t0 = time.perf_counter()
        r = f(*args)
        return (time.perf_counter() - t0) * 1e3, r

    esc = re.escape
    exprs = {"literal_fixed": None, "literal_regex": esc(word), "dot_star": esc(word[:3]) + b".*" + esc(word[-2:]), "anchored": b"^" + esc(word[:3]) + b"|" + esc(word[-3:]) + b"$"}
    line_feeds = call(lib.zarc_gpu_search_batch_device, b"\n")[0]
    doc = {"entries": n, "uncompressed_bytes": raw, "compressed_bytes": int(dlen.sum()), "line_feeds": line_feeds, "literal": word.decode("latin-1"),
           "unit": "ms of wall clock per call (T_SEARCH: device time of the search kernels)", "calls": {}}
    rows = {k: [] for k in ["verify"] + list(exprs)}
    t_search = {k: [] for k in exprs}
    matches = {}
    for r in range(a.runs + 1):
        tv, _ = clock(verify)
        got = {}
        for name, rx in exprs.items():
            t, got[name] = clock(call, lib.zarc_gpu_search_batch_device if rx is None else lib.zarc_gpu_search_regex_batch_device, word if rx is None else rx)
            if r: rows[name].append(t); t_search[name].append(eng.kernel_ms(_lib.T_SEARCH))
            matches[name] = got[name][0]
        assert got["literal_fixed"][0] == got["literal_regex"][0] and (got["literal_fixed"][1] == got["literal_regex"][1]).all() and \
            (got["literal_fixed"][2] == got["literal_regex"][2]).all(), "the regex search of a literal against the fixed-string search"
        if r: rows["verify"].append(tv)
    doc["calls"]["verify"] = summary(rows["verify"])
    for name, rx in exprs.items():
        rec = dict(summary(rows[name]), T_SEARCH_median=round(statistics.median(t_search[name]), 3), positions_matched=matches[name])
        if rx is not None:
            rec["expression"] = rx.decode("latin-1")
            rec["states"] = eng.regex_compile(rx)[0]
        rec["over_verify_median"] = round(rec["median"] / doc["calls"]["verify"]["median"], 4)
        rec["scan_gb_per_s"] = round(raw / (rec["T_SEARCH_median"] / 1e3) / 1e9, 1) if rec["T_SEARCH_median"] > 0 else None
        doc["calls"][name] = rec
        print("%s %s: %.1f ms (verify %.1f)  T_SEARCH %.2f ms  %s GB/s" % (shape, name, rec["median"], doc["calls"]["verify"]["median"], rec["T_SEARCH_median"], rec["scan_gb_per_s"]),
              file=sys.stderr, flush=True)
    eng.free(d_dst)
    eng.close()
    return doc


doc = {"runs": a.runs, "library_sha16": hashlib.sha256(open(_lib.DEFAULT_LIB, "rb").read()).hexdigest()[:16], "shapes": {}}
for shape in a.shapes.split(","):
    doc["shapes"][shape] = shape_doc(shape)
text = json.dumps(doc, indent=1, sort_keys=True)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
