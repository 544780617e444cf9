#!/usr/bin/env python3
"""What a set of patterns costs in one pass (zarc_gpu_search_set_batch_device) against K one-pattern calls
(zarc_gpu_search_batch_device) and against verify alone (zarc_gpu_verify_batch_device), frames resident in HBM, one device.
Shapes: BASELINE configs[1] (10 000 x 1 MiB synthetic entries, level 3, checksum on) and `small` (the million-entry log-normal shape of
bench.py --config small).  Sets: K = 1, 2, 4, 16, 64, 256, 1024 random 8-byte patterns that occur nowhere (asserted), and one set of
8-byte strings cut from about 1 % of the frames, one each (`planted`; the share of frames with a match is recorded).
Every K is measured in rounds of verify, one one-pattern call, the set call and -- for K <= 16 -- K one-pattern calls one after the
other, --runs rounds after one warm-up round; the document keeps min / median / max of the wall clock of each and the median of
T_SEARCH of the one-pattern and the set call.  Beyond K = 16 the K calls are not run: K x the one-call median, labelled `derived`.
`crossover`: the smallest K at which the set call's median is below the K calls' (measured or derived).
  usage: set_rate.py [--shapes c2,small] [--runs 5] [--out profiles/r11_set_rate.json]"""
import argparse, ctypes, hashlib, json, math, os, random, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,small")
ap.add_argument("--entries", type=int, default=0, help="entries of a shape (default: 10000 for c2, 1000000 for small)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--ks", default="1,2,4,16,64,256,1024")
ap.add_argument("--out", default="")
a = ap.parse_args()
c = ctypes
MEASURED_UP_TO = 16


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def sizes_of(shape):
    if shape == "small":
        rnd = random.Random(822)
        return [max(1, min(16 << 20, int(math.exp(rnd.gauss(math.log(822.0), 1.819))))) for _ in range(a.entries or 1000000)]
    return [1 << 20] * (a.entries or 10000)


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
    eng.corpus_fill(d_src, off, lens, first_index=0, kind=-1)
    # the planted set: 8 bytes from the middle of every 100th frame that has them (at most 1024: the largest set)
    step = max(100, (n + 1023) // 1024)
    planted = []
    for i in range(0, n, step):
        if int(lens[i]) >= 64: planted.append(bytes(eng.d2h(d_src + int(off[i]) + int(lens[i]) // 2, 8)))
    planted = sorted(set(planted))[:1024]
    doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
    assert (st == 0).all()
    eng.free(d_src)
    print("%s: %d entries, %d bytes packed" % (shape, n, raw), file=sys.stderr, flush=True)
    u64p = c.POINTER(c.c_uint64)
    digest, status = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    count, first, which = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    pexp, pdig, pst = dig.ctypes.data_as(c.c_void_p), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int))
    frames = (c.c_void_p(d_dst), doff.ctypes.data_as(u64p), dlen.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), pexp)
    out = (pdig, pst, count.ctypes.data_as(u64p), first.ctypes.data_as(u64p))

    def verify():
        assert lib.zarc_gpu_verify_batch_device(h, n, *frames, pdig, pst) == 0 and (status == 0).all()

    def single(pat):   # (the raw calls: Engine's wrappers build a tuple per frame, a million of them here)
        assert lib.zarc_gpu_search_batch_device(h, n, *frames, c.cast(c.c_char_p(pat), c.c_void_p), len(pat), 0, *out) == 0 and (status == 0).all()
        return int(count.sum())

    def set_call(ps, hits):
        assert lib.zarc_gpu_search_set_batch_device(h, n, *frames, c.byref(ps), 0, *out, which.ctypes.data_as(u64p), hits) == 0 and (status == 0).all()
        return int(count.sum())

    def clock(f, *args):
        t0 = time.perf_counter()
        r = f(*args)
        return (time.perf_counter() - t0) * 1e3, r

    doc = {"entries": n, "uncompressed_bytes": raw, "compressed_bytes": int(dlen.sum()), "unit": "ms of wall clock per call (T_SEARCH: device time of the scan kernels)", "sets": {}}
    rnd = random.Random(11)
    cases = [("K=%d" % k, [bytes(rnd.randrange(256) for _ in range(8)) for _ in range(k)], True) for k in (int(v) for v in a.ks.split(","))]
    if planted: cases.append(("planted", planted, False))
    for name, pats, absent in cases:
        K = len(pats)
        ps = _lib.PatternSet.of(pats)
        hits = (c.c_uint64 * K)()
        rows = {"verify": [], "one_call": [], "set_call": [], "k_calls": []}
        t_one, t_set = [], []
        for r in range(a.runs + 1):
            tv, _ = clock(verify)
            t1, m1 = clock(single, pats[0])
            ts1 = eng.kernel_ms(_lib.T_SEARCH)
            tk, mk = clock(set_call, ps, hits)
            tss = eng.kernel_ms(_lib.T_SEARCH)
            tks = None
            if K <= MEASURED_UP_TO:
                t0 = time.perf_counter()
                per = [single(p) for p in pats]
                tks = (time.perf_counter() - t0) * 1e3
                assert list(hits) == per, "hits of the set call against the K one-pattern calls"
            if absent: assert mk == 0 and m1 == 0, "a random pattern occurs in the content"
            if r == 0: continue   # warm-up
            rows["verify"].append(tv); rows["one_call"].append(t1); rows["set_call"].append(tk); t_one.append(ts1); t_set.append(tss)
            if tks is not None: rows["k_calls"].append(tks)
        rec = {"patterns": K, "verify": summary(rows["verify"]), "one_call": summary(rows["one_call"]), "set_call": summary(rows["set_call"]),
               "T_SEARCH_one_call_median": round(statistics.median(t_one), 3), "T_SEARCH_set_call_median": round(statistics.median(t_set), 3)}
        if rows["k_calls"]: rec["k_calls"] = dict(summary(rows["k_calls"]), how="measured")
        else: rec["k_calls"] = {"median": round(K * rec["one_call"]["median"], 3), "how": "derived: K x the one-call median"}
        rec["set_over_verify_median"] = round(rec["set_call"]["median"] / rec["verify"]["median"], 4)
        rec["set_minus_verify_ms"] = round(rec["set_call"]["median"] - rec["verify"]["median"], 3)
        rec["k_calls_over_set_median"] = round(rec["k_calls"]["median"] / rec["set_call"]["median"], 3)
        rec["scan_tb_per_s"] = round(raw / (rec["T_SEARCH_set_call_median"] / 1e3) / 1e12, 3) if rec["T_SEARCH_set_call_median"] > 0 else None
        if not absent:
            rec["positions_matched"] = mk
            rec["frames_with_a_match"] = int((count > 0).sum())
            rec["share_of_frames_with_a_match"] = round(rec["frames_with_a_match"] / n, 5)
        doc["sets"][name] = rec
        print("%s %s: verify %.1f  one %.1f  set %.1f  K calls %.1f (%s)  T_SEARCH one %.2f set %.2f" % (
            shape, name, rec["verify"]["median"], rec["one_call"]["median"], rec["set_call"]["median"], rec["k_calls"]["median"], rec["k_calls"]["how"].split(":")[0],
            rec["T_SEARCH_one_call_median"], rec["T_SEARCH_set_call_median"]), file=sys.stderr, flush=True)
    below = [r["patterns"] for k, r in doc["sets"].items() if k != "planted" and r["set_call"]["median"] < r["k_calls"]["median"]]
    doc["crossover"] = {"smallest_K_with_the_set_call_below_K_calls": min(below) if below else None}
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
