#!/usr/bin/env python3
"""Rates of zarc_gpu_search_batch* against zarc_gpu_verify_batch*, and against what a caller does without it: unpack through host memory,
then a scan of the bytes on one host thread.  Shapes: BASELINE configs[1] (10 000 x 1 MiB synthetic entries, level 3, checksum on) and
`small` (the million-entry log-normal shape of bench.py --config small).  Patterns: one that occurs nowhere, and one of the content that
occurs about once per 4 KiB (chosen from a sample of the corpus, its real count is recorded).  Every pair is measured alternating
A, B, A, B ... in this one process, --runs repetitions each after one warm-up of each; the document keeps min / median / max of each
side and the relative spread s = (max - min) / median of the A side, and for the search calls the medians of T_SEARCH, T_BLAKE3 and
T_XXH64 (device time of the kernels, summed over the parts of a call) with the judgement T_SEARCH <= T_BLAKE3 * (1 + s).
  usage: search_rate.py [--shapes c2,small] [--runs 5] [--out profiles/r09_search_rate.json]"""
import argparse, ctypes, hashlib, json, math, os, random, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,small")
ap.add_argument("--entries", type=int, default=0, help="entries of a shape (default: 10000 for c2, 1000000 for small)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--host-scan-runs", type=int, default=2, help="repetitions of unpack + host scan (slow: one thread over every byte)")
ap.add_argument("--out", default="")
a = ap.parse_args()
GIB = float(1 << 30)
c = ctypes
ABSENT = b"\x00\xfe\x01zarc-nowhere\xff\x02"


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def pair(name, run_a, run_b, nbytes, timers=None):
    """alternating A, B, A, B ...; rates in GiB/s of `nbytes` per call; timers(): device times of the B call just made"""
    run_a(); run_b()
    ra, rb, tm = [], [], []
    for _ in range(a.runs):
        t0 = time.perf_counter(); run_a(); ra.append(nbytes / (time.perf_counter() - t0) / GIB)
        t0 = time.perf_counter(); run_b(); rb.append(nbytes / (time.perf_counter() - t0) / GIB)
        if timers: tm.append(timers())
    A, B = summary(ra), summary(rb)
    s = (A["max"] - A["min"]) / A["median"]
    rec = {"A": A, "B": B, "spread_A": round(s, 4), "unit": "GiB/s of uncompressed bytes", "B_over_A_median": round(B["median"] / A["median"], 4)}
    if tm:
        med = {k: round(statistics.median(t[k] for t in tm), 3) for k in tm[0]}
        rec["kernel_ms_median_of_B"] = med
        rec["T_SEARCH_over_T_BLAKE3"] = round(med["T_SEARCH"] / med["T_BLAKE3"], 4) if med["T_BLAKE3"] > 0 else None
        rec["search_is_a_bandwidth_pass"] = bool(med["T_SEARCH"] <= med["T_BLAKE3"] * (1 + s))
        rec["search_kernel_tb_per_s"] = round(nbytes / (med["T_SEARCH"] / 1e3) / 1e12, 3) if med["T_SEARCH"] > 0 else None
    print("%s: A %s  B %s  s %.3f %s" % (name, A["all"], B["all"], s, rec.get("kernel_ms_median_of_B", "")), file=sys.stderr, flush=True)
    return rec


def sizes_of(shape):
    if shape == "small":
        rnd = random.Random(822)
        return [max(1, min(16 << 20, int(math.exp(rnd.gauss(math.log(822.0), 1.819))))) for _ in range(a.entries or 1000000)]
    return [1 << 20] * (a.entries or 10000)


def pick_frequent(sample, per=4096):
    """a 3- or 4-byte string of the sample whose count is nearest to one per `per` bytes"""
    rnd = random.Random(9)
    best, best_d = None, None
    for _ in range(400):
        at = rnd.randrange(0, len(sample) - 8)
        for m in (3, 4):
            p = bytes(sample[at:at + m])
            d = abs(math.log(max(sample.count(p), 0.5) * per / len(sample)))
            if best is None or d < best_d: best, best_d = p, d
    return best


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
    sample = bytes(eng.d2h(d_src, min(total, 4 << 20)))
    patterns = {"absent": ABSENT, "frequent": pick_frequent(sample)}
    doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
    assert (st == 0).all()
    eng.free(d_src)
    doc = {"entries": n, "uncompressed_bytes": raw, "compressed_bytes": int(dlen.sum()), "patterns": {k: v.hex() for k, v in patterns.items()}, "matches": {}}
    timers = lambda: {"T_SEARCH": eng.kernel_ms(_lib.T_SEARCH), "T_BLAKE3": eng.kernel_ms(_lib.T_BLAKE3), "T_XXH64": eng.kernel_ms(_lib.T_XXH64),
                      "T_DECODE": eng.kernel_ms(_lib.T_DECODE), "T_TOTAL": eng.kernel_ms(_lib.T_TOTAL)}
    # ---- device form: verify (A) against search (B)
    def verify_dev():
        d, s = eng.verify_device(d_dst, doff, dlen, lens, expect=dig); assert (s == 0).all()
    u64p = c.POINTER(c.c_uint64)
    digest, status = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    count, first = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    pexp, pdig, pst = dig.ctypes.data_as(c.c_void_p), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int))
    for name, pat in patterns.items():
        def search_dev():   # (the raw call: Engine.search_device builds a tuple per frame, a million of them here)
            assert lib.zarc_gpu_search_batch_device(h, n, c.c_void_p(d_dst), doff.ctypes.data_as(u64p), dlen.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), pexp,
                                                    c.cast(c.c_char_p(pat), c.c_void_p), len(pat), 0, pdig, pst, count.ctypes.data_as(u64p),
                                                    first.ctypes.data_as(u64p)) == 0 and (status == 0).all()
            doc["matches"][name] = int(count.sum())
        doc["device_verify_vs_search_" + name] = pair("%s device form, verify / search (%s)" % (shape, name), verify_dev, search_dev, raw, timers)
    assert doc["matches"]["absent"] == 0
    doc["bytes_per_frequent_match"] = round(raw / max(doc["matches"]["frequent"], 1), 1)
    # ---- host form, pageable: the frames dense in one host buffer; unpack's outputs in another
    fal = (dlen + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    foff = np.concatenate(([0], np.cumsum(fal)[:-1])).astype(np.uint64)
    ftotal = int(fal.sum())
    blob = eng.d2h(d_dst, int(doff[-1] + dlen[-1]))
    eng.free(d_dst)
    hf = np.zeros(ftotal + 64, dtype=np.uint8)
    for i in range(n):
        hf[int(foff[i]):int(foff[i]) + int(dlen[i])] = blob[int(doff[i]):int(doff[i]) + int(dlen[i])]
    del blob
    out = bytearray(total + 64)
    obase = c.addressof((c.c_char * len(out)).from_buffer(out))
    fptr, optr = (foff + np.uint64(hf.ctypes.data)), (off + np.uint64(obase))
    args_f = (fptr.ctypes.data_as(c.POINTER(c.c_void_p)), dlen.ctypes.data_as(c.POINTER(c.c_size_t)), lens.ctypes.data_as(c.POINTER(c.c_size_t)))
    counters = {}
    def verify_host():
        assert lib.zarc_gpu_verify_batch(h, n, *args_f, pexp, pdig, pst) == 0 and (status == 0).all()
    for name, pat in patterns.items():
        def search_host():
            assert lib.zarc_gpu_search_batch(h, n, *args_f, pexp, c.cast(c.c_char_p(pat), c.c_void_p), len(pat), 0, pdig, pst, count.ctypes.data_as(u64p),
                                             first.ctypes.data_as(u64p)) == 0 and (status == 0).all()
            assert int(count.sum()) == doc["matches"][name]
            counters[name] = [eng.copy_bytes(w) for w in range(4)]
        rec = pair("%s host form (pageable), verify / search (%s)" % (shape, name), verify_host, search_host, raw, timers)
        rec["copy_bytes_h2d_d2h_ring_direct"] = counters[name]
        doc["host_pageable_verify_vs_search_" + name] = rec
    # ---- what a caller does today: unpack through host memory, then one thread over the bytes (bytearray.count over the whole output
    # arena in one call: no per-entry slicing, so this side is flattered)
    today = {}
    for name, pat in patterns.items():
        rates, split = [], []
        for r in range(a.host_scan_runs + 1):
            t0 = time.perf_counter()
            assert lib.zarc_gpu_unpack_batch(h, n, *args_f, optr.ctypes.data_as(c.POINTER(c.c_void_p)), pexp, pdig, pst) == 0 and (status == 0).all()
            t1 = time.perf_counter()
            found = out.count(pat)
            t2 = time.perf_counter()
            if r: rates.append(raw / (t2 - t0) / GIB); split.append([round(t1 - t0, 3), round(t2 - t1, 3)])
        today[name] = {"rate": summary(rates), "seconds_unpack_scan": split, "matches_in_arena": found, "unit": "GiB/s of uncompressed bytes"}
        today[name]["search_over_today_median"] = round(doc["host_pageable_verify_vs_search_" + name]["B"]["median"] / today[name]["rate"]["median"], 2)
        print("%s unpack + host scan (%s): %s" % (shape, name, today[name]), file=sys.stderr, flush=True)
    doc["host_pageable_unpack_then_host_scan"] = today
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
