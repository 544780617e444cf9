#!/usr/bin/env python3
"""Rates of zarc_gpu_search_lines_batch* against zarc_gpu_search_batch*, and against what a caller does without it: unpack through host
memory, then a scan of the same bytes line by line on one host thread.  Shapes: BASELINE configs[1] (10 000 x 1 MiB synthetic entries,
level 3, checksum on) and `small` (the million-entry log-normal shape of bench.py --config small).  Needle densities: `none` (occurs
nowhere), `per_mib` (a string of the content whose count is nearest to one per MiB; its real count is recorded) and `every` (the byte that
lies in the largest share of a sample's lines; that share is recorded).  Every pair is measured alternating A, B, A, B ... in this one
process, --runs repetitions each after one warm-up of each; the document keeps min / median / max of each side, the relative spread
s = (max - min) / median of the A side, the medians of T_LINES next to T_SEARCH (device time, summed over the parts of a call), the
lines found and delivered, and for the host form the bytes that came back (D2H).  rec_cap and max_line bound what one call delivers.
  usage: lines_rate.py [--shapes c2,small] [--entries N] [--runs 5] [--rec-cap 1048576] [--max-line 256] [--out profiles/r10_lines_rate.json]"""
import argparse, ctypes, hashlib, json, math, os, random, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,small")
ap.add_argument("--entries", type=int, default=0, help="entries of a shape (default: 10000 for c2, 1000000 for small)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--host-scan-runs", type=int, default=1, help="repetitions of unpack + host scan (slow: one thread over every byte)")
ap.add_argument("--rec-cap", type=int, default=1 << 20)
ap.add_argument("--max-line", type=int, default=256)
ap.add_argument("--out", default="")
a = ap.parse_args()
GIB = float(1 << 30)
c = ctypes
ABSENT = b"\x00\xfe\x01zarc-nowhere\xff\x02"


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def pair(name, run_a, run_b, nbytes, timers):
    """alternating A, B, A, B ...; rates in GiB/s of `nbytes` per call; timers(): device times of the B call just made"""
    run_a(); run_b()
    ra, rb, tm = [], [], []
    for _ in range(a.runs):
        t0 = time.perf_counter(); run_a(); ra.append(nbytes / (time.perf_counter() - t0) / GIB)
        t0 = time.perf_counter(); run_b(); rb.append(nbytes / (time.perf_counter() - t0) / GIB)
        tm.append(timers())
    A, B = summary(ra), summary(rb)
    rec = {"A_search": A, "B_search_lines": B, "spread_A": round((A["max"] - A["min"]) / A["median"], 4), "unit": "GiB/s of uncompressed bytes",
           "lines_call_over_search_call_time_median": round(statistics.median(ra) / statistics.median(rb), 4),
           "kernel_ms_median_of_B": {k: round(statistics.median(t[k] for t in tm), 3) for k in tm[0]}}
    print("%s: A %s  B %s  %s" % (name, A["all"], B["all"], rec["kernel_ms_median_of_B"]), file=sys.stderr, flush=True)
    return rec


def sizes_of(shape):
    if shape == "small":
        rnd = random.Random(822)
        return [max(1, min(16 << 20, int(math.exp(rnd.gauss(math.log(822.0), 1.819))))) for _ in range(a.entries or 1000000)]
    return [1 << 20] * (a.entries or 10000)


def pick_per_mib(sample):
    """a 5- to 8-byte string of the sample, without 0x0A, whose count is nearest to one per MiB"""
    rnd = random.Random(10)
    best, best_d = None, None
    for _ in range(300):
        at = rnd.randrange(0, len(sample) - 16)
        for m in (5, 6, 8):
            p = bytes(sample[at:at + m])
            if b"\n" in p: continue
            d = abs(math.log(max(sample.count(p), 0.5) * (1 << 20) / len(sample)))
            if best is None or d < best_d: best, best_d = p, d
    return best


def pick_every(sample):
    lines = sample.split(b"\n")
    share = lambda b: sum(1 for l in lines if b in l) / len(lines)
    best = max((bytes([v]) for v in b" etao,0"), key=share)
    return best, round(share(best), 4)


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
    sample = bytes(eng.d2h(d_src, min(total, 16 << 20)))
    every, every_share = pick_every(sample)
    patterns = {"none": ABSENT, "per_mib": pick_per_mib(sample), "every": every}
    doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
    assert (st == 0).all()
    eng.free(d_src)
    doc = {"entries": n, "uncompressed_bytes": raw, "compressed_bytes": int(dlen.sum()), "patterns": {k: v.hex() for k, v in patterns.items()},
           "share_of_sample_lines_holding_every": every_share, "rec_cap": a.rec_cap, "max_line": a.max_line, "found": {}}
    timers = lambda: {"T_LINES": eng.kernel_ms(_lib.T_LINES), "T_SEARCH": eng.kernel_ms(_lib.T_SEARCH), "T_BLAKE3": eng.kernel_ms(_lib.T_BLAKE3),
                      "T_DECODE": eng.kernel_ms(_lib.T_DECODE), "T_TOTAL": eng.kernel_ms(_lib.T_TOTAL)}
    u64p = c.POINTER(c.c_uint64)
    digest, status = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    count, first, lines = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    pexp, pdig, pst = dig.ctypes.data_as(c.c_void_p), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int))
    pc, pf, pl = count.ctypes.data_as(u64p), first.ctypes.data_as(u64p), lines.ctypes.data_as(u64p)
    rec = (_lib.Line * a.rec_cap)()
    ru, tu = c.c_size_t(), c.c_size_t()
    text_cap = a.rec_cap * a.max_line
    d_text = eng.malloc(text_cap)
    # ---- device form: search (A) against search_lines (B)
    for name, pat in patterns.items():
        pp = c.cast(c.c_char_p(pat), c.c_void_p)
        def search_dev():   # (the raw calls: the Engine methods build a tuple per frame, a million of them here)
            assert lib.zarc_gpu_search_batch_device(h, n, c.c_void_p(d_dst), doff.ctypes.data_as(u64p), dlen.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), pexp,
                                                    pp, len(pat), 0, pdig, pst, pc, pf) == 0 and (status == 0).all()
        def lines_dev():
            assert lib.zarc_gpu_search_lines_batch_device(h, n, c.c_void_p(d_dst), doff.ctypes.data_as(u64p), dlen.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), pexp,
                                                          pp, len(pat), 0, 0, a.max_line, pdig, pst, pc, pf, pl, rec, a.rec_cap, c.byref(ru), c.c_void_p(d_text), text_cap,
                                                          c.byref(tu)) == 0 and (status == 0).all()
            doc["found"][name] = {"matches": int(count.sum()), "lines": int(lines.sum()), "delivered": ru.value, "text_bytes": tu.value}
        doc["device_search_vs_lines_" + name] = pair("%s device form, search / search_lines (%s)" % (shape, name), search_dev, lines_dev, raw, timers)
    eng.free(d_text)
    assert doc["found"]["none"]["lines"] == 0
    # ---- host form, pageable: the frames dense in one host buffer; unpack's outputs in another
    fal = (dlen + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    foff = np.concatenate(([0], np.cumsum(fal)[:-1])).astype(np.uint64)
    blob = eng.d2h(d_dst, int(doff[-1] + dlen[-1]))
    eng.free(d_dst)
    hf = np.zeros(int(fal.sum()) + 64, dtype=np.uint8)
    for i in range(n):
        hf[int(foff[i]):int(foff[i]) + int(dlen[i])] = blob[int(doff[i]):int(doff[i]) + int(dlen[i])]
    del blob
    out = bytearray(total + 64)
    obase = c.addressof((c.c_char * len(out)).from_buffer(out))
    fptr, optr = (foff + np.uint64(hf.ctypes.data)), (off + np.uint64(obase))
    args_f = (fptr.ctypes.data_as(c.POINTER(c.c_void_p)), dlen.ctypes.data_as(c.POINTER(c.c_size_t)), lens.ctypes.data_as(c.POINTER(c.c_size_t)))
    text = np.empty(text_cap, dtype=np.uint8)
    counters = {}
    for name, pat in patterns.items():
        pp = c.cast(c.c_char_p(pat), c.c_void_p)
        def search_host():
            assert lib.zarc_gpu_search_batch(h, n, *args_f, pexp, pp, len(pat), 0, pdig, pst, pc, pf) == 0 and (status == 0).all()
        def lines_host():
            assert lib.zarc_gpu_search_lines_batch(h, n, *args_f, pexp, pp, len(pat), 0, 0, a.max_line, pdig, pst, pc, pf, pl, rec, a.rec_cap, c.byref(ru),
                                                   text.ctypes.data_as(c.c_void_p), text_cap, c.byref(tu)) == 0 and (status == 0).all()
            assert (int(lines.sum()), ru.value, tu.value) == (doc["found"][name]["lines"], doc["found"][name]["delivered"], doc["found"][name]["text_bytes"])
            counters[name] = [eng.copy_bytes(w) for w in range(4)]
        r = pair("%s host form (pageable), search / search_lines (%s)" % (shape, name), search_host, lines_host, raw, timers)
        r["copy_bytes_h2d_d2h_ring_direct"] = counters[name]
        doc["host_pageable_search_vs_lines_" + name] = r
    # ---- what a caller does today: unpack through host memory, then one thread over the bytes, line by line where the needle occurs
    # (bytes.find from match to match and to the line's ends: no per-line Python work where nothing matches, so this side is flattered)
    today = {}
    for name, pat in patterns.items():
        rates, split = [], []
        for r in range(a.host_scan_runs + 1):
            t0 = time.perf_counter()
            assert lib.zarc_gpu_unpack_batch(h, n, *args_f, optr.ctypes.data_as(c.POINTER(c.c_void_p)), pexp, pdig, pst) == 0 and (status == 0).all()
            t1 = time.perf_counter()
            found, at = 0, out.find(pat)
            while at >= 0 and found < a.rec_cap:
                end = out.find(b"\n", at)
                if end < 0: end = len(out)
                found += 1                                   # (out.rfind(b"\n", 0, at) gives the start; the line's bytes are out[start + 1:end])
                at = out.find(pat, end + 1)
            t2 = time.perf_counter()
            if r: rates.append(raw / (t2 - t0) / GIB); split.append([round(t1 - t0, 3), round(t2 - t1, 3)])
        today[name] = {"rate": summary(rates), "seconds_unpack_scan": split, "lines_in_arena": found, "d2h_bytes": raw, "unit": "GiB/s of uncompressed bytes"}
        today[name]["lines_over_today_median"] = round(doc["host_pageable_search_vs_lines_" + name]["B_search_lines"]["median"] / max(today[name]["rate"]["median"], 1e-9), 2)
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
