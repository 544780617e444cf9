#!/usr/bin/env python3
"""Rates of zarc_gpu_search_matches_batch_device (grep -o) against the matcher's plain lines call with the same caps, frames resident in HBM.
Shapes: BASELINE configs[1] (10 000 x 1 MiB synthetic entries, level 3, checksum on) and `small` (the million-entry log-normal shape of
bench.py --config small).  Matchers: a fixed string of the content whose count is nearest to one per MiB, and the expression `[a-z]+ing `.
Every pair is measured alternating A, B, A, B ... in this one process, --runs repetitions each after one warm-up of each; the document keeps
min / median / max of each side, the relative spread s = (max - min) / median of the A side -- the only margin to read a difference against
-- the medians of T_LINES and T_SEARCH of the B side (device time, summed over the parts of a call), and what the B side found and
delivered.  No ratio is fixed in advance.  Without a usable device the tool says so and claims no rate.
  usage: only_rate.py [--shapes c2,small] [--entries N] [--runs 5] [--cap 1048576] [--max-line 256] [--out profiles/r17_only_rate.json]"""
import argparse, ctypes, hashlib, json, math, os, random, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,small")
ap.add_argument("--entries", type=int, default=0, help="entries of a shape (default: 10000 for c2, 1000000 for small)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--cap", type=int, default=1 << 20, help="rec_cap of the lines call; line_cap and rec_cap of the matches call")
ap.add_argument("--max-line", type=int, default=256)
ap.add_argument("--out", default="")
a = ap.parse_args()
GIB = float(1 << 30)
c = ctypes
EXPRESSION = b"[a-z]+ing "


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
    rec = {"A_lines": A, "B_matches": B, "spread_A": round((A["max"] - A["min"]) / A["median"], 4), "unit": "GiB/s of uncompressed bytes",
           "matches_call_over_lines_call_time_median": round(statistics.median(ra) / statistics.median(rb), 4),
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
    needle = pick_per_mib(sample)
    doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
    assert (st == 0).all()
    eng.free(d_src)
    matchers = {"literal": _lib.MatcherDesc.of(_lib.MATCH_FIXED, needle), "expression": _lib.MatcherDesc.of(_lib.MATCH_REGEX, EXPRESSION)}
    doc = {"entries": n, "uncompressed_bytes": raw, "compressed_bytes": int(dlen.sum()), "needle": needle.hex(), "expression": EXPRESSION.decode(), "cap": a.cap,
           "max_line": a.max_line, "found": {}}
    timers = lambda: {"T_LINES": eng.kernel_ms(_lib.T_LINES), "T_SEARCH": eng.kernel_ms(_lib.T_SEARCH), "T_DECODE": eng.kernel_ms(_lib.T_DECODE),
                      "T_TOTAL": eng.kernel_ms(_lib.T_TOTAL)}
    u64p = c.POINTER(c.c_uint64)
    digest, status = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    count, first, lines, other = (np.zeros(n, dtype=np.uint64) for _ in range(4))
    pexp, pdig, pst = dig.ctypes.data_as(c.c_void_p), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int))
    pc, pf, pl, po = (x.ctypes.data_as(u64p) for x in (count, first, lines, other))
    lrec, mrec = (_lib.Line * a.cap)(), (_lib.Match * a.cap)()
    ru, tu = c.c_size_t(), c.c_size_t()
    text_cap = a.cap * a.max_line
    d_text = eng.malloc(text_cap)
    frames = (c.c_void_p(d_dst), doff.ctypes.data_as(u64p), dlen.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), pexp)
    tail = (c.byref(ru), c.c_void_p(d_text), text_cap, c.byref(tu))
    off_sel = _lib.LineSelect(0, 0, 0, 0)
    for mname, m in matchers.items():
        def plain():   # the selection off: the entry point launches exactly the kernels of the matcher's own lines call
            assert lib.zarc_gpu_select_lines_batch_device(h, n, *frames, c.byref(m), c.byref(off_sel), 0, a.max_line, pdig, pst, pc, pf, None, None, pl, po, lrec, a.cap, *tail) == 0
            assert (status == 0).all()
            doc["found"][mname + "_lines"] = {"start_positions": int(count.sum()), "matching_lines": int(lines.sum()), "delivered": ru.value, "text_bytes": tu.value}

        def only():
            assert lib.zarc_gpu_search_matches_batch_device(h, n, *frames, c.byref(m), 0, a.max_line, a.cap, pdig, pst, pc, pf, None, None, pl, po, mrec, a.cap, *tail) == 0
            assert (status == 0).all()
            doc["found"][mname + "_matches"] = {"start_positions": int(count.sum()), "matching_lines": int(lines.sum()), "matches": int(other.sum()), "delivered": ru.value,
                                                "text_bytes": tu.value}
        doc["%s_lines_vs_matches" % mname] = pair("%s %s, lines / matches" % (shape, mname), plain, only, raw, timers)
    eng.free(d_text)
    eng.free(d_dst)
    eng.close()
    return doc


try:
    ndev = _lib.load().zarc_gpu_device_count()
except OSError as e:
    ndev, why = 0, str(e)
else:
    why = "zarc_gpu_device_count() is 0"
if ndev < 1:
    print("only_rate: no usable device (%s): nothing measured, no rate claimed" % why, file=sys.stderr)
    sys.exit(1)
doc = {"runs": a.runs, "library_sha16": hashlib.sha256(open(_lib.DEFAULT_LIB, "rb").read()).hexdigest()[:16], "shapes": {}}
for shape in a.shapes.split(","):
    doc["shapes"][shape] = shape_doc(shape)
text = json.dumps(doc, indent=1, sort_keys=True)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
