#!/usr/bin/env python3
"""Rates of zarc_gpu_select_lines_batch_device (grep -C 2, -v, -v -C 2) against the plain lines call of the same matcher, frames resident in
HBM.  Shapes: BASELINE configs[1] (10 000 x 1 MiB synthetic entries, level 3, checksum on), `small` (the million-entry log-normal shape of
bench.py --config small) and `nolf` (1 MiB entries without a single line feed: every frame is one line of sixteen slices).  Matchers: a fixed
string of the content whose count is nearest to one per MiB, the set of that string and one that occurs nowhere, and the string as an
expression.  Every pair is measured alternating A, B, A, B ... in this one process, --runs repetitions each after one warm-up of each; the
document keeps min / median / max of each side, the relative spread s = (max - min) / median of the A side -- the only margin to read a
difference against -- the medians of T_LINES and T_SEARCH of the B side (device time, summed over the parts of a call), and what the B side
found and delivered.  rec_cap and max_line bound what one call delivers: under -v nearly every line is a hit and the records run out early.
  usage: select_rate.py [--shapes c2,small,nolf] [--entries N] [--runs 5] [--rec-cap 1048576] [--max-line 256] [--out profiles/r15_select_rate.json]"""
import argparse, ctypes, hashlib, json, math, os, random, re, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,small,nolf")
ap.add_argument("--entries", type=int, default=0, help="entries of a shape (default: 10000 for c2, 1000000 for small, 2000 for nolf)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--rec-cap", type=int, default=1 << 20)
ap.add_argument("--max-line", type=int, default=256)
ap.add_argument("--out", default="")
a = ap.parse_args()
GIB = float(1 << 30)
c = ctypes
ABSENT = b"\x00\xfe\x01zarc-nowhere\xff\x02"
SELECTIONS = {"C2": (0, 2, 2), "v": (_lib.SELECT_INVERT, 0, 0), "v_C2": (_lib.SELECT_INVERT, 2, 2)}


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
    rec = {"A_lines": A, "B_select": B, "spread_A": round((A["max"] - A["min"]) / A["median"], 4), "unit": "GiB/s of uncompressed bytes",
           "select_call_over_lines_call_time_median": round(statistics.median(ra) / statistics.median(rb), 4),
           "kernel_ms_median_of_B": {k: round(statistics.median(t[k] for t in tm), 3) for k in tm[0]}}
    print("%s: A %s  B %s  %s" % (name, A["all"], B["all"], rec["kernel_ms_median_of_B"]), file=sys.stderr, flush=True)
    return rec


def sizes_of(shape):
    if shape == "small":
        rnd = random.Random(822)
        return [max(1, min(16 << 20, int(math.exp(rnd.gauss(math.log(822.0), 1.819))))) for _ in range(a.entries or 1000000)]
    return [1 << 20] * (a.entries or (2000 if shape == "nolf" else 10000))


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
    if shape == "nolf":                                   # the same content with every line feed a space, 64 MiB at a time
        step = 64 << 20
        for at in range(0, total, step):
            piece = bytes(eng.d2h(d_src + at, min(step, total - at))).replace(b"\n", b" ")
            eng.h2d(d_src + at, piece)
        sample = sample.replace(b"\n", b" ")
    needle = pick_per_mib(sample)
    doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
    assert (st == 0).all()
    eng.free(d_src)
    matchers = {"fixed": _lib.MatcherDesc.of(_lib.MATCH_FIXED, needle), "set": _lib.MatcherDesc.of(_lib.MATCH_SET, [needle, ABSENT]),
                "regex": _lib.MatcherDesc.of(_lib.MATCH_REGEX, re.escape(needle))}
    doc = {"entries": n, "uncompressed_bytes": raw, "compressed_bytes": int(dlen.sum()), "needle": needle.hex(), "rec_cap": a.rec_cap, "max_line": a.max_line,
           "found": {}}
    timers = lambda: {"T_LINES": eng.kernel_ms(_lib.T_LINES), "T_SEARCH": eng.kernel_ms(_lib.T_SEARCH), "T_DECODE": eng.kernel_ms(_lib.T_DECODE),
                      "T_TOTAL": eng.kernel_ms(_lib.T_TOTAL)}
    u64p = c.POINTER(c.c_uint64)
    digest, status = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    count, first, lines, selected = (np.zeros(n, dtype=np.uint64) for _ in range(4))
    pexp, pdig, pst = dig.ctypes.data_as(c.c_void_p), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int))
    pc, pf, pl, ps = (x.ctypes.data_as(u64p) for x in (count, first, lines, selected))
    rec = (_lib.Line * a.rec_cap)()
    ru, tu = c.c_size_t(), c.c_size_t()
    text_cap = a.rec_cap * a.max_line
    d_text = eng.malloc(text_cap)
    frames = (c.c_void_p(d_dst), doff.ctypes.data_as(u64p), dlen.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), pexp)
    out = (rec, a.rec_cap, c.byref(ru), c.c_void_p(d_text), text_cap, c.byref(tu))
    off_sel = _lib.LineSelect(0, 0, 0, 0)
    for mname, m in matchers.items():
        def plain():   # the selection off: the entry point then launches exactly the kernels of the matcher's own lines call (the raw call: no tuple per frame)
            assert lib.zarc_gpu_select_lines_batch_device(h, n, *frames, c.byref(m), c.byref(off_sel), 0, a.max_line, pdig, pst, pc, pf, None, None, pl, ps, *out) == 0
            assert (status == 0).all()
        for sname, (flags, before, after) in SELECTIONS.items():
            q = _lib.LineSelect(flags, before, after, 0)
            def select():
                assert lib.zarc_gpu_select_lines_batch_device(h, n, *frames, c.byref(m), c.byref(q), 0, a.max_line, pdig, pst, pc, pf, None, None, pl, ps, *out) == 0
                assert (status == 0).all()
                doc["found"][mname + "_" + sname] = {"matches": int(count.sum()), "hit_lines": int(lines.sum()), "selected": int(selected.sum()), "delivered": ru.value,
                                                     "text_bytes": tu.value}
            doc["%s_lines_vs_select_%s" % (mname, sname)] = pair("%s %s, lines / select %s" % (shape, mname, sname), plain, select, raw, timers)
    eng.free(d_text)
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
