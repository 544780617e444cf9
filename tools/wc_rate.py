#!/usr/bin/env python3
"""Rates of zarc_gpu_count_batch_device (zarc wc) against zarc_gpu_verify_batch_device, frames resident in HBM.
Shapes: BASELINE configs[1] (10 000 x 1 MiB synthetic entries, level 3, checksum on) and `small` (the million-entry log-normal shape of
bench.py --config small).  Side A is verify_device; side B is count_device over the same frames: what the count costs on top of the verify
pass it runs behind.  The pair is measured alternating A, B, A, B ... in this one process, --runs repetitions each after one warm-up of
each; the document keeps min / median / max of each side, the relative spread s = (max - min) / median of the A side -- the only margin to
read a difference against -- and the medians of T_WC (zarc_wc_count and zarc_wc_carry together: one timer covers both), of the decode and
hash timers and of T_TOTAL of the B side (device time, summed over the parts of a call), with the sums of the counts as a fingerprint.  No
ratio is fixed in advance.  Without a usable device the tool says so and claims no rate.
  usage: wc_rate.py [--shapes c2,small] [--entries N] [--runs 5] [--out profiles/r20_wc_rate.json]"""
import argparse, ctypes, hashlib, json, math, os, random, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,small")
ap.add_argument("--entries", type=int, default=0, help="entries of a shape (default: 10000 for c2, 1000000 for small)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()
GIB = float(1 << 30)
c = ctypes
TIMERS = {"T_WC": _lib.T_WC, "T_DECODE": _lib.T_DECODE, "T_BLAKE3": _lib.T_BLAKE3, "T_XXH64": _lib.T_XXH64, "T_TOTAL": _lib.T_TOTAL}


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def pair(name, run_a, run_b, nbytes, timers):
    """alternating A, B, A, B ...; rates in GiB/s of `nbytes` per call; timers(): device times of the call just made"""
    run_a(); run_b()
    ra, rb, ta, tb = [], [], [], []
    for _ in range(a.runs):
        t0 = time.perf_counter(); run_a(); ra.append(nbytes / (time.perf_counter() - t0) / GIB)
        ta.append(timers())
        t0 = time.perf_counter(); run_b(); rb.append(nbytes / (time.perf_counter() - t0) / GIB)
        tb.append(timers())
    A, B = summary(ra), summary(rb)
    med = lambda tm: {k: round(statistics.median(t[k] for t in tm), 3) for k in tm[0]}
    rec = {"A_verify": A, "B_count": B, "spread_A": round((A["max"] - A["min"]) / A["median"], 4), "unit": "GiB/s of uncompressed bytes",
           "B_over_A_time_median": round(statistics.median(ra) / statistics.median(rb), 4),
           "kernel_ms_median_of_A": med(ta), "kernel_ms_median_of_B": med(tb)}
    print("%s: A %s  B %s  %s" % (name, A["all"], B["all"], rec["kernel_ms_median_of_B"]), file=sys.stderr, flush=True)
    return rec


def sizes_of(shape):
    if shape == "small":
        rnd = random.Random(822)
        return [max(1, min(16 << 20, int(math.exp(rnd.gauss(math.log(822.0), 1.819))))) for _ in range(a.entries or 1000000)]
    return [1 << 20] * (a.entries or 10000)


WC_T = np.dtype([(k, "<u8") for k in ("lines", "words", "chars", "max_line", "max_line_start", "max_line_no", "r0", "r1")])   # zarc_gpu_wc


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
    doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
    assert (st == 0).all()
    eng.free(d_src)
    doc = {"entries": n, "uncompressed_bytes": raw, "compressed_bytes": int(dlen.sum())}
    timers = lambda: {k: eng.kernel_ms(v) for k, v in TIMERS.items()}
    u64p = c.POINTER(c.c_uint64)
    digest, status = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    pexp, pdig, pst = dig.ctypes.data_as(c.c_void_p), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int))
    res = np.zeros(n, dtype=WC_T)
    pres = res.ctypes.data_as(c.POINTER(_lib.Wc))
    frames = (c.c_void_p(d_dst), doff.ctypes.data_as(u64p), dlen.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), pexp)

    def verify():
        assert lib.zarc_gpu_verify_batch_device(h, n, *frames, pdig, pst) == 0
        assert (status == 0).all()

    def count():
        assert lib.zarc_gpu_count_batch_device(h, n, *frames, pdig, pst, pres) == 0
        assert (status == 0).all()

    doc.update(pair("%s count" % shape, verify, count, raw, timers))
    doc["sums"] = {k: int(res[k].sum()) for k in ("lines", "words", "chars")}
    doc["max_line_max"] = int(res["max_line"].max())
    assert (res["chars"] <= lens).all() and (res["max_line"] <= lens).all() and (res["r0"] == 0).all()
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
    print("wc_rate: no usable device (%s): nothing measured, no rate claimed" % why, file=sys.stderr)
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
