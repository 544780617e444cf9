#!/usr/bin/env python3
"""Rates of zarc_gpu_compare_batch_device (zarc compare) against zarc_gpu_verify_batch_device, frames and other sides resident in HBM.
Shapes: BASELINE configs[1] (10 000 x 1 MiB synthetic entries, level 3, checksum on) and `small` (the million-entry log-normal shape of
bench.py --config small).  Side A is verify_device; side B is compare_device over the same frames against (identical) the very bytes
they were packed from, (changed) those with one byte changed per frame, and (inserted) those with 100 bytes inserted in the middle of
every frame -- different lengths, so the shifted backward pass runs.  Each pair is measured alternating A, B, A, B ... in this one
process, --runs repetitions each after one warm-up of each; the document keeps min / median / max of each side, the relative spread
s = (max - min) / median of the A side -- the only margin to read a difference against -- and the medians of the compare kernels' time
(zarc_gpu_last_compare_ms: zarc_cmp_scan and zarc_cmp_carry together), of the decode and hash timers and of T_TOTAL (device time, summed
over the parts of a call), with the sums of the results as a fingerprint.
The route before: on the first --route-entries entries of the 1 MiB shape, host-form unpack plus a numpy comparison of every entry with
its other side, against host-form compare of the same pairs (both move the frames up; one moves the content down, the other the other
sides up).  No ratio is fixed in advance.  Without a usable device the tool says so and claims no rate.
  usage: compare_rate.py [--shapes c2,small] [--entries N] [--runs 5] [--route-entries 1000] [--out profiles/r21_compare_rate.json]"""
import argparse, ctypes, hashlib, json, math, os, random, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,small")
ap.add_argument("--entries", type=int, default=0, help="entries of a shape (default: 10000 for c2, 1000000 for small)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--route-entries", type=int, default=1000)
ap.add_argument("--out", default="")
a = ap.parse_args()
GIB = float(1 << 30)
c = ctypes
TIMERS = {"T_DECODE": _lib.T_DECODE, "T_BLAKE3": _lib.T_BLAKE3, "T_XXH64": _lib.T_XXH64, "T_TOTAL": _lib.T_TOTAL}
INSERT = 100
CMP_T = np.dtype([("relation", "<u4"), ("byte_a", "<u4"), ("byte_b", "<u4"), ("r0", "<u4")] +
                 [(k, "<u8") for k in ("prefix", "line", "differing", "suffix", "r1", "r2")])   # zarc_gpu_cmp


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def pair(name, run_a, run_b, nbytes, timers, names=("A_verify", "B_compare")):
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
    rec = {names[0]: A, names[1]: B, "spread_A": round((A["max"] - A["min"]) / A["median"], 4), "unit": "GiB/s of uncompressed bytes",
           "B_over_A_time_median": round(statistics.median(ra) / statistics.median(rb), 4),
           "kernel_ms_median_of_A": med(ta), "kernel_ms_median_of_B": med(tb)}
    print("%s: A %s  B %s  %s" % (name, A["all"], B["all"], rec["kernel_ms_median_of_B"]), file=sys.stderr, flush=True)
    return rec


def sizes_of(shape):
    if shape == "small":
        rnd = random.Random(822)
        return [max(1, min(16 << 20, int(math.exp(rnd.gauss(math.log(822.0), 1.819))))) for _ in range(a.entries or 1000000)]
    return [1 << 20] * (a.entries or 10000)


def layout(lens):
    al = (lens + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    return np.concatenate(([0], np.cumsum(al)[:-1])).astype(np.uint64), int(al.sum())


def shape_doc(shape):
    eng = Engine(0)
    eng.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    eng.set_parameter(_lib.P_COMPRESSION_LEVEL, 3)
    lib, h = eng.lib, eng.h
    lens = np.array(sizes_of(shape), dtype=np.uint64)
    n = len(lens)
    off, total = layout(lens)
    raw = int(lens.sum())
    blocks = np.maximum((lens + np.uint64(65535)) // np.uint64(65536), np.uint64(1))
    cap = int(((lens + np.uint64(3) * blocks + np.uint64(18 + 15)) // np.uint64(16) * np.uint64(16)).sum())   # sum of zarc_gpu_bound()
    d_src, d_dst = eng.malloc(total + _lib.PAD), eng.malloc(cap + _lib.PAD)
    eng.corpus_fill(d_src, off, lens, first_index=0, kind=-1)
    doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
    assert (st == 0).all()
    doc = {"entries": n, "uncompressed_bytes": raw, "compressed_bytes": int(dlen.sum())}
    timers = lambda: dict({k: eng.kernel_ms(v) for k, v in TIMERS.items()}, compare_ms=eng.compare_ms())
    u64p = c.POINTER(c.c_uint64)
    digest, status = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    pexp, pdig, pst = dig.ctypes.data_as(c.c_void_p), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int))
    res = np.zeros(n, dtype=CMP_T)
    pres = res.ctypes.data_as(c.POINTER(_lib.Cmp))
    frames = (c.c_void_p(d_dst), doff.ctypes.data_as(u64p), dlen.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), pexp)

    def verify():
        assert lib.zarc_gpu_verify_batch_device(h, n, *frames, pdig, pst) == 0
        assert (status == 0).all()

    def compare_with(d_other, ooff, olen):
        def run():
            assert lib.zarc_gpu_compare_batch_device(h, n, *frames, c.c_void_p(d_other), ooff.ctypes.data_as(u64p), olen.ctypes.data_as(u64p), pdig, pst, pres) == 0
            assert (status == 0).all()
        return run

    # identical: the sources themselves
    doc["identical"] = pair("%s identical" % shape, verify, compare_with(d_src, off, lens), raw, timers)
    assert (res["relation"] == _lib.CMP_EQUAL).all() and (res["prefix"] == lens).all() and (res["differing"] == 0).all() and (res["r0"] == 0).all()
    doc["identical"]["sum_of_lines"] = int(res["line"].sum())
    # changed: one byte per frame, in the middle
    host = np.frombuffer(eng.d2h(d_src, total), dtype=np.uint8).copy()
    mid = off + lens // np.uint64(2)
    host[mid.astype(np.int64)] ^= 1
    eng.h2d(d_src, host)
    doc["changed"] = pair("%s changed" % shape, verify, compare_with(d_src, off, lens), raw, timers)
    assert (res["relation"] == _lib.CMP_DIFFER).all() and (res["prefix"] == lens // np.uint64(2)).all() and (res["differing"] == 1).all()
    assert (res["suffix"] == lens - lens // np.uint64(2) - np.uint64(1)).all()
    doc["changed"]["sum_of_lines"] = int(res["line"].sum())
    host[mid.astype(np.int64)] ^= 1
    # inserted: 100 bytes in the middle of every frame
    eng.free(d_src)
    olen = lens + np.uint64(INSERT)
    ooff, ototal = layout(olen)
    other = np.zeros(ototal, dtype=np.uint8)
    ins = np.arange(128, 128 + INSERT, dtype=np.uint8)                             # (the corpus has random and record entries: any byte occurs)
    for s, o, l in zip(off.astype(np.int64), ooff.astype(np.int64), lens.astype(np.int64)):
        m = l // 2
        other[o:o + m] = host[s:s + m]
        other[o + m:o + m + INSERT] = ins
        other[o + m] = host[s + m] ^ 0xFF                                          # the first inserted byte differs from the byte it displaces
        other[o + m + INSERT:o + l + INSERT] = host[s + m:s + l]
    del host
    d_other = eng.malloc(ototal + _lib.PAD)
    eng.h2d(d_other, other)
    del other
    doc["inserted"] = pair("%s inserted" % shape, verify, compare_with(d_other, ooff, olen), raw, timers)
    # the edit point is the first difference by construction, and the common tail is all that lies behind it (the overlap cap allows no more)
    assert (res["relation"] == _lib.CMP_DIFFER).all() and (res["prefix"] == lens // np.uint64(2)).all()
    assert (res["suffix"] == lens - lens // np.uint64(2)).all() and (res["byte_b"] == (res["byte_a"] ^ 0xFF)).all()
    doc["inserted"]["sum_of_differing"] = int(res["differing"].sum())
    eng.free(d_other)
    eng.free(d_dst)
    eng.close()
    return doc


def route_doc():
    """host forms on the first --route-entries entries of the 1 MiB shape: unpack + numpy comparison against compare"""
    eng = Engine(0)
    eng.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    eng.set_parameter(_lib.P_COMPRESSION_LEVEL, 3)
    n = a.route_entries
    lens = np.full(n, 1 << 20, dtype=np.uint64)
    off, total = layout(lens)
    d_src = eng.malloc(total + _lib.PAD)
    eng.corpus_fill(d_src, off, lens, first_index=0, kind=-1)
    host = eng.d2h(d_src, total)
    eng.free(d_src)
    ents = [bytes(host[int(o):int(o) + (1 << 20)]) for o in off]
    packed = eng.pack(ents)
    frames, digests, raw_lens = [p[0] for p in packed], [p[1] for p in packed], [1 << 20] * n
    others = [e[:1 << 19] + bytes([e[1 << 19] ^ 1]) + e[(1 << 19) + 1:] for e in ents]
    views = [np.frombuffer(o, dtype=np.uint8) for o in others]

    def before():
        out = eng.unpack(frames, raw_lens, digests)
        diff = 0
        for (data, _, st), v in zip(out, views):
            assert st == 0
            ne = np.frombuffer(data, dtype=np.uint8) != v
            diff += int(np.count_nonzero(ne))
        assert diff == n

    def after():
        verdicts, res = eng.compare(frames, raw_lens, others, expect=digests)
        assert all(st == 0 for _, st in verdicts) and all(r[:4] == (_lib.CMP_DIFFER, 1 << 19, r[2], 1) for r in res)

    timers = lambda: {"T_TOTAL": eng.kernel_ms(_lib.T_TOTAL), "compare_ms": eng.compare_ms()}
    doc = {"entries": n, "uncompressed_bytes": n << 20}
    doc.update(pair("route before", before, after, n << 20, timers, names=("A_unpack_plus_numpy", "B_compare_host_form")))
    eng.close()
    return doc


try:
    ndev = _lib.load().zarc_gpu_device_count()
except OSError as e:
    ndev, why = 0, str(e)
else:
    why = "zarc_gpu_device_count() is 0"
if ndev < 1:
    print("compare_rate: no usable device (%s): nothing measured, no rate claimed" % why, file=sys.stderr)
    sys.exit(1)
doc = {"runs": a.runs, "library_sha16": hashlib.sha256(open(_lib.DEFAULT_LIB, "rb").read()).hexdigest()[:16], "shapes": {}}
for shape in a.shapes.split(","):
    doc["shapes"][shape] = shape_doc(shape)
if a.route_entries > 0:
    doc["route_before"] = route_doc()
text = json.dumps(doc, indent=1, sort_keys=True)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
