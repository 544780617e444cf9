#!/usr/bin/env python3
"""Rates of zarc_gpu_verify_batch* against zarc_gpu_unpack_batch*, and of pack with the read-back check (ZARC_GPU_PX_CHECK_FRAMES) on
against off.  Shapes: BASELINE configs[1] (10 000 x 1 MiB synthetic entries, level 3, checksum on) and `small` (the million-entry
log-normal shape of bench.py --config small).  Every pair is measured alternating A, B, A, B ... in this one process, --runs
repetitions each after one warm-up of each; the document keeps min / median / max of each side, the relative spread
s = (max - min) / median of the A side, and whether median(B) >= median(A) * (1 - s) where that is a condition (verify against unpack).
  usage: verify_rate.py [--shapes c2,small] [--runs 5] [--level9-gib 8] [--out profiles/r06_verify_rate.json]"""
import argparse, ctypes, hashlib, json, math, os, random, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,small")
ap.add_argument("--entries", type=int, default=0, help="entries of a shape (default: 10000 for c2, 1000000 for small)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--level9-gib", type=float, default=8.0, help="pack check on/off at level 9 on this many GiB of 4 MiB frames (configs[3] shape); 0 = skip")
ap.add_argument("--diag-lib", default="", help="libzarc_gpu_diag.so: also record the device time of zarc_check_compare (HIP events; the diagnostic build prints it)")
ap.add_argument("--out", default="")
a = ap.parse_args()
GIB = float(1 << 30)
c = ctypes
hip = c.CDLL("libamdhip64.so")
hip.hipHostMalloc.argtypes = [c.POINTER(c.c_void_p), c.c_size_t, c.c_uint]
hip.hipHostFree.argtypes = [c.c_void_p]


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def pair(name, run_a, run_b, nbytes, condition):
    """alternating A, B, A, B ...; rates in GiB/s of `nbytes` per call"""
    run_a(); run_b()
    ra, rb = [], []
    for _ in range(a.runs):
        t0 = time.perf_counter(); run_a(); ra.append(nbytes / (time.perf_counter() - t0) / GIB)
        t0 = time.perf_counter(); run_b(); rb.append(nbytes / (time.perf_counter() - t0) / GIB)
    A, B = summary(ra), summary(rb)
    s = (A["max"] - A["min"]) / A["median"]
    rec = {"A": A, "B": B, "spread_A": round(s, 4), "unit": "GiB/s of uncompressed bytes"}
    if condition:
        rec["condition"] = "median(B) >= median(A) * (1 - s)"
        rec["holds"] = bool(B["median"] >= A["median"] * (1 - s))
    print("%s: A %s  B %s  s %.3f %s" % (name, A["all"], B["all"], s, rec.get("holds", "")), file=sys.stderr, flush=True)
    return rec


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
    d_src, d_dst, d_out = eng.malloc(total + _lib.PAD), eng.malloc(cap + _lib.PAD), eng.malloc(total + _lib.PAD)
    eng.corpus_fill(d_src, off, lens, first_index=0, kind=-1)
    doc = {"entries": n, "uncompressed_bytes": raw}
    # ---- pack, check off (A) against on (B): recorded, no condition
    def pack(check):
        eng.set_parameter(_lib.PX_CHECK_FRAMES, check)
        r = eng.pack_device(d_src, off, lens, d_dst, cap)
        eng.set_parameter(_lib.PX_CHECK_FRAMES, 0)
        return r
    doc["pack_check_off_vs_on_device"] = pair(shape + " pack, check off / on", lambda: pack(0), lambda: pack(1), raw, False)
    doff, dlen, dig, st = pack(0)
    assert (st == 0).all()
    comp = int(dlen.sum())
    doc["compressed_bytes"] = comp
    # ---- device form: unpack (A) against verify (B)
    def unpack_dev():
        d, s = eng.unpack_device(d_dst, doff, dlen, d_out, off, lens, expect=dig); assert (s == 0).all() and (d == dig).all()
    def verify_dev():
        d, s = eng.verify_device(d_dst, doff, dlen, lens, expect=dig); assert (s == 0).all() and (d == dig).all()
    doc["device_unpack_vs_verify"] = pair(shape + " device form, unpack / verify", unpack_dev, verify_dev, raw, True)
    # ---- host form, pageable and pinned: the frames dense in one host buffer, the outputs in another
    fal = (dlen + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    foff = np.concatenate(([0], np.cumsum(fal)[:-1])).astype(np.uint64)
    ftotal = int(fal.sum())
    blob = eng.d2h(d_dst, int(doff[-1] + dlen[-1]))
    eng.free(d_src); eng.free(d_dst); eng.free(d_out)
    digest = np.zeros((n, 32), dtype=np.uint8)
    status = np.zeros(n, dtype=np.int32)
    for kind in ("pageable", "pinned"):
        if kind == "pinned":
            pf, po = c.c_void_p(), c.c_void_p()
            assert hip.hipHostMalloc(c.byref(pf), ftotal + 64, 0) == 0 and hip.hipHostMalloc(c.byref(po), total + 64, 0) == 0
            fbase, obase = pf.value, po.value
            hf = np.ctypeslib.as_array((c.c_uint8 * ftotal).from_address(fbase))
        else:
            hf, ho = np.zeros(ftotal + 64, dtype=np.uint8), np.zeros(total + 64, dtype=np.uint8)
            fbase, obase = hf.ctypes.data, ho.ctypes.data
        for i in range(n):
            hf[int(foff[i]):int(foff[i]) + int(dlen[i])] = blob[int(doff[i]):int(doff[i]) + int(dlen[i])]
        fptr, optr = (foff + np.uint64(fbase)), (off + np.uint64(obase))
        args_f = (fptr.ctypes.data_as(c.POINTER(c.c_void_p)), dlen.ctypes.data_as(c.POINTER(c.c_size_t)), lens.ctypes.data_as(c.POINTER(c.c_size_t)))
        tail = (dig.ctypes.data_as(c.c_void_p), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int)))
        counters = {}
        def unpack_host():
            assert lib.zarc_gpu_unpack_batch(h, n, *args_f, optr.ctypes.data_as(c.POINTER(c.c_void_p)), *tail) == 0 and (status == 0).all()
            counters["unpack"] = [eng.copy_bytes(w) for w in range(4)]
        def verify_host():
            assert lib.zarc_gpu_verify_batch(h, n, *args_f, *tail) == 0 and (status == 0).all()
            counters["verify"] = [eng.copy_bytes(w) for w in range(4)]
        rec = pair("%s host form (%s), unpack / verify" % (shape, kind), unpack_host, verify_host, raw, True)
        rec["copy_bytes_h2d_d2h_ring_direct"] = counters
        doc["host_%s_unpack_vs_verify" % kind] = rec
        if kind == "pinned":
            del hf
            hip.hipHostFree(pf); hip.hipHostFree(po)
    eng.close()
    return doc


def level9_doc(gib):
    eng = Engine(0)
    eng.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    eng.set_parameter(_lib.P_COMPRESSION_LEVEL, 9)
    n = int(gib * GIB) // (4 << 20)
    lens = np.full(n, 4 << 20, dtype=np.uint64)
    off = np.arange(n, dtype=np.uint64) * np.uint64(4 << 20)
    cap = n * int(eng.bound(4 << 20))
    d_src, d_dst = eng.malloc(n * (4 << 20) + _lib.PAD), eng.malloc(cap + _lib.PAD)
    eng.corpus_fill(d_src, off, lens, first_index=0, kind=2)
    def pack(check):
        eng.set_parameter(_lib.PX_CHECK_FRAMES, check)
        r = eng.pack_device(d_src, off, lens, d_dst, cap)
        eng.set_parameter(_lib.PX_CHECK_FRAMES, 0)
        assert (r[3] == 0).all()
    rec = pair("level 9, %d x 4 MiB: pack, check off / on" % n, lambda: pack(0), lambda: pack(1), n * (4 << 20), False)
    rec["entries"] = n
    eng.free(d_src); eng.free(d_dst)
    eng.close()
    return rec


def compare_ms(sizes, level, kind):
    """device time of zarc_check_compare in one checked pack call of this shape, from the diagnostic build's report on stderr"""
    import re, tempfile
    os.environ["ZARC_GPU_CHECK_STATS"] = "1"
    eng = Engine(0, a.diag_lib)
    eng.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    eng.set_parameter(_lib.P_COMPRESSION_LEVEL, level)
    eng.set_parameter(_lib.PX_CHECK_FRAMES, 1)
    lens = np.array(sizes, dtype=np.uint64)
    al = (lens + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    off = np.concatenate(([0], np.cumsum(al)[:-1])).astype(np.uint64)
    blocks = np.maximum((lens + np.uint64(65535)) // np.uint64(65536), np.uint64(1))
    cap = int(((lens + np.uint64(3) * blocks + np.uint64(18 + 15)) // np.uint64(16) * np.uint64(16)).sum())
    d_src, d_dst = eng.malloc(int(al.sum()) + _lib.PAD), eng.malloc(cap + _lib.PAD)
    eng.corpus_fill(d_src, off, lens, first_index=0, kind=kind)
    out = []
    for _ in range(3):
        with tempfile.TemporaryFile() as tmp:
            sys.stderr.flush()
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                r = eng.pack_device(d_src, off, lens, d_dst, cap)
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            out.append(round(sum(float(x) for x in re.findall(rb"zarc_check_compare: ([0-9.]+) ms", tmp.read())), 3))
        assert (r[3] == 0).all()
    eng.free(d_src); eng.free(d_dst)
    eng.close()
    raw = int(lens.sum())
    best = min(out)
    return {"ms": out, "bytes_read": 2 * raw, "tb_per_s_at_min": round(2 * raw / (best / 1e3) / 1e12, 3) if best > 0 else None}


doc = {"runs": a.runs, "library_sha16": hashlib.sha256(open(_lib.DEFAULT_LIB, "rb").read()).hexdigest()[:16], "shapes": {}}
for shape in a.shapes.split(","):
    doc["shapes"][shape] = shape_doc(shape)
if a.level9_gib > 0:
    doc["pack_check_off_vs_on_level9"] = level9_doc(a.level9_gib)
if a.diag_lib:
    doc["zarc_check_compare"] = {s_: compare_ms(sizes_of(s_), 3, -1) for s_ in a.shapes.split(",")}
    if a.level9_gib > 0:
        doc["zarc_check_compare"]["level9"] = compare_ms([4 << 20] * (int(a.level9_gib * GIB) // (4 << 20)), 9, 2)
text = json.dumps(doc, indent=1, sort_keys=True)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
