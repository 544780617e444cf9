#!/usr/bin/env python3
"""Rates of zarc_gpu_read_ranges_batch_device (zarc cat) against zarc_gpu_verify_batch_device, frames resident in HBM.
Shapes: BASELINE configs[1] (10 000 x 1 MiB synthetic entries, level 3, checksum on) and `small` (the million-entry log-normal shape of
bench.py --config small).  Side A is verify_device; side B is read_ranges_device with one range for every frame: the first ten lines, the last
ten lines, 1 000 lines from the middle, 4 KiB of bytes from the middle, all bytes (the gather alone).  A further, host-form pair over the
first --host-entries frames measures Engine.unpack plus slicing on the host against Engine.read_ranges for the first ten lines: the PCIe
saving the call exists for (both sides include the binding's marshalling).
Every pair is measured alternating A, B, A, B ... in this one process, --runs repetitions each after one warm-up of each; the document keeps
min / median / max of each side, the relative spread s = (max - min) / median of the A side -- the only margin to read a difference against
-- the median of T_RANGE of the B side (device time, summed over the parts of a call) and the bytes delivered; for the all-bytes case the
gather's rate, delivered bytes over T_RANGE.  No ratio is fixed in advance.  Without a usable device the tool says so and claims no rate.
  usage: range_rate.py [--shapes c2,small] [--entries N] [--runs 5] [--host-entries N] [--out profiles/r19_range_rate.json]"""
import argparse, ctypes, hashlib, json, math, os, random, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,small")
ap.add_argument("--entries", type=int, default=0, help="entries of a shape (default: 10000 for c2, 1000000 for small)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--host-entries", type=int, default=0, help="frames of the host-form pair (default: 1000 for c2, 100000 for small)")
ap.add_argument("--out", default="")
a = ap.parse_args()
GIB = float(1 << 30)
c = ctypes
L, B, END, ALL = _lib.RANGE_LINES, _lib.RANGE_BYTES, _lib.RANGE_FROM_END, _lib.RANGE_ALL


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def pair(name, run_a, run_b, nbytes, timers, names=("A_verify", "B_read_ranges")):
    """alternating A, B, A, B ...; rates in GiB/s of `nbytes` per call; timers(): device times of the B call just made"""
    run_a(); run_b()
    ra, rb, tm = [], [], []
    for _ in range(a.runs):
        t0 = time.perf_counter(); run_a(); ra.append(nbytes / (time.perf_counter() - t0) / GIB)
        t0 = time.perf_counter(); run_b(); rb.append(nbytes / (time.perf_counter() - t0) / GIB)
        tm.append(timers())
    A, Bs = summary(ra), summary(rb)
    rec = {names[0]: A, names[1]: Bs, "spread_A": round((A["max"] - A["min"]) / A["median"], 4), "unit": "GiB/s of uncompressed bytes",
           "B_over_A_time_median": round(statistics.median(ra) / statistics.median(rb), 4),
           "kernel_ms_median_of_B": {k: round(statistics.median(t[k] for t in tm), 3) for k in tm[0]}}
    print("%s: A %s  B %s  %s" % (name, A["all"], Bs["all"], rec["kernel_ms_median_of_B"]), file=sys.stderr, flush=True)
    return rec


def sizes_of(shape):
    if shape == "small":
        rnd = random.Random(822)
        return [max(1, min(16 << 20, int(math.exp(rnd.gauss(math.log(822.0), 1.819))))) for _ in range(a.entries or 1000000)]
    return [1 << 20] * (a.entries or 10000)


RANGE_T = np.dtype([("unit", "<u4"), ("flags", "<u4"), ("skip", "<u8"), ("take", "<u8")])                       # zarc_gpu_range
RESULT_T = np.dtype([(k, "<u8") for k in ("units", "first", "taken", "start", "length", "text_off", "text_len", "reserved")])  # zarc_gpu_range_result


def ranges_of(n, unit, flags, skip, take):
    """n ranges; skip and take are numbers or arrays of n"""
    arr = np.zeros(n, dtype=RANGE_T)
    arr["unit"], arr["flags"], arr["skip"], arr["take"] = unit, flags, skip, take
    return arr


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
    doc = {"entries": n, "uncompressed_bytes": raw, "compressed_bytes": int(dlen.sum()), "cases": {}}
    timers = lambda: {"T_RANGE": eng.kernel_ms(_lib.T_RANGE), "T_DECODE": eng.kernel_ms(_lib.T_DECODE), "T_TOTAL": eng.kernel_ms(_lib.T_TOTAL)}
    u64p = c.POINTER(c.c_uint64)
    digest, status = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    pexp, pdig, pst = dig.ctypes.data_as(c.c_void_p), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int))
    res = np.zeros(n, dtype=RESULT_T)
    pres = res.ctypes.data_as(c.POINTER(_lib.RangeResult))
    tu = c.c_size_t()
    text_cap = raw
    d_text = eng.malloc(text_cap + 16)
    frames = (c.c_void_p(d_dst), doff.ctypes.data_as(u64p), dlen.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), pexp)

    def verify():
        assert lib.zarc_gpu_verify_batch_device(h, n, *frames, pdig, pst) == 0
        assert (status == 0).all()

    def read(rng, cap_bytes=text_cap):
        assert lib.zarc_gpu_read_ranges_batch_device(h, n, *frames, rng.ctypes.data_as(c.POINTER(_lib.Range)), 0, pdig, pst, pres, c.c_void_p(d_text), cap_bytes, c.byref(tu)) == 0
        assert (status == 0).all()

    # a counting call tells the lines of every frame: the middle is theirs
    read(ranges_of(n, L, 0, 0, 0), 0)
    units = res["units"].copy()
    doc["lines"] = int(units.sum())
    cases = {
        "head_10_lines": ranges_of(n, L, 0, 0, 10),
        "tail_10_lines": ranges_of(n, L, END, 0, 10),
        "middle_1000_lines": ranges_of(n, L, 0, np.maximum(units // np.uint64(2), np.uint64(500)) - np.uint64(500), 1000),
        "middle_4096_bytes": ranges_of(n, B, 0, np.maximum(lens // np.uint64(2), np.uint64(2048)) - np.uint64(2048), 4096),
        "all_bytes": ranges_of(n, B, 0, 0, ALL),
    }
    for name, rng in cases.items():
        rec = pair("%s %s" % (shape, name), verify, lambda: read(rng), raw, timers)
        rec["delivered_bytes"] = tu.value
        rec["taken_units"] = int(res["taken"].sum())
        if name == "all_bytes":
            assert tu.value == raw
            rec["gather_GB_per_s"] = round(tu.value / 1e9 / (rec["kernel_ms_median_of_B"]["T_RANGE"] / 1e3), 1)   # (BYTES ranges: T_RANGE is the carry and the gather)
        doc["cases"][name] = rec
    eng.free(d_text)
    # the host form: the whole content over PCIe and ten lines cut on the host, against ten lines cut on the device
    m = min(n, a.host_entries or (1000 if shape != "small" else 100000))
    span = int(doff[m - 1] + dlen[m - 1])
    blob = bytes(eng.d2h(d_dst, span))
    eng.free(d_dst)
    hframes = [blob[int(doff[i]):int(doff[i] + dlen[i])] for i in range(m)]
    hlens, hdig = [int(x) for x in lens[:m]], [bytes(dig[i]) for i in range(m)]
    hraw = sum(hlens)
    hranges = [(L, 0, 0, 10)] * m
    moved = {}

    def unpack_and_slice():
        out = eng.unpack(hframes, hlens, hdig)
        heads = [b"".join(d.split(b"\n", 10)[:10]) for d, _, _ in out]
        moved["A"] = (eng.copy_bytes(_lib.C_H2D), eng.copy_bytes(_lib.C_D2H), sum(len(x) for x in heads))

    def read_host():
        _, _, text = eng.read_ranges(hframes, hlens, hranges, expect=hdig, text_cap=hraw)
        moved["B"] = (eng.copy_bytes(_lib.C_H2D), eng.copy_bytes(_lib.C_D2H), len(text))
    rec = pair("%s host form, head 10 lines" % shape, unpack_and_slice, read_host, hraw, timers, names=("A_unpack_and_slice", "B_read_ranges"))
    rec["entries"], rec["uncompressed_bytes"] = m, hraw
    rec["copy_bytes_A_h2d_d2h"], rec["copy_bytes_B_h2d_d2h"] = moved["A"][:2], moved["B"][:2]
    doc["host_form_head_10_lines"] = rec
    eng.close()
    return doc


try:
    ndev = _lib.load().zarc_gpu_device_count()
except OSError as e:
    ndev, why = 0, str(e)
else:
    why = "zarc_gpu_device_count() is 0"
if ndev < 1:
    print("range_rate: no usable device (%s): nothing measured, no rate claimed" % why, file=sys.stderr)
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
