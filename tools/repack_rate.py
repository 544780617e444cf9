#!/usr/bin/env python3
"""Rates of zarc_gpu_repack_batch* (B) against the only route there was before it (A): zarc_gpu_unpack_batch* into buffers, then
zarc_gpu_pack_batch* from them.  Shapes: `c2` (BASELINE configs[1]: 1 MiB synthetic entries, level-3 frames to level 3, checksum on),
`libzstd` (the same content as frames libzstd 1.5 made at level 3) and `small` (the million-entry log-normal shape of bench.py --config
small); each through pageable and through page-locked caller memory, and in the device forms.  `large` is 2 x 1 GiB: what the carried
checksum buys where XXH64 is one long chain per entry (the XXH64 times of both routes, from zarc_gpu_last_kernel_ms).
Every pair is measured alternating A, B, A, B ... in this one process, --runs repetitions each after one warm-up of each; the document
keeps min / median / max of each side, the relative spread s = (max - min) / median of the A side, and whether B is faster than A by
more than that: median(B) > median(A) * (1 + s).
  usage: repack_rate.py [--shapes c2,libzstd,small,large] [--runs 5] [--entries N] [--out profiles/r07_repack_rate.json]"""
import argparse, ctypes, hashlib, json, math, os, random, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,libzstd,small,large")
ap.add_argument("--entries", type=int, default=0, help="entries of a shape (default: 10000 for c2 and libzstd, 1000000 for small, 2 for large)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()
GIB = float(1 << 30)
c = ctypes
hip = c.CDLL("libamdhip64.so")
hip.hipHostMalloc.argtypes = [c.POINTER(c.c_void_p), c.c_size_t, c.c_uint]
hip.hipHostFree.argtypes = [c.c_void_p]
U64 = np.uint64


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def pair(name, run_a, run_b, nbytes, runs):
    """alternating A, B, A, B ...; rates in GiB/s of `nbytes` per call"""
    run_a(); run_b()
    ra, rb = [], []
    for _ in range(runs):
        t0 = time.perf_counter(); run_a(); ra.append(nbytes / (time.perf_counter() - t0) / GIB)
        t0 = time.perf_counter(); run_b(); rb.append(nbytes / (time.perf_counter() - t0) / GIB)
    A, B = summary(ra), summary(rb)
    s = (A["max"] - A["min"]) / A["median"]
    rec = {"A_unpack_then_pack": A, "B_repack": B, "spread_A": round(s, 4), "unit": "GiB/s of uncompressed bytes",
           "claim": "median(B) > median(A) * (1 + s)", "holds": bool(B["median"] > A["median"] * (1 + s))}
    print("%s: A %s  B %s  s %.3f %s" % (name, A["all"], B["all"], s, rec["holds"]), file=sys.stderr, flush=True)
    return rec


def sizes_of(shape):
    if shape == "small":
        rnd = random.Random(822)
        return [max(1, min(16 << 20, int(math.exp(rnd.gauss(math.log(822.0), 1.819))))) for _ in range(a.entries or 1000000)]
    if shape == "large":
        return [1 << 30] * (a.entries or 2)
    return [1 << 20] * (a.entries or 10000)


def layout(lens):
    al = (lens + U64(15)) // U64(16) * U64(16)
    return np.concatenate(([0], np.cumsum(al)[:-1])).astype(U64), int(al.sum())


def shape_doc(shape):
    eng = Engine(0)
    eng.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    eng.set_parameter(_lib.P_COMPRESSION_LEVEL, 3)
    lib, h = eng.lib, eng.h
    lens = np.array(sizes_of(shape), dtype=U64)
    n, raw = len(lens), int(lens.sum())
    off, total = layout(lens)
    blocks = np.maximum((lens + U64(65535)) // U64(65536), U64(1))
    cap = int(((lens + U64(3) * blocks + U64(18 + 15)) // U64(16) * U64(16)).sum())   # sum of zarc_gpu_bound()
    d_src, d_dst = eng.malloc(total + _lib.PAD), eng.malloc(cap + _lib.PAD)
    eng.corpus_fill(d_src, off, lens, first_index=0, kind=-1)
    # ---- the old frames, dense in host memory: the engine's own, or libzstd's of the same content
    if shape == "libzstd":
        import harness
        z = next(z for z in harness.libzstds() if z.version.startswith("1.5"))
        content = eng.d2h(d_src, total)
        with ThreadPoolExecutor(16) as ex:
            made = list(ex.map(lambda i: z.compress(content[int(off[i]):int(off[i]) + int(lens[i])].tobytes(), 3, 1), range(n)))
        flen = np.array([len(f) for f in made], dtype=U64)
        foff, ftotal = layout(flen)
        blob = np.zeros(ftotal + _lib.PAD, dtype=np.uint8)
        for f, o in zip(made, foff):
            blob[int(o):int(o) + len(f)] = np.frombuffer(f, dtype=np.uint8)
        dig = eng.blake3_device(d_src, off, lens)
        del made, content
    else:
        doff, flen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
        assert (st == 0).all()
        foff, ftotal = layout(flen)
        packed = eng.d2h(d_dst, int(doff[-1] + flen[-1]))
        blob = np.zeros(ftotal + _lib.PAD, dtype=np.uint8)
        for i in range(n):
            blob[int(foff[i]):int(foff[i]) + int(flen[i])] = packed[int(doff[i]):int(doff[i]) + int(flen[i])]
        del packed
    doc = {"entries": n, "uncompressed_bytes": raw, "old_frame_bytes": int(flen.sum())}
    runs = a.runs
    # ---- device forms: unpack_device + pack_device (A) against repack_device (B)
    d_frames, d_out = eng.malloc(ftotal + _lib.PAD), d_src   # (the content buffer is free to be A's intermediate)
    eng.h2d(d_frames, blob)
    ms = {}
    def a_dev():
        d, s = eng.unpack_device(d_frames, foff, flen, d_out, off, lens, expect=dig); assert (s == 0).all()
        x = eng.kernel_ms(_lib.T_XXH64)
        r = eng.pack_device(d_out, off, lens, d_dst, cap); assert (r[3] == 0).all()
        ms["A"] = {"xxh64_unpack": round(x, 3), "xxh64_pack": round(eng.kernel_ms(_lib.T_XXH64), 3)}
        return r
    def b_dev():
        r = eng.repack_device(d_frames, foff, flen, lens, d_dst, cap, expect=dig); assert (r[3] == 0).all()
        ms["B"] = {"xxh64": round(eng.kernel_ms(_lib.T_XXH64), 3), "decode": round(eng.kernel_ms(_lib.T_DECODE), 3), "match": round(eng.kernel_ms(_lib.T_MATCH), 3),
                   "entropy": round(eng.kernel_ms(_lib.T_ENTROPY), 3), "assemble": round(eng.kernel_ms(_lib.T_ASSEMBLE), 3), "total": round(eng.kernel_ms(_lib.T_TOTAL), 3)}
        return r
    ra, rb = a_dev(), b_dev()
    assert (ra[1] == rb[1]).all() and (ra[2] == rb[2]).all()      # the same lengths and digests; the tests compare the bytes
    doc["new_frame_bytes"] = int(rb[1].sum())
    rec = pair(shape + " device forms", a_dev, b_dev, raw, runs)
    rec["kernel_ms_last_call"] = dict(ms)
    doc["device"] = rec
    eng.free(d_frames); eng.free(d_src); eng.free(d_dst)
    if shape == "large":
        eng.close()
        return doc
    # ---- host forms, pageable and page-locked caller memory
    digest = np.zeros((n, 32), dtype=np.uint8)
    status = np.zeros(n, dtype=np.int32)
    dst_off, dst_len = np.zeros(n, dtype=U64), np.zeros(n, dtype=U64)
    for kind in ("pageable", "pinned"):
        if kind == "pinned":
            ptrs = [c.c_void_p() for _ in range(3)]
            for p, size in zip(ptrs, (ftotal + 64, total + 64, cap + 64)):
                assert hip.hipHostMalloc(c.byref(p), size, 0) == 0
            fbase, obase, dbase = (p.value for p in ptrs)
            np.ctypeslib.as_array((c.c_uint8 * ftotal).from_address(fbase))[:] = blob[:ftotal]
        else:
            hf, ho, hd = blob, np.zeros(total + 64, dtype=np.uint8), np.zeros(cap + 64, dtype=np.uint8)
            fbase, obase, dbase = hf.ctypes.data, ho.ctypes.data, hd.ctypes.data
        fptr, optr = (foff + U64(fbase)), (off + U64(obase))
        vpp, szp = c.POINTER(c.c_void_p), c.POINTER(c.c_size_t)
        counters = {}
        def a_host():
            assert lib.zarc_gpu_unpack_batch(h, n, fptr.ctypes.data_as(vpp), flen.ctypes.data_as(szp), lens.ctypes.data_as(szp), optr.ctypes.data_as(vpp),
                                             dig.ctypes.data_as(c.c_void_p), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int))) == 0
            cu = [eng.copy_bytes(w) for w in range(4)]
            assert lib.zarc_gpu_pack_batch(h, n, optr.ctypes.data_as(vpp), lens.ctypes.data_as(szp), c.c_void_p(dbase), cap, dst_off.ctypes.data_as(szp),
                                           dst_len.ctypes.data_as(szp), digest.ctypes.data_as(c.c_void_p), status.ctypes.data_as(c.POINTER(c.c_int))) == 0
            counters["A"] = {"unpack": cu, "pack": [eng.copy_bytes(w) for w in range(4)]}
        def b_host():
            assert lib.zarc_gpu_repack_batch(h, n, fptr.ctypes.data_as(vpp), flen.ctypes.data_as(szp), lens.ctypes.data_as(szp), dig.ctypes.data_as(c.c_void_p),
                                             c.c_void_p(dbase), cap, dst_off.ctypes.data_as(szp), dst_len.ctypes.data_as(szp), digest.ctypes.data_as(c.c_void_p),
                                             status.ctypes.data_as(c.POINTER(c.c_int))) == 0 and (status == 0).all()
            counters["B"] = [eng.copy_bytes(w) for w in range(4)]
        rec = pair("%s host forms (%s)" % (shape, kind), a_host, b_host, raw, runs)
        rec["copy_bytes_h2d_d2h_ring_direct"] = counters
        doc["host_" + kind] = rec
        if kind == "pinned":
            for p in ptrs:
                hip.hipHostFree(p)
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
