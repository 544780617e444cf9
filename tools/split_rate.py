#!/usr/bin/env python3
"""Pack / unpack rates with block splitting (ZARC_GPU_PX_BLOCK_SPLIT) off and on, same corpus and sizes as BASELINE configs[1]
(10 000 x 1 MiB synthetic entries, level 3, checksum on), everything resident in HBM, kernel times from HIP events
(zarc_gpu_last_kernel_ms).  With the switch on the split kernel runs inside the entropy-stage interval, so T_ENTROPY is the entropy
stage plus the cut decision.  One JSON document on stdout (and in --out).
  usage: split_rate.py [--entries 10000] [--runs 3] [--warmup 1] [--level 3] [--real 40] [--out profiles/r05_split_rate.json]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zarc_amd import Engine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--entries", type=int, default=10000)
ap.add_argument("--size", type=int, default=1 << 20)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--level", type=int, default=3)
ap.add_argument("--out", default="")
ap.add_argument("--real", type=int, default=0, help="also measure on the real-data items, the list of their 1 MiB entries repeated this many times")
a = ap.parse_args()
GIB = float(1 << 30)
eng = Engine(0)
eng.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
eng.set_parameter(_lib.P_COMPRESSION_LEVEL, a.level)
n = a.entries
lens = np.full(n, a.size, dtype=np.uint64)
off = (np.arange(n, dtype=np.uint64) * np.uint64((a.size + 15) // 16 * 16))
total = int(off[-1]) + a.size
eng2_bound = eng.bound(a.size)
cap = n * int(eng2_bound)
d_src, d_dst, d_out = eng.malloc(total + _lib.PAD), eng.malloc(cap + _lib.PAD), eng.malloc(total + _lib.PAD)
eng.corpus_fill(d_src, off, lens, first_index=0, kind=-1)
doc = {"entries": n, "entry_bytes": a.size, "level": a.level, "runs": a.runs, "warmup": a.warmup, "settings": {}}
for split in (0, 1, 0, 1)[:2 if a.runs < 2 else 4]:   # off, on, off, on: a drift of the machine shows as a gap between the two visits of a setting
    eng.set_parameter(_lib.PX_BLOCK_SPLIT, split)
    rec = doc["settings"].setdefault("split_%d" % split, {"pack_gibs": [], "entropy_ms": [], "match_ms": [], "assemble_ms": [], "unpack_gibs": [], "decode_ms": [],
                                                          "dec_seqs_ms": [], "dec_lits_ms": [], "dec_frames_ms": []})
    for _ in range(a.warmup):
        doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
    for _ in range((a.runs + 1) // 2 if a.runs >= 2 else a.runs):
        t0 = time.perf_counter()
        doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
        dt = time.perf_counter() - t0
        assert (st == 0).all()
        rec["pack_gibs"].append(round(n * a.size / dt / GIB, 2))
        rec["entropy_ms"].append(round(eng.kernel_ms(_lib.T_ENTROPY), 2))
        rec["match_ms"].append(round(eng.kernel_ms(_lib.T_MATCH), 2))
        rec["assemble_ms"].append(round(eng.kernel_ms(_lib.T_ASSEMBLE), 2))
    rec["compressed_bytes"] = int(dlen.sum())
    for _ in range(a.warmup):
        dig2, st2 = eng.unpack_device(d_dst, doff, dlen, d_out, off, lens, expect=dig)
    for _ in range((a.runs + 1) // 2 if a.runs >= 2 else a.runs):
        t0 = time.perf_counter()
        dig2, st2 = eng.unpack_device(d_dst, doff, dlen, d_out, off, lens, expect=dig)
        dt = time.perf_counter() - t0
        assert (st2 == 0).all() and (dig2 == dig).all()
        rec["unpack_gibs"].append(round(n * a.size / dt / GIB, 2))
        rec["decode_ms"].append(round(eng.kernel_ms(_lib.T_DECODE), 2))
        rec["dec_seqs_ms"].append(round(eng.kernel_ms(_lib.T_DEC_SEQS), 2))
        rec["dec_lits_ms"].append(round(eng.kernel_ms(_lib.T_DEC_LITS), 2))
        rec["dec_frames_ms"].append(round(eng.kernel_ms(_lib.T_DEC_FRAMES), 2))
    print("split %d: pack %s GiB/s, entropy stage %s ms, unpack %s GiB/s, %d bytes" % (split, rec["pack_gibs"], rec["entropy_ms"], rec["unpack_gibs"], rec["compressed_bytes"]),
          file=sys.stderr, flush=True)
for p in (d_src, d_dst, d_out):
    eng.free(p)
eng.close()

# The synthetic corpus has nothing to cut (its frames come out the same bytes): the decoder's side of the switch shows on data that
# does split -- the items of tests/support/realdata.py present on the box, cut into 1 MiB entries, the list repeated to ~2 GiB.
if a.real:
    sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
    import realdata
    ents = [v[o:o + a.size] for k, v in sorted(realdata.items().items()) if v is not None and k != "periodic_4m" for o in range(0, len(v), a.size)]
    ents = [e for e in ents if len(e) == a.size] * a.real
    n = len(ents)
    blob = np.frombuffer(b"".join(ents), dtype=np.uint8)
    lens = np.full(n, a.size, dtype=np.uint64)
    off = np.arange(n, dtype=np.uint64) * np.uint64(a.size)
    cap = n * int(eng2_bound)
    eng = Engine(0)
    eng.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    eng.set_parameter(_lib.P_COMPRESSION_LEVEL, a.level)
    d_src, d_dst, d_out = eng.malloc(n * a.size + _lib.PAD), eng.malloc(cap + _lib.PAD), eng.malloc(n * a.size + _lib.PAD)
    eng.h2d(d_src, blob)
    real = doc["real_data"] = {"entries": n, "settings": {}}
    for split in (0, 1, 0, 1):
        eng.set_parameter(_lib.PX_BLOCK_SPLIT, split)
        rec = real["settings"].setdefault("split_%d" % split, {"pack_gibs": [], "entropy_ms": [], "unpack_gibs": [], "decode_ms": [], "dec_seqs_ms": [], "dec_lits_ms": [], "dec_frames_ms": []})
        doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
        for _ in range(3):
            t0 = time.perf_counter()
            doff, dlen, dig, st = eng.pack_device(d_src, off, lens, d_dst, cap)
            dt = time.perf_counter() - t0
            assert (st == 0).all()
            rec["pack_gibs"].append(round(n * a.size / dt / GIB, 2))
            rec["entropy_ms"].append(round(eng.kernel_ms(_lib.T_ENTROPY), 2))
        rec["compressed_bytes"] = int(dlen.sum())
        dig2, st2 = eng.unpack_device(d_dst, doff, dlen, d_out, off, lens, expect=dig)
        for _ in range(3):
            t0 = time.perf_counter()
            dig2, st2 = eng.unpack_device(d_dst, doff, dlen, d_out, off, lens, expect=dig)
            dt = time.perf_counter() - t0
            assert (st2 == 0).all() and (dig2 == dig).all()
            rec["unpack_gibs"].append(round(n * a.size / dt / GIB, 2))
            for key, t in (("decode_ms", _lib.T_DECODE), ("dec_seqs_ms", _lib.T_DEC_SEQS), ("dec_lits_ms", _lib.T_DEC_LITS), ("dec_frames_ms", _lib.T_DEC_FRAMES)):
                rec[key].append(round(eng.kernel_ms(t), 2))
        print("real data, split %d: pack %s GiB/s, entropy stage %s ms, unpack %s GiB/s, %d bytes" % (split, rec["pack_gibs"], rec["entropy_ms"], rec["unpack_gibs"], rec["compressed_bytes"]),
              file=sys.stderr, flush=True)
    for p in (d_src, d_dst, d_out):
        eng.free(p)
    eng.close()
text = json.dumps(doc, indent=1, sort_keys=True)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
