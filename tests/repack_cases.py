"""Checks of zarc_gpu_repack_batch*, shared by the emulator tests (test_repack.py) and the GPU tests (test_gpu_repack.py).  The oracle is
the engine itself, unchanged: a repacked frame must be, byte for byte, what pack makes of what unpack delivers, and every verdict must be
verify's.  Every comparison is equality.

Run as a script (`python repack_cases.py LIB CHECK`) this file is the child process of check_the_check_fires: the fault injection of the
diagnostic build is steered by environment variables, which the library reads when the call runs."""
import ctypes
import json
import os
import struct
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    for p in (ROOT, HERE, os.path.join(HERE, "support"), os.path.join(HERE, "golden")):
        sys.path.insert(0, p)

import parity_cases as pc  # noqa: E402
import verify_cases as vc  # noqa: E402
from zarc_amd import _lib  # noqa: E402

MODES = vc.MODES  # (level, block splitting, compression): levels 1, 3, 9, 15, level 3 with 9007 on, store mode
MODE_ID = lambda m: "level%d_split%d_%s" % (m[0], m[1], "zstd" if m[2] else "store")  # noqa: E731


def mode(engine, m, **kw):
    return vc.settings(engine, level=m[0], split=m[1], compress=m[2], **kw)


# ---- raw calls: the return code and every output array ---------------------------------------------------------------------------------
def raw_repack(engine, frames, raw_lens, expect=None, cap=None):
    """-> (rc, new_frames, digests, statuses, dst_lens); new_frames[i] is None where dst_len[i] == 0"""
    n = len(frames)
    bufs = [bytes(f) for f in frames]
    ptrs, lens = vc._ptrs(bufs)
    rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
    if cap is None:
        cap = sum(engine.bound(int(r)) for r in raw_lens)
    dst = np.zeros(max(cap, 1), dtype=np.uint8)
    dst_off, dst_len = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    dig = np.zeros((n, 32), dtype=np.uint8)
    status = (ctypes.c_int * n)()
    exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8)) if expect is not None else None
    rc = engine.lib.zarc_gpu_repack_batch(engine.h, n, ptrs, lens, rl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
                                          dst.ctypes.data_as(ctypes.c_void_p), cap, dst_off, dst_len, dig.ctypes.data_as(ctypes.c_void_p), status)
    new = [bytes(dst[dst_off[i]:dst_off[i] + dst_len[i]]) if dst_len[i] else None for i in range(n)]
    if rc == 0:  # slots as in pack: slot i starts where the bounds of the entries before it end
        at = 0
        for i in range(n):
            assert dst_off[i] == at, i
            at += engine.bound(int(raw_lens[i]))
    return rc, new, [bytes(d) for d in dig], [int(s) for s in status], [int(x) for x in dst_len]


def decodes_everywhere(oracle, libzstds, frame, raw, tag):
    rc, out, used = oracle.zstd_decode(frame, len(raw))
    assert rc == 0 and used == len(frame) and out == raw, tag
    for z in libzstds:
        got, err = z.decompress(frame, len(raw))
        assert got == raw, (tag, z.version, err)


# ---- 1. repack equals pack of unpack ---------------------------------------------------------------------------------------------------
def check_equals_pack_of_unpack(engine, oracle, libzstds, frames, raw_lens, expect, target, raws=None, tag="", want_cache=None):
    """one batch into one target mode: frames, lengths and digests are pack's of unpack's, statuses and digests are verify's, the copy
    counters are the two sums, and every new frame is Zstandard for the oracle decoder and every libzstd on the box"""
    assert libzstds, "no libzstd on this box: the cross-decoding half of this check would be vacuous"
    with mode(engine, target):
        rc, new, dig, st, dlen = raw_repack(engine, frames, raw_lens, expect)
        h2d, d2h, ring, direct = vc.copy_counters(engine)
    assert rc == 0, (tag, rc)
    assert h2d == sum(len(f) for f in frames) and d2h == sum(dlen) and ring + direct == h2d + d2h, (tag, h2d, d2h, ring, direct)
    ver = engine.verify(frames, raw_lens, expect)
    assert st == [v[1] for v in ver] and dig == [v[0] for v in ver], tag
    un = engine.unpack(frames, raw_lens, expect)
    good = [i for i in range(len(frames)) if st[i] == _lib.FRAME_OK]
    contents = [un[i][0] for i in good]
    if raws is not None:
        assert contents == [raws[i] for i in good], tag
    key = (target, hash(tuple(contents)))
    if want_cache is not None and key in want_cache:
        want = want_cache[key]
    else:
        with mode(engine, target):
            want = engine.pack(contents)
        if want_cache is not None:
            want_cache[key] = want
    for j, i in enumerate(good):
        assert new[i] == want[j][0] and dlen[i] == len(want[j][0]) and dig[i] == want[j][1], (tag, i)
        decodes_everywhere(oracle, libzstds, new[i], contents[j], (tag, i))
    for i in range(len(frames)):
        if st[i] != _lib.FRAME_OK:
            assert dlen[i] == 0 and new[i] is None, (tag, i)
    return new, dig, st


def check_golden(engine, oracle, corpus, libzstds, golden_frames, limit=None, every_target=True):
    """the committed libzstd frames into the target modes: all of them into each (GPU), or dealt round over the modes (emulator)"""
    frames, raw_lens, expect, raws = vc.golden_set(corpus, oracle, golden_frames, limit)
    assert len(frames) > 20
    cache = {}
    for t, target in enumerate(MODES):
        sel = list(range(len(frames))) if every_target else [i for i in range(len(frames)) if i % len(MODES) == t]
        _, _, st = check_equals_pack_of_unpack(engine, oracle, libzstds, [frames[i] for i in sel], [raw_lens[i] for i in sel], [expect[i] for i in sel], target,
                                               [raws[i] for i in sel], "golden -> %s" % MODE_ID(target), cache)
        assert st == [_lib.FRAME_OK] * len(sel)


def own_cases(corpus, big):
    cases = pc.encode_cases(corpus, big)
    if not big:  # the emulator's encoder runs at some hundred KB/s: every kind of entry once, about 1 MB in all
        cases = {k: cases[k] for k in ("empty", "one", "abc", "zeros", "rand", "k0_1000", "k1_64k", "k0_200k", "k1_131073", "few", "per3", "cold_tail")}
    return [cases[k] for k in cases]


def check_own_frames(engine, oracle, corpus, libzstds, big, source, targets, cache=None):
    raws = own_cases(corpus, big)
    with mode(engine, source):
        packed = engine.pack(raws)
    for target in targets:
        _, _, st = check_equals_pack_of_unpack(engine, oracle, libzstds, [f for f, _ in packed], [len(r) for r in raws], [d for _, d in packed], target, raws,
                                               "%s -> %s" % (MODE_ID(source), MODE_ID(target)), cache)
        assert st == [_lib.FRAME_OK] * len(raws)


def thinned_targets(source):
    """the emulator's matrix: two targets per source, so that every mode is a source once and a target twice"""
    i = MODES.index(source)
    return (MODES[(i + 1) % len(MODES)], MODES[(i + 3) % len(MODES)])


def check_real_items(engine, oracle, libzstds, real_items):
    raws = [v for v in real_items.values()]
    cache = {}
    for source in ((3, 0, True), (9, 0, True)):
        with mode(engine, source):
            packed = engine.pack(raws)
        for target in MODES:
            _, _, st = check_equals_pack_of_unpack(engine, oracle, libzstds, [f for f, _ in packed], [len(r) for r in raws], [d for _, d in packed], target, raws,
                                                   "real %s -> %s" % (MODE_ID(source), MODE_ID(target)), cache)
            assert st == [_lib.FRAME_OK] * len(raws)


# ---- 2. the error list among good frames -----------------------------------------------------------------------------------------------
def check_errors(engine, oracle, corpus, libzstds, golden_frames):
    bad_f, bad_r, bad_e, _ = vc.error_list(oracle, corpus, golden_frames)   # [0] of it is a good frame
    good_raw = [corpus.entry(600 + i, n, i % 4) for i, n in enumerate((30000, 0, 70000, 9, 140000, 2000, 66000, 1))]
    packed = engine.pack(good_raw)
    # a frame that names a dictionary (Dictionary_ID flag 1, id 7): the engine has none
    own = packed[0][0]
    assert own[:4] == b"\x28\xb5\x2f\xfd" and own[4] & 3 == 0
    dict_frame = own[:4] + bytes([own[4] | 1]) + own[5:6] + b"\x07" + own[6:] if not own[4] & 0x20 else own[:4] + bytes([own[4] | 1]) + b"\x07" + own[5:]
    bad_f, bad_r, bad_e = bad_f + [dict_frame], bad_r + [len(good_raw[0])], bad_e + [packed[0][1]]
    frames, raw_lens, expect, is_good = [], [], [], []
    for i in range(len(good_raw)):
        frames.append(packed[i][0]); raw_lens.append(len(good_raw[i])); expect.append(packed[i][1]); is_good.append(True)
        frames.append(bad_f[i]); raw_lens.append(bad_r[i]); expect.append(bad_e[i]); is_good.append(i == 0)
    for target in ((3, 0, True), (9, 0, True), (3, 0, False)):
        new, dig, st = check_equals_pack_of_unpack(engine, oracle, libzstds, frames, raw_lens, expect, target, None, "errors -> %s" % MODE_ID(target))
        bad_st = [s for s, g in zip(st, is_good) if not g]
        assert bad_st[0] == _lib.FRAME_CHECKSUM and bad_st[1] == _lib.FRAME_BAD_MAGIC and bad_st[4] == _lib.FRAME_DIGEST and bad_st[5] == _lib.FRAME_SRCSIZE
        assert bad_st[2] != _lib.FRAME_OK and bad_st[3] != _lib.FRAME_OK and bad_st[6] == _lib.FRAME_UNSUPPORTED, bad_st
        # the good neighbours: byte-identical to a batch without the bad ones
        keep = [i for i, g in enumerate(is_good) if g]
        with mode(engine, target):
            rc, alone, dig_a, st_a, _ = raw_repack(engine, [frames[i] for i in keep], [raw_lens[i] for i in keep], [expect[i] for i in keep])
        assert rc == 0 and st_a == [0] * len(keep)
        assert alone == [new[i] for i in keep] and dig_a == [dig[i] for i in keep]


# ---- 3. copy counters ------------------------------------------------------------------------------------------------------------------
def check_counters(engine, corpus):
    ents = [corpus.entry(80, 30000, 0), corpus.entry(81, 70000, 1), corpus.entry(82, 5000, 2), b"", corpus.entry(83, 40000, 3)]
    packed = engine.pack(ents)
    frames, raw_lens = [f for f, _ in packed], [len(e) for e in ents]
    frames[2] = frames[2][:-2]           # a refused frame comes in and nothing of it goes out
    outs = []
    for chunk in (0, 20000):             # one staged chunk, several
        with vc.settings(engine, chunk=chunk):
            rc, new, dig, st, dlen = raw_repack(engine, frames, raw_lens)
            h2d, d2h, ring, direct = vc.copy_counters(engine)
        assert rc == 0 and st[2] != 0 and dlen[2] == 0 and [s for i, s in enumerate(st) if i != 2] == [0] * 4
        assert h2d == sum(len(f) for f in frames) and d2h == sum(dlen) and ring + direct == h2d + d2h, (chunk, h2d, d2h, ring, direct)
        outs.append((new, dig, st))
    assert outs[0] == outs[1]
    return frames, raw_lens, outs[0]


def check_device_form(engine, oracle, corpus):
    """the device form gives the host form's frames, counts no copies, and reports both halves' times"""
    frames, raw_lens, (new, dig, st) = check_counters(engine, corpus)
    d_frames, foff, _ = vc._arena(engine, frames)
    cap = sum(engine.bound(r) for r in raw_lens)
    d_dst = engine.malloc(cap + 256)
    try:
        dst_off, dst_len, dig_d, st_d = engine.repack_device(d_frames, foff, [len(f) for f in frames], raw_lens, d_dst, cap)
        assert vc.copy_counters(engine) == (0, 0, 0, 0)
        ms = {t: engine.kernel_ms(t) for t in range(10)}
        blob = engine.d2h(d_dst, cap)
        got = [bytes(blob[int(o):int(o) + int(l)]) if l else None for o, l in zip(dst_off, dst_len)]
        assert got == new and [bytes(x) for x in dig_d] == dig and list(st_d) == st
        for t in (_lib.T_DECODE, _lib.T_DEC_FRAMES, _lib.T_BLAKE3, _lib.T_XXH64, _lib.T_MATCH, _lib.T_ENTROPY, _lib.T_ASSEMBLE):
            assert ms[t] >= 0, (t, ms)
        assert ms[_lib.T_TOTAL] >= ms[_lib.T_DECODE] + ms[_lib.T_MATCH] + ms[_lib.T_ENTROPY] + ms[_lib.T_ASSEMBLE] - 1e-3, ms
        dig_v, st_v = engine.verify_device(d_frames, foff, [len(f) for f in frames], raw_lens)
        assert list(st_v) == st and [bytes(x) for x in dig_v] == dig
    finally:
        engine.free(d_frames)
        engine.free(d_dst)


# ---- 4. bounded scratch ----------------------------------------------------------------------------------------------------------------
def check_bounded_scratch(engine, corpus, big):
    """ZARC_GPU_PX_SCRATCH_MB = 2, as verify_cases.check_bounded_scratch: the decoded bytes alone are several times the budget, so the batch
    is halved again and again, and the last entry's encoder scratch alone exceeds it, so that one runs by itself"""
    unit = (512 << 10) if big else (128 << 10)
    raws = [corpus.entry(7000 + i, unit, i % 4) for i in range(24)] + [corpus.entry(7100, 6 * unit, 0), b""]
    packed = engine.pack(raws)
    frames, raw_lens, expect = [f for f, _ in packed], [len(r) for r in raws], [d for _, d in packed]
    frames[3] = frames[3][:-1]          # and something to tell apart
    expect[7] = bytes(32)
    assert sum(raw_lens) > (2 << 20) and 6 * unit * 4 > (2 << 20)   # decoded bytes beyond the budget; the large entry's encoder scratch alone as well
    for target in ((3, 0, True), (3, 1, True)) if big else ((1, 0, True),):
        with mode(engine, target):
            free = raw_repack(engine, frames, raw_lens, expect)
            engine.set_parameter(_lib.PX_SCRATCH_MB, 2)
            try:
                bounded = raw_repack(engine, frames, raw_lens, expect)
                h2d, d2h = vc.copy_counters(engine)[:2]
            finally:
                engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
        assert free[0] == 0 and bounded == free
        assert (h2d, d2h) == (sum(len(f) for f in frames), sum(free[4]))
        assert free[3][3] != 0 and free[3][7] == _lib.FRAME_DIGEST and [s for i, s in enumerate(free[3]) if i not in (3, 7)] == [0] * 24
        assert free[1][3] is None and free[1][7] is None and all(f for i, f in enumerate(free[1]) if i not in (3, 7))


# ---- 5. shapes -------------------------------------------------------------------------------------------------------------------------
def check_large_among_small(engine, oracle, corpus, libzstds, libzstd15, big):
    """many small frames and a few of 4 MiB and more, which the decoder cuts into pieces and the match finder into segments; entries of
    no bytes among them"""
    text = corpus.entry(5151, (4 << 20) + 700000, 0)
    rnd = corpus.entry(5152, (4 << 20) + 300001, 3)
    tiny = [corpus.entry(5200 + i, (40 + 37 * i) if i % 9 else 0, i % 4) for i in range(3000 if big else 70)]
    own = engine.pack([text])[0][0]
    tframes = [f for f, _ in engine.pack(tiny)]
    frames = tframes[:30] + [own] + tframes[30:] + [libzstd15.compress(rnd, 3, 1)]
    raws = tiny[:30] + [text] + tiny[30:] + [rnd]
    if big:
        frames.append(libzstd15.compress(text, 19, 1)); raws.append(text)
    for target in ((3, 0, True), (9, 0, True), (3, 0, False)) if big else ((1, 0, True),):
        _, _, st = check_equals_pack_of_unpack(engine, oracle, libzstds, frames, [len(r) for r in raws], [oracle.blake3(r) for r in raws], target, raws,
                                               "large among small -> %s" % MODE_ID(target))
        assert st == [0] * len(frames)


def check_checksum_carried(engine, oracle, corpus, libzstds, libzstd15):
    """old frames without a checksum (store mode, checksum flag 0, libzstd without) into frames with one: the trailer is the oracle's
    XXH64 of the content; and the reverse: no trailer"""
    raws = [corpus.entry(900 + i, n, i % 4) for i, n in enumerate((50000, 0, 70001, 33, 140000))]
    sources = {}
    engine.set_parameter(_lib.P_CHECKSUM_FLAG, 0)
    try:
        sources["c0"] = [f for f, _ in engine.pack(raws)]
    finally:
        engine.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    with mode(engine, (3, 0, False)):
        sources["store"] = [f for f, _ in engine.pack(raws)]
    sources["libzstd c0"] = [libzstd15.compress(r, 3, 0) for r in raws]
    sources["c1"] = [f for f, _ in engine.pack(raws)]
    raw_lens, expect = [len(r) for r in raws], [oracle.blake3(r) for r in raws]
    for name, frames in sources.items():
        if name != "c1":
            assert all(not f[4] & 4 for f in frames), name      # Content_Checksum_flag clear
        for target in ((3, 0, True), (9, 0, True), (3, 1, True)):
            new, _, st = check_equals_pack_of_unpack(engine, oracle, libzstds, frames, raw_lens, expect, target, raws, "%s -> checksum" % name)
            assert st == [0] * len(raws)
            for f, r in zip(new, raws):
                assert f[4] & 4 and f[-4:] == struct.pack("<I", oracle.xxh64(r) & 0xFFFFFFFF), name
    engine.set_parameter(_lib.P_CHECKSUM_FLAG, 0)
    try:
        with_ck, _, _ = check_equals_pack_of_unpack(engine, oracle, libzstds, sources["c1"], raw_lens, expect, (3, 0, True), raws, "checksum -> none")
        assert with_ck == sources["c0"] and all(not f[4] & 4 for f in with_ck)
    finally:
        engine.set_parameter(_lib.P_CHECKSUM_FLAG, 1)


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------------------
def check_arguments(engine):
    lib, h = engine.lib, engine.h
    c = ctypes
    frame = b"\x28\xb5\x2f\xfd\x20\x00\x01\x00\x00"   # an empty frame
    ptrs, lens = vc._ptrs([frame])
    rl = (c.c_size_t * 1)(0)
    cap = engine.bound(0)
    dst = np.zeros(cap, dtype=np.uint8); pdst = dst.ctypes.data_as(c.c_void_p)
    doff, dlen = (c.c_size_t * 1)(), (c.c_size_t * 1)()
    dig = np.zeros((1, 32), dtype=np.uint8); pdig = dig.ctypes.data_as(c.c_void_p)
    st = (c.c_int * 1)()
    assert lib.zarc_gpu_repack_batch(h, 0, None, None, None, None, None, 0, None, None, None, None) == _lib.OK
    assert lib.zarc_gpu_repack_batch_device(h, 0, None, None, None, None, None, None, 0, None, None, None, None) == _lib.OK
    assert lib.zarc_gpu_repack_batch(h, 1, ptrs, lens, rl, None, pdst, cap, doff, dlen, pdig, st) == _lib.OK and st[0] == 0 and dlen[0] > 0
    good = [ptrs, lens, rl, None, pdst, cap, doff, dlen, pdig, st]
    for k in (0, 1, 2, 4, 6, 7, 8, 9):      # every pointer but expect; status is required
        args = list(good); args[k] = None
        assert lib.zarc_gpu_repack_batch(h, 1, *args) == _lib.E_PARAM, k
    nullp = (c.c_void_p * 1)(None)
    assert lib.zarc_gpu_repack_batch(h, 1, nullp, lens, rl, None, pdst, cap, doff, dlen, pdig, st) == _lib.E_PARAM
    assert lib.zarc_gpu_repack_batch(h, 1, ptrs, lens, rl, None, pdst, cap - 1, doff, dlen, pdig, st) == _lib.E_DSTSIZE
    big = (c.c_size_t * 1)(0xFFFFFFF0)
    assert lib.zarc_gpu_repack_batch(h, 1, ptrs, lens, big, None, pdst, cap, doff, dlen, pdig, st) == _lib.E_UNSUPPORTED   # (before the slot arithmetic: not DSTSIZE)
    assert lib.zarc_gpu_repack_batch(h, 1, ptrs, big, rl, None, pdst, cap, doff, dlen, pdig, st) == _lib.E_UNSUPPORTED
    u64 = lambda v: (c.c_uint64 * 1)(v)  # noqa: E731
    dummy = c.c_void_p(16)  # never dereferenced: the call is refused before
    d_good = [dummy, u64(0), u64(9), u64(0), None, dummy, cap, u64(0), u64(0), pdig, st]
    for k in (0, 1, 2, 3, 5, 7, 8, 9, 10):
        args = list(d_good); args[k] = None
        assert lib.zarc_gpu_repack_batch_device(h, 1, *args) == _lib.E_PARAM, k
    args = list(d_good); args[6] = cap - 1
    assert lib.zarc_gpu_repack_batch_device(h, 1, *args) == _lib.E_DSTSIZE
    args = list(d_good); args[3] = u64(0xFFFFFFF0)
    assert lib.zarc_gpu_repack_batch_device(h, 1, *args) == _lib.E_UNSUPPORTED
    args = list(d_good); args[2] = u64(1 << 32)
    assert lib.zarc_gpu_repack_batch_device(h, 1, *args) == _lib.E_UNSUPPORTED
    assert lib.zarc_gpu_abi_version() == 2


# ---- 7. read-back check ----------------------------------------------------------------------------------------------------------------
def fire_frames(engine, corpus):
    """verify_cases.fire_batch as frames, with a refused frame in front of the one the fault goes into: entry 5 stays entry 5"""
    ents = vc.fire_batch(corpus)
    packed = engine.pack(ents)
    frames = [f for f, _ in packed]
    frames[2] = frames[2][:-3]
    return frames, [len(e) for e in ents], [d for _, d in packed]


def check_switch_changes_nothing(engine, corpus, big):
    frames, raw_lens, expect = fire_frames(engine, corpus)
    for target in MODES if big else ((1, 0, True), (3, 1, True), (3, 0, False)):
        res = []
        for check in (0, 1):
            for chunk in (0, 30000):
                with mode(engine, target, check=check, chunk=chunk):
                    res.append(raw_repack(engine, frames, raw_lens, expect))
        assert res[0][0] == 0 and res[0][3][2] != 0 and res[0][1][2] is None and sum(s == 0 for s in res[0][3]) == 7
        assert res[1] == res[0] and res[2] == res[0] and res[3] == res[0], target


def _child_main(lib_path, check):
    import harness
    from zarc_amd import Engine
    e = Engine(0, lib_path)
    e.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    frames, raw_lens, expect = fire_frames(e, harness.Corpus())
    e.set_parameter(_lib.PX_CHECK_FRAMES, int(check))
    rc, new, digs, st, dlen = raw_repack(e, frames, raw_lens, expect)
    print(json.dumps({"rc": rc, "status": st, "dst_len": dlen, "message": e.lib.zarc_gpu_last_error(e.h).decode(), "name": e.lib.zarc_gpu_error_name(rc).decode()}))


def run_child(lib_path, check, env_extra):
    env = dict(os.environ)
    env.pop("ZARC_GPU_CHECK_FLIP_BODY", None); env.pop("ZARC_GPU_CHECK_FLIP_TAIL", None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), lib_path, str(check)], env=env, stdout=subprocess.PIPE, check=True, timeout=900).stdout
    return json.loads(out.decode().strip().splitlines()[-1])


def check_the_check_fires(diag_lib_path):
    """the flip hook of the diagnostic build (its pack calls inside the child are unchecked: the switch goes on behind them)"""
    import re
    r = run_child(diag_lib_path, 1, {})
    assert r["rc"] == 0 and r["status"][2] != 0 and [s for i, s in enumerate(r["status"]) if i != 2] == [0] * 7, r
    good_len = r["dst_len"]
    assert good_len[2] == 0
    r2 = run_child(diag_lib_path, 1, {"ZARC_GPU_CHECK_FLIP_BODY": "5"})
    assert r2["rc"] == _lib.E_CHECK and r2["name"] == "Frame failed its read-back check", r2
    assert r2["status"][5] == _lib.FRAME_CORRUPT and r2["dst_len"][5] == 0 and r2["dst_len"][:5] == good_len[:5], r2
    assert [s for i, s in enumerate(r2["status"]) if i != 5] == [s for i, s in enumerate(r["status"]) if i != 5], r2
    m = re.search(r"entry (\d+) .*byte (\d+)", r2["message"])
    assert m and int(m.group(1)) == 5 and int(m.group(2)) < 100000, r2
    r3 = run_child(diag_lib_path, 1, {"ZARC_GPU_CHECK_FLIP_TAIL": "5"})
    assert r3["rc"] == _lib.E_CHECK and r3["status"][5] == _lib.FRAME_CORRUPT, r3
    assert re.search(r"entry 5\b", r3["message"]) and "trailer" in r3["message"], r3
    r4 = run_child(diag_lib_path, 0, {"ZARC_GPU_CHECK_FLIP_BODY": "5", "ZARC_GPU_CHECK_FLIP_TAIL": "5"})
    assert r4["rc"] == 0 and r4["status"] == r["status"] and r4["dst_len"] == good_len, r4      # the check did not run


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])
