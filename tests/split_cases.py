"""Checks of the encoder with ZARC_GPU_PX_BLOCK_SPLIT = 1, shared by the emulator tests (test_split.py) and the GPU tests
(test_gpu_split.py).  The CPU statement of the split-on encoder is tests/support/split_model.c (splitmodel.SplitModel)."""
import json
import os

import parity_cases as pc
import realdata
import splitmodel
from zarc_amd import _lib

SIZES = (0, 1, 5, 65535, 65536, 65537, 131072, 900001)
# the ELF / machine-code / JSON items of tests/support/realdata.py: the ones block splitting is for
BINARY_ITEMS = ("elf_head_4m", "elf_mid_4m", "libc_2m", "python_bin_2m", "torch_64m_2m", "torch_300m_2m", "json_2m", "json_node_2m")
# the review's probes: recorded, not gated
PROBES = (("hipblaslt_4m_2m", "/opt/rocm/lib/libhipblaslt.so", 4 << 20, 2 << 20), ("llvm15_40m_2m", "/usr/lib/x86_64-linux-gnu/libLLVM-15.so.1", 40 << 20, 2 << 20))


def sharp_halves(corpus):
    """Text, then random bytes, then relocation-table-like binary records, all inside ONE 64 KiB block: the statistics change twice."""
    return corpus.entry(61, 22000, 0) + corpus.entry(62, 20000, 3) + realdata.reloc_like(23000)


def split_inputs(corpus, big):
    """name -> bytes: the parity_cases encoder inputs, the sizes around the block size, and what the issue names."""
    c = dict(pc.encode_cases(corpus, big))
    for n in SIZES:
        c["size_%d" % n] = corpus.entry(70 + n % 7, n, -1)
    c["incompressible"] = corpus.entry(63, 200000, 3)
    c["one_byte"] = b"\x5a" * 150000
    c["sharp_halves"] = sharp_halves(corpus)
    # many short pieces: the statistics change every few KiB, over several table groups (the plan guard's ground)
    c["many_pieces"] = b"".join(corpus.entry(900 + i, 3000 + 700 * (i % 5), i % 4) for i in range(600 if big else 90))
    if big:
        c["five_mib"] = b"".join(corpus.entry(80 + k, 1 << 20, k % 3) for k in range(5))  # frame-pass pieces, segment-by-segment search
    return c


class split_on:
    """with split_on(engine, level, checksum): ... -- the switch on, and everything back afterwards"""

    def __init__(self, engine, level=3, checksum=1):
        self.e, self.level, self.checksum = engine, level, checksum

    def __enter__(self):
        self.e.set_parameter(_lib.P_COMPRESSION_LEVEL, self.level)
        self.e.set_parameter(_lib.P_CHECKSUM_FLAG, self.checksum)
        self.e.set_parameter(_lib.PX_BLOCK_SPLIT, 1)
        return self.e

    def __exit__(self, *a):
        self.e.set_parameter(_lib.PX_BLOCK_SPLIT, 0)
        self.e.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
        self.e.set_parameter(_lib.P_COMPRESSION_LEVEL, 3)


def check_frames(engine, oracle, model, libzstds, cases, level, checksum=1):
    """Every split-on frame: equal to the CPU model, valid for the oracle decoder and every libzstd, within zarc_gpu_bound, and restored
    by the engine's own decoder.  Returns {name: blocks}."""
    assert libzstds, "no libzstd on this box: the cross-decoding half of this check would be vacuous"
    names = list(cases)
    with split_on(engine, level, checksum):
        res = engine.pack([cases[k] for k in names])
    blocks = {}
    for k, (frame, dig) in zip(names, res):
        raw = cases[k]
        assert dig == oracle.blake3(raw), (k, level)
        assert frame == model.encode(raw, level, checksum), (k, level, checksum)      # bit-exact vs the CPU statement
        rc, out, used = oracle.zstd_decode(frame, len(raw))
        assert rc == 0 and used == len(frame) and out == raw, (k, level)             # valid Zstandard
        for z in libzstds:
            got, err = z.decompress(frame, len(raw))
            assert got == raw, (k, level, z.version, err)
        assert len(frame) <= engine.bound(len(raw)), (k, level)
        blocks[k] = splitmodel.count_blocks(frame)
    back = engine.unpack([f for f, _ in res], [len(cases[k]) for k in names], [d for _, d in res])
    for k, (out, dig, st) in zip(names, back):
        assert st == _lib.FRAME_OK and out == cases[k] and dig == oracle.blake3(cases[k]), (k, level)
    return blocks


def check_switch_off_unchanged(engine, fresh, oracle, corpus, big):
    """A handle that had the switch on and off again, and a fresh handle, give the frames of the frozen model."""
    cases = pc.encode_cases(corpus, big)
    names = list(cases)
    engine.set_parameter(_lib.PX_BLOCK_SPLIT, 1)
    engine.set_parameter(_lib.PX_BLOCK_SPLIT, 0)
    try:
        for level in (1, 3, 9, 15):
            for e in (engine, fresh):
                e.set_parameter(_lib.P_COMPRESSION_LEVEL, level)
                for k, (frame, _) in zip(names, e.pack([cases[k] for k in names])):
                    assert frame == oracle.zge_encode(cases[k], oracle.params(level=level)), (k, level)
    finally:
        engine.set_parameter(_lib.P_COMPRESSION_LEVEL, 3)
        fresh.set_parameter(_lib.P_COMPRESSION_LEVEL, 3)


def probes():
    out = {}
    for name, path, off, n in PROBES:
        if os.path.exists(path) and os.path.getsize(path) >= off + n:
            with open(path, "rb") as f:
                f.seek(off)
                out[name] = f.read(n)
    return out


def ratio_table(engine, libzstd15, items, levels=(3, 9)):
    """{level: {item: {"off", "on", "libzstd", "blocks_off", "blocks_on"}}} -- frames of the engine with the switch off and on, libzstd
    1.5.x at the same level (the project's yardstick)."""
    names = list(items)
    table = {}
    for level in levels:
        engine.set_parameter(_lib.P_COMPRESSION_LEVEL, level)
        try:
            off = [f for f, _ in engine.pack([items[k] for k in names])]
            with split_on(engine, level):
                on = [f for f, _ in engine.pack([items[k] for k in names])]
        finally:
            engine.set_parameter(_lib.P_COMPRESSION_LEVEL, 3)
        table[level] = {k: {"off": len(a), "on": len(b), "libzstd": len(libzstd15.compress(items[k], level)),
                            "blocks_off": splitmodel.count_blocks(a), "blocks_on": splitmodel.count_blocks(b)}
                        for k, a, b in zip(names, off, on)}
    return table


def check_ratio(engine, libzstd15, real_items, where, out_path=None):
    """No item larger with the switch on, every item inside the existing ratio bounds, the binary items strictly smaller in sum.  The
    per-item table (probes included, ungated) goes to out_path."""
    table = ratio_table(engine, libzstd15, real_items)
    extra = ratio_table(engine, libzstd15, probes()) if probes() else {}
    doc = {"libzstd": libzstd15.version, "where": where, "split_chunks": 16, "gated": {str(l): t for l, t in table.items()},
           "probes_ungated": {str(l): t for l, t in extra.items()}}
    for level, t in list(table.items()) + [(("probe", l), t) for l, t in extra.items()]:
        for k, r in sorted(t.items()):
            print("  L%s %-18s off %8d on %8d (%+.2f %%) libzstd %8d  off/z %.4f on/z %.4f  blocks %d -> %d" % (
                level, k, r["off"], r["on"], 100.0 * (r["on"] - r["off"]) / r["off"], r["libzstd"], r["off"] / r["libzstd"], r["on"] / r["libzstd"],
                r["blocks_off"], r["blocks_on"]))
    if out_path:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    for level, t in table.items():
        larger = {k: (r["off"], r["on"]) for k, r in t.items() if r["on"] > r["off"]}
        assert not larger, (level, larger)                                                            # (a)
        bad = realdata.gate({(k, level): r["on"] / r["libzstd"] for k, r in t.items()}, "%s, split on" % where)
        assert not bad, bad                                                                           # (b)
        binary = [k for k in BINARY_ITEMS if k in t]
        assert binary, "none of the binary items is on this box"
        assert sum(t[k]["on"] for k in binary) < sum(t[k]["off"] for k in binary), level              # (c)
    return doc
