"""Block splitting (ZARC_GPU_PX_BLOCK_SPLIT) on the HIP emulator and the CPU model: no GPU needed.  The same checks run on the MI355X
in test_gpu_split.py."""
import os
import shutil
import subprocess

import pytest

import split_cases as sc
import splitmodel
from zarc_amd import Engine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    return splitmodel.SplitModel()


def test_parameter_is_known_and_checked(emu_engine):
    lib, h = emu_engine.lib, emu_engine.h
    assert _lib.PX_BLOCK_SPLIT == 9007
    assert lib.zarc_gpu_set_parameter(h, 9007, 1) == _lib.OK
    assert lib.zarc_gpu_set_parameter(h, 9007, 2) == _lib.E_PARAM
    assert lib.zarc_gpu_set_parameter(h, 9007, -1) == _lib.E_PARAM
    assert lib.zarc_gpu_set_parameter(h, 9007, 0) == _lib.OK
    assert lib.zarc_gpu_abi_version() == 2


def test_switch_off_changes_nothing(emu_engine, emu_lib_path, oracle, corpus):
    fresh = Engine(0, emu_lib_path)
    fresh.set_parameter(_lib.P_CHECKSUM_FLAG, 1)
    try:
        sc.check_switch_off_unchanged(emu_engine, fresh, oracle, corpus, big=False)
    finally:
        fresh.close()


def test_split_frames_equal_the_model_and_decode_everywhere(emu_engine, oracle, corpus, libzstds, model):
    cases = sc.split_inputs(corpus, big=False)
    blocks = sc.check_frames(emu_engine, oracle, model, libzstds, cases, level=3)
    n = len(cases["sharp_halves"])
    assert n <= 65536 and blocks["sharp_halves"] > 1, blocks["sharp_halves"]   # more blocks than ceil(n / 65536)
    assert blocks["many_pieces"] > (len(cases["many_pieces"]) + 65535) // 65536


@pytest.mark.parametrize("level", [1, 9, 15])
def test_split_frames_other_levels(emu_engine, oracle, corpus, libzstds, model, level):
    cases = sc.split_inputs(corpus, big=False)
    keep = ["sharp_halves", "many_pieces", "grp_10blk", "cold_hot", "far_repeat", "k0_200k", "incompressible", "one_byte", "runs"] + ["size_%d" % n for n in sc.SIZES]
    blocks = sc.check_frames(emu_engine, oracle, model, libzstds, {k: cases[k] for k in keep}, level=level)
    assert blocks["sharp_halves"] > 1


def test_split_frames_without_checksum(emu_engine, oracle, corpus, libzstds, model):
    cases = sc.split_inputs(corpus, big=False)
    keep = ["sharp_halves", "many_pieces", "size_0", "size_65537", "one_byte"]
    sc.check_frames(emu_engine, oracle, model, libzstds, {k: cases[k] for k in keep}, level=3, checksum=0)


def test_five_mib_entry(emu_engine, oracle, corpus, libzstds, model):
    """Frames above 4 MiB are searched segment by segment and decoded in frame-pass pieces."""
    data = b"".join(corpus.entry(80 + k, 1 << 20, k % 3) for k in range(5))
    sc.check_frames(emu_engine, oracle, model, libzstds, {"five_mib": data}, level=3)


def test_bound_holds_on_incompressible_input(emu_engine, oracle, corpus, libzstds, model):
    """Pieces plus headers of a parent never exceed one raw block: zarc_gpu_bound() keeps its formula with the switch on."""
    cases = {"rand_%d" % n: corpus.entry(300 + i, n, 3) for i, n in enumerate((1000, 65536, 65537, 300000))}
    cases["rand_text_rand"] = corpus.entry(310, 30000, 3) + corpus.entry(311, 3000, 0) + corpus.entry(312, 32000, 3)
    sc.check_frames(emu_engine, oracle, model, libzstds, cases, level=3)
    for n in (0, 1, 65536, 65537, 1 << 20):
        assert emu_engine.bound(n) == (n + 3 * max(1, -(-n // 65536)) + 18 + 15) // 16 * 16


def test_store_mode_ignores_the_switch(emu_engine, corpus):
    ents = [corpus.entry(320, 200000, 0), sc.sharp_halves(corpus), b""]
    emu_engine.enable_compression(False)
    try:
        off = emu_engine.pack(ents)
        with sc.split_on(emu_engine):
            on = emu_engine.pack(ents)
    finally:
        emu_engine.enable_compression(True)
    assert on == off


def test_plan_guard_stays_silent_on_many_short_pieces(emu_engine, oracle, corpus, model):
    """Inputs that give many short pieces over several table groups: no call returns ZARC_GPU_E_DEVICE (Engine.pack raises on it) and
    the model, which carries the same guard as -3, agrees byte for byte."""
    import realdata
    rl = realdata.reloc_like(400000)

    def seg(i, j):  # 7 .. 13 KiB of text, random bytes, binary records or word lists: the statistics change several times per 64 KiB
        k, n = (i + j) % 4, 7000 + 1500 * ((i * 7 + j) % 5)
        return rl[(i * 9973) % 300000:][:n] if k == 2 else corpus.entry(2000 + 97 * j + i, n, (0, 3, 0, 1)[k])
    ents = [b"".join(seg(i, j) for i in range(70)) for j in range(3)]   # 700 000 bytes each: eleven parents, two table groups
    for level in (3, 9):
        with sc.split_on(emu_engine, level):
            res = emu_engine.pack(ents)
        for raw, (frame, _) in zip(ents, res):
            assert frame == model.encode(raw, level)
            assert splitmodel.count_blocks(frame) > (len(raw) + 65535) // 65536 + 3   # the inputs do give many pieces


class ModelAsEngine:
    """pack() by the CPU statements of the encoder (switch off: the frozen model; on: split_model.c) -- what the emulator frames equal."""

    def __init__(self, oracle, model):
        self.oracle, self.model, self.p = oracle, model, {_lib.P_COMPRESSION_LEVEL: 3, _lib.P_CHECKSUM_FLAG: 1, _lib.PX_BLOCK_SPLIT: 0}

    def set_parameter(self, k, v):
        self.p[k] = v

    def pack(self, ents):
        lv, ck = self.p[_lib.P_COMPRESSION_LEVEL], self.p[_lib.P_CHECKSUM_FLAG]
        if self.p[_lib.PX_BLOCK_SPLIT]:
            return [(self.model.encode(e, lv, ck), None) for e in ents]
        return [(self.oracle.zge_encode(e, self.oracle.params(level=lv, checksum=ck)), None) for e in ents]


def test_ratio_on_real_data(oracle, model, libzstd15, real_items):
    """tests/support/realdata.py at levels 3 and 9 against libzstd 1.5.x: no item larger with the switch on, every item inside the
    existing bounds, the ELF / machine-code / JSON items strictly smaller in sum.  On the CPU statements here (emulator frames equal
    them, see above); test_gpu_split.py runs the same gate on the MI355X's frames."""
    sc.check_ratio(ModelAsEngine(oracle, model), libzstd15, real_items, "CPU model")


# ---- host layers: zarc pack --split-blocks ----
@pytest.fixture(scope="module")
def zarc_bin():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "_build/zarc"])
    return os.path.join(ROOT, "tests", "emu", "_build", "zarc")


def _tree(tmp_path, corpus):
    src = tmp_path / "src"
    (src / "sub").mkdir(parents=True)
    (src / "mixed.bin").write_bytes(sc.sharp_halves(corpus))
    (src / "sub" / "text.txt").write_bytes(corpus.entry(401, 180000, 0))
    (src / "sub" / "many.bin").write_bytes(b"".join(corpus.entry(410 + i, 3000, i % 4) for i in range(60)))
    (src / "empty").write_bytes(b"")
    return src


def _run(zarc, args, cwd, devices=None):
    env = dict(os.environ)
    if devices:
        env["HIPEMU_DEVICES"] = str(devices)
    return subprocess.run([zarc] + args, cwd=str(cwd), env=env, capture_output=True, text=True)


def test_cli_split_blocks(zarc_bin, tmp_path, corpus, emu_engine, libzstds):
    src = _tree(tmp_path, corpus)
    r = _run(zarc_bin, ["-vv", "pack", "--output", str(tmp_path / "on.zarc"), "--split-blocks", "src"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "split_blocks=1" in r.stderr                                   # the verbose parameter echo
    assert "--split-blocks" in _run(zarc_bin, ["pack", "--help"], tmp_path).stderr
    r = _run(zarc_bin, ["pack", "--output", str(tmp_path / "off.zarc"), "src"], tmp_path)
    assert r.returncode == 0, r.stderr
    on, off = (tmp_path / "on.zarc").read_bytes(), (tmp_path / "off.zarc").read_bytes()
    assert len(on) < len(off)                                             # mixed.bin splits
    # without the flag the archive is today's: the mixed file's frame is the frozen model's
    import harness
    o = harness.Oracle()
    assert o.zge_encode(sc.sharp_halves(corpus)) in off and o.zge_encode(sc.sharp_halves(corpus)) not in on
    # every content frame of the split archive decodes under libzstd too
    m = splitmodel.SplitModel()
    for p in (src / "mixed.bin", src / "sub" / "text.txt", src / "sub" / "many.bin"):
        frame = m.encode(p.read_bytes(), 3)
        assert frame in on, p
        for z in libzstds:
            assert z.decompress(frame, p.stat().st_size)[0] == p.read_bytes()
    out = tmp_path / "out"
    out.mkdir()
    r = _run(zarc_bin, ["unpack", str(tmp_path / "on.zarc")], out)
    assert r.returncode == 0, r.stderr
    for p in ("mixed.bin", "sub/text.txt", "sub/many.bin", "empty"):
        assert (out / "src" / p).read_bytes() == (src / p).read_bytes(), p
    # two devices deal the batch between two handles: the same archive
    r = _run(zarc_bin, ["pack", "--output", str(tmp_path / "on2.zarc"), "--split-blocks", "--gpus", "2", "src"], tmp_path, devices=2)
    assert r.returncode == 0, r.stderr
    on2 = (tmp_path / "on2.zarc").read_bytes()

    def dir_at(img):  # epilogue: digest_type u8 | directory_offset i64 (negative, from the end); the directory carries a timestamp
        import struct
        return len(img) + struct.unpack("<q", img[-22 + 1:-22 + 9])[0]
    assert dir_at(on2) == dir_at(on) and on2[:dir_at(on2)] == on[:dir_at(on)]
