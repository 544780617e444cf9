"""`zarc repack` (zarc_amd/host/zarc_cli.cpp), and through it ArchiveWriter::repack_from and Encoder::repack_frames on one and on two
devices: an archive becomes another archive with the same directory and the content frames `zarc pack` writes at the target flags; a
frame that is not good costs the whole run and leaves nothing behind.  tests/host/repack_test.cpp compares the parsed directories."""
import base64
import filecmp
import os
import re
import subprocess

import pytest

from test_cli import make_tree
from test_container import parse_archive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SRC = os.path.join(ROOT, "tests", "host", "repack_test.cpp")
SUMMARY = re.compile(r"repacked (\d+) frames \((\d+) -> (\d+) bytes\), (\d+) kept")


def build_host_test(out_dir, lib_dir, lib_name):
    exe = os.path.join(str(out_dir), "repack_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, HOST_SRC, "-L" + lib_dir, "-l" + lib_name,
                           "-Wl,-rpath," + lib_dir, "-pthread"])
    return exe


def same_tree(a, b):
    """contents, modes, modification times and link targets of two unpacked trees"""
    for root, dirs, files in os.walk(a):
        rel = os.path.relpath(root, a)
        other = os.path.join(b, rel)
        assert sorted(os.listdir(root)) == sorted(os.listdir(other)), rel
        for name in dirs + files:
            x, y = os.path.join(root, name), os.path.join(other, name)
            sx, sy = os.lstat(x), os.lstat(y)
            assert sx.st_mode == sy.st_mode, x
            if os.path.islink(x):
                assert os.readlink(x) == os.readlink(y)
                continue
            assert sx.st_mtime_ns == sy.st_mtime_ns, x
            if os.path.isfile(x):
                assert filecmp.cmp(x, y, shallow=False), x
                try:
                    assert {k: os.getxattr(x, k) for k in os.listxattr(x)} == {k: os.getxattr(y, k) for k in os.listxattr(y)}, x
                except OSError:
                    pass


def run_repack_cases(binary, tmp_path, corpus, oracle, gpus, env, host_exe):
    files = make_tree(tmp_path, corpus)   # duplicates (a.txt == sub/c.txt), a symlink, directories, xattrs where the file system takes them

    def dec(frame, raw_len):
        st, o, _ = oracle.zstd_decode(frame, raw_len)
        assert st == 0
        return o

    def zarc(*args, cwd=tmp_path, check=True):
        r = subprocess.run([binary] + [str(a) for a in args], cwd=cwd, capture_output=True, timeout=1800, env=env)
        assert not check or r.returncode == 0, (args, r.stderr[-600:])
        return r

    def frames_of(img):
        a = parse_archive(img, dec, oracle.blake3)
        return a, {bytes(f[2]): img[f[1]:f[1] + f[3]] for f in a["frames"]}

    src_arc = tmp_path / "in.zarc"
    zarc("pack", "--output", src_arc, "--level", "3", "src")
    img_in = src_arc.read_bytes()
    a_in, fr_in = frames_of(img_in)
    raw_len = {bytes(f[2]): f[4] for f in a_in["frames"]}
    listing = zarc("list-files", "--decorate", src_arc).stdout
    unpack_in = tmp_path / "unpacked_in"
    unpack_in.mkdir()
    zarc("unpack", src_arc, cwd=unpack_in)

    for k, flags in enumerate((["--level", "9"], ["--store"], ["--split-blocks", "--check"], ["--level", "1"])):
        out_arc, ref_arc = tmp_path / ("out%d.zarc" % k), tmp_path / ("ref%d.zarc" % k)
        r = zarc("repack", src_arc, "--output", out_arc, *flags)
        digest = re.fullmatch(rb"digest: ([A-Za-z0-9+/]{43}=)\n", r.stdout).group(1)
        m = SUMMARY.search(r.stderr.decode())
        img = out_arc.read_bytes()
        a, fr = frames_of(img)
        assert base64.b64encode(img[-54:-22]) == digest
        assert m and [int(x) for x in m.groups()] == [4, sum(len(f) for f in fr_in.values()), sum(len(f) for f in fr.values()), 0], r.stderr
        # the directory: every file entry as it was; frame records new in offset and length only
        assert a["files"] == a_in["files"] and a["editions"] == a_in["editions"]
        assert [(f[0], bytes(f[2]), f[4]) for f in a["frames"]] == [(1, bytes(f[2]), f[4]) for f in a_in["frames"]]
        assert zarc("list-files", "--decorate", out_arc).stdout == listing
        # the content frames: what pack writes for the same tree at the same flags, byte for byte, in the same places
        zarc("pack", "--output", ref_arc, *[f for f in flags if f != "--check"], "src")
        ref = ref_arc.read_bytes()
        a_ref, fr_ref = frames_of(ref)
        assert fr == fr_ref and img[:a["dir_at"]] == ref[:a_ref["dir_at"]], flags
        for d, f in fr.items():
            assert dec(f, raw_len[d]) == dec(fr_in[d], raw_len[d]) and oracle.blake3(dec(f, raw_len[d])) == d
        if k == 0:
            unpack_out = tmp_path / "unpacked_out"
            unpack_out.mkdir()
            zarc("unpack", out_arc, cwd=unpack_out)
            same_tree(str(unpack_in), str(unpack_out))
            if host_exe:
                o = subprocess.check_output([host_exe, str(src_arc), str(out_arc)], timeout=1800, env=env)
                assert b"repack directories equal: 9 files, 4 frames" in o and b"repack OK" in o and (gpus < 2 or b"on 2 device(s) OK" in o), o
            if gpus > 1:       # --gpus 2: the same file
                two = tmp_path / "out_two.zarc"
                zarc("repack", src_arc, "--output", two, "--gpus", str(gpus), *flags)
                assert two.read_bytes() == img

    # --keep-smaller: from level 9 down to level 1 some frames grow; those are copied, and the count says how many
    lens_old = {d: len(f) for d, f in frames_of((tmp_path / "out0.zarc").read_bytes())[1].items()}
    plain = tmp_path / "down.zarc"
    zarc("repack", tmp_path / "out0.zarc", "--output", plain, "--level", "1")
    lens_new = {d: len(f) for d, f in frames_of(plain.read_bytes())[1].items()}
    kept_want = sum(lens_new[d] >= lens_old[d] for d in lens_old)
    ks = tmp_path / "down_ks.zarc"
    r = zarc("repack", tmp_path / "out0.zarc", "--output", ks, "--level", "1", "--keep-smaller")
    fr_old, fr_ks = frames_of((tmp_path / "out0.zarc").read_bytes())[1], frames_of(ks.read_bytes())[1]
    assert int(SUMMARY.search(r.stderr.decode()).group(4)) == kept_want and kept_want >= 1
    for d in lens_old:
        assert len(fr_ks[d]) <= lens_old[d]
        assert fr_ks[d] == (fr_old[d] if lens_new[d] >= lens_old[d] else frames_of(plain.read_bytes())[1][d])
    assert zarc("verify", ks).returncode == 0

    # --verify: the input's digest is checked before anything is decoded
    good_digest = base64.b64encode(img_in[-54:-22]).decode()
    assert zarc("repack", src_arc, "--output", tmp_path / "v.zarc", "--verify", good_digest).returncode == 0
    r = zarc("repack", src_arc, "--output", tmp_path / "v2.zarc", "--verify", "A" * 43 + "=", check=False)
    assert r.returncode == 1 and b"integrity failure" in r.stderr and not (tmp_path / "v2.zarc").exists()
    # level tiers and advisory parameters are announced as in pack
    r = zarc("repack", src_arc, "--output", tmp_path / "w.zarc", "--level", "19", "--zstd", "Strategy=btopt")
    assert b"level-15 finder" in r.stderr and b"advisory" in r.stderr

    # one corrupt frame (the one a.txt and sub/c.txt share): non-zero exit, both paths named, nothing left at --output
    shared = oracle.blake3(files["a.txt"])
    fr = next(f for f in a_in["frames"] if bytes(f[2]) == shared)
    broken = bytearray(img_in); broken[fr[1] + fr[3] // 2] ^= 0xFF
    bad_arc = tmp_path / "broken.zarc"
    bad_arc.write_bytes(bytes(broken))
    outdir = tmp_path / "outdir"
    outdir.mkdir()
    for g in ([0, gpus] if gpus > 1 else [0]):
        r = zarc("repack", bad_arc, "--output", outdir / "never.zarc", *(["--gpus", str(g)] if g else []), check=False)
        errors = sorted(l for l in r.stderr.decode().splitlines() if l.startswith("ERROR "))
        assert r.returncode == 1 and len(errors) == 2 and errors[0].endswith(" path=src/a.txt") and errors[1].endswith(" path=src/sub/c.txt"), r.stderr
        assert all("digest=%s " % base64.b64encode(shared).decode() in e for e in errors)
        assert os.listdir(outdir) == []


def test_repack_cli_emulated(emu_lib_path, tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "host"])
    binary = os.path.join(ROOT, "tests", "emu", "_build", "zarc")
    host_exe = build_host_test(tmp_path, os.path.dirname(emu_lib_path), "zarc_gpu_emu")
    run_repack_cases(binary, tmp_path, corpus, oracle, gpus=2, env=dict(os.environ, HIPEMU_DEVICES="2"), host_exe=host_exe)


@pytest.mark.gpu
def test_repack_cli_gpu(tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zarc_amd", "csrc"), "host"])
    binary = os.path.join(ROOT, "zarc_amd", "zarc")
    host_exe = build_host_test(tmp_path, os.path.join(ROOT, "zarc_amd"), "zarc_gpu")
    from zarc_amd import _lib
    ndev = _lib.load().zarc_gpu_device_count()
    run_repack_cases(binary, tmp_path, corpus, oracle, gpus=2 if ndev >= 2 else 0, env=None, host_exe=host_exe)
