"""`zarc cat` (zarc_amd/host/zarc_cli.cpp), and through it ArchiveReader::read_ranges and FrameReader::range_content_frames on one and on two
devices: the content of the files of an archive, or one byte or line range of each, on stdout; each distinct frame read once, nothing
written.  Expected output comes from Python over the files' bytes (range_cases.ref_range), in directory order, and -- where the tools are
installed -- from head, tail and sed run on the source tree."""
import os
import re
import shutil
import subprocess

import pytest

import range_cases as rc
from test_cli import make_tree
from test_container import parse_archive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, B = rc.L, rc.B

# option form -> (the range of include/zarc_gpu.h's table, the tool that prints the same or None)
FORMS = [
    (("--head", "3"), rc.head(3), ["head", "-n", "3"]),
    (("--head", "0"), rc.head(0), ["head", "-n", "0"]),
    (("--head", "-3"), rc.head_minus(3), ["head", "-n", "-3"]),
    (("--head", "-100000"), rc.head_minus(100000), ["head", "-n", "-100000"]),
    (("--tail", "3"), rc.tail(3), ["tail", "-n", "3"]),
    (("--tail", "+4"), rc.tail_plus(4), ["tail", "-n", "+4"]),
    (("--tail", "+0"), rc.tail_plus(1), ["tail", "-n", "+0"]),
    (("--lines", "2:5"), rc.span(2, 5), ["sed", "-n", "2,5p"]),
    (("--lines", "7:7"), rc.span(7, 7), ["sed", "-n", "7,7p"]),
    (("--lines", "3:"), rc.tail_plus(3), ["sed", "-n", "3,$p"]),
    (("--head-bytes", "100"), rc.head(100, B), ["head", "-c", "100"]),
    (("--head-bytes", "-100"), rc.head_minus(100, B), ["head", "-c", "-100"]),
    (("--tail-bytes", "50"), rc.tail(50, B), ["tail", "-c", "50"]),
    (("--tail-bytes", "+10"), rc.tail_plus(10, B), ["tail", "-c", "+10"]),
    (("--bytes", "5:105"), (B, 0, 5, 100), None),
    (("--bytes", "7:"), (B, 0, 7, rc.ALL), None),
    (("--bytes", "9:9"), (B, 0, 9, 0), None),
]


def cut(d, rng):
    _, _, _, start, length = rc.ref_range(d, rng)
    return d[start:start + length]


def run_cat_cases(binary, tmp_path, corpus, oracle, gpus, env):
    files = make_tree(tmp_path, corpus)                      # a.txt == sub/c.txt: 5 files, 4 distinct contents (one of them empty)
    arc = tmp_path / "out.zarc"
    subprocess.run([binary, "pack", "--output", str(arc), "src"], cwd=tmp_path, capture_output=True, timeout=900, check=True, env=env)
    img = arc.read_bytes()
    listed = subprocess.run([binary, "list-files", "--only-files", str(arc)], capture_output=True, timeout=600, check=True, env=env).stdout.decode().split("\n")
    order = [p for p in listed if p[4:] in files]            # directory order of the normal files ("src/" + name)
    assert sorted(order) == sorted("src/" + k for k in files)
    empty = tmp_path / "nothing_here"
    empty.mkdir()

    def cat(*args, g=0, archive=arc):
        cmd = [binary, "cat"] + list(args) + (["--gpus", str(g)] if g else []) + [str(archive)]
        r = subprocess.run(cmd, cwd=empty, capture_output=True, timeout=900, env=env)
        assert os.listdir(empty) == []                       # it creates nothing
        return r.returncode, r.stdout, r.stderr.decode("latin-1").splitlines()

    def want(rng, only=None, header=False, skip=()):
        out, n = b"", 0
        for p in order:
            if (only and not re.search(only, p)) or p in skip: continue
            part = files[p[4:]] if rng is None else cut(files[p[4:]], rng)
            if header: out += (b"\n" if n else b"") + b"==> " + p.encode() + b" <==\n"
            out += part
            n += 1
        return out

    def tool(cmd, header=False):
        if not shutil.which(cmd[0]): return None
        tenv = dict(os.environ, LC_ALL="C")
        if header: return subprocess.run([cmd[0], "-v"] + cmd[1:] + order, cwd=tmp_path, capture_output=True, check=True, env=tenv).stdout
        return b"".join(subprocess.run(cmd + [p], cwd=tmp_path, capture_output=True, check=True, env=tenv).stdout for p in order)

    whole = want(None)
    assert len(whole) == sum(len(files[p[4:]]) for p in order) and files["a.txt"].count(b"\n") > 10 and files["sub/deep/d.rec"].count(b"\n") > 10
    # without a range option: the files' bytes
    rc0, out, err = cat()
    assert rc0 == 0 and out == whole and err[-1] == "printed 5 files (4 frames, %d bytes), 0 failed" % len(whole)
    # every option form against the reference and against the tools
    compared = 0
    for opt, rng, cmd in FORMS:
        exp = want(rng)
        rc1, out, err = cat(*opt)
        assert rc1 == 0 and out == exp, opt
        assert err[-1] == "printed 5 files (4 frames, %d bytes), 0 failed" % len(exp), opt   # the shared frame: read once, printed twice
        if cmd:
            t = tool(cmd)
            if t is not None:
                assert t == exp, (opt, cmd)
                compared += 1
    assert want(rc.head(3)).count(cut(files["a.txt"], rc.head(3))) >= 2 and want(rc.head(3)) != want(rc.tail(3)) != want(rc.span(2, 5))
    if shutil.which("head") and shutil.which("tail") and shutil.which("sed"): assert compared == sum(1 for f in FORMS if f[2])
    # --header is head -v, byte for byte
    exp = want(rc.head(3), header=True)
    assert cat("--header", "--head", "3")[:2] == (0, exp) and exp.startswith(b"==> " + order[0].encode() + b" <==\n") and b"\n\n==> " in exp
    t = tool(["head", "-n", "3"], header=True)
    assert t is None or t == exp
    assert cat("--header")[:2] == (0, want(None, header=True))
    # --filter, --gpus
    assert cat("--tail", "2", "--filter", r"sub/")[:2] == (0, want(rc.tail(2), only=r"sub/")) and want(rc.tail(2), only=r"sub/") != want(rc.tail(2))
    if gpus > 1:
        for opt in (("--head", "5"), ("--tail", "+3"), ()):
            assert cat(*opt, g=gpus)[:2] == cat(*opt)[:2]
    # --batch-bytes too small for a call: the rest comes by continuation calls, the output is the same
    exp = want(rc.tail_plus(2))
    assert len(exp) > 300000
    for bb, opt, e1 in (("100000", ("--tail", "+2"), exp), ("70001", ("--tail", "+2"), exp),
                        ("1", ("--head-bytes", "20", "--filter", r"\.txt$"), want(rc.head(20, B), only=r"\.txt$"))):   # (a byte a call)
        rc1, out, err = cat("--batch-bytes", bb, *opt)
        assert rc1 == 0 and out == e1, bb
    # usage errors
    for bad in (["--head", "3", "--tail", "3"], ["--head", "x"], ["--head", "3k"], ["--head", "--3"], ["--tail", "-3"], ["--lines", "0:3"], ["--lines", "5:3"],
                ["--lines", "5"], ["--bytes", "5"], ["--bytes", "9:3"], ["--batch-bytes", "0"], ["--head", "99999999999999999999999"], ["--frobnicate"], ["--head"]):
        rc1, out, err = cat(*bad)
        assert rc1 == 2 and out == b"" and not any(l.startswith("printed") for l in err), bad

    # one byte flipped in the middle of the frame that a.txt and sub/c.txt share: both files print nothing, the others are printed
    def dec(frame, raw_len):
        st, o, _ = oracle.zstd_decode(frame, raw_len)
        assert st == 0
        return o
    arch = parse_archive(img, dec, oracle.blake3)
    fr = next(f for f in arch["frames"] if f[2] == oracle.blake3(files["a.txt"]))
    broken = bytearray(img); broken[fr[1] + fr[3] // 2] ^= 0xFF
    bad_arc = tmp_path / "broken.zarc"
    bad_arc.write_bytes(bytes(broken))
    for opt in (("--head", "4", "--header"), ()):
        rc1, out, err = cat(*opt, archive=bad_arc)
        errors = sorted(l for l in err if l.startswith("ERROR "))
        assert rc1 == 1 and len(errors) == 2 and errors[0].endswith(" path=src/a.txt") and errors[1].endswith(" path=src/sub/c.txt"), err
        exp = want(rc.head(4) if opt else None, header=bool(opt), skip=("src/a.txt", "src/sub/c.txt"))
        assert out == exp and len(exp) > 100
        assert err[-1].startswith("printed 5 files (4 frames, ") and err[-1].endswith(", 2 failed")


def test_cat_cli_emulated(emu_lib_path, tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "host"])
    binary = os.path.join(ROOT, "tests", "emu", "_build", "zarc")
    run_cat_cases(binary, tmp_path, corpus, oracle, gpus=2, env=dict(os.environ, HIPEMU_DEVICES="2"))


@pytest.mark.gpu
def test_cat_cli_gpu(tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zarc_amd", "csrc"), "host"])
    binary = os.path.join(ROOT, "zarc_amd", "zarc")
    from zarc_amd import _lib
    ndev = _lib.load().zarc_gpu_device_count()
    run_cat_cases(binary, tmp_path, corpus, oracle, gpus=2 if ndev >= 2 else 0, env=None)
