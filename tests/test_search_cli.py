"""`zarc grep` (zarc_amd/host/zarc_cli.cpp), and through it ArchiveReader::search_frames and FrameReader::search_content_frames on one and
on two devices: which files of an archive contain a byte string, each distinct frame searched once, nothing written.  Expected counts and
offsets come from Python's `re` over the files' bytes (search_cases.ref)."""
import os
import re
import subprocess

import pytest

import search_cases as sc
from test_cli import make_tree
from test_container import parse_archive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC = bytes.fromhex("28B52FFD")


def run_grep_cases(binary, tmp_path, corpus, oracle, gpus, env):
    files = make_tree(tmp_path, corpus)                      # a.txt == sub/c.txt: 5 files, 4 distinct contents (one of them empty)
    arc = tmp_path / "out.zarc"
    out = subprocess.run([binary, "pack", "--output", str(arc), "src"], cwd=tmp_path, capture_output=True, timeout=900, check=True, env=env)
    digest = re.fullmatch(rb"digest: ([A-Za-z0-9+/]{43}=)\n", out.stdout).group(1).decode()
    img = arc.read_bytes()
    listed = subprocess.run([binary, "list-files", "--only-files", str(arc)], capture_output=True, timeout=600, check=True, env=env).stdout.decode().split("\n")
    order = [p for p in listed if p[4:] in files]            # directory order of the normal files ("src/" + name)
    assert sorted(order) == sorted("src/" + k for k in files)
    empty = tmp_path / "nothing_here"
    empty.mkdir()

    def grep(*args, g=0, archive=arc):
        cmd = [binary, "grep"] + list(args) + (["--gpus", str(g)] if g else []) + [str(archive)]
        r = subprocess.run(cmd, cwd=empty, capture_output=True, timeout=900, env=env)
        assert os.listdir(empty) == []                       # it creates nothing
        return r.returncode, r.stdout.decode("latin-1").splitlines(), r.stderr.decode("latin-1").splitlines()

    def want(needle, icase=False, fmt="c", only=None):
        lines = []
        for p in order:
            if only and not re.search(only, p): continue
            count, first = sc.ref(files[p[4:]], needle, icase)
            if count: lines.append(p if fmt == "l" else ("%s:%d" % (p, count) if fmt == "c" else "%s:%d:%d" % (p, count, first)))
        return lines

    total = sum(len(d) for d in {v for v in files.values()})
    needle = files["a.txt"][5000:5007]
    text = needle.decode("latin-1")
    assert b"\x00" not in needle and not needle.startswith(b"-")
    rc, lines, err = grep(text)
    assert rc == 0 and lines == want(needle) and len(lines) >= 2 and lines[0].startswith("src/a.txt:") and any(l.startswith("src/sub/c.txt:") for l in lines)
    assert err == ["digest: %s" % digest, "searched 5 files (4 frames, %d bytes), %d match, 0 failed" % (total, len(lines))]   # 4 frames: the shared one once
    assert grep("-F", text, "--verify", digest) == (0, lines, err[1:])
    rc, lines, err = grep("no such \x7f thing anywhere")
    assert rc == 1 and lines == [] and err[-1] == "searched 5 files (4 frames, %d bytes), 0 match, 0 failed" % total
    assert grep("-l", text)[:2] == (0, want(needle, fmt="l"))
    assert grep("-b", text)[:2] == (0, want(needle, fmt="b"))
    assert grep("-lb", text)[:2] == (0, want(needle, fmt="l"))
    swapped = needle.swapcase()
    assert swapped != needle
    assert grep(swapped.decode("latin-1"))[:2] == (0 if want(swapped) else 1, want(swapped))
    assert grep("-i", swapped.decode("latin-1"))[:2] == (0, want(swapped, icase=True)) and want(swapped, icase=True) != want(swapped)
    hexneedle = files["b.bin"][33333:33338]                  # incompressible bytes a shell could not pass
    rc, lines, _ = grep("--hex", hexneedle.hex())
    assert rc == 0 and lines == want(hexneedle) and lines[0].startswith("src/b.bin:")
    assert grep("--hex", "-b", hexneedle.hex().upper())[:2] == (0, want(hexneedle, fmt="b"))
    rc, lines, err = grep(text, "--filter", r"sub/")
    assert rc == 0 and lines == want(needle, only=r"sub/") and len(lines) == len(want(needle)) - 1
    assert err[-1].startswith("searched 2 files (2 frames, 312000 bytes), ")
    assert grep(text, "--filter", r"b\.bin$")[0] == 1
    # usage errors: exit status 2, nothing searched
    for bad in ([""], ["x" * 257], ["--hex", "abc"], ["--hex", "zz"], ["--hex", ""], ["-q", text], [text, "--gpus", "0"]):
        rc, lines, err = grep(*bad)
        assert rc == 2 and lines == [] and not any(l.startswith("searched") for l in err), bad
    assert subprocess.run([binary, "grep", text], capture_output=True, timeout=600, env=env).returncode == 2      # no archive
    assert grep("x" * 256)[0] == 1
    rc, lines, err = grep(text, "--verify", "A" * 43 + "=")
    assert rc == 2 and lines == [] and len(err) == 1 and "integrity failure" in err[0]      # and nothing was searched

    # one byte flipped in the middle of the frame that a.txt and sub/c.txt share: both files fail, the others are still reported
    def dec(frame, raw_len):
        st, o, _ = oracle.zstd_decode(frame, raw_len)
        assert st == 0
        return o
    a = parse_archive(img, dec, oracle.blake3)
    fr = next(f for f in a["frames"] if f[2] == oracle.blake3(files["a.txt"]))
    assert img[fr[1]:fr[1] + 4] == MAGIC
    broken = bytearray(img); broken[fr[1] + fr[3] // 2] ^= 0xFF
    bad_arc = tmp_path / "broken.zarc"
    bad_arc.write_bytes(bytes(broken))
    rec = files["sub/deep/d.rec"][150000:150006]
    results = {}
    for g in ([0, gpus] if gpus > 1 else [0]):
        rc, lines, err = grep("--hex", rec.hex(), g=g, archive=bad_arc)
        errors = sorted(l for l in err if l.startswith("ERROR "))
        assert rc == 2 and len(errors) == 2 and errors[0].endswith(" path=src/a.txt") and errors[1].endswith(" path=src/sub/c.txt"), err
        others = [l for l in want(rec) if not l.startswith(("src/a.txt:", "src/sub/c.txt:"))]
        assert lines == others and any(l.startswith("src/sub/deep/d.rec:") for l in lines)
        assert err[-1] == "searched 5 files (4 frames, %d bytes), %d match, 2 failed" % (total, len(lines))
        results[g] = (rc, tuple(lines), tuple(sorted(err)))
        results["good", g] = grep("-b", text, g=g)
        assert results["good", g][:2] == (0, want(needle, fmt="b"))
    assert len({v for k, v in results.items() if not isinstance(k, tuple)}) == 1      # --gpus 2: the same lines and exit status
    assert len({(v[0], tuple(v[1]), tuple(sorted(v[2]))) for k, v in results.items() if isinstance(k, tuple)}) == 1


def test_search_cli_emulated(emu_lib_path, tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "host"])
    binary = os.path.join(ROOT, "tests", "emu", "_build", "zarc")
    run_grep_cases(binary, tmp_path, corpus, oracle, gpus=2, env=dict(os.environ, HIPEMU_DEVICES="2"))


@pytest.mark.gpu
def test_search_cli_gpu(tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zarc_amd", "csrc"), "host"])
    binary = os.path.join(ROOT, "zarc_amd", "zarc")
    from zarc_amd import _lib
    ndev = _lib.load().zarc_gpu_device_count()
    run_grep_cases(binary, tmp_path, corpus, oracle, gpus=2 if ndev >= 2 else 0, env=None)
