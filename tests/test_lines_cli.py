"""`zarc grep` in lines mode (zarc_amd/host/zarc_cli.cpp), and through it ArchiveReader::search_lines and FrameReader::lines_content_frames on
one and on two devices: the matching lines of the files of an archive, each distinct frame searched once, nothing written.  Expected
output comes from Python over the files' bytes (lines_cases.ref_lines), in directory order."""
import os
import re
import subprocess

import pytest

import lines_cases as lc
import search_cases as sc
from test_cli import make_tree
from test_container import parse_archive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_lines_cases(binary, tmp_path, corpus, oracle, gpus, env):
    files = make_tree(tmp_path, corpus)                      # a.txt == sub/c.txt: 5 files, 4 distinct contents (one of them empty)
    arc = tmp_path / "out.zarc"
    subprocess.run([binary, "pack", "--output", str(arc), "src"], cwd=tmp_path, capture_output=True, timeout=900, check=True, env=env)
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
        return r.returncode, r.stdout, r.stderr.decode("latin-1").splitlines()

    def want(needle, icase=False, n=False, b=False, m=0, max_line=4096, only=None, a=False, fmt="lines"):
        out, warn, hits = b"", [], 0
        for p in order:
            if only and not re.search(only, p): continue
            d = files[p[4:]]
            ls = lc.ref_lines(d, needle, icase)
            if not ls: continue
            hits += 1
            shown = ls[:m] if m else ls
            texts = [d[s:s + min(l, max_line)] for s, l, _, _ in shown]
            if fmt == "l": out += p.encode() + b"\n"
            elif fmt == "c": out += b"%s:%d\n" % (p.encode(), len(shown))
            elif not a and any(b"\x00" in t for t in texts): out += b"Binary file %s matches\n" % p.encode()
            else:
                for (s, l, no, _), t in zip(shown, texts):
                    out += p.encode() + b":" + (b"%d:" % no if n else b"") + (b"%d:" % s if b else b"") + t + b"\n"
                    if l > max_line: warn.append("WARN line cut path=%s line=%d length=%d" % (p, no, l))
        return out, warn, hits

    total = sum(len(d) for d in {v for v in files.values()})
    at = next(k for k in range(5000, 6000) if b"\n" not in files["a.txt"][k:k + 7] and b"\x00" not in files["a.txt"][k:k + 7])
    needle = files["a.txt"][at:at + 7]
    text = needle.decode("latin-1")
    assert not text.startswith("-")
    rc, out, err = grep("--lines", text)
    exp, _, hits = want(needle)
    assert rc == 0 and out == exp and hits >= 2 and out.count(b"src/a.txt:") >= 1 and out.count(b"src/sub/c.txt:") == out.count(b"src/a.txt:")   # the shared frame: both files
    assert err[-1] == "searched 5 files (4 frames, %d bytes), %d match, 0 failed" % (total, hits)
    assert grep("-n", text)[:2] == (0, want(needle, n=True)[0]) and want(needle, n=True)[0] != exp
    assert grep("-bn", text)[:2] == (0, want(needle, n=True, b=True)[0])
    assert grep("--lines", "-b", text)[:2] == (0, want(needle, b=True)[0])
    assert grep("-c", text)[:2] == (0, want(needle, fmt="c")[0])
    assert grep("-l", "--lines", text)[:2] == (0, want(needle, fmt="l")[0])
    assert grep("--lines", text, "--filter", r"sub/")[:2] == (0, want(needle, only=r"sub/")[0])
    swapped = needle.swapcase()
    assert swapped != needle and want(swapped, icase=True)[0] != want(swapped)[0]
    assert grep("-in", swapped.decode("latin-1"))[:2] == (0, want(swapped, icase=True, n=True)[0])
    # a needle of many lines: -m, -c with -m, and the records of a call running out (--batch-lines) change nothing on stdout
    common = next(bytes([c]) for c in b"aeiost" if len(lc.ref_lines(files["a.txt"], bytes([c]))) > 3 and len(lc.ref_lines(files["sub/deep/d.rec"], bytes([c]))) > 3)
    word = common.decode()
    assert grep("-m", "1", "-n", word)[:2] == (0, want(common, n=True, m=1)[0])
    assert grep("-m", "2", "-c", word)[:2] == (0, want(common, m=2, fmt="c")[0])
    full = grep("-n", "-m", "2", word)
    assert full[:2] == (0, want(common, n=True, m=2)[0]) and full[1].count(b"\n") > 3
    assert grep("-n", "-m", "2", "--batch-lines", "3", word)[:2] == full[:2]
    assert grep("-n", "-a", "--batch-lines", "3", "-m", "3", word)[:2] == (0, want(common, n=True, m=3, a=True)[0])
    rc, out, err = grep("--lines", "--batch-lines", "2", "--filter", r"a\.txt$", word)     # first in its call and still too many: said, not dropped silently
    lines_a = lc.ref_lines(files["a.txt"], common)
    assert rc == 0 and out == b"".join(b"src/a.txt:" + files["a.txt"][s:s + l] + b"\n" for s, l, _, _ in lines_a[:2])
    assert "WARN path=src/a.txt: %d more matching lines not shown" % (len(lines_a) - 2) in err
    # --max-line: the first bytes and a warning per cut line
    rc, out, err = grep("-n", "--max-line", "8", text)
    exp8, warn8, _ = want(needle, n=True, max_line=8)
    assert rc == 0 and out == exp8 and warn8 and [l for l in err if l.startswith("WARN line cut")] == warn8
    # binary content: a needle inside a line of b.bin that holds a NUL byte
    bb = files["b.bin"]
    s, l = next((s, l) for s, l in ((m.start(), len(m.group())) for m in re.finditer(rb"[^\n]+", bb)) if b"\x00" in bb[s:s + l] and l >= 8 and s > 100)
    k = next(k for k in range(s, s + l - 4) if b"\x00" not in bb[k:k + 5])
    hexneedle = bb[k:k + 5]
    rc, out, _ = grep("--lines", "--hex", hexneedle.hex())
    assert rc == 0 and out == want(hexneedle)[0] and b"Binary file src/b.bin matches\n" in out
    rc, out, _ = grep("-a", "-n", "--hex", hexneedle.hex())
    assert rc == 0 and out == want(hexneedle, n=True, a=True)[0] and b"Binary file" not in out and bb[s:s + l] in out
    # errors: a newline in the pattern, values out of range; -q stays a usage error; no match is exit status 1
    for bad in (["--lines", "--hex", "610a62"], ["-n", "a\nb"], ["--max-line", "0", text], ["--max-line", "65537", text], ["--batch-lines", "0", text], ["-m", "0", text],
                ["-q", "--lines", text]):
        rc, out, err = grep(*bad)
        assert rc == 2 and out == b"" and not any(l.startswith("searched") for l in err), bad
    rc, out, err = grep("--lines", "no such \x7f thing anywhere")
    assert rc == 1 and out == b"" and err[-1] == "searched 5 files (4 frames, %d bytes), 0 match, 0 failed" % total
    # without the new flags: exactly the old output
    rc, out, err = grep(text)
    old = ["%s:%d" % (p, sc.ref(files[p[4:]], needle)[0]) for p in order if sc.ref(files[p[4:]], needle)[0]]
    assert rc == 0 and out.decode().splitlines() == old

    # one byte flipped in the middle of the frame that a.txt and sub/c.txt share: both files fail, the others' lines are still printed
    def dec(frame, raw_len):
        st, o, _ = oracle.zstd_decode(frame, raw_len)
        assert st == 0
        return o
    arch = parse_archive(img, dec, oracle.blake3)
    fr = next(f for f in arch["frames"] if f[2] == oracle.blake3(files["a.txt"]))
    broken = bytearray(img); broken[fr[1] + fr[3] // 2] ^= 0xFF
    bad_arc = tmp_path / "broken.zarc"
    bad_arc.write_bytes(bytes(broken))
    results = {}
    for g in ([0, gpus] if gpus > 1 else [0]):
        rc, out, err = grep("-an", "-m", "4", word, g=g, archive=bad_arc)
        errors = sorted(l for l in err if l.startswith("ERROR "))
        assert rc == 2 and len(errors) == 2 and errors[0].endswith(" path=src/a.txt") and errors[1].endswith(" path=src/sub/c.txt"), err
        exp, _, hits = want(common, n=True, m=4, a=True, only=r"^(?!src/a\.txt$|src/sub/c\.txt$)")
        assert out == exp and b"src/sub/deep/d.rec:" in out
        assert err[-1] == "searched 5 files (4 frames, %d bytes), %d match, 2 failed" % (total, hits)
        results[g] = (rc, out, tuple(sorted(err)))
        results["good", g] = grep("-bn", text, g=g)[:2]
        assert results["good", g] == (0, want(needle, n=True, b=True)[0])
        results["many", g] = grep("-n", "-m", "2", "--batch-lines", "3", word, g=g)[:2]
        assert results["many", g] == full[:2]
    assert len({v for k, v in results.items() if not isinstance(k, tuple)}) == 1      # --gpus 2: the same output and exit status


def test_lines_cli_emulated(emu_lib_path, tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "host"])
    binary = os.path.join(ROOT, "tests", "emu", "_build", "zarc")
    run_lines_cases(binary, tmp_path, corpus, oracle, gpus=2, env=dict(os.environ, HIPEMU_DEVICES="2"))


@pytest.mark.gpu
def test_lines_cli_gpu(tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zarc_amd", "csrc"), "host"])
    binary = os.path.join(ROOT, "zarc_amd", "zarc")
    from zarc_amd import _lib
    ndev = _lib.load().zarc_gpu_device_count()
    run_lines_cases(binary, tmp_path, corpus, oracle, gpus=2 if ndev >= 2 else 0, env=None)
