"""`zarc grep -E` (zarc_amd/host/zarc_cli.cpp), and through it ArchiveReader::search_regex / search_regex_lines and the regex calls of
FrameReader on one and on two devices: a regular expression matched on the device line by line, each distinct frame once, nothing written.
Expected counts, offsets and lines come from Python's `re` over the files' bytes (regex_cases.positions); the lines are also compared with the
system's `grep -n -E` where there is one.  What `zarc grep` prints WITHOUT -E is compared with a recording made with the program as it was
before it had the flag (tests/golden/grep_before_regex.json: the invocations of grep_before_sets.json and a few with -e / -f / --tally)."""
import json
import os
import re
import shutil
import subprocess

import pytest

import regex_cases as zr
import set_cases as zs
from test_set_cli import run_old, setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDING = os.path.join(ROOT, "tests", "golden", "grep_before_regex.json")


def set_commands(files, listfile):
    """invocations with the flags of the set search, which must not change either"""
    a = files["a.txt"][5000:5007].decode("latin-1")
    b = files["a.txt"][9000:9005].decode("latin-1")
    listfile.write_bytes(files["a.txt"][5000:5007] + b"\n" + files["sub/deep/d.rec"][150000:150006].hex().encode() + b"\n")
    return [["-e", a, "-e", b], ["-b", "-e", a, "-e", b], ["-n", "-e", a, "-e", b], ["--tally", "-e", a, "-e", "no such thing", "-e", b], ["-f", str(listfile)],
            ["-c", "-i", "-e", a.swapcase()], ["-e", ""], ["--tally"], ["-l", "-e", "(a|b)+"], ["a.*b"], ["-n", "^e"]]


def run_recorded(grep, files, listfile):
    out = run_old(grep, files)
    for cmd in set_commands(files, listfile):
        rc, so, err = grep(*cmd)
        out.append([rc, so.decode("latin-1"), next((l for l in err if l.startswith("searched ")), "")])
    return out


def run_regex_cases(binary, tmp_path, corpus, gpus, env):
    files, arc, order, grep = setup(binary, tmp_path, corpus, env)
    total = sum(len(d) for d in {v for v in files.values()})

    def want(rx, icase=False, fmt="c", only=None):
        lines = []
        for p in order:
            if only and not re.search(only, p): continue
            count, first = zr.ref(files[p[4:]], rx, icase)
            if count: lines.append(p if fmt == "l" else ("%s:%d" % (p, count) if fmt == "c" else "%s:%d:%d" % (p, count, first)))
        return "".join(l + "\n" for l in lines).encode()

    def want_lines(rx, icase=False, n=False, only=None, count=False):
        out = b""
        for p in order:
            if only and not re.search(only, p): continue
            d = files[p[4:]]
            recs = zs.ref_lines(d, zr.positions(d, rx, icase))
            if count:
                if recs: out += b"%s:%d\n" % (p.encode(), len(recs))
                continue
            for s, l, no, _ in recs:
                out += p.encode() + b":" + (b"%d:" % no if n else b"") + d[s:s + l] + b"\n"
        return out

    words = re.findall(rb"[a-z]{4,9}", files["a.txt"][:4000])
    w1 = words[10]
    A = w1[:3] + b"[a-z]* [a-z]+ "                                           # a word that begins like w1, and the word behind it
    line = next(l for l in files["a.txt"].split(b"\n")[2:] if re.match(rb"[a-z]{3,} ", l) and re.search(rb" [a-z]{3,}$", l))
    B = b"^" + re.match(rb"[a-z]+", line).group() + b" .* " + re.search(rb"[a-z]+$", line).group() + b"$|^[a-z]{1,5}$"   # anchored on both sides
    tA, tB = A.decode(), B.decode()
    # ---- -E alone, with -i, -b, -l, --filter
    rc, out, err = grep("-E", tA)
    assert rc == 0 and out == want(A) and out.count(b"\n") >= 2
    assert err[-1] == "searched 5 files (4 frames, %d bytes), %d match, 0 failed" % (total, out.count(b"\n"))   # 4 frames: the shared one once
    assert grep("--extended-regexp", tA)[:2] == (0, out) and grep("-bE", tA)[:2] == (0, want(A, fmt="b")) and grep("-E", "-l", tA)[:2] == (0, want(A, fmt="l"))
    assert grep("-E", tA, "--filter", r"sub/")[:2] == (0, want(A, only=r"sub/"))
    up = A.upper().replace(b"[A-Z]", b"[a-z]")
    assert want(up) == b"" and grep("-E", up.decode())[:2] == (1, b"") and grep("-E", "-i", up.decode())[:2] == (0, want(up, icase=True)) and want(up, icase=True) == want(A, icase=True)
    # ---- lines mode: --lines -n, -c, -l, -m, -a; Python's reference and the system's grep over the files the archive was packed from
    rc, out, err = grep("-E", "--lines", "-n", tA, "--filter", r"\.txt$")
    assert rc == 0 and out == want_lines(A, n=True, only=r"\.txt$") and out.count(b"\n") >= 4
    if shutil.which("grep"):
        for rx in (tA, tB):
            sys_out = b""
            for p in order:
                if p.endswith(".txt"):
                    sys_out += subprocess.run(["grep", "-n", "-E", "-H", "-a", "-e", rx, p], cwd=tmp_path, capture_output=True, timeout=60, env=dict(os.environ, LC_ALL="C")).stdout
            assert grep("-E", "-n", rx, "--filter", r"\.txt$")[1] == sys_out, rx
    assert grep("-E", "-n", tB)[:2] == (0, want_lines(B, n=True)) and want_lines(B) != b""
    assert grep("-E", "-c", tA)[:2] == (0, want_lines(A, count=True)) and grep("-E", "-c", "-l", tA)[:2] == (0, want(A, fmt="l"))
    assert grep("-E", "-a", "--lines", tA)[:2] == (0, want_lines(A))
    assert grep("-E", "-n", "-m", "2", "--batch-lines", "3", tA)[1] == grep("-E", "-n", "-m", "2", tA)[1] != b""
    assert grep("-E", "-n", "--max-line", "10", tA)[1] == b"".join(l.split(b":", 2)[0] + b":" + l.split(b":", 2)[1] + b":" + l.split(b":", 2)[2][:10] + b"\n"
                                                                  for l in want_lines(A, n=True).split(b"\n")[:-1])
    # ---- several expressions are one alternation
    both = ("(%s)|(%s)" % (tA, tB)).encode()
    for mode in ([], ["-b"], ["--lines", "-n"], ["-c"], ["-l"]):
        assert grep("-E", *mode, "-e", tA, "-e", tB)[:2] == grep("-E", *mode, both.decode())[:2], mode
    assert grep("-E", "-e", tA, "-e", tB)[:2] == (0, want(both)) and grep("-E", "-n", "-e", tA, "-e", tB)[1] == want_lines(both, n=True)
    assert grep("-E", "-e", tA)[:2] == grep("-E", tA)[:2]
    listfile = tmp_path / "expressions"
    listfile.write_bytes(A + b"\n" + B + b"\n")
    assert grep("-E", "-f", str(listfile))[:2] == (0, want(both)) and grep("-E", "-n", "-f", str(listfile), "-e", "zzzz9")[1] == want_lines(both, n=True)
    # ---- exit statuses and refusals: a bad expression is refused before the archive is looked at
    assert grep("-E", "no such thing 7+")[:2] == (1, b"")
    missing = tmp_path / "no such archive"
    for bad, text in ((["-E", "a(b"], "offset 1: unbalanced ("), (["-E", "a**"], "offset 2:"), (["-E", ".{7}a"], "needs 256 states"), (["-E", "x*"], "without consuming"),
                      (["-E", "a\\b"], "offset 1:"), (["-E", "-e", "ab", "-e", "c)"], "unbalanced"), (["-E", "-n", "a\nb"], "line feed"), (["-E", ""], "empty expression"),
                      (["-E", "x" * 1025], "at most 1024")):
        for archive in (arc, missing):
            rc, out, err = grep(*bad, archive=archive)
            assert rc == 2 and out == b"" and any(text in l for l in err) and not any(l.startswith("searched") for l in err), (bad, err)
            assert not any("No such file" in l or "cannot" in l for l in err), err
    assert grep("-E", "ab", archive=missing)[0] == 2                        # ... a good one then meets the missing file
    listfile.write_bytes(A + b"\n\n")
    for bad in (["--hex", "-E", "6162"], ["--tally", "-E", "ab"], ["--tally", "-E", "-e", "ab"], ["-E", "-f", str(listfile)], ["-E", "-e", tA, "one argument too many"], ["-E"]):
        rc, out, err = grep(*bad)
        assert rc == 2 and out == b"" and not any(l.startswith("searched") for l in err), bad
    # ---- two devices: the same
    if gpus > 1:
        for cmd in (["-E", "-b", tA], ["-E", "-n", "-e", tA, "-e", tB], ["-E", "-c", tB]):
            assert grep(*cmd, g=gpus)[:2] == grep(*cmd)[:2], cmd
    # ---- without -E: what the program printed before it had the flag
    assert run_recorded(grep, files, tmp_path / "recorded_patterns") == json.load(open(RECORDING))


def test_regex_cli_emulated(emu_lib_path, tmp_path, corpus):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "host"])
    binary = os.path.join(ROOT, "tests", "emu", "_build", "zarc")
    run_regex_cases(binary, tmp_path, corpus, gpus=2, env=dict(os.environ, HIPEMU_DEVICES="2"))


@pytest.mark.gpu
def test_regex_cli_gpu(tmp_path, corpus):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zarc_amd", "csrc"), "host"])
    binary = os.path.join(ROOT, "zarc_amd", "zarc")
    from zarc_amd import _lib
    ndev = _lib.load().zarc_gpu_device_count()
    run_regex_cases(binary, tmp_path, corpus, gpus=2 if ndev >= 2 else 0, env=None)
