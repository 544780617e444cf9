"""`zarc grep -v / -A / -B / -C` (zarc_amd/host/zarc_cli.cpp), and through it the LineSelect argument of ArchiveReader's and FrameReader's
lines calls on one and on two devices: the lines a search does not match and the lines around a hit, selected on the device, each distinct
frame searched once, nothing written.  Expected output comes from Python over the files' bytes (select_cases.ref_select) in GNU grep's
format; it is also compared with the system's `grep -n` with the same flags where there is one.  What `zarc grep` prints WITHOUT the new
flags is compared with a recording made with the program as it was before it had them (tests/golden/grep_before_select.json: the
invocations of grep_before_regex.json and a few with -E)."""
import json
import os
import re
import shutil
import subprocess

import pytest

import select_cases as zc
from test_regex_cli import run_recorded
from test_set_cli import setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDING = os.path.join(ROOT, "tests", "golden", "grep_before_select.json")


def regex_commands():
    """invocations with -E, which must not change either"""
    return [["-E", "[a-z]+ing "], ["-E", "-n", "^[a-z]{1,5}$"], ["-E", "-c", "-i", "THE [a-z]+"], ["-E", "-b", "-e", "ab+", "-e", "q[a-z]"], ["-E", "-l", "x$"],
            ["-E", "a(b"], ["-E", "-n", "-m", "2", "e.*e"]]


def run_before(grep, files, listfile):
    out = run_recorded(grep, files, listfile)
    for cmd in regex_commands():
        rc, so, err = grep(*cmd)
        out.append([rc, so.decode("latin-1"), next((l for l in err if l.startswith("searched ")), "")])
    return out


def run_select_cases(binary, tmp_path, corpus, gpus, env):
    files, arc, order, grep = setup(binary, tmp_path, corpus, env)
    total = sum(len(d) for d in {v for v in files.values()})

    def want(kind, what, v=False, A=0, B=0, n=False, b=False, m=0, icase=False, only=None, fmt="lines"):
        """-> (stdout, files with a hit line): GNU grep's output over the files in directory order"""
        out, hits, printed = b"", 0, False
        for p in order:
            if only and not re.search(only, p): continue
            d = files[p[4:]]
            nhit, sel, _ = zc.ref_select(d, kind, what, icase, v, B, A)
            if not nhit: continue
            hits += 1
            if fmt == "l": out += p.encode() + b"\n"; continue
            if fmt == "c": out += b"%s:%d\n" % (p.encode(), min(nhit, m) if m else nhit); continue
            seen, stop, last = 0, None, None
            for s, l, no, match in sel:
                if stop is not None and no > stop: break
                hit = stop is None and (match is not None) != v
                if (A or B) and printed and last != no - 1: out += b"--\n"
                sep = b":" if hit else b"-"
                out += p.encode() + sep + (b"%d" % no + sep if n else b"") + (b"%d" % s + sep if b else b"") + d[s:s + min(l, 4096)] + b"\n"
                printed, last = True, no
                if hit and m:
                    seen += 1
                    if seen == m: stop = no + A
        return out, hits

    F, Z, R = zc.FIXED, zc.SET, zc.REGEX
    ok = lambda d, k, n_: all(32 < c < 127 for c in d[k:k + n_]) and not d[k:k + n_].startswith(b"-")
    needle = next(files["a.txt"][k:k + 7] for k in range(5000, 6000) if ok(files["a.txt"], k, 7))
    second = next(files["a.txt"][k:k + 5] for k in range(9000, 10000) if ok(files["a.txt"], k, 5) and files["a.txt"][k:k + 5] not in needle)
    text, text2 = needle.decode(), second.decode()
    nlines = len(zc.all_lines(files["a.txt"]))
    common = next(w for w in re.findall(rb"[a-z]{4,9}", files["a.txt"][:4000]) if 3 < len(zc.lc.ref_lines(files["a.txt"], w)) < nlines // 2)   # a word of some lines
    word = common.decode()
    rx = common[:3] + b"[a-z]* [a-z]+ |" + re.escape(needle)
    txt = ["--filter", r"\.txt$"]

    # ---- -A, -B, -C around the lines of a fixed string; the separators between groups and between files
    exp, hits = want(F, needle, A=2, n=True)
    rc, out, err = grep("-a", "-n", "-A", "2", text)
    assert rc == 0 and out == exp and hits >= 2 and b"--\n" in out and re.search(rb"^src/a\.txt-\d+-", out, re.M) and re.search(rb"^src/a\.txt:\d+:", out, re.M)
    assert err[-1] == "searched 5 files (4 frames, %d bytes), %d match, 0 failed" % (total, hits)
    assert grep("-a", "-n", "-B", "2", text)[:2] == (0, want(F, needle, B=2, n=True)[0])
    assert grep("-a", "-C", "2", text)[:2] == (0, want(F, needle, A=2, B=2)[0])
    assert grep("-a", "-bn", "-C2", text)[:2] == (0, want(F, needle, A=2, B=2, n=True, b=True)[0])
    assert grep("-a", "-B", "1", "-A", "3", "-n", word)[:2] == (0, want(F, common, A=3, B=1, n=True)[0])            # groups that merge
    assert grep("-a", "-n", "-C", "4294967295", text, *txt)[:2] == (0, want(F, needle, A=zc.ALL, B=zc.ALL, n=True, only=r"\.txt$")[0])
    assert grep("-a", "-n", "-C", "99999999999", text, *txt)[1] == grep("-a", "-n", "-C", "4294967295", text, *txt)[1]   # saturates
    # ---- -v, with -n, -c, -l, -i, context
    assert grep("-a", "-v", word)[:2] == (0, want(F, common, v=True)[0]) and want(F, common, v=True)[0].count(b"\n") > 50
    assert grep("-a", "-vn", "-C1", word)[:2] == (0, want(F, common, v=True, A=1, B=1, n=True)[0])
    assert b"-" in re.sub(rb"[^\n]*:\d+:[^\n]*\n", b"", want(F, common, v=True, A=1, B=1, n=True)[0])                 # matching lines as context of inverted hits
    assert grep("-c", "-v", word)[:2] == (0, want(F, common, v=True, fmt="c")[0])
    assert grep("-l", "-v", word)[:2] == (0, want(F, common, v=True, fmt="l")[0])
    assert grep("-a", "-v", "-i", word.upper(), *txt)[:2] == (0, want(F, common.upper(), v=True, icase=True, only=r"\.txt$")[0])
    assert grep("-a", "-v", word, "--filter", r"sub/")[:2] == (0, want(F, common, v=True, only=r"sub/")[0])
    # ---- -m NUM with context: the file stops after its NUM-th hit line, whose trailing context is still printed, as context
    assert grep("-a", "-n", "-m", "2", "-A", "2", "-B", "1", word)[:2] == (0, want(F, common, A=2, B=1, n=True, m=2)[0])
    assert grep("-a", "-n", "-m", "1", "-A", "30", word, *txt)[:2] == (0, want(F, common, A=30, n=True, m=1, only=r"\.txt$")[0])
    tail = want(F, common, A=30, n=True, m=1, only=r"a\.txt$")[0].split(b"\n")[1:-1]
    assert any(common in l.split(b"-", 2)[2] for l in tail) and all(re.match(rb"src/a\.txt-\d+-", l) for l in tail)   # later matches print as context
    assert grep("-a", "-n", "-m", "3", "-v", word)[:2] == (0, want(F, common, v=True, n=True, m=3)[0])
    assert grep("-c", "-m", "2", "-v", word)[:2] == (0, want(F, common, v=True, fmt="c", m=2)[0])
    cut = want(F, common, v=True, A=1, n=True, m=2)[0]                      # a call's records running out between two frames changes nothing
    assert grep("-a", "-vn", "-m", "2", "-A", "1", "--batch-lines", "5", word)[:2] == grep("-a", "-vn", "-m", "2", "-A", "1", word)[:2] == (0, cut) and cut.count(b"\n") > 8
    # ---- a set (-e / -f) and an expression (-E)
    assert grep("-a", "-n", "-C", "1", "-e", text, "-e", text2)[:2] == (0, want(Z, [needle, second], A=1, B=1, n=True)[0])
    listfile = tmp_path / "select_patterns"
    listfile.write_bytes(needle + b"\n" + second + b"\n")
    assert grep("-a", "-v", "-f", str(listfile), *txt)[:2] == (0, want(Z, [needle, second], v=True, only=r"\.txt$")[0])
    assert grep("-a", "-E", "-n", "-A", "1", rx.decode())[:2] == (0, want(R, rx, A=1, n=True)[0]) and want(R, rx, A=1, n=True)[0].count(b"--\n") >= 1
    assert grep("-a", "-E", "-vc", rx.decode())[:2] == (0, want(R, rx, v=True, fmt="c")[0])
    # ---- the same literal as a fixed string, a set of one and an expression
    one = grep("-a", "-vn", "-C", "2", text, *txt)
    assert one[:2] == grep("-a", "-vn", "-C", "2", "-e", text, *txt)[:2] == grep("-a", "-E", "-vn", "-C", "2", re.escape(needle).decode(), *txt)[:2]
    # ---- the system's grep over the files the archive was packed from
    if shutil.which("grep"):
        txts = [p for p in order if p.endswith(".txt")]
        for flags, pat in ((["-A", "2"], text), (["-B", "2"], text), (["-C", "1"], word), (["-v"], word), (["-v", "-C", "1"], word), (["-m", "2", "-A", "2", "-B", "1"], word),
                           (["-E", "-C", "1"], rx.decode())):
            sys_out = subprocess.run(["grep", "-n", "-H", "-a"] + (flags if "-E" in flags else ["-F"] + flags) + ["-e", pat] + txts, cwd=tmp_path, capture_output=True,
                                     timeout=60, env=dict(os.environ, LC_ALL="C")).stdout
            assert grep("-a", "-n", *flags, pat, *txt)[1] == sys_out and sys_out, flags
    # ---- exit statuses and refusals
    assert grep("-v", "x", "--filter", r"empty")[0] == 1 and [p for p in order if "empty" in p]      # an empty file has no line: nothing to invert
    assert grep("-a", "-A", "1", "no such \x7f thing anywhere")[:2] == (1, b"")
    for bad in (["-v", "--tally", text], ["-A", "1", "--tally", "-e", text], ["-C", "2", "--tally", text], ["-o", text], ["-w", text], ["-x", text], ["-A", "x", text],
                ["-C", "-1", text], ["-B"], ["-vo", text]):
        rc, out, err = grep(*bad)
        assert rc == 2 and out == b"" and not any(l.startswith("searched") for l in err), bad
    # ---- two devices: the same
    if gpus > 1:
        for cmd in (["-a", "-vn", "-C1", word], ["-a", "-n", "-m", "2", "-A", "2", "-B", "1", word], ["-a", "-E", "-n", "-A", "1", rx.decode()], ["-c", "-v", "-e", text, "-e", text2]):
            assert grep(*cmd, g=gpus)[:2] == grep(*cmd)[:2], cmd
    # ---- without the new flags: what the program printed before it had them
    assert run_before(grep, files, tmp_path / "recorded_patterns") == json.load(open(RECORDING))


def test_select_cli_emulated(emu_lib_path, tmp_path, corpus):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "host"])
    binary = os.path.join(ROOT, "tests", "emu", "_build", "zarc")
    run_select_cases(binary, tmp_path, corpus, gpus=2, env=dict(os.environ, HIPEMU_DEVICES="2"))


@pytest.mark.gpu
def test_select_cli_gpu(tmp_path, corpus):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zarc_amd", "csrc"), "host"])
    binary = os.path.join(ROOT, "zarc_amd", "zarc")
    from zarc_amd import _lib
    ndev = _lib.load().zarc_gpu_device_count()
    run_select_cases(binary, tmp_path, corpus, gpus=2 if ndev >= 2 else 0, env=None)
