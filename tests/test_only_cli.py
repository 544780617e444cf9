"""`zarc grep --only-matching` (grep's -o; zarc_amd/host/zarc_cli.cpp), and through it ArchiveReader::search_matches and FrameReader::matches_content_frames on one
and on two devices: every match of a matching line, cut out on the device, each distinct frame searched once, nothing written.  Expected
output comes from Python over the files' bytes (only_cases.ref_frame) in GNU grep's format; it is also compared with the system's
`grep -o -n -b -H -a` where there is one.  What `zarc grep` prints WITHOUT the flag is compared with a recording made with the program as it was
before it had the flag (tests/golden/grep_before_only.json: the invocations of grep_before_select.json)."""
import json
import os
import re
import shutil
import subprocess

import pytest

import only_cases as oc
from test_select_cli import run_before
from test_set_cli import setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDING = os.path.join(ROOT, "tests", "golden", "grep_before_only.json")


O = "--only-matching"   # grep's -o; `zarc grep` takes the long form only: `-o PATTERN` was a usage error before this flag existed and stays one


def run_only_cases(binary, tmp_path, corpus, gpus, env):
    files, arc, order, grep = setup(binary, tmp_path, corpus, env)
    total = sum(len(d) for d in {v for v in files.values()})
    word_ends = lambda line, s: range(min(len(line), s + 40), s, -1)     # the expressions below match inside one word, and no word has 40 bytes

    def want(kind, what, n=False, b=False, m=0, icase=False, only=None, max_line=4096):
        """-> (stdout, files with a match, matches): GNU grep -o's output over the files in directory order"""
        out, hits, total_matches = b"", 0, 0
        for p in order:
            if only and not re.search(only, p): continue
            d = files[p[4:]]
            lines = oc.ref_frame(d, kind, what, icase, **(dict(ends=word_ends) if kind == oc.REGEX else {}))
            if not lines: continue
            hits += 1
            for _, _, no, ms in lines[:m or len(lines)]:
                for s, l, _ in ms:
                    out += p.encode() + b":" + (b"%d:" % no if n else b"") + (b"%d:" % s if b else b"") + d[s:s + min(l, max_line)] + b"\n"
                    total_matches += 1
        return out, hits, total_matches

    F, Z, R = oc.FIXED, oc.SET, oc.REGEX
    ok = lambda d, k, n_: all(32 < c < 127 for c in d[k:k + n_]) and not d[k:k + n_].startswith(b"-")
    needle = next(files["a.txt"][k:k + 7] for k in range(5000, 6000) if ok(files["a.txt"], k, 7))
    second = next(files["a.txt"][k:k + 5] for k in range(9000, 10000) if ok(files["a.txt"], k, 5) and files["a.txt"][k:k + 5] not in needle)
    text, text2 = needle.decode(), second.decode()
    assert max(len(w) for w in re.findall(rb"[a-z]+", files["a.txt"])) < 40
    common = next(w for w in re.findall(rb"[a-z]{4,9}", files["a.txt"][:4000]) if len(oc.lc.ref_lines(files["a.txt"], w)) > 3)   # a word of several lines
    word = common.decode()
    rx = common[:2] + b"[a-z]*|" + re.escape(needle) + b"|[a-z]+" + common[-2:] + b"$"
    txt = ["--filter", r"\.txt$"]

    # ---- one fixed string: -o alone, with -n, -b, both; -b is the match's own offset
    exp, hits, nm = want(F, common)
    rc, out, err = grep("-a", O, word)
    assert rc == 0 and out == exp and hits >= 2 and nm > hits and out.count(b"\n") == nm
    assert err[-1] == "searched 5 files (4 frames, %d bytes), %d match, 0 failed" % (total, hits)
    assert grep("-a", O, "-n", word)[:2] == (0, want(F, common, n=True)[0])
    assert grep("-a", O, "-bn", word)[:2] == (0, want(F, common, n=True, b=True)[0])
    assert grep("-a", O, "-i", word.upper(), *txt)[:2] == (0, want(F, common.upper(), icase=True, only=r"\.txt$")[0])
    # ---- -m NUM counts lines; -c and -l ignore -o
    two = want(F, common, n=True, m=2)
    assert grep("-a", O, "-n", "-m", "2", word)[:2] == (0, two[0]) and two[0].count(b"\n") >= 2 * two[1]
    assert grep(O, "-l", word) == grep("-l", word) and grep(O, "-c", "-m", "2", word) == grep("-c", "-m", "2", word)
    # ---- a set (-e / -f) and an expression (-E): the longest at the leftmost position, then on from its end
    assert grep("-a", O, "-nb", "-e", text, "-e", text2, "-e", word, "-e", word[:2])[:2] == (0, want(Z, [needle, second, common, common[:2]], n=True, b=True)[0])
    listfile = tmp_path / "only_patterns"
    listfile.write_bytes(needle + b"\n" + second + b"\n")
    assert grep("-a", O, "-f", str(listfile), *txt)[:2] == (0, want(Z, [needle, second], only=r"\.txt$")[0])
    exp = want(R, rx, n=True, b=True)
    assert grep("-a", "-E", O, "-nb", rx.decode())[:2] == (0, exp[0]) and exp[2] > exp[1] and len({l.split(b":", 3)[3] for l in exp[0].split(b"\n")[:-1]}) > 3
    assert grep("-a", "-E", O, "-i", rx.decode().upper().replace("[A-Z]", "[a-z]"))[1] == want(R, rx.upper().replace(b"[A-Z]", b"[a-z]"), icase=True)[0]
    # ---- the same literal as a fixed string, a set of one and an expression
    assert grep("-a", O, "-nb", text)[:2] == grep("-a", O, "-nb", "-e", text)[:2] == grep("-a", "-E", O, "-nb", re.escape(needle).decode())[:2] == (0, want(F, needle, n=True, b=True)[0])
    # ---- --max-line cuts a match and says so; --batch-lines bounds a call and changes nothing
    rc, out, err = grep("-a", O, "--max-line", "3", word)
    assert (rc, out) == (0, want(F, common, max_line=3)[0]) and len(common) > 3 and any(l.startswith("WARN match cut") for l in err)
    full = grep("-a", O, "-nb", word)[:2]
    per = [sum(len(ms) for _, _, _, ms in oc.ref_frame(d, F, b"e")[:2]) for d in {v for v in files.values()}]          # matches of every distinct frame under -m 2
    fits = str(max(per))                                                   # every frame fits a call of its own, all of them do not: frames are searched again
    assert sum(per) > max(per) >= 2 and sum(1 for x in per if x) >= 3 and grep("-a", O, "-nb", "--batch-lines", fits, "-m", "2", "e")[:2] == grep("-a", O, "-nb", "-m", "2", "e")[:2]
    rc, out, err = grep("-a", O, "-nb", "--batch-lines", "3", word)          # a frame that is first in its call and has more than fit says so
    assert rc == 0 and out and set(out.split(b"\n")) < set(full[1].split(b"\n")) and any("not shown" in l for l in err)
    # ---- the binary-file rule looks at the delivered matches
    assert oc.ref_frame(files["b.bin"], R, rb"\0[^\0]") and not oc.ref_frame(files["a.txt"], R, rb"\0[^\0]")
    rc, out, err = grep("-E", O, r"\0[^\0]", "--filter", r"b\.bin$")
    assert (rc, out) == (0, b"Binary file src/b.bin matches\n")
    assert grep("-a", "-E", O, "-b", "-m", "3", r"\0[^\0]", "--filter", r"b\.bin$")[:2] == (0, want(R, rb"\0[^\0]", b=True, m=3, only=r"b\.bin$")[0])
    # ---- the system's grep over the files the archive was packed from
    if shutil.which("grep"):
        txts = [p for p in order if p.endswith(".txt")]
        for flags, pats in ((["-F"], [word]), (["-F", "-m", "2"], [word]), (["-F"], [text, text2, word[:2]]), (["-E"], [rx.decode()]), (["-F", "-i"], [word.upper()])):
            sys_out = subprocess.run(["grep", "-o", "-n", "-b", "-H", "-a"] + flags + [x for p in pats for x in ("-e", p)] + txts, cwd=tmp_path, capture_output=True,
                                     timeout=60, env=dict(os.environ, LC_ALL="C")).stdout
            ours = [f for f in flags if f != "-F"] + ([x for p in pats for x in ("-e", p)] if len(pats) > 1 else pats)
            assert grep("-a", O, "-nb", *ours, *txt)[1] == sys_out and sys_out, flags
    # ---- exit statuses and refusals
    assert grep("-a", O, "no such \x7f thing anywhere")[:2] == (1, b"") and grep(O, "x", "--filter", r"empty")[0] == 1
    for bad in ([O, "-v", text], [O, "-A", "1", text], [O, "-B1", text], [O, "-C", "2", text], [O, "--tally", text], [O, "--tally", "-e", text],
                ["-v", O, text], ["-o", text], ["-on", text], ["-vo", text], ["-ow", text]):                  # (the short form stays the usage error it was)
        rc, out, err = grep(*bad)
        assert rc == 2 and out == b"" and not any(l.startswith("searched") for l in err), bad
    # an expression -E takes and -o cannot: refused before the archive is opened, with the states it needs
    assert grep("-E", "-c", "(a|b)*a(a|b){6}")[0] in (0, 1)
    rc, out, err = grep("-E", O, "(a|b)*a(a|b){6}", archive=tmp_path / "no such archive")
    assert rc == 2 and out == b"" and len(err) == 1 and O in err[0] and "needs 129 states" in err[0]
    # ---- two devices: the same
    if gpus > 1:
        for cmd in (["-a", O, "-nb", word], ["-a", O, "-n", "-m", "2", word], ["-a", "-E", O, "-nb", rx.decode()], ["-a", O, "-b", "-e", text, "-e", text2],
                    ["-a", O, "-nb", "--batch-lines", fits, "-m", "2", "e"]):
            assert grep(*cmd, g=gpus)[:2] == grep(*cmd)[:2], cmd
    # ---- without the new flag: what the program printed before it had it
    assert run_before(grep, files, tmp_path / "recorded_patterns") == json.load(open(RECORDING))


def test_only_cli_emulated(emu_lib_path, tmp_path, corpus):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "host"])
    binary = os.path.join(ROOT, "tests", "emu", "_build", "zarc")
    run_only_cases(binary, tmp_path, corpus, gpus=2, env=dict(os.environ, HIPEMU_DEVICES="2"))


@pytest.mark.gpu
def test_only_cli_gpu(tmp_path, corpus):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zarc_amd", "csrc"), "host"])
    binary = os.path.join(ROOT, "zarc_amd", "zarc")
    from zarc_amd import _lib
    ndev = _lib.load().zarc_gpu_device_count()
    run_only_cases(binary, tmp_path, corpus, gpus=2 if ndev >= 2 else 0, env=None)
