"""`zarc grep -e / -f / --tally` (zarc_amd/host/zarc_cli.cpp), and through it ArchiveReader::search_set / search_set_lines and the set calls of
FrameReader on one and on two devices: a set of fixed strings searched in one pass, each distinct frame once, nothing written.  Expected
counts, offsets, lines and tallies come from Python's `re` over the files' bytes (set_cases.ref); the lines are also compared with the
system's `grep -n -F -e A -e B` where there is one.  What `zarc grep` prints without the new flags is compared with a recording made
with the program as it was before they existed (tests/golden/grep_before_sets.json)."""
import json
import os
import re
import shutil
import subprocess

import pytest

import set_cases as zs
from test_cli import make_tree
from test_container import parse_archive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDING = os.path.join(ROOT, "tests", "golden", "grep_before_sets.json")


def old_commands(files):
    """the commands of test_search_cli.py's first case (all but the one that passes the archive's digest, which differs from user to user)"""
    needle = files["a.txt"][5000:5007]
    text = needle.decode("latin-1")
    swapped = needle.swapcase().decode("latin-1")
    hexneedle = files["b.bin"][33333:33338].hex()
    return [[text], ["-F", text], ["no such \x7f thing anywhere"], ["-l", text], ["-b", text], ["-lb", text], [swapped], ["-i", swapped], ["--hex", hexneedle],
            ["--hex", "-b", hexneedle.upper()], [text, "--filter", r"sub/"], [text, "--filter", r"b\.bin$"], [""], ["x" * 257], ["--hex", "abc"], ["--hex", "zz"],
            ["--hex", ""], ["-q", text], [text, "--gpus", "0"], ["x" * 256], ["--lines", text], ["-n", "-m", "2", "e"], ["-c", "e"]]


def run_old(grep, files):
    """-> per command [exit status, stdout, the summary line of stderr]"""
    out = []
    for cmd in old_commands(files):
        rc, so, err = grep(*cmd)
        out.append([rc, so.decode("latin-1"), next((l for l in err if l.startswith("searched ")), "")])
    return out


def setup(binary, tmp_path, corpus, env):
    files = make_tree(tmp_path, corpus)                      # a.txt == sub/c.txt: 5 files, 4 distinct contents (one of them empty)
    arc = tmp_path / "out.zarc"
    subprocess.run([binary, "pack", "--output", str(arc), "src"], cwd=tmp_path, capture_output=True, timeout=900, check=True, env=env)
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
    return files, arc, order, grep


def run_set_cases(binary, tmp_path, corpus, oracle, gpus, env):
    files, arc, order, grep = setup(binary, tmp_path, corpus, env)
    total = sum(len(d) for d in {v for v in files.values()})
    ok = lambda d, k, n: all(32 < c < 127 for c in d[k:k + n]) and not d[k:k + n].startswith(b"-")   # what an argument carries as it is
    A = next(files["a.txt"][k:k + 7] for k in range(5000, 6000) if ok(files["a.txt"], k, 7))
    B = next(files["a.txt"][k:k + 5] for k in range(9000, 10000) if ok(files["a.txt"], k, 5) and files["a.txt"][k:k + 5] not in A)
    C = next(files["sub/deep/d.rec"][k:k + 6] for k in range(150000, 300000 - 6) if ok(files["sub/deep/d.rec"], k, 6))
    tA, tB, tC = (x.decode("latin-1") for x in (A, B, C))

    def want(pats, icase=False, fmt="c", only=None):
        lines = []
        for p in order:
            if only and not re.search(only, p): continue
            count, first = zs.ref(files[p[4:]], pats, icase)[:2]
            if count: lines.append(p if fmt == "l" else ("%s:%d" % (p, count) if fmt == "c" else "%s:%d:%d" % (p, count, first)))
        return "".join(l + "\n" for l in lines).encode()

    def want_lines(pats, icase=False, n=False, only=None):
        out = b""
        for p in order:
            if only and not re.search(only, p): continue
            d = files[p[4:]]
            for s, l, no, _ in zs.ref_lines(d, zs.ref(d, pats, icase)[4]):
                out += p.encode() + b":" + (b"%d:" % no if n else b"") + d[s:s + l] + b"\n"
        return out

    # ---- -e, -f, --hex: the union's count per file
    set3 = [A, B, C]
    rc, out, err = grep("-e", tA, "-e", tB, "-e", tC)
    assert rc == 0 and out == want(set3) and out.count(b"\n") >= 3
    assert err[-1] == "searched 5 files (4 frames, %d bytes), %d match, 0 failed" % (total, out.count(b"\n"))   # 4 frames: the shared one once
    listfile = tmp_path / "patterns"
    listfile.write_bytes(A + b"\n" + B + b"\n" + C + b"\n")
    assert grep("-f", str(listfile))[:2] == (0, out)
    listfile.write_bytes(A + b"\n" + B + b"\n" + C)                          # no final LF: the last line is a pattern all the same
    assert grep("-f", str(listfile))[:2] == (0, out)
    assert grep("-e", tA, "-f", str(listfile))[:2] == (0, out)              # the same pattern twice: searched once
    assert grep("--hex", "-e", A.hex(), "-e", B.hex().upper(), "-e", C.hex())[:2] == (0, out)
    assert grep("-b", "-e", tA, "-e", tB, "-e", tC)[:2] == (0, want(set3, fmt="b"))
    assert grep("-l", "-e", tA, "-e", tB, "-e", tC)[:2] == (0, want(set3, fmt="l"))
    assert grep("-e", tA, "-e", tC, "--filter", r"sub/")[:2] == (0, want([A, C], only=r"sub/"))
    crlf = tmp_path / "crlf"
    crlf.write_bytes(A + b"\r\n")                                           # a 0x0D stays part of the pattern
    assert grep("-f", str(crlf))[:2] == (1, want([A + b"\r"])) and want([A + b"\r"]) == b""
    swA = A.swapcase()
    assert swA != A and want([swA, C], icase=True) != want([swA, C])
    assert grep("-i", "-e", swA.decode("latin-1"), "-e", tC)[:2] == (0, want([swA, C], icase=True))
    assert grep("-i", "-e", swA.decode("latin-1"), "-e", tA, "-e", tC)[:2] == (0, want([swA, C], icase=True))   # equal after folding: dropped
    # ---- one -e is the positional pattern, byte for byte, in both modes
    for mode in ([], ["-b"], ["--lines", "-n"], ["-c"], ["-l"]):
        assert grep(*mode, "-e", tA)[:2] == grep(*mode, tA)[:2], mode
    assert grep("-e", tA)[1] == want([A]) and grep("-n", "-e", tA)[1] == want_lines([A], n=True)
    # ---- lines of the union: Python's reference, and the system's grep over the files the archive was packed from
    rc, out, err = grep("--lines", "-n", "-e", tA, "-e", tB, "--filter", r"\.txt$")
    assert rc == 0 and out == want_lines([A, B], n=True, only=r"\.txt$") and out.count(b"\n") >= 4
    if shutil.which("grep"):
        sys_out = b""
        for p in order:
            if p.endswith(".txt"):
                r = subprocess.run(["grep", "-n", "-F", "-H", "-a", "-e", tA, "-e", tB, p], cwd=tmp_path, capture_output=True, timeout=60, env=dict(os.environ, LC_ALL="C"))
                sys_out += r.stdout
        assert out == sys_out
    assert grep("--lines", "-e", tA, "-e", tB, "-e", tC, "-a")[:2] == (0, want_lines(set3))
    assert grep("-c", "-e", tA, "-e", tB)[1] == b"".join(b"%s:%d\n" % (p.encode(), len(zs.ref_lines(files[p[4:]], zs.ref(files[p[4:]], [A, B])[4])))
                                                         for p in order if zs.ref(files[p[4:]], [A, B])[0])
    assert grep("-n", "-m", "2", "--batch-lines", "3", "-e", tA, "-e", tB)[1] == grep("-n", "-m", "2", "-e", tA, "-e", tB)[1]
    # ---- --tally: one line per pattern as typed, in order, zeros included; a frame that two files share counts once
    distinct = list({v for v in files.values()})
    tally = lambda pats, typed, icase=False: "".join("%d\t%s\n" % (sum(len(zs.positions(d, p, icase)) for d in distinct), t) for p, t in zip(pats, typed)).encode()
    none = "no such \x7f thing"
    rc, out, err = grep("--tally", "-e", tA, "-e", none, "-e", tC, "-e", tA)
    assert rc == 0 and out == tally([A, none.encode("latin-1"), C, A], [tA, none, tC, tA])
    assert out.splitlines()[1].startswith(b"0\t") and out.splitlines()[0] == out.splitlines()[3] and not out.startswith(b"0\t")
    assert grep("--tally", "--hex", "-e", A.hex(), "-e", C.hex())[:2] == (0, tally([A, C], [A.hex(), C.hex()]))   # as typed: in hex
    assert grep("--tally", tA)[:2] == (0, tally([A], [tA]))
    assert grep("--tally", "-i", "-e", swA.decode("latin-1"))[:2] == (0, tally([swA], [swA.decode("latin-1")], icase=True))
    rc, out, err = grep("--tally", "-e", none)
    assert rc == 1 and out == b"0\t" + none.encode("latin-1") + b"\n"
    # ---- exit statuses and refusals
    assert grep("-e", none, "-e", none + "2")[:2] == (1, b"")
    listfile.write_bytes(A + b"\n\n" + B + b"\n")
    rc, out, err = grep("-f", str(listfile))
    assert rc == 2 and out == b"" and any("empty line" in l for l in err) and not any(l.startswith("searched") for l in err)
    many = tmp_path / "many"
    many.write_bytes(b"".join(b"pattern %d\n" % k for k in range(1025)))
    for bad in (["-e", ""], ["-e", "x" * 257], ["-f", str(tmp_path / "no such file")], ["-f", str(many)], ["-n", "-e", "a\nb"], ["--hex", "-e", "abc"],
                ["-e", tA, "one argument too many"], ["-e"], ["--tally"]):
        rc, out, err = grep(*bad)
        assert rc == 2 and out == b"" and not any(l.startswith("searched") for l in err), bad
    many.write_bytes(b"".join(b"pattern %d\n" % k for k in range(1023)) + A + b"\n")
    assert grep("-f", str(many))[:2] == (0, want([A]))                      # 1024 patterns: the fullest set

    # ---- one byte flipped in the frame that a.txt and sub/c.txt share: both files fail, the others are still reported; two devices: the same
    def dec(frame, raw_len):
        st, o, _ = oracle.zstd_decode(frame, raw_len)
        assert st == 0
        return o
    img = arc.read_bytes()
    a = parse_archive(img, dec, oracle.blake3)
    fr = next(f for f in a["frames"] if f[2] == oracle.blake3(files["a.txt"]))
    broken = bytearray(img); broken[fr[1] + fr[3] // 2] ^= 0xFF
    bad_arc = tmp_path / "broken.zarc"
    bad_arc.write_bytes(bytes(broken))
    results = {}
    for g in ([0, gpus] if gpus > 1 else [0]):
        rc, out, err = grep("-e", tA, "-e", tC, g=g, archive=bad_arc)
        errors = sorted(l for l in err if l.startswith("ERROR "))
        assert rc == 2 and len(errors) == 2 and errors[0].endswith(" path=src/a.txt") and errors[1].endswith(" path=src/sub/c.txt"), err
        assert out == want([A, C], only=r"^(?!src/a\.txt$|src/sub/c\.txt$)") and b"src/sub/deep/d.rec:" in out
        results[g] = (rc, out, tuple(sorted(err)))
        results["good", g] = (grep("-b", "-e", tA, "-e", tB, "-e", tC, g=g)[:2], grep("-n", "-e", tA, "-e", tB, g=g)[:2],
                              grep("--tally", "-e", tA, "-e", none, "-e", tC, g=g)[:2])
        assert results["good", g][0] == (0, want(set3, fmt="b")) and results["good", g][1] == (0, want_lines([A, B], n=True))
    assert len({v for k, v in results.items() if not isinstance(k, tuple)}) == 1
    assert len({v for k, v in results.items() if isinstance(k, tuple)}) == 1

    # ---- without the new flags: what the program printed before it had them
    assert run_old(grep, files) == json.load(open(RECORDING))


def test_set_cli_emulated(emu_lib_path, tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "host"])
    binary = os.path.join(ROOT, "tests", "emu", "_build", "zarc")
    run_set_cases(binary, tmp_path, corpus, oracle, gpus=2, env=dict(os.environ, HIPEMU_DEVICES="2"))


@pytest.mark.gpu
def test_set_cli_gpu(tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zarc_amd", "csrc"), "host"])
    binary = os.path.join(ROOT, "zarc_amd", "zarc")
    from zarc_amd import _lib
    ndev = _lib.load().zarc_gpu_device_count()
    run_set_cases(binary, tmp_path, corpus, oracle, gpus=2 if ndev >= 2 else 0, env=None)
