"""`zarc wc` (zarc_amd/host/zarc_cli.cpp), and through it ArchiveReader::count_frames and FrameReader::count_content_frames on one and on two
devices: lines, words, characters, bytes and the longest line of the files of an archive; each distinct frame counted once, nothing written.
Expected output comes from Python over the files' bytes (wc_cases.ref_wc), in directory order, and -- where it is installed -- from wc run on
the source tree."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

import wc_cases as wc
from test_container import parse_archive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("-l", "-w", "-m", "-c", "--max-line-bytes")          # the fixed order of the columns


def make_tree(base, corpus):
    src = base / "src"
    (src / "copy").mkdir(parents=True)
    text = corpus.entry(950, 30000, 0)
    assert all(c == 10 or 32 <= c < 127 for c in text) and text.count(b"\n") > 10
    tabs = bytearray(corpus.entry(951, 20000, 0))
    for p in range(7, len(tabs), 41):
        if tabs[p] == 32: tabs[p] = 9
    assert tabs.count(b"\t") > 20
    files = {
        "ascii.txt": text,
        "tabs.txt": bytes(tabs),
        "utf8.txt": ("héllo wörld €uro \U0001F600 end\n" * 700 + "läst line without a line feed").encode(),
        "blob.bin": corpus.entry(952, 70000, 3),
        "empty": b"",
        "copy/ascii2.txt": text,                             # same content as ascii.txt: one frame
    }
    for name, data in files.items(): (src / name).write_bytes(data)
    return files


def line(want, flags, path, longest=False):
    """one line of output: the selected counts in the fixed order, each followed by one space, then the path"""
    lines, words, chars, nbytes, max_line, start, no = want
    flags = (set(flags) | ({"--max-line-bytes"} if longest else set())) or {"-l", "-w", "-c"}   # --longest selects its column
    cols = []
    if "-l" in flags: cols.append(str(lines))
    if "-w" in flags: cols.append(str(words))
    if "-m" in flags: cols.append(str(chars))
    if "-c" in flags: cols.append(str(nbytes))
    if "--max-line-bytes" in flags: cols.append("%d:%d:%d" % (max_line, no, start) if longest and path != "total" else str(max_line))
    return "".join(c + " " for c in cols) + path


def run_wc_cases(binary, tmp_path, corpus, oracle, gpus, env):
    files = make_tree(tmp_path, corpus)
    arc = tmp_path / "out.zarc"
    subprocess.run([binary, "pack", "--output", str(arc), "src"], cwd=tmp_path, capture_output=True, timeout=900, check=True, env=env)
    img = arc.read_bytes()
    listed = subprocess.run([binary, "list-files", "--only-files", str(arc)], capture_output=True, timeout=600, check=True, env=env).stdout.decode().split("\n")
    order = [p for p in listed if p[4:] in files]            # directory order of the normal files ("src/" + name)
    assert sorted(order) == sorted("src/" + k for k in files)
    empty = tmp_path / "nothing_here"
    empty.mkdir()
    ref = {}
    for p in order:
        d = files[p[4:]]
        l, w, m, longest, start, no = wc.ref_wc(d)
        ref[p] = (l, w, m, len(d), longest, start, no)
    assert ref["src/empty"] == (0,) * 7 and ref["src/utf8.txt"][2] < ref["src/utf8.txt"][3] and ref["src/blob.bin"][2] < 70000

    def run(*args, g=0, archive=arc):
        cmd = [binary, "wc"] + list(args) + (["--gpus", str(g)] if g else []) + [str(archive)]
        r = subprocess.run(cmd, cwd=empty, capture_output=True, timeout=900, env=env)
        assert os.listdir(empty) == []                       # it creates nothing
        return r.returncode, r.stdout.decode().split("\n"), r.stderr.decode("latin-1").splitlines()

    def want(flags, only=None, longest=False, skip=()):
        sel = [p for p in order if not (only and not re.search(only, p)) and p not in skip]
        out = [line(ref[p], flags, p, longest) for p in sel]
        if len(sel) > 1:
            t = [sum(ref[p][k] for p in sel) for k in range(4)] + [max(ref[p][4] for p in sel), 0, 0]
            out.append(line(t, flags, "total", longest))
        return out + [""]

    # every combination of the count options, the default among them, and the total line
    for k in range(len(FLAGS) + 1):
        for flags in itertools.combinations(FLAGS, k):
            rc, out, err = run(*flags)
            assert rc == 0 and out == want(flags), flags
            assert err[-1] == "counted 6 files (5 frames), 0 failed", flags      # the shared frame: counted once, reported twice
    assert want(())[-2].endswith(" total") and want(()) == want(("-l", "-w", "-c")) and run("-c", "-l")[1] == want(("-l", "-c"))
    # --longest, --filter, --gpus
    exp = want(("-l",), longest=True)
    assert run("-l", "--longest")[:2] == (0, exp) and re.fullmatch(r"\d+ \d+:\d+:\d+ src/\S+", exp[0]) and re.fullmatch(r"\d+ \d+ total", exp[-2])
    assert run("--longest")[1] == want((), longest=True) == want(("--max-line-bytes",), longest=True)
    one = want(("-w",), only=r"utf8")
    assert run("-w", "--filter", r"utf8")[:2] == (0, one) and len(one) == 2     # one file: no total
    assert run("--filter", r"utf8", "--filter", r"^src/tabs")[1] == want((), only=r"utf8|^src/tabs") and len(want((), only=r"utf8|^src/tabs")) == 4   # any filter passes a file
    if gpus > 1:
        for flags in ((), ("-m", "--longest"), ("-l", "-w", "-m", "-c", "--max-line-bytes")):
            assert run(*flags, g=gpus)[:2] == run(*flags)[:2] == (0, want([f for f in flags if f != "--longest"], longest="--longest" in flags))
    # the installed wc, fields not spacing: -l -w -c on the printable-ASCII files, -L where there is no tab, -m under a UTF-8 locale
    if shutil.which("wc"):
        def tool(opts, paths, lc="C"):
            r = subprocess.run(["wc"] + opts + paths, cwd=tmp_path, capture_output=True, check=True, env=dict(os.environ, LC_ALL=lc))
            return [l.split() for l in r.stdout.decode().splitlines()]
        plain = [p for p in order if p.endswith(".txt") and "utf8" not in p]
        assert len(plain) == 3
        ours = [l.split() for l in run("-l", "-w", "-c", "--filter", r"(ascii|tabs).*\.txt$")[1][:-1]]
        assert tool(["-l", "-w", "-c"], plain) == ours and len(ours) == 4
        ours = [l.split() for l in run("--max-line-bytes", "--filter", r"ascii\.txt$")[1][:-1]]
        assert tool(["-L"], ["src/ascii.txt"]) == ours
        locales = subprocess.run(["locale", "-a"], capture_output=True).stdout.decode().split() if shutil.which("locale") else []
        utf8 = next((l for l in locales if re.search(r"utf-?8$", l, re.I)), None)
        if utf8:
            ours = [l.split() for l in run("-m", "--filter", r"utf8")[1][:-1]]
            assert tool(["-m"], ["src/utf8.txt"], lc=utf8) == ours
    # usage errors: exit status 2 before the archive is opened
    missing = tmp_path / "no_such.zarc"
    for bad in (["--frobnicate"], ["-L"], ["-lw"], ["--filter"], ["--gpus", "0"], ["--gpus", "65"], ["-l", str(arc)]):
        rc, out, err = run(*bad, archive=missing)
        assert rc == 2 and out == [""] and not any(l.startswith(("counted", "digest")) for l in err), bad
    r = subprocess.run([binary, "wc", "-l"], cwd=empty, capture_output=True, timeout=900, env=env)
    assert r.returncode == 2 and r.stdout == b""

    # one byte flipped in the middle of the frame that ascii.txt and copy/ascii2.txt share: both files get a message and no line, the others are listed
    def dec(frame, raw_len):
        st, o, _ = oracle.zstd_decode(frame, raw_len)
        assert st == 0
        return o
    arch = parse_archive(img, dec, oracle.blake3)
    fr = next(f for f in arch["frames"] if f[2] == oracle.blake3(files["ascii.txt"]))
    broken = bytearray(img); broken[fr[1] + fr[3] // 2] ^= 0xFF
    bad_arc = tmp_path / "broken.zarc"
    bad_arc.write_bytes(bytes(broken))
    rc, out, err = run("-l", "-m", "--longest", archive=bad_arc)
    errors = sorted(l for l in err if l.startswith("ERROR "))
    assert rc == 1 and len(errors) == 2 and errors[0].endswith(" path=src/ascii.txt") and errors[1].endswith(" path=src/copy/ascii2.txt"), err
    assert out == want(("-l", "-m"), longest=True, skip=("src/ascii.txt", "src/copy/ascii2.txt")) and len(out) == 6
    assert err[-1] == "counted 6 files (5 frames), 2 failed"


def test_wc_cli_emulated(emu_lib_path, tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "host"])
    binary = os.path.join(ROOT, "tests", "emu", "_build", "zarc")
    run_wc_cases(binary, tmp_path, corpus, oracle, gpus=2, env=dict(os.environ, HIPEMU_DEVICES="2"))


@pytest.mark.gpu
def test_wc_cli_gpu(tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zarc_amd", "csrc"), "host"])
    binary = os.path.join(ROOT, "zarc_amd", "zarc")
    from zarc_amd import _lib
    ndev = _lib.load().zarc_gpu_device_count()
    run_wc_cases(binary, tmp_path, corpus, oracle, gpus=2 if ndev >= 2 else 0, env=None)
