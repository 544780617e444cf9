"""`zarc compare` (zarc_amd/host/zarc_cli.cpp), and through it ArchiveReader::compare_frames and FrameReader::compare_content_frames: an
archive against the tree on disk, content only, nothing written.  The tree is packed, then changed on disk: a byte changed, a file grown,
one cut short, one deleted, one replaced by a directory, the rest left alone.  Expected lines come from Python over both sides' bytes
(compare_cases.ref_cmp), in directory order."""
import os
import re
import subprocess

import pytest

import compare_cases as cc
from test_container import parse_archive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_tree(base, corpus):
    src = base / "src"
    (src / "sub").mkdir(parents=True)
    text = corpus.entry(960, 9000, 0)
    files = {
        "same.txt": text,
        "changed.txt": corpus.entry(961, 70000, 0),
        "grown.log": corpus.entry(962, 5000, 0),
        "cut.txt": corpus.entry(963, 6000, 0),
        "edited.txt": corpus.entry(964, 8000, 0),
        "gone.txt": b"soon deleted\n",
        "turned.txt": b"soon a directory\n",
        "empty": b"",
        "blob.bin": corpus.entry(965, 3000, 3),
        "sub/copy.txt": text,                                # same content as same.txt: one frame, two pairs
    }
    for name, data in files.items(): (src / name).write_bytes(data)
    return files


def change_tree(src, files):
    """-> what is on disk afterwards: name -> bytes, None (missing) or "dir" """
    disk = dict(files)
    b = bytearray(files["changed.txt"]); b[65536 + 7] ^= 0x01
    disk["changed.txt"] = bytes(b)
    disk["grown.log"] = files["grown.log"] + b"one more line\n"
    disk["cut.txt"] = files["cut.txt"][:4321]
    disk["edited.txt"] = files["edited.txt"][:3000] + b"[inserted]" + files["edited.txt"][3000:]
    disk["sub/copy.txt"] = files["sub/copy.txt"][:-1] + b"!"
    for name in ("changed.txt", "grown.log", "cut.txt", "edited.txt", "sub/copy.txt"): (src / name).write_bytes(disk[name])
    os.remove(src / "gone.txt"); disk["gone.txt"] = None
    os.remove(src / "turned.txt"); (src / "turned.txt").mkdir(); disk["turned.txt"] = "dir"
    return disk


def want_line(path, a, b):
    """the line of one file, or None where it is identical"""
    if b is None: return path + ": missing"
    if b == "dir": return path + ": not a regular file"
    relation, prefix, line, differing, suffix, _, _ = cc.ref_cmp(a, b)
    if relation == cc.EQUAL: return None
    if relation == cc.FRAME_IS_PREFIX: return "%s: archive copy is a prefix: %d of %d bytes, line %d" % (path, len(a), len(b), line)
    if relation == cc.OTHER_IS_PREFIX: return "%s: file is a prefix: %d of %d bytes, line %d" % (path, len(b), len(a), line)
    s = "%s: differ: byte %d, line %d, %d bytes differ" % (path, prefix + 1, line, differing)
    if len(a) != len(b): s += ", sizes %d and %d, common tail %d" % (len(a), len(b), suffix)
    return s


def run_compare_cases(binary, tmp_path, corpus, oracle, gpus, env):
    files = make_tree(tmp_path, corpus)
    arc = tmp_path / "out.zarc"
    subprocess.run([binary, "pack", "--output", str(arc), "src"], cwd=tmp_path, capture_output=True, timeout=900, check=True, env=env)
    listed = subprocess.run([binary, "list-files", "--only-files", str(arc)], capture_output=True, timeout=600, check=True, env=env).stdout.decode().split("\n")
    order = [p for p in listed if p[4:] in files]            # directory order of the normal files ("src/" + name)
    assert sorted(order) == sorted("src/" + k for k in files)

    def run(*args, cwd=tmp_path, archive=arc, verb="compare"):
        r = subprocess.run([binary, verb] + list(args) + [str(archive)], cwd=cwd, capture_output=True, timeout=900, env=env)
        return r.returncode, r.stdout.decode().split("\n"), r.stderr.decode("latin-1").splitlines()

    def snapshot():
        return sorted((d, sorted(ds), sorted(fs)) for d, ds, fs in os.walk(tmp_path))

    # the tree as it was packed: everything identical, exit status 0
    before = snapshot()
    rc, out, err = run()
    assert (rc, out) == (0, [""]) and err[-1] == "compared 10 files: 10 identical, 0 differ, 0 missing, 0 failed", err
    assert run("--report-identical")[:2] == (0, [p + ": identical" for p in order] + [""])
    assert run("-C", str(tmp_path), cwd=tmp_path / "src")[:2] == run("--directory", ".")[:2] == (0, [""])
    assert run("--filter", r"same|blob", "--report-identical")[1] == [p + ": identical" for p in order if "same" in p or "blob" in p] + [""]

    disk = change_tree(tmp_path / "src", files)
    before = snapshot()
    lines = {p: want_line(p, files[p[4:]], disk[p[4:]]) for p in order}
    assert lines["src/changed.txt"] == "src/changed.txt: differ: byte %d, line %d, 1 bytes differ" % (65536 + 8, 1 + files["changed.txt"][:65536 + 7].count(b"\n"))
    assert lines["src/grown.log"] == "src/grown.log: archive copy is a prefix: 5000 of 5014 bytes, line %d" % (1 + files["grown.log"].count(b"\n"))
    assert lines["src/cut.txt"].startswith("src/cut.txt: file is a prefix: 4321 of 6000 bytes, line ")
    assert lines["src/edited.txt"].endswith(" bytes differ, sizes 8000 and 8010, common tail 5000") and ": differ: byte 3001, line " in lines["src/edited.txt"]
    assert lines["src/sub/copy.txt"].startswith("src/sub/copy.txt: differ: byte 9000, ") and lines["src/same.txt"] is None    # one frame, two answers
    assert (lines["src/gone.txt"], lines["src/turned.txt"]) == ("src/gone.txt: missing", "src/turned.txt: not a regular file")
    exp = [lines[p] for p in order if lines[p]] + [""]
    assert len(exp) == 8
    rc, out, err = run()
    assert (rc, out) == (1, exp) and err[-1] == "compared 10 files: 3 identical, 6 differ, 1 missing, 0 failed", (out, err)
    assert run("--brief")[:2] == (1, [p for p in order if lines[p]] + [""])
    assert run("--report-identical")[:2] == (1, [lines[p] or p + ": identical" for p in order] + [""])
    assert run("--batch-bytes", "1")[:2] == (1, exp)                            # a batch per file
    assert run("--filter", r"\.log$", "--filter", "^src/empty")[:2] == (1, [lines["src/grown.log"], ""])
    assert run("--filter", r"same|blob|empty")[:2] == (0, [""])
    assert run("--filter", r"gone")[:2] == (1, ["src/gone.txt: missing", ""])
    assert run("-C", str(tmp_path / "nothing_here"))[:2] == (1, [p + ": missing" for p in order] + [""])
    if gpus > 1: assert run("--gpus", str(gpus))[:2] == (1, exp)
    assert snapshot() == before                                                  # it creates and changes nothing
    # `zarc c` and `zarc ca` are still cat
    cat = run("--filter", r"gone", verb="cat")
    assert cat[0] == 0 and cat[1] == ["soon deleted", ""]
    assert run("--filter", r"gone", verb="c")[:2] == run("--filter", r"gone", verb="ca")[:2] == cat[:2]
    assert run("--filter", r"gone", verb="comp")[:2] == (1, ["src/gone.txt: missing", ""])
    # usage errors: exit status 2 before the archive is opened
    missing = tmp_path / "no_such.zarc"
    for bad in (["--frobnicate"], ["-C"], ["--filter"], ["--gpus", "0"], ["--gpus", "65"], ["--batch-bytes", "0"], ["--batch-bytes", "x"], ["--brief", str(arc)]):
        rc, out, err = run(*bad, archive=missing)
        assert rc == 2 and out == [""] and not any(l.startswith(("compared", "digest")) for l in err), bad
    r = subprocess.run([binary, "compare", "--brief"], cwd=tmp_path, capture_output=True, timeout=900, env=env)
    assert r.returncode == 2 and r.stdout == b""
    # trouble is 2, never 1 ("something differs"): an archive that is not there, one that is no archive, a file that cannot be read
    garbage = tmp_path / "garbage.zarc"
    garbage.write_bytes(b"this is no archive\n" * 40)
    for broken in (missing, garbage):
        rc, out, err = run(archive=broken)
        assert rc == 2 and out == [""] and any(l.startswith("Error: ") for l in err), (broken, err)
    if os.geteuid() != 0:                                                        # (root reads whatever the mode says)
        os.chmod(tmp_path / "src" / "blob.bin", 0)
        try:
            rc, out, err = run("--filter", r"blob|empty")
            assert (rc, out) == (2, ["src/blob.bin: unreadable (Permission denied)", ""]) and err[-1] == "compared 2 files: 1 identical, 0 differ, 0 missing, 1 failed"
        finally:
            os.chmod(tmp_path / "src" / "blob.bin", 0o644)
    # one byte flipped in the middle of the frame that same.txt and sub/copy.txt share: both pairs are bad frames, exit status 2, the
    # other files are reported as before
    def dec(frame, raw_len):
        st, o, _ = oracle.zstd_decode(frame, raw_len)
        assert st == 0
        return o
    img = arc.read_bytes()
    arch = parse_archive(img, dec, oracle.blake3)
    fr = next(f for f in arch["frames"] if f[2] == oracle.blake3(files["same.txt"]))
    broken = bytearray(img); broken[fr[1] + fr[3] // 2] ^= 0xFF
    bad_arc = tmp_path / "broken.zarc"
    bad_arc.write_bytes(bytes(broken))
    rc, out, err = run(archive=bad_arc)
    shared = ("src/same.txt", "src/sub/copy.txt")
    assert rc == 2 and err[-1] == "compared 10 files: 2 identical, 5 differ, 1 missing, 2 failed", (out, err)
    assert len(out) == 9 and [l for l in out if not l.startswith(shared)] == [lines[p] for p in order if lines[p] and p not in shared] + [""]
    assert all(re.fullmatch(re.escape(p) + r": bad frame \(.+\)", l) for p, l in zip(sorted(shared), sorted(l for l in out if l.startswith(shared)))), out
    assert run("--brief", archive=bad_arc)[:2] == (2, [p for p in order if lines[p] or p in shared] + [""])


def test_compare_cli_emulated(emu_lib_path, tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "host"])
    binary = os.path.join(ROOT, "tests", "emu", "_build", "zarc")
    run_compare_cases(binary, tmp_path, corpus, oracle, gpus=2, env=dict(os.environ, HIPEMU_DEVICES="2"))


@pytest.mark.gpu
def test_compare_cli_gpu(tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zarc_amd", "csrc"), "host"])
    binary = os.path.join(ROOT, "zarc_amd", "zarc")
    from zarc_amd import _lib
    ndev = _lib.load().zarc_gpu_device_count()
    run_compare_cases(binary, tmp_path, corpus, oracle, gpus=2 if ndev >= 2 else 0, env=None)
