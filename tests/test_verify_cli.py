"""`zarc verify` and `zarc pack --check` (zarc_amd/host/zarc_cli.cpp), and through them ArchiveReader::check_frames and
FrameReader::check_content_frames on one and on two devices: an archive is tested without anything being written, each distinct
frame once; a damaged frame costs every file that shares it and no other."""
import os
import re
import subprocess

import pytest

from test_cli import make_tree
from test_container import parse_archive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC = bytes.fromhex("28B52FFD")


def run_verify_cases(binary, tmp_path, corpus, oracle, gpus, env, diag_binary):
    files = make_tree(tmp_path, corpus)                      # a.txt == sub/c.txt: 5 files, 4 distinct contents (one of them empty)
    arc, arc_checked = tmp_path / "out.zarc", tmp_path / "checked.zarc"
    out = subprocess.run([binary, "pack", "--output", str(arc), "src"], cwd=tmp_path, capture_output=True, timeout=900, check=True, env=env)
    digest = re.fullmatch(rb"digest: ([A-Za-z0-9+/]{43}=)\n", out.stdout).group(1).decode()
    img = arc.read_bytes()

    def dec(frame, raw_len):
        st, o, _ = oracle.zstd_decode(frame, raw_len)
        assert st == 0
        return o
    a = parse_archive(img, dec, oracle.blake3)
    empty = tmp_path / "nothing_here"
    empty.mkdir()

    def verify(archive, *more, g=0):
        cmd = [binary, "verify", str(archive)] + list(more) + (["--gpus", str(g)] if g else [])
        r = subprocess.run(cmd, cwd=empty, capture_output=True, timeout=900, env=env)
        assert os.listdir(empty) == []                       # it creates nothing
        return r.returncode, r.stderr.decode().splitlines()

    total = sum(len(d) for d in {v for v in files.values()})
    rc, lines = verify(arc)
    assert rc == 0 and lines == ["digest: %s" % digest, "verified 5 files (4 frames, %d bytes), 0 failed" % total], lines
    assert verify(arc, "--verify", digest) == (0, lines[1:])
    rc, lines = verify(arc, "--verify", "A" * 43 + "=")
    assert rc == 1 and len(lines) == 1 and "integrity failure" in lines[0]          # and no frame was decoded: nothing else is said
    rc, lines = verify(arc, "--filter", r"\.txt$")
    assert rc == 0 and lines[-1] == "verified 2 files (1 frames, 12000 bytes), 0 failed"

    # one byte flipped in the middle of the frame that a.txt and sub/c.txt share
    shared = oracle.blake3(files["a.txt"])
    fr = next(f for f in a["frames"] if f[2] == shared)
    assert img[fr[1]:fr[1] + 4] == MAGIC
    broken = bytearray(img); broken[fr[1] + fr[3] // 2] ^= 0xFF
    bad_arc = tmp_path / "broken.zarc"
    bad_arc.write_bytes(bytes(broken))
    results = {}
    for g in ([0, gpus] if gpus > 1 else [0]):
        rc, lines = verify(bad_arc, g=g)
        errors = sorted(l for l in lines if l.startswith("ERROR "))
        assert rc == 1 and len(errors) == 2 and errors[0].endswith(" path=src/a.txt") and errors[1].endswith(" path=src/sub/c.txt"), lines
        assert lines[-1] == "verified 5 files (4 frames, %d bytes), 2 failed" % total
        results[g] = (rc, tuple(sorted(lines)))
        rc, lines = verify(bad_arc, "--filter", r"b\.bin|d\.rec|empty", g=g)
        assert rc == 0 and lines[-1].endswith(", 0 failed") and not any(l.startswith("ERROR") for l in lines)
        assert verify(arc, g=g)[0] == 0
    assert len(set(results.values())) == 1                     # --gpus 2: the same lines and exit status

    # pack --check writes the archive pack writes (up to the directory, whose timestamp differs)
    subprocess.run([binary, "pack", "--check", "--output", str(arc_checked), "src"], cwd=tmp_path, capture_output=True, timeout=900, check=True, env=env)
    img2 = arc_checked.read_bytes()
    assert img2[:a["dir_at"]] == img[:a["dir_at"]] and verify(arc_checked)[0] == 0
    if diag_binary:                                          # a diagnostic build: the check can be seen failing
        env_flip = dict(env or os.environ, ZARC_GPU_CHECK_FLIP_BODY="1")
        left = tmp_path / "left.zarc"
        r = subprocess.run([diag_binary, "pack", "--check", "--output", str(left), "src"], cwd=tmp_path, capture_output=True, timeout=900, env=env_flip)
        assert r.returncode == 1 and b"read-back check" in r.stderr and re.search(rb"Error: src/\S+: ", r.stderr), r.stderr[-500:]
        r = subprocess.run([diag_binary, "list-files", str(left)], capture_output=True, timeout=600, env=env)
        assert r.returncode != 0                             # neither directory nor trailer: not a zarc archive
        r = subprocess.run([diag_binary, "pack", "--output", str(left), "src"], cwd=tmp_path, capture_output=True, timeout=900, env=env_flip)
        assert r.returncode == 0                             # without --check nothing is injected and nothing is looked at


def test_verify_cli_emulated(emu_lib_path, tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "host"])
    binary = os.path.join(ROOT, "tests", "emu", "_build", "zarc")
    env2 = dict(os.environ, HIPEMU_DEVICES="2")
    run_verify_cases(binary, tmp_path, corpus, oracle, gpus=2, env=env2, diag_binary=binary)   # the emulator build is a diagnostic build


@pytest.mark.gpu
def test_verify_cli_gpu(tmp_path, corpus, oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zarc_amd", "csrc"), "host"])
    binary = os.path.join(ROOT, "zarc_amd", "zarc")
    from zarc_amd import _lib
    ndev = _lib.load().zarc_gpu_device_count()
    run_verify_cases(binary, tmp_path, corpus, oracle, gpus=2 if ndev >= 2 else 0, env=None, diag_binary=None)
