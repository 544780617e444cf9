"""A search_set_lines call gives the same however it is cut: the check shared by the emulator test (test_set_cut.py) and the GPU test
(test_gpu_set_cut.py).  It stands in a module of its own so that set_cases.py and the tests that import it stay as they were.

search_set_lines carries the most from one part of a call to the next: hits are added per part, the remainder of rec_cap, the text offset
and the index of the part's first frame go on.  The uncut call (no scratch budget, one staged chunk) is checked against the `re` reference
of set_cases; the same call cut by the scratch budget, by the staging chunk, and by both must return exactly what it returned."""
import numpy as np

import search_cases as sc
import set_cases as zs
import verify_cases as vc
from zarc_amd import _lib

KIB = (300, 296, 44, 288, 292, 300, 280, 284)   # eight text frames, 2 084 KiB in all
PATTERNS = [b"e ", b"odnwnecr", b"uhq"]         # length classes 2, 4 and more, 3; all of them occur in the corpus' text


def check_lines_cut_invariance(engine, corpus, compress=True):
    """The frames hold more than twice the 1 MiB budget, so the batch is halved and its larger half is halved again.  A staging chunk of
    650 000 bytes gives four host chunks ([0,1] [2,3,4] [5,6] [7]); one of 1 300 000 bytes gives two, the first of which (1 220 KiB) is over
    the budget again.  max_lines is 40 and every frame has more matching lines than that, so rec_cap = 255 runs out in the seventh frame:
    behind every cut."""
    raws = [corpus.entry(6600 + i, k * 1024, 0) for i, k in enumerate(KIB)]
    packed = frames, raw_lens, digests = sc.pack(engine, raws, compress=compress)
    kw = dict(max_lines=40, rec_cap=255)
    free = zs.check_set_lines(engine, packed, raws, PATTERNS, tag="uncut", **kw)
    assert all(r[5] > 40 for r in free[0]) and len(free[1]) == 255 and free[1][-1][0] == 6 and all(h > 0 for h in free[2])
    d_frames, foff, _ = vc._arena(engine, frames)
    try:
        exp = np.frombuffer(b"".join(digests), dtype=np.uint8)
        for mb, chunk in ((1, 0), (0, 650000), (1, 1300000)):
            engine.set_parameter(_lib.PX_SCRATCH_MB, mb)
            engine.set_parameter(_lib.PX_STAGE_CHUNK, chunk)
            try:
                assert engine.search_set_lines(frames, raw_lens, PATTERNS, expect=digests, **kw) == free, ("host form", mb, chunk)
                if not chunk:
                    dev = engine.search_set_lines_device(d_frames, foff, [len(f) for f in frames], raw_lens, PATTERNS, expect=exp, **kw)
                    assert dev == free, ("device form", mb)
            finally:
                engine.set_parameter(_lib.PX_SCRATCH_MB, 0)
                engine.set_parameter(_lib.PX_STAGE_CHUNK, 0)
    finally:
        engine.free(d_frames)
