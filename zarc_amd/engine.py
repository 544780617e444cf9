"""Thin Python view of the engine handle (include/zarc_gpu.h).  Plumbing only: every byte of the data path
is processed by the HIP kernels inside libzarc_gpu.so."""
import ctypes

import numpy as np

from . import _lib
from ._lib import ZarcGpuError


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


class Engine:
    """One engine handle = one HIP stream on one device (CCtx/DCtx analogue, crates/zarc/src/encode.rs:58-78)."""

    def __init__(self, device=0, lib_path=None):
        import os
        self.lib_path = lib_path or os.environ.get("ZARC_GPU_LIB") or _lib.DEFAULT_LIB
        self.lib = _lib.load(self.lib_path)
        h = ctypes.c_void_p()
        rc = self.lib.zarc_gpu_create(ctypes.byref(h), device)
        if rc != 0:
            raise ZarcGpuError(rc, self.lib.zarc_gpu_error_name(rc).decode(),
                               "zarc_gpu_create failed: no usable HIP device (there is no CPU fallback)")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.zarc_gpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZarcGpuError(rc, self.lib.zarc_gpu_error_name(rc).decode(), self.lib.zarc_gpu_last_error(self.h).decode())

    # ---- parameters (Encoder::set_zstd_parameter / enable_compression) ----
    def set_parameter(self, param_id, value):
        self._check(self.lib.zarc_gpu_set_parameter(self.h, param_id, value))

    def enable_compression(self, compress):
        """Encoder::enable_compression (crates/zarc/src/encode.rs:95-97): False -> raw-block ("stored") frames."""
        self.lib.zarc_gpu_enable_compression(self.h, 1 if compress else 0)

    def params(self):
        p = _lib.Params()
        self.lib.zarc_gpu_get_params(self.h, ctypes.byref(p))
        return p

    def bound(self, n):
        return self.lib.zarc_gpu_bound(n)

    def kernel_ms(self, which):
        return float(self.lib.zarc_gpu_last_kernel_ms(self.h, which))

    def copy_bytes(self, which):
        """Content bytes the most recent batch call moved (_lib.C_H2D / C_D2H / C_RING / C_DIRECT); device forms report 0."""
        return int(self.lib.zarc_gpu_last_copy_bytes(self.h, which))

    # ---- device memory helpers ----
    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(self.lib.zarc_gpu_device_malloc(self.h, ctypes.byref(p), nbytes))
        return p.value

    def free(self, dptr):
        self._check(self.lib.zarc_gpu_device_free(self.h, ctypes.c_void_p(dptr)))

    def h2d(self, dptr, data):
        buf = (ctypes.c_char * len(data)).from_buffer_copy(data) if not isinstance(data, np.ndarray) else None
        src = buf if buf is not None else data.ctypes.data_as(ctypes.c_void_p)
        n = len(data) if buf is not None else data.nbytes
        self._check(self.lib.zarc_gpu_memcpy_h2d(self.h, ctypes.c_void_p(dptr), src, n))

    def d2h(self, dptr, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        self._check(self.lib.zarc_gpu_memcpy_d2h(self.h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(dptr), nbytes))
        return out

    # ---- device-resident batch calls ----
    def corpus_fill(self, dptr, off, length, first_index=0, kind=-1):
        off, poff = _u64(off)
        length, plen = _u64(length)
        self._check(self.lib.zarc_gpu_corpus_fill_device(self.h, len(off), ctypes.c_void_p(dptr), poff, plen, first_index, kind))

    def blake3_device(self, dptr, off, length):
        off, poff = _u64(off)
        length, plen = _u64(length)
        dig = np.zeros((len(off), 32), dtype=np.uint8)
        self._check(self.lib.zarc_gpu_blake3_batch_device(self.h, len(off), ctypes.c_void_p(dptr), poff, plen, dig.ctypes.data_as(ctypes.c_void_p)))
        return dig

    def xxh64_device(self, dptr, off, length):
        off, poff = _u64(off)
        length, plen = _u64(length)
        out = np.zeros(len(off), dtype=np.uint64)
        self._check(self.lib.zarc_gpu_xxh64_batch_device(self.h, len(off), ctypes.c_void_p(dptr), poff, plen,
                                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out

    def pack_device(self, d_src, off, length, d_dst, dst_cap):
        off, poff = _u64(off)
        length, plen = _u64(length)
        n = len(off)
        dst_off = np.zeros(n, dtype=np.uint64)
        dst_len = np.zeros(n, dtype=np.uint64)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        self._check(self.lib.zarc_gpu_pack_batch_device(
            self.h, n, ctypes.c_void_p(d_src), poff, plen, ctypes.c_void_p(d_dst), dst_cap,
            dst_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), dst_len.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return dst_off, dst_len, dig, status

    def unpack_device(self, d_frames, frame_off, frame_len, d_dst, dst_off, raw_len, expect=None):
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        dst_off, pdo = _u64(dst_off)
        raw_len, prl = _u64(raw_len)
        n = len(frame_off)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        self._check(self.lib.zarc_gpu_unpack_batch_device(
            self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, ctypes.c_void_p(d_dst), pdo, prl,
            exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
            dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return dig, status

    def verify_device(self, d_frames, frame_off, frame_len, raw_len, expect=None):
        """unpack_device without an output: -> (digests, statuses), exactly unpack's."""
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        raw_len, prl = _u64(raw_len)
        n = len(frame_off)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        self._check(self.lib.zarc_gpu_verify_batch_device(
            self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, prl,
            exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
            dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return dig, status

    def repack_device(self, d_frames, frame_off, frame_len, raw_len, d_dst, dst_cap, expect=None):
        """verify_device joined to pack_device: frames with status OK are encoded again with the handle's parameters into d_dst.
        -> (dst_off, dst_len, digests, statuses)"""
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        raw_len, prl = _u64(raw_len)
        n = len(frame_off)
        dst_off, dst_len = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        self._check(self.lib.zarc_gpu_repack_batch_device(
            self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, prl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
            ctypes.c_void_p(d_dst), dst_cap, dst_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            dst_len.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return dst_off, dst_len, dig, status

    def search_device(self, d_frames, frame_off, frame_len, raw_len, pattern, icase=False, expect=None, _fn="zarc_gpu_search_batch_device"):
        """verify_device plus a search of what was decoded, where it lies: -> list of (status, digest, count, first) per frame.
        `pattern` is a fixed byte string (host memory, 1..256 bytes); count = matching start positions, first = the lowest or None."""
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        raw_len, prl = _u64(raw_len)
        n = len(frame_off)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        count, first = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        pat = bytes(pattern)
        self._check(getattr(self.lib, _fn)(
            self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, prl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
            ctypes.cast(ctypes.c_char_p(pat), ctypes.c_void_p), len(pat), _lib.SEARCH_ICASE if icase else 0,
            dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
            count.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), first.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return [(int(status[i]), bytes(dig[i]), int(count[i]), None if int(first[i]) == _lib.SEARCH_NONE else int(first[i])) for i in range(n)]

    def search_lines_device(self, d_frames, frame_off, frame_len, raw_len, pattern, icase=False, expect=None, max_lines=0, max_line=4096, rec_cap=4096,
                            _fn="zarc_gpu_search_lines_batch_device", invert=False, before=0, after=0):
        """search_device plus the matching lines: -> (results, records) as search_lines() gives them.  The text is gathered into a device
        buffer of rec_cap * max_line bytes and copied back from there."""
        if invert or before or after:
            kind = _lib.MATCH_REGEX if _fn == "zarc_gpu_search_regex_lines_batch_device" else _lib.MATCH_FIXED
            return self.select_lines_device(d_frames, frame_off, frame_len, raw_len, kind, pattern, icase, expect, max_lines, max_line, rec_cap, invert, before,
                                            after)[:2]
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        raw_len, prl = _u64(raw_len)
        n = len(frame_off)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        count, first, lines = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        pat = bytes(pattern)
        rec = (_lib.Line * max(rec_cap, 1))()
        rec_used, text_used = ctypes.c_size_t(), ctypes.c_size_t()
        text_cap = rec_cap * max_line
        d_text = self.malloc(max(text_cap, 1))
        try:
            u64p = ctypes.POINTER(ctypes.c_uint64)
            self._check(getattr(self.lib, _fn)(
                self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, prl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
                ctypes.cast(ctypes.c_char_p(pat), ctypes.c_void_p), len(pat), _lib.SEARCH_ICASE if icase else 0, max_lines, max_line,
                dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), count.ctypes.data_as(u64p), first.ctypes.data_as(u64p),
                lines.ctypes.data_as(u64p), rec, rec_cap, ctypes.byref(rec_used), ctypes.c_void_p(d_text), text_cap, ctypes.byref(text_used)))
            text = bytes(self.d2h(d_text, text_used.value)) if text_used.value else b""
        finally:
            self.free(d_text)
        return self._lines_result(n, status, dig, count, first, lines, rec, rec_used.value, text)

    def search_set_device(self, d_frames, frame_off, frame_len, raw_len, patterns, icase=False, expect=None):
        """search_device for a set of patterns in one pass -> (results, hits) as search_set() gives them."""
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        raw_len, prl = _u64(raw_len)
        n = len(frame_off)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        count, first, which = (np.zeros(n, dtype=np.uint64) for _ in range(3))
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        ps = _lib.PatternSet.of(patterns)
        hits = (ctypes.c_uint64 * max(ps.count, 1))()
        u64p = ctypes.POINTER(ctypes.c_uint64)
        self._check(self.lib.zarc_gpu_search_set_batch_device(
            self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, prl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
            ctypes.byref(ps), _lib.SEARCH_ICASE if icase else 0, dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
            count.ctypes.data_as(u64p), first.ctypes.data_as(u64p), which.ctypes.data_as(u64p), hits))
        return self._set_result(n, status, dig, count, first, which), [int(v) for v in hits[:ps.count]]

    def search_set_lines_device(self, d_frames, frame_off, frame_len, raw_len, patterns, icase=False, expect=None, max_lines=0, max_line=4096, rec_cap=4096,
                                invert=False, before=0, after=0):
        """search_lines_device for a set of patterns -> (results, records, hits) as search_set_lines() gives them."""
        if invert or before or after:
            return self.select_lines_device(d_frames, frame_off, frame_len, raw_len, _lib.MATCH_SET, patterns, icase, expect, max_lines, max_line, rec_cap, invert,
                                            before, after)
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        raw_len, prl = _u64(raw_len)
        n = len(frame_off)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        count, first, which, lines = (np.zeros(n, dtype=np.uint64) for _ in range(4))
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        ps = _lib.PatternSet.of(patterns)
        hits = (ctypes.c_uint64 * max(ps.count, 1))()
        rec = (_lib.Line * max(rec_cap, 1))()
        rec_used, text_used = ctypes.c_size_t(), ctypes.c_size_t()
        text_cap = rec_cap * max_line
        d_text = self.malloc(max(text_cap, 1))
        try:
            u64p = ctypes.POINTER(ctypes.c_uint64)
            self._check(self.lib.zarc_gpu_search_set_lines_batch_device(
                self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, prl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
                ctypes.byref(ps), _lib.SEARCH_ICASE if icase else 0, max_lines, max_line,
                dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), count.ctypes.data_as(u64p), first.ctypes.data_as(u64p),
                which.ctypes.data_as(u64p), hits, lines.ctypes.data_as(u64p), rec, rec_cap, ctypes.byref(rec_used), ctypes.c_void_p(d_text), text_cap,
                ctypes.byref(text_used)))
            text = bytes(self.d2h(d_text, text_used.value)) if text_used.value else b""
        finally:
            self.free(d_text)
        return self._set_lines_result(n, status, dig, count, first, which, lines, rec, rec_used.value, text) + ([int(v) for v in hits[:ps.count]],)

    @staticmethod
    def _set_result(n, status, dig, count, first, which):
        none = lambda v: None if int(v) == _lib.SEARCH_NONE else int(v)
        return [(int(status[i]), bytes(dig[i]), int(count[i]), none(first[i]), none(which[i])) for i in range(n)]

    @staticmethod
    def _set_lines_result(n, status, dig, count, first, which, lines, rec, rec_used, text):
        none = lambda v: None if int(v) == _lib.SEARCH_NONE else int(v)
        results = [(int(status[i]), bytes(dig[i]), int(count[i]), none(first[i]), none(which[i]), int(lines[i])) for i in range(n)]
        records = [(r.frame, r.start, r.length, r.number, r.match, text[r.text_off:r.text_off + r.text_len]) for r in rec[:rec_used]]
        return results, records

    @staticmethod
    def _lines_result(n, status, dig, count, first, lines, rec, rec_used, text):
        results = [(int(status[i]), bytes(dig[i]), int(count[i]), None if int(first[i]) == _lib.SEARCH_NONE else int(first[i]), int(lines[i])) for i in range(n)]
        records = [(r.frame, r.start, r.length, r.number, r.match, text[r.text_off:r.text_off + r.text_len]) for r in rec[:rec_used]]
        return results, records

    # ---- host-memory batch calls (the shape of the reference's API: slices in, bytes out) ----
    def blake3(self, entries):
        n = len(entries)
        bufs = [bytes(e) for e in entries]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        dig = np.zeros((n, 32), dtype=np.uint8)
        self._check(self.lib.zarc_gpu_blake3_batch(self.h, n, ptrs, lens, dig.ctypes.data_as(ctypes.c_void_p)))
        return [bytes(d) for d in dig]

    def pack(self, entries):
        """-> list of (frame_bytes, digest).  Mirrors Encoder::add_data_frame for a batch of entries."""
        n = len(entries)
        bufs = [bytes(e) for e in entries]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        cap = sum(self.bound(len(b)) for b in bufs)
        dst = np.zeros(max(cap, 1), dtype=np.uint8)
        dst_off = (ctypes.c_size_t * n)()
        dst_len = (ctypes.c_size_t * n)()
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        self._check(self.lib.zarc_gpu_pack_batch(self.h, n, ptrs, lens, dst.ctypes.data_as(ctypes.c_void_p), cap, dst_off, dst_len,
                                                 dig.ctypes.data_as(ctypes.c_void_p), status))
        return [(bytes(dst[dst_off[i]:dst_off[i] + dst_len[i]]), bytes(dig[i])) for i in range(n)]

    def pack_dedup(self, entries, seen):
        """Hash-first pack (Encoder::add_data_frame: hash, look the digest up, compress only new content; content_frame.rs:26-33).
        `seen` is a set of digests (bytes) the caller has frames for; it is updated with what this call compresses.
        -> list of (frame_bytes or None for a skipped duplicate, digest, status)."""
        n = len(entries)
        bufs = [bytes(e) for e in entries]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        cap = sum(self.bound(len(b)) for b in bufs)
        dst = np.zeros(max(cap, 1), dtype=np.uint8)
        dst_off, dst_len = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        calls = []

        def known(_ctx, d, i):
            key = bytes(d[:32])
            calls.append(i)
            if key in seen:
                return 1
            seen.add(key)
            return 0
        cb = _lib.KNOWN_FN(known)
        self._check(self.lib.zarc_gpu_pack_batch_dedup(self.h, n, ptrs, lens, dst.ctypes.data_as(ctypes.c_void_p), cap, dst_off, dst_len,
                                                       dig.ctypes.data_as(ctypes.c_void_p), status, cb, None))
        assert calls == list(range(n))       # once per entry, in index order
        return [(bytes(dst[dst_off[i]:dst_off[i] + dst_len[i]]) if status[i] != _lib.FRAME_DUPLICATE else None, bytes(dig[i]), int(status[i]))
                for i in range(n)]

    def pack_device_dedup(self, d_src, off, length, d_dst, dst_cap, seen):
        off, poff = _u64(off)
        length, plen = _u64(length)
        n = len(off)
        dst_off, dst_len = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)

        def known(_ctx, d, i):
            key = bytes(d[:32])
            if key in seen:
                return 1
            seen.add(key)
            return 0
        cb = _lib.KNOWN_FN(known)
        self._check(self.lib.zarc_gpu_pack_batch_device_dedup(
            self.h, n, ctypes.c_void_p(d_src), poff, plen, ctypes.c_void_p(d_dst), dst_cap,
            dst_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), dst_len.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), cb, None))
        return dst_off, dst_len, dig, status

    def unpack(self, frames, raw_lens, expect=None):
        """-> list of (bytes, digest, status).  Mirrors read_content_frame + FrameIterator::verify for a batch."""
        n = len(frames)
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        outs = [np.zeros(max(int(r), 1), dtype=np.uint8) for r in raw_lens]
        optrs = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        self._check(self.lib.zarc_gpu_unpack_batch(self.h, n, ptrs, lens, rl, optrs,
                                                   exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
                                                   dig.ctypes.data_as(ctypes.c_void_p), status))
        return [(bytes(outs[i][:int(raw_lens[i])]), bytes(dig[i]), int(status[i])) for i in range(n)]

    def verify(self, frames, raw_lens, expect=None):
        """-> list of (digest, status): FrameIterator::verify for a batch.  What unpack() reports for the same frames, without the bytes:
        only the compressed frames cross to the device and nothing but 36 bytes per frame comes back."""
        n = len(frames)
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        self._check(self.lib.zarc_gpu_verify_batch(self.h, n, ptrs, lens, rl,
                                                   exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
                                                   dig.ctypes.data_as(ctypes.c_void_p), status))
        return [(bytes(dig[i]), int(status[i])) for i in range(n)]

    def search(self, frames, raw_lens, pattern, icase=False, expect=None, _fn="zarc_gpu_search_batch"):
        """-> list of (status, digest, count, first) per frame: verify()'s verdict, the number of start positions at which the fixed byte
        string `pattern` (1..256 bytes; icase folds ASCII letters only) occurs in the frame's content, and the lowest of them (None without
        a match).  Only the compressed frames cross to the device; no content comes back."""
        n = len(frames)
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        count, first = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        pat = bytes(pattern)
        self._check(getattr(self.lib, _fn)(self.h, n, ptrs, lens, rl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
                                                   ctypes.cast(ctypes.c_char_p(pat), ctypes.c_void_p), len(pat), _lib.SEARCH_ICASE if icase else 0,
                                                   dig.ctypes.data_as(ctypes.c_void_p), status, count, first))
        return [(int(status[i]), bytes(dig[i]), int(count[i]), None if int(first[i]) == _lib.SEARCH_NONE else int(first[i])) for i in range(n)]

    def search_lines(self, frames, raw_lens, pattern, icase=False, expect=None, max_lines=0, max_line=4096, rec_cap=4096, _fn="zarc_gpu_search_lines_batch",
                     invert=False, before=0, after=0):
        """search() plus the lines that hold a match -> (results, records).  results[i] = (status, digest, count, first, lines): search()'s
        answer and the number of matching lines of frame i (all of them, whatever the caps).  records = [(frame, start, length, number,
        match, text_bytes)] ordered by (frame, start): per frame the first min(lines, max_lines or all) matching lines while rec_cap
        lasts; a line is a run of bytes without 0x0A, text_bytes its first min(length, max_line) bytes.  The pattern must not contain
        0x0A.  Only the compressed frames cross to the device and only the delivered lines' bytes come back.
        invert / before / after select lines as grep -v / -B / -A do (include/zarc_gpu.h, zarc_gpu_select_lines_batch): with any
        of them set, every result tuple gains `selected` at its end, `lines` counts the hit lines, the records are the selected lines and a
        record's match is None when its line holds no match."""
        if invert or before or after:
            kind = _lib.MATCH_REGEX if _fn == "zarc_gpu_search_regex_lines_batch" else _lib.MATCH_FIXED
            return self.select_lines(frames, raw_lens, kind, pattern, icase, expect, max_lines, max_line, rec_cap, invert, before, after)[:2]
        n = len(frames)
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        count, first, lines = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        pat = bytes(pattern)
        rec = (_lib.Line * max(rec_cap, 1))()
        rec_used, text_used = ctypes.c_size_t(), ctypes.c_size_t()
        text_cap = rec_cap * max_line
        text = np.empty(max(text_cap, 1), dtype=np.uint8)
        self._check(getattr(self.lib, _fn)(
            self.h, n, ptrs, lens, rl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
            ctypes.cast(ctypes.c_char_p(pat), ctypes.c_void_p), len(pat), _lib.SEARCH_ICASE if icase else 0, max_lines, max_line,
            dig.ctypes.data_as(ctypes.c_void_p), status, count, first, lines, rec, rec_cap, ctypes.byref(rec_used),
            text.ctypes.data_as(ctypes.c_void_p), text_cap, ctypes.byref(text_used)))
        return self._lines_result(n, status, dig, count, first, lines, rec, rec_used.value, bytes(text[:text_used.value]))

    def search_regex(self, frames, raw_lens, regex, icase=False, expect=None):
        """search() with a regular expression (include/zarc_gpu.h has the dialect) in place of the fixed string: count = the positions at
        which a match starts inside its line, first = the lowest of them.  A bad expression raises with code E_PARAM, one whose automaton
        needs more than 64 states with E_UNSUPPORTED."""
        return self.search(frames, raw_lens, regex, icase, expect, _fn="zarc_gpu_search_regex_batch")

    def search_regex_lines(self, frames, raw_lens, regex, icase=False, expect=None, max_lines=0, max_line=4096, rec_cap=4096, invert=False, before=0, after=0):
        """search_lines() with a regular expression -> (results, records); a record's match is the lowest matching start of its line"""
        return self.search_lines(frames, raw_lens, regex, icase, expect, max_lines, max_line, rec_cap, _fn="zarc_gpu_search_regex_lines_batch",
                                 invert=invert, before=before, after=after)

    def search_regex_device(self, d_frames, frame_off, frame_len, raw_len, regex, icase=False, expect=None):
        """search_device() with a regular expression (host memory)"""
        return self.search_device(d_frames, frame_off, frame_len, raw_len, regex, icase, expect, _fn="zarc_gpu_search_regex_batch_device")

    def search_regex_lines_device(self, d_frames, frame_off, frame_len, raw_len, regex, icase=False, expect=None, max_lines=0, max_line=4096, rec_cap=4096,
                                  invert=False, before=0, after=0):
        """search_lines_device() with a regular expression (host memory)"""
        return self.search_lines_device(d_frames, frame_off, frame_len, raw_len, regex, icase, expect, max_lines, max_line, rec_cap,
                                        _fn="zarc_gpu_search_regex_lines_batch_device", invert=invert, before=before, after=after)

    def regex_compile(self, regex, icase=False):
        """-> (states, start, accept, delta): the table the device walks for `regex`, a line's bytes from the last to the first; accept and
        delta are bytes objects of `states` and `states * 256` entries.  Raises as search_regex() does.  Needs no device."""
        return regex_compile(self.lib, regex, icase)

    def search_set(self, frames, raw_lens, patterns, icase=False, expect=None):
        """search() for a set of 1..1024 fixed byte strings in ONE pass -> (results, hits).  results[i] = (status, digest, count, first,
        which): count = the start positions at which at least one pattern matches (a position counts once), first the lowest of them,
        which the lowest index of a pattern matching there (both None without a match).  hits[k] = the positions at which pattern k
        matches, summed over the frames of the call.  The frame-end rule is per pattern."""
        n = len(frames)
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        count, first, which = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        ps = _lib.PatternSet.of(patterns)
        hits = (ctypes.c_uint64 * max(ps.count, 1))()
        self._check(self.lib.zarc_gpu_search_set_batch(self.h, n, ptrs, lens, rl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
                                                       ctypes.byref(ps), _lib.SEARCH_ICASE if icase else 0, dig.ctypes.data_as(ctypes.c_void_p), status,
                                                       count, first, which, hits))
        return self._set_result(n, status, dig, count, first, which), [int(v) for v in hits[:ps.count]]

    def search_set_lines(self, frames, raw_lens, patterns, icase=False, expect=None, max_lines=0, max_line=4096, rec_cap=4096, invert=False, before=0, after=0):
        """search_lines() for a set of patterns -> (results, records, hits).  results[i] = (status, digest, count, first, which, lines) with
        search_set()'s meaning; a line matches when a matching start position of ANY pattern lies in it, and a record's match is the lowest
        such position of its line.  No pattern may contain 0x0A.  records and the caps are search_lines()'s, invert / before / after too."""
        if invert or before or after:
            return self.select_lines(frames, raw_lens, _lib.MATCH_SET, patterns, icase, expect, max_lines, max_line, rec_cap, invert, before, after)
        n = len(frames)
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        count, first, which, lines = ((ctypes.c_uint64 * n)() for _ in range(4))
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        ps = _lib.PatternSet.of(patterns)
        hits = (ctypes.c_uint64 * max(ps.count, 1))()
        rec = (_lib.Line * max(rec_cap, 1))()
        rec_used, text_used = ctypes.c_size_t(), ctypes.c_size_t()
        text_cap = rec_cap * max_line
        text = np.empty(max(text_cap, 1), dtype=np.uint8)
        self._check(self.lib.zarc_gpu_search_set_lines_batch(
            self.h, n, ptrs, lens, rl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
            ctypes.byref(ps), _lib.SEARCH_ICASE if icase else 0, max_lines, max_line,
            dig.ctypes.data_as(ctypes.c_void_p), status, count, first, which, hits, lines, rec, rec_cap, ctypes.byref(rec_used),
            text.ctypes.data_as(ctypes.c_void_p), text_cap, ctypes.byref(text_used)))
        return self._set_lines_result(n, status, dig, count, first, which, lines, rec, rec_used.value, bytes(text[:text_used.value])) + ([int(v) for v in hits[:ps.count]],)

    # ---- the selected lines (zarc_gpu_select_lines_batch*): one call behind the three matchers ----
    @staticmethod
    def _select_result(kind, n, status, dig, count, first, which, hits, lines, selected, rec, rec_used, text):
        none = lambda v: None if int(v) == _lib.SEARCH_NONE else int(v)
        mid = (lambda i: (none(which[i]),)) if kind == _lib.MATCH_SET else (lambda i: ())
        results = [(int(status[i]), bytes(dig[i]), int(count[i]), none(first[i])) + mid(i) + (int(lines[i]), int(selected[i])) for i in range(n)]
        records = [(r.frame, r.start, r.length, r.number, none(r.match), text[r.text_off:r.text_off + r.text_len]) for r in rec[:rec_used]]
        return results, records, ([int(v) for v in hits] if kind == _lib.MATCH_SET else None)

    def select_lines(self, frames, raw_lens, kind, what, icase=False, expect=None, max_lines=0, max_line=4096, rec_cap=4096, invert=False, before=0, after=0):
        """The lines a search selects -> (results, records, hits).  kind: _lib.MATCH_FIXED / MATCH_REGEX (what: bytes) or MATCH_SET (what: a
        list of bytes).  results[i] = (status, digest, count, first[, which], lines, selected): the matcher's plain search answer, the hit
        lines (matching lines, with invert the others) and the selected lines (hits plus `before` lines in front and `after` behind each).
        records = the selected lines as search_lines() delivers matching lines, match None for a line without a match; hits: a set's
        per-pattern counts, else None."""
        n = len(frames)
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        count, first, which, lines, selected = ((ctypes.c_uint64 * n)() for _ in range(5))
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        m = _lib.MatcherDesc.of(kind, what, _lib.SEARCH_ICASE if icase else 0)
        q = _lib.LineSelect(_lib.SELECT_INVERT if invert else 0, before, after, 0)
        is_set = kind == _lib.MATCH_SET
        hits = (ctypes.c_uint64 * max(len(what), 1))() if is_set else None
        rec = (_lib.Line * max(rec_cap, 1))()
        rec_used, text_used = ctypes.c_size_t(), ctypes.c_size_t()
        text_cap = rec_cap * max_line
        text = np.empty(max(text_cap, 1), dtype=np.uint8)
        self._check(self.lib.zarc_gpu_select_lines_batch(
            self.h, n, ptrs, lens, rl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None, ctypes.byref(m), ctypes.byref(q), max_lines, max_line,
            dig.ctypes.data_as(ctypes.c_void_p), status, count, first, which if is_set else None, hits, lines, selected, rec, rec_cap, ctypes.byref(rec_used),
            text.ctypes.data_as(ctypes.c_void_p), text_cap, ctypes.byref(text_used)))
        return self._select_result(kind, n, status, dig, count, first, which, hits[:len(what)] if is_set else None, lines, selected, rec, rec_used.value,
                                   bytes(text[:text_used.value]))

    def select_lines_device(self, d_frames, frame_off, frame_len, raw_len, kind, what, icase=False, expect=None, max_lines=0, max_line=4096, rec_cap=4096,
                            invert=False, before=0, after=0):
        """select_lines() over frames on the device; the text is gathered into a device buffer of rec_cap * max_line bytes and copied back"""
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        raw_len, prl = _u64(raw_len)
        n = len(frame_off)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        count, first, which, lines, selected = ((ctypes.c_uint64 * max(n, 1))() for _ in range(5))
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        m = _lib.MatcherDesc.of(kind, what, _lib.SEARCH_ICASE if icase else 0)
        q = _lib.LineSelect(_lib.SELECT_INVERT if invert else 0, before, after, 0)
        is_set = kind == _lib.MATCH_SET
        hits = (ctypes.c_uint64 * max(len(what), 1))() if is_set else None
        rec = (_lib.Line * max(rec_cap, 1))()
        rec_used, text_used = ctypes.c_size_t(), ctypes.c_size_t()
        text_cap = rec_cap * max_line
        d_text = self.malloc(max(text_cap, 1))
        try:
            self._check(self.lib.zarc_gpu_select_lines_batch_device(
                self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, prl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None, ctypes.byref(m),
                ctypes.byref(q), max_lines, max_line, dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), count, first,
                which if is_set else None, hits, lines, selected, rec, rec_cap, ctypes.byref(rec_used), ctypes.c_void_p(d_text), text_cap, ctypes.byref(text_used)))
            text = bytes(self.d2h(d_text, text_used.value)) if text_used.value else b""
        finally:
            self.free(d_text)
        return self._select_result(kind, n, status, dig, count, first, which, hits[:len(what)] if is_set else None, lines, selected, rec, rec_used.value, text)

    # ---- only the matches (zarc_gpu_search_matches_batch*): grep -o ----
    @staticmethod
    def _matches_result(kind, n, status, dig, count, first, which, hits, lines, matches, rec, rec_used, text):
        none = lambda v: None if int(v) == _lib.SEARCH_NONE else int(v)
        mid = (lambda i: (none(which[i]),)) if kind == _lib.MATCH_SET else (lambda i: ())
        results = [(int(status[i]), bytes(dig[i]), int(count[i]), none(first[i])) + mid(i) + (int(lines[i]), int(matches[i])) for i in range(n)]
        records = [(r.frame, r.start, r.length, r.number, r.line_start, none(r.which), text[r.text_off:r.text_off + r.text_len]) for r in rec[:rec_used]]
        return results, records, ([int(v) for v in hits] if kind == _lib.MATCH_SET else None)

    def search_matches(self, frames, raw_lens, kind, what, icase=False, expect=None, max_lines=0, max_line=4096, line_cap=4096, rec_cap=4096):
        """Every match of the matching lines, as grep -o cuts them out -> (results, records, hits).  kind / what as select_lines().
        results[i] = (status, digest, count, first[, which], lines, matches): the matcher's plain lines answer and the matches in the
        frame's first min(lines, max_lines, what line_cap leaves) matching lines.  records = (frame, start, length, number, line_start,
        which, text) per match in (frame, start) order, at most rec_cap of them; text: the match's first min(length, max_line) bytes;
        which: a set's pattern, else None.  hits: a set's per-pattern counts, else None."""
        n = len(frames)
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        count, first, which, lines, matches = ((ctypes.c_uint64 * n)() for _ in range(5))
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        m = _lib.MatcherDesc.of(kind, what, _lib.SEARCH_ICASE if icase else 0)
        is_set = kind == _lib.MATCH_SET
        hits = (ctypes.c_uint64 * max(len(what), 1))() if is_set else None
        rec = (_lib.Match * max(rec_cap, 1))()
        rec_used, text_used = ctypes.c_size_t(), ctypes.c_size_t()
        text_cap = rec_cap * max_line
        text = np.empty(max(text_cap, 1), dtype=np.uint8)
        self._check(self.lib.zarc_gpu_search_matches_batch(
            self.h, n, ptrs, lens, rl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None, ctypes.byref(m), max_lines, max_line, line_cap,
            dig.ctypes.data_as(ctypes.c_void_p), status, count, first, which if is_set else None, hits, lines, matches, rec, rec_cap, ctypes.byref(rec_used),
            text.ctypes.data_as(ctypes.c_void_p), text_cap, ctypes.byref(text_used)))
        return self._matches_result(kind, n, status, dig, count, first, which, hits[:len(what)] if is_set else None, lines, matches, rec, rec_used.value,
                                    bytes(text[:text_used.value]))

    def search_matches_device(self, d_frames, frame_off, frame_len, raw_len, kind, what, icase=False, expect=None, max_lines=0, max_line=4096, line_cap=4096,
                              rec_cap=4096):
        """search_matches() over frames on the device; the text is gathered into a device buffer of rec_cap * max_line bytes and copied back"""
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        raw_len, prl = _u64(raw_len)
        n = len(frame_off)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        count, first, which, lines, matches = ((ctypes.c_uint64 * max(n, 1))() for _ in range(5))
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        m = _lib.MatcherDesc.of(kind, what, _lib.SEARCH_ICASE if icase else 0)
        is_set = kind == _lib.MATCH_SET
        hits = (ctypes.c_uint64 * max(len(what), 1))() if is_set else None
        rec = (_lib.Match * max(rec_cap, 1))()
        rec_used, text_used = ctypes.c_size_t(), ctypes.c_size_t()
        text_cap = rec_cap * max_line
        d_text = self.malloc(max(text_cap, 1))
        try:
            self._check(self.lib.zarc_gpu_search_matches_batch_device(
                self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, prl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None, ctypes.byref(m),
                max_lines, max_line, line_cap, dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), count, first,
                which if is_set else None, hits, lines, matches, rec, rec_cap, ctypes.byref(rec_used), ctypes.c_void_p(d_text), text_cap, ctypes.byref(text_used)))
            text = bytes(self.d2h(d_text, text_used.value)) if text_used.value else b""
        finally:
            self.free(d_text)
        return self._matches_result(kind, n, status, dig, count, first, which, hits[:len(what)] if is_set else None, lines, matches, rec, rec_used.value, text)

    def regex_compile_ends(self, regex, icase=False):
        """-> (states, start, accept, delta): the FORWARD table a matches call walks from a match's first byte to find its end (layout:
        include/zarc_gpu.h, zarc_gpu_regex_compile_ends).  Raises as search_matches() does.  Needs no device."""
        return regex_compile(self.lib, regex, icase, ends=True)

    @staticmethod
    def _ranges(ranges, n):
        """-> the zarc_gpu_range array of `ranges`: one (unit, flags, skip, take) per frame"""
        assert len(ranges) == n, "one range per frame"
        arr = (_lib.Range * max(n, 1))()
        for i, (unit, flags, skip, take) in enumerate(ranges):
            arr[i].unit, arr[i].flags, arr[i].skip, arr[i].take = unit, flags, skip, take
        return arr

    @staticmethod
    def _range_result(n, res):
        return [(r.units, r.first, r.taken, r.start, r.length, r.text_off, r.text_len) for r in res[:n]]

    def read_ranges(self, frames, raw_lens, ranges, expect=None, max_bytes=0, text_cap=1 << 20):
        """verify() plus one byte or line range of every frame, cut out on the device -> (verdicts, res, text).  ranges[i] = (unit, flags,
        skip, take) with unit RANGE_BYTES / RANGE_LINES, flags 0 / RANGE_FROM_END, take RANGE_ALL for "all the rest" (include/zarc_gpu.h has
        the arithmetic).  verdicts = verify()'s list of (digest, status); res[i] = (units, first, taken, start, length, text_off,
        text_len): the first five are the truth whatever the caps, the frame's delivered bytes are text[text_off:text_off + text_len] --
        the first min(length, max_bytes or all, what text_cap leaves) of its range.  Only the compressed frames cross to the device and
        only len(text) bytes come back."""
        n = len(frames)
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        rng = self._ranges(ranges, n)
        res = (_lib.RangeResult * max(n, 1))()
        text = np.empty(max(text_cap, 1), dtype=np.uint8)
        text_used = ctypes.c_size_t()
        self._check(self.lib.zarc_gpu_read_ranges_batch(
            self.h, n, ptrs, lens, rl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None, rng, max_bytes,
            dig.ctypes.data_as(ctypes.c_void_p), status, res, text.ctypes.data_as(ctypes.c_void_p), text_cap, ctypes.byref(text_used)))
        return [(bytes(dig[i]), int(status[i])) for i in range(n)], self._range_result(n, res), bytes(text[:text_used.value])

    def read_ranges_device(self, d_frames, frame_off, frame_len, raw_len, ranges, expect=None, max_bytes=0, text_cap=1 << 20):
        """read_ranges() over frames resident on the device -> (verdicts, res, text).  The text is gathered into a device buffer of
        text_cap bytes and copied back from there."""
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        raw_len, prl = _u64(raw_len)
        n = len(frame_off)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        rng = self._ranges(ranges, n)
        res = (_lib.RangeResult * max(n, 1))()
        text_used = ctypes.c_size_t()
        d_text = self.malloc(max(text_cap, 1))
        try:
            self._check(self.lib.zarc_gpu_read_ranges_batch_device(
                self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, prl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None, rng, max_bytes,
                dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), res, ctypes.c_void_p(d_text), text_cap,
                ctypes.byref(text_used)))
            text = bytes(self.d2h(d_text, text_used.value)) if text_used.value else b""
        finally:
            self.free(d_text)
        return [(bytes(dig[i]), int(status[i])) for i in range(n)], self._range_result(n, res), text

    @staticmethod
    def _wc_result(n, res):
        return [(r.lines, r.words, r.chars, r.max_line, r.max_line_start, r.max_line_no) for r in res[:n]]

    def count(self, frames, raw_lens, expect=None):
        """verify() plus what `wc` says of every frame, counted on the device -> (verdicts, counts).  verdicts = verify()'s list of
        (digest, status); counts[i] = (lines, words, chars, max_line, max_line_start, max_line_no): 0x0A bytes, runs of bytes that are
        not white space, bytes that are no UTF-8 continuation byte, the byte length of the longest line, where the lowest such line
        starts and its 1-based number (include/zarc_gpu.h has the definitions).  A frame that did not decode gives zeros.  Only the
        compressed frames cross to the device and 64 bytes a frame come back."""
        n = len(frames)
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        res = (_lib.Wc * max(n, 1))()
        self._check(self.lib.zarc_gpu_count_batch(
            self.h, n, ptrs, lens, rl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
            dig.ctypes.data_as(ctypes.c_void_p), status, res))
        return [(bytes(dig[i]), int(status[i])) for i in range(n)], self._wc_result(n, res)

    def count_device(self, d_frames, frame_off, frame_len, raw_len, expect=None):
        """count() over frames resident on the device -> (verdicts, counts)"""
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        raw_len, prl = _u64(raw_len)
        n = len(frame_off)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        res = (_lib.Wc * max(n, 1))()
        self._check(self.lib.zarc_gpu_count_batch_device(
            self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, prl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
            dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), res))
        return [(bytes(dig[i]), int(status[i])) for i in range(n)], self._wc_result(n, res)

    @staticmethod
    def _cmp_result(n, res):
        return [(r.relation, r.prefix, r.line, r.differing, r.suffix, r.byte_a, r.byte_b) for r in res[:n]]

    def compare(self, frames, raw_lens, others, expect=None):
        """verify() plus what `cmp` says of every frame's content against others[i], compared on the device -> (verdicts, results).
        verdicts = verify()'s list of (digest, status); results[i] = (relation, prefix, line, differing, suffix, byte_a, byte_b): one of
        _lib.CMP_*, the offset of the first differing byte (the common length where there is none), 1 + the line feeds of the content
        in front of it, the number of differing bytes below the common length, the length of the common tail (which never overlaps
        the common head), and the two bytes at `prefix` (_lib.CMP_EOF where that side ends there); include/zarc_gpu.h has the
        definitions.  A frame that did not decode gives zeros.  The compressed frames and the other sides cross to the device and 64
        bytes a pair come back."""
        n = len(frames)
        assert len(others) == n
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        obufs = [bytes(o) for o in others]
        optrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in obufs])
        olens = (ctypes.c_size_t * n)(*[len(b) for b in obufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        res = (_lib.Cmp * max(n, 1))()
        self._check(self.lib.zarc_gpu_compare_batch(
            self.h, n, ptrs, lens, rl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None, optrs, olens,
            dig.ctypes.data_as(ctypes.c_void_p), status, res))
        return [(bytes(dig[i]), int(status[i])) for i in range(n)], self._cmp_result(n, res)

    def compare_device(self, d_frames, frame_off, frame_len, raw_len, d_other, other_off, other_len, expect=None):
        """compare() over frames and other sides resident on the device (other_off 16-byte aligned, _lib.PAD readable bytes behind
        the arena) -> (verdicts, results)"""
        frame_off, pfo = _u64(frame_off)
        frame_len, pfl = _u64(frame_len)
        raw_len, prl = _u64(raw_len)
        other_off, poo = _u64(other_off)
        other_len, pol = _u64(other_len)
        n = len(frame_off)
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(expect, dtype=np.uint8)
        res = (_lib.Cmp * max(n, 1))()
        self._check(self.lib.zarc_gpu_compare_batch_device(
            self.h, n, ctypes.c_void_p(d_frames), pfo, pfl, prl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
            ctypes.c_void_p(d_other), poo, pol, dig.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), res))
        return [(bytes(dig[i]), int(status[i])) for i in range(n)], self._cmp_result(n, res)

    def compare_ms(self):
        """device time of zarc_cmp_* of the most recent call, summed over its parts; <= 0 after any call but compare"""
        return float(self.lib.zarc_gpu_last_compare_ms(self.h))

    def repack(self, frames, raw_lens, expect=None):
        """-> (new_frames, digests, statuses).  Every frame is judged as verify() judges it; a frame with status 0 is encoded again with
        the handle's current parameters -- the bytes pack() makes of what unpack() delivers -- and every other one gives None.  Only the
        old frames cross to the device and only the new ones come back."""
        n = len(frames)
        bufs = [bytes(f) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        rl = (ctypes.c_size_t * n)(*[int(r) for r in raw_lens])
        cap = sum(self.bound(int(r)) for r in raw_lens)
        dst = np.zeros(max(cap, 1), dtype=np.uint8)
        dst_off, dst_len = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
        dig = np.zeros((n, 32), dtype=np.uint8)
        status = (ctypes.c_int * n)()
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(expect), dtype=np.uint8))
        self._check(self.lib.zarc_gpu_repack_batch(self.h, n, ptrs, lens, rl, exp.ctypes.data_as(ctypes.c_void_p) if exp is not None else None,
                                                   dst.ctypes.data_as(ctypes.c_void_p), cap, dst_off, dst_len, dig.ctypes.data_as(ctypes.c_void_p), status))
        new = [bytes(dst[dst_off[i]:dst_off[i] + dst_len[i]]) if status[i] == _lib.FRAME_OK else None for i in range(n)]
        return new, [bytes(d) for d in dig], [int(x) for x in status]


def regex_compile(lib, regex, icase=False, ends=False):
    """Engine.regex_compile (ends: regex_compile_ends) without a handle: `lib` is what _lib.load() returns"""
    pat = bytes(regex)
    dfa = _lib.RegexDfa()
    err = ctypes.create_string_buffer(512)
    rc = (lib.zarc_gpu_regex_compile_ends if ends else lib.zarc_gpu_regex_compile)(ctypes.cast(ctypes.c_char_p(pat), ctypes.c_void_p), len(pat), _lib.SEARCH_ICASE if icase else 0, ctypes.byref(dfa), err, len(err))
    if rc != _lib.OK:
        raise _lib.ZarcGpuError(rc, lib.zarc_gpu_error_name(rc).decode(), err.value.decode("latin-1"))
    return dfa.states, dfa.start, bytes(dfa.accept[:dfa.states]), bytes(dfa.delta[:dfa.states * 256])
