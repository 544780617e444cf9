"""ctypes binding of the C ABI in include/zarc_gpu.h (libzarc_gpu.so, built by zarc_amd/csrc/Makefile).

The library is the product: HIP kernels for gfx950 behind an extern "C" boundary.  There is no Python or
CPU implementation of the data path -- if the shared object is missing or no HIP device is usable this
module raises instead of degrading.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libzarc_gpu.so")

ABI_VERSION = 2  # include/zarc_gpu.h: ZARC_GPU_ABI_VERSION
DIGEST_LEN = 32
ALIGN = 16
PAD = 64

# call-level errors
OK, E_DEVICE, E_NOMEM, E_PARAM, E_UNSUPPORTED, E_DSTSIZE, E_CHECK = 0, -1, -2, -3, -4, -5, -6
# per-frame status
FRAME_OK, FRAME_CORRUPT, FRAME_CHECKSUM, FRAME_DIGEST, FRAME_DSTSIZE, FRAME_BAD_MAGIC, FRAME_UNSUPPORTED, FRAME_SRCSIZE, FRAME_DUPLICATE = range(9)
# parameter ids (ZSTD_cParameter values, what zstd_safe::CParameter maps to)
P_COMPRESSION_LEVEL, P_WINDOW_LOG, P_HASH_LOG, P_CHAIN_LOG, P_SEARCH_LOG, P_MIN_MATCH, P_TARGET_LENGTH, P_STRATEGY = 100, 101, 102, 103, 104, 105, 106, 107
P_ENABLE_LDM, P_LDM_HASH_LOG, P_LDM_MIN_MATCH, P_LDM_BUCKET_SIZE_LOG, P_LDM_HASH_RATE_LOG = 160, 161, 162, 163, 164
P_CONTENT_SIZE_FLAG, P_CHECKSUM_FLAG, P_DICT_ID_FLAG = 200, 201, 202
# engine tuning (batching only; frames are identical for every value)
PX_SCRATCH_MB, PX_STAGE_CHUNK, PX_STAGE_THREAD, PX_COPY_THREADS, PX_DEC_GROUPS, PX_ZERO_COPY = 9001, 9002, 9003, 9004, 9005, 9006
# ... and the one engine switch that DOES change the frames: 1 = 64 KiB blocks are cut where their literal statistics change (default 0)
PX_BLOCK_SPLIT = 9007
# read-back check of pack: 1 = every frame of a pack call is decoded again and compared with its source before the call returns (default 0)
PX_CHECK_FRAMES = 9008
# pack: 1 (default) = the FSE state chains of blocks that share their tables run on one wave per 1 MiB group; 0 = per block; N > 1 = as 1
# for blocks of fewer than N sequences.  Frames are identical for every value
PX_SEQ_STATES = 9009
# zarc_gpu_last_copy_bytes: content bytes the most recent batch call moved over PCIe
C_H2D, C_D2H, C_RING, C_DIRECT = range(4)
# timers
T_BLAKE3, T_XXH64, T_MATCH, T_ENTROPY, T_ASSEMBLE, T_DECODE, T_TOTAL, T_DEC_SEQS, T_DEC_LITS, T_DEC_FRAMES = range(10)
T_SEARCH = 10  # zarc_search_scan of a search call (summed over its parts)
T_LINES = 11   # zarc_lines_* of a search_lines call (summed over its parts)
# zarc_gpu_search_batch*: flags, the longest pattern, first[i] of a frame without a match
SEARCH_ICASE, SEARCH_MAX_PATTERN, SEARCH_NONE = 1, 256, 2 ** 64 - 1
SEARCH_MAX_SET = 1024  # zarc_gpu_search_set_*: the largest set
LINES_MAX_LINE = 65536  # zarc_gpu_search_lines_batch*: the largest max_line
MATCH_FIXED, MATCH_SET, MATCH_REGEX = 0, 1, 2  # zarc_gpu_select_lines_batch*: zarc_gpu_matcher.kind
SELECT_INVERT = 1  # ... and zarc_gpu_line_select.flags
REGEX_MAX_PATTERN, REGEX_MAX_STATES = 1024, 64  # zarc_gpu_search_regex_*: the longest expression, the most states of its automaton
T_RANGE = 12   # zarc_range_* of a read_ranges call (summed over its parts)
# zarc_gpu_read_ranges_batch*: zarc_gpu_range.unit, .flags, and the take that means "all the rest"
RANGE_BYTES, RANGE_LINES, RANGE_FROM_END, RANGE_ALL = 0, 1, 1, 2 ** 64 - 1
T_WC = 13      # zarc_wc_* of a count call (summed over its parts)
T_COUNT = 14   # the number of timers
# zarc_gpu_compare_batch*: zarc_gpu_cmp.relation, and byte_a / byte_b where that side has no byte at `prefix`
CMP_NONE, CMP_EQUAL, CMP_DIFFER, CMP_FRAME_IS_PREFIX, CMP_OTHER_IS_PREFIX = 0, 1, 2, 3, 4
CMP_EOF = 256

EXPORTS = [
    "zarc_gpu_abi_version", "zarc_gpu_level_finder", "zarc_gpu_parameter_advisory", "zarc_gpu_device_count", "zarc_gpu_create", "zarc_gpu_destroy", "zarc_gpu_set_parameter", "zarc_gpu_get_params",
    "zarc_gpu_enable_compression", "zarc_gpu_bound", "zarc_gpu_error_name", "zarc_gpu_frame_status_name", "zarc_gpu_last_error",
    "zarc_gpu_pack_batch", "zarc_gpu_pack_batch_device", "zarc_gpu_pack_batch_dedup", "zarc_gpu_pack_batch_device_dedup", "zarc_gpu_unpack_batch", "zarc_gpu_unpack_batch_device",
    "zarc_gpu_verify_batch", "zarc_gpu_verify_batch_device", "zarc_gpu_last_copy_bytes", "zarc_gpu_repack_batch", "zarc_gpu_repack_batch_device",
    "zarc_gpu_search_batch", "zarc_gpu_search_batch_device", "zarc_gpu_search_lines_batch", "zarc_gpu_search_lines_batch_device",
    "zarc_gpu_search_set_batch", "zarc_gpu_search_set_batch_device", "zarc_gpu_search_set_lines_batch", "zarc_gpu_search_set_lines_batch_device",
    "zarc_gpu_regex_compile", "zarc_gpu_search_regex_batch", "zarc_gpu_search_regex_batch_device", "zarc_gpu_search_regex_lines_batch",
    "zarc_gpu_search_regex_lines_batch_device", "zarc_gpu_select_lines_batch", "zarc_gpu_select_lines_batch_device",
    "zarc_gpu_regex_compile_ends", "zarc_gpu_search_matches_batch", "zarc_gpu_search_matches_batch_device",
    "zarc_gpu_read_ranges_batch", "zarc_gpu_read_ranges_batch_device", "zarc_gpu_count_batch", "zarc_gpu_count_batch_device",
    "zarc_gpu_compare_batch", "zarc_gpu_compare_batch_device", "zarc_gpu_last_compare_ms",
    "zarc_gpu_blake3_batch", "zarc_gpu_blake3_batch_device", "zarc_gpu_xxh64_batch_device", "zarc_gpu_last_kernel_ms",
    "zarc_gpu_corpus_fill_device", "zarc_gpu_device_malloc", "zarc_gpu_device_free", "zarc_gpu_memcpy_h2d", "zarc_gpu_memcpy_d2h",
]


# int known(void *ctx, const uint8_t digest[32], size_t index): nonzero = the caller has this content already (hash-first dedup)
KNOWN_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t)


class Params(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("level", "checksum_flag", "content_size_flag", "window_log", "hash_log", "chain_log",
                                            "search_log", "min_match", "target_length", "strategy", "compress")]


class Line(ctypes.Structure):
    """zarc_gpu_line: one matching line of a search_lines call"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("frame", "start", "length", "number", "match", "text_off", "text_len")]


class Match(ctypes.Structure):
    """zarc_gpu_match: one match of a search_matches call"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("frame", "start", "length", "number", "line_start", "which", "text_off", "text_len")]


class PatternSet(ctypes.Structure):
    """zarc_gpu_pattern_set: the patterns of a search_set call (host memory)"""
    _fields_ = [("bytes", ctypes.c_void_p), ("off", ctypes.POINTER(ctypes.c_uint64)), ("len", ctypes.POINTER(ctypes.c_uint64)), ("count", ctypes.c_size_t)]

    @classmethod
    def of(cls, patterns):
        """-> the structure over `patterns` (a list of bytes); it keeps what it points to alive"""
        pats = [bytes(p) for p in patterns]
        n = len(pats)
        s = cls()
        s._blob = ctypes.create_string_buffer(b"".join(pats), max(sum(len(p) for p in pats), 1))
        s._off = (ctypes.c_uint64 * max(n, 1))()
        s._len = (ctypes.c_uint64 * max(n, 1))()
        at = 0
        for k, p in enumerate(pats):
            s._off[k], s._len[k] = at, len(p)
            at += len(p)
        s.bytes, s.off, s.len, s.count = ctypes.cast(s._blob, ctypes.c_void_p), s._off, s._len, n
        return s


class MatcherDesc(ctypes.Structure):
    """zarc_gpu_matcher: what a select_lines call searches for (host memory)"""
    _fields_ = [("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("text", ctypes.c_void_p), ("text_len", ctypes.c_size_t), ("set", ctypes.POINTER(PatternSet))]

    @classmethod
    def of(cls, kind, what, flags=0):
        """-> the structure over `what` (FIXED / REGEX: bytes; SET: a list of bytes); it keeps what it points to alive"""
        m = cls()
        m.kind, m.flags = kind, flags
        if kind == MATCH_SET:
            m._set = PatternSet.of(what)
            m.set = ctypes.pointer(m._set)
        else:
            m._text = ctypes.create_string_buffer(bytes(what), max(len(what), 1))
            m.text, m.text_len = ctypes.cast(m._text, ctypes.c_void_p), len(what)
        return m


class LineSelect(ctypes.Structure):
    """zarc_gpu_line_select: which lines a select_lines call delivers"""
    _fields_ = [(n, ctypes.c_uint32) for n in ("flags", "before", "after", "reserved")]


class Range(ctypes.Structure):
    """zarc_gpu_range: the range of one frame of a read_ranges call (host memory)"""
    _fields_ = [("unit", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("skip", ctypes.c_uint64), ("take", ctypes.c_uint64)]


class RangeResult(ctypes.Structure):
    """zarc_gpu_range_result: what a read_ranges call found and delivered of one frame"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("units", "first", "taken", "start", "length", "text_off", "text_len", "reserved")]


class Wc(ctypes.Structure):
    """zarc_gpu_wc: what a count call found of one frame"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("lines", "words", "chars", "max_line", "max_line_start", "max_line_no")] + [("reserved", ctypes.c_uint64 * 2)]


class Cmp(ctypes.Structure):
    """zarc_gpu_cmp: what a compare call found of one pair"""
    _fields_ = [(n, ctypes.c_uint32) for n in ("relation", "byte_a", "byte_b", "reserved0")] + \
               [(n, ctypes.c_uint64) for n in ("prefix", "line", "differing", "suffix")] + [("reserved", ctypes.c_uint64 * 2)]


class RegexDfa(ctypes.Structure):
    """zarc_gpu_regex_dfa: the table zarc_gpu_regex_compile makes; it reads a line from its last byte to its first"""
    _fields_ = [("states", ctypes.c_uint32), ("start", ctypes.c_uint32), ("accept", ctypes.c_uint8 * 64), ("delta", ctypes.c_uint8 * (64 * 256))]


class ZarcGpuError(RuntimeError):
    def __init__(self, code, name, detail=""):
        super().__init__("%s (%d)%s" % (name, code, (": " + detail) if detail else ""))
        self.code = code


def load(path=None):
    """Load the shared library and declare every entry point.  Raises OSError if it is not built."""
    path = path or os.environ.get("ZARC_GPU_LIB") or DEFAULT_LIB
    if not os.path.exists(path):
        raise OSError("libzarc_gpu.so not found at %s -- build it with `make -C zarc_amd/csrc` "
                      "(or __graft_entry__.build()); there is no CPU fallback" % path)
    lib = ctypes.CDLL(path)
    c = ctypes
    vp, sz, u64p, u8p, ip = c.c_void_p, c.c_size_t, c.POINTER(c.c_uint64), c.POINTER(c.c_uint8), c.POINTER(c.c_int)
    szp, vpp = c.POINTER(c.c_size_t), c.POINTER(c.c_void_p)
    lib.zarc_gpu_abi_version.restype = c.c_int
    got = lib.zarc_gpu_abi_version()
    if got != ABI_VERSION:  # checked BEFORE the newer symbols are resolved: a stale library fails here, by version, not at a symbol lookup
        raise OSError("%s has ABI version %d, this binding needs %d -- rebuild it (make -C zarc_amd/csrc)" % (path, got, ABI_VERSION))
    lib.zarc_gpu_device_count.restype = c.c_int
    lib.zarc_gpu_level_finder.argtypes = [c.c_int]
    lib.zarc_gpu_parameter_advisory.argtypes = [c.c_int]
    lib.zarc_gpu_create.argtypes = [c.POINTER(vp), c.c_int]
    lib.zarc_gpu_destroy.argtypes = [vp]
    lib.zarc_gpu_destroy.restype = None
    lib.zarc_gpu_set_parameter.argtypes = [vp, c.c_int, c.c_int]
    lib.zarc_gpu_get_params.argtypes = [vp, c.POINTER(Params)]
    lib.zarc_gpu_get_params.restype = None
    lib.zarc_gpu_enable_compression.argtypes = [vp, c.c_int]
    lib.zarc_gpu_enable_compression.restype = None
    lib.zarc_gpu_bound.argtypes = [sz]
    lib.zarc_gpu_bound.restype = sz
    for f in (lib.zarc_gpu_error_name, lib.zarc_gpu_frame_status_name):
        f.argtypes = [c.c_int]
        f.restype = c.c_char_p
    lib.zarc_gpu_last_error.argtypes = [vp]
    lib.zarc_gpu_last_error.restype = c.c_char_p
    lib.zarc_gpu_pack_batch.argtypes = [vp, sz, vpp, szp, vp, sz, szp, szp, vp, ip]
    lib.zarc_gpu_pack_batch_device.argtypes = [vp, sz, vp, u64p, u64p, vp, sz, u64p, u64p, vp, ip]
    lib.zarc_gpu_pack_batch_dedup.argtypes = [vp, sz, vpp, szp, vp, sz, szp, szp, vp, ip, KNOWN_FN, vp]
    lib.zarc_gpu_pack_batch_device_dedup.argtypes = [vp, sz, vp, u64p, u64p, vp, sz, u64p, u64p, vp, ip, KNOWN_FN, vp]
    lib.zarc_gpu_unpack_batch.argtypes = [vp, sz, vpp, szp, szp, vpp, vp, vp, ip]
    lib.zarc_gpu_unpack_batch_device.argtypes = [vp, sz, vp, u64p, u64p, vp, u64p, u64p, vp, vp, ip]
    lib.zarc_gpu_verify_batch.argtypes = [vp, sz, vpp, szp, szp, vp, vp, ip]
    lib.zarc_gpu_verify_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p, vp, vp, ip]
    lib.zarc_gpu_repack_batch.argtypes = [vp, sz, vpp, szp, szp, vp, vp, sz, szp, szp, vp, ip]
    lib.zarc_gpu_repack_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p, vp, vp, sz, u64p, u64p, vp, ip]
    lib.zarc_gpu_search_batch.argtypes = [vp, sz, vpp, szp, szp, vp, vp, sz, c.c_uint, vp, ip, u64p, u64p]
    lib.zarc_gpu_search_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p, vp, vp, sz, c.c_uint, vp, ip, u64p, u64p]
    lp = c.POINTER(Line)
    lib.zarc_gpu_search_lines_batch.argtypes = [vp, sz, vpp, szp, szp, vp, vp, sz, c.c_uint, c.c_uint64, c.c_uint64, vp, ip, u64p, u64p, u64p, lp, sz, szp, vp, sz, szp]
    lib.zarc_gpu_search_lines_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p, vp, vp, sz, c.c_uint, c.c_uint64, c.c_uint64, vp, ip, u64p, u64p, u64p, lp, sz,
                                                       szp, vp, sz, szp]
    sp = c.POINTER(PatternSet)
    lib.zarc_gpu_search_set_batch.argtypes = [vp, sz, vpp, szp, szp, vp, sp, c.c_uint, vp, ip, u64p, u64p, u64p, u64p]
    lib.zarc_gpu_search_set_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p, vp, sp, c.c_uint, vp, ip, u64p, u64p, u64p, u64p]
    lib.zarc_gpu_search_set_lines_batch.argtypes = [vp, sz, vpp, szp, szp, vp, sp, c.c_uint, c.c_uint64, c.c_uint64, vp, ip, u64p, u64p, u64p, u64p, u64p, lp, sz,
                                                    szp, vp, sz, szp]
    lib.zarc_gpu_search_set_lines_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p, vp, sp, c.c_uint, c.c_uint64, c.c_uint64, vp, ip, u64p, u64p, u64p, u64p, u64p,
                                                           lp, sz, szp, vp, sz, szp]
    lib.zarc_gpu_regex_compile.argtypes = [vp, sz, c.c_uint, c.POINTER(RegexDfa), c.c_char_p, sz]
    lib.zarc_gpu_search_regex_batch.argtypes = lib.zarc_gpu_search_batch.argtypes
    lib.zarc_gpu_search_regex_batch_device.argtypes = lib.zarc_gpu_search_batch_device.argtypes
    lib.zarc_gpu_search_regex_lines_batch.argtypes = lib.zarc_gpu_search_lines_batch.argtypes
    lib.zarc_gpu_search_regex_lines_batch_device.argtypes = lib.zarc_gpu_search_lines_batch_device.argtypes
    mp, qp = c.POINTER(MatcherDesc), c.POINTER(LineSelect)
    lib.zarc_gpu_select_lines_batch.argtypes = [vp, sz, vpp, szp, szp, vp, mp, qp, c.c_uint64, c.c_uint64, vp, ip, u64p, u64p, u64p, u64p, u64p, u64p, lp, sz, szp,
                                                vp, sz, szp]
    lib.zarc_gpu_select_lines_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p, vp, mp, qp, c.c_uint64, c.c_uint64, vp, ip, u64p, u64p, u64p, u64p, u64p, u64p,
                                                       lp, sz, szp, vp, sz, szp]
    lib.zarc_gpu_regex_compile_ends.argtypes = lib.zarc_gpu_regex_compile.argtypes
    xp = c.POINTER(Match)
    lib.zarc_gpu_search_matches_batch.argtypes = [vp, sz, vpp, szp, szp, vp, mp, c.c_uint64, c.c_uint64, sz, vp, ip, u64p, u64p, u64p, u64p, u64p, u64p, xp, sz, szp,
                                                  vp, sz, szp]
    lib.zarc_gpu_search_matches_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p, vp, mp, c.c_uint64, c.c_uint64, sz, vp, ip, u64p, u64p, u64p, u64p, u64p, u64p,
                                                         xp, sz, szp, vp, sz, szp]
    rp, rrp = c.POINTER(Range), c.POINTER(RangeResult)
    lib.zarc_gpu_read_ranges_batch.argtypes = [vp, sz, vpp, szp, szp, vp, rp, c.c_uint64, vp, ip, rrp, vp, sz, szp]
    lib.zarc_gpu_read_ranges_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p, vp, rp, c.c_uint64, vp, ip, rrp, vp, sz, szp]
    wp = c.POINTER(Wc)
    lib.zarc_gpu_count_batch.argtypes = [vp, sz, vpp, szp, szp, vp, vp, ip, wp]
    lib.zarc_gpu_count_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p, vp, vp, ip, wp]
    cp = c.POINTER(Cmp)
    lib.zarc_gpu_compare_batch.argtypes = [vp, sz, vpp, szp, szp, vp, vpp, szp, vp, ip, cp]
    lib.zarc_gpu_compare_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p, vp, vp, u64p, u64p, vp, ip, cp]
    lib.zarc_gpu_last_compare_ms.argtypes = [vp]
    lib.zarc_gpu_last_compare_ms.restype = c.c_float
    lib.zarc_gpu_last_copy_bytes.argtypes = [vp, c.c_int]
    lib.zarc_gpu_last_copy_bytes.restype = c.c_uint64
    lib.zarc_gpu_blake3_batch.argtypes = [vp, sz, vpp, szp, vp]
    lib.zarc_gpu_blake3_batch_device.argtypes = [vp, sz, vp, u64p, u64p, vp]
    lib.zarc_gpu_xxh64_batch_device.argtypes = [vp, sz, vp, u64p, u64p, u64p]
    lib.zarc_gpu_last_kernel_ms.argtypes = [vp, c.c_int]
    lib.zarc_gpu_last_kernel_ms.restype = c.c_float
    lib.zarc_gpu_corpus_fill_device.argtypes = [vp, sz, vp, u64p, u64p, c.c_uint64, c.c_int]
    lib.zarc_gpu_device_malloc.argtypes = [vp, c.POINTER(vp), sz]
    lib.zarc_gpu_device_free.argtypes = [vp, vp]
    lib.zarc_gpu_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    lib.zarc_gpu_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    return lib
