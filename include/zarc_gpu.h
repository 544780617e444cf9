/*
 * zarc_gpu.h -- C ABI of the MI355X (gfx950) content engine for the Zarc archive format.
 *
 * This is the drop-in boundary for the ONE hot path of passcod/zarc: the per-entry content pipeline
 * (BLAKE3 content digest + Zstandard frame encode/decode + XXH64 frame checksum).  Every entry point
 * names the reference interface it replaces (paths relative to the reference tree):
 *
 *   pack   : Encoder::add_data_frame            crates/zarc/src/encode/content_frame.rs:20-60
 *            Encoder::write_compressed_frame    crates/zarc/src/encode/lowlevel_frames.rs:19-39
 *   unpack : Decoder::read_content_frame        crates/zarc/src/decode/frame_iterator.rs:14-27
 *            FrameIterator::{next,digest,verify} crates/zarc/src/decode/frame_iterator.rs:38-104
 *            ZstdFrameIterator::decompress_step crates/zarc/src/decode/zstd_iterator.rs:88-153
 *   verify : FrameIterator::verify for a batch, without the bytes   crates/zarc/src/decode/frame_iterator.rs:83-88 (and what
 *            `zarc unpack` does with its answer, crates/zarc-cli/src/unpack.rs:118-120)
 *   repack : Decoder::read_content_frame        crates/zarc/src/decode/frame_iterator.rs:14-27   joined on the device to
 *            Encoder::add_data_frame            crates/zarc/src/encode/content_frame.rs:20-60    (the reference has no such call: it
 *            would read every entry out and add it again)
 *   digest : DigestType::verify_data            crates/zarc/src/integrity.rs:107-117
 *   ctx    : CCtx::try_create / init(0) / set_parameter / reset     crates/zarc/src/encode.rs:58-97
 *            DCtx::try_create                   crates/zarc/src/decode/zstd_iterator.rs:29
 *   errors : map_zstd_error / error::zstd       crates/zarc/src/lib.rs:27-30, decode/error.rs:35-38
 *
 * The reference processes one entry per call on one CPU thread; the engine takes a *batch* of entries
 * (frames are independent by construction: a fresh session per frame, content_frame.rs:37-39, and a
 * fresh DCtx per frame, zstd_iterator.rs:28-29) and runs them concurrently on one GPU.  Host plumbing
 * (dedup on digest, running offsets, directory, trailer) stays with the caller -- see INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes only; 0 = success, negative = ZARC_GPU_E_*; nothing throws or
 * aborts across this boundary; the callee never frees caller memory.  A handle is single-owner (one
 * host thread at a time), several handles may coexist.  There is NO CPU fallback: without a usable
 * HIP device zarc_gpu_create fails with ZARC_GPU_E_DEVICE.
 */
#ifndef ZARC_GPU_H
#define ZARC_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZARC_GPU_ABI_VERSION 2 /* 2: round 3's entry points (device_count, *_dedup, FRAME_DUPLICATE, PX_ZERO_COPY) + round 4's (warnings, levels).
                                  zarc_gpu_verify_batch*, zarc_gpu_last_copy_bytes, ZARC_GPU_PX_CHECK_FRAMES and ZARC_GPU_E_CHECK were added WITHOUT a new
                                  version (they are new symbols and new ids; nothing older changed): a library from before them fails a caller
                                  that wants them at the symbol lookup, not by version.  zarc_gpu_repack_batch* joined them the same way, for the
                                  same reason, and zarc_gpu_search_batch* with ZARC_GPU_T_SEARCH after them (ZARC_GPU_T_COUNT grew from 10 to 11:
                                  zarc_gpu_last_kernel_ms of an older library answers < 0 for the new id, as for any id it does not know), and
                                  zarc_gpu_search_lines_batch* with ZARC_GPU_T_LINES after those (ZARC_GPU_T_COUNT grew from 11 to 12), then
                                  zarc_gpu_search_set_*, and zarc_gpu_regex_compile with zarc_gpu_search_regex_* (new symbols; ZARC_GPU_T_COUNT stays 12), then
                                  zarc_gpu_select_lines_batch* (new symbols and types; nothing existing changes), then zarc_gpu_search_matches_batch* with
                                  zarc_gpu_regex_compile_ends and zarc_gpu_match (the same: new symbols and one new type), then
                                  zarc_gpu_read_ranges_batch* with ZARC_GPU_T_RANGE (new symbols and types; ZARC_GPU_T_COUNT grew from 12 to 13), then
                                  zarc_gpu_count_batch* with zarc_gpu_wc and ZARC_GPU_T_WC (the same; ZARC_GPU_T_COUNT grew from 13 to 14), then
                                  zarc_gpu_compare_batch* with zarc_gpu_cmp and zarc_gpu_last_compare_ms (new symbols and one new type; ZARC_GPU_T_COUNT stays 14) */
#define ZARC_GPU_DIGEST_LEN 32  /* DigestType::digest_len(), crates/zarc/src/integrity.rs:100-104 */
#define ZARC_GPU_ALIGN 16       /* device-resident entries / outputs must start 16-byte aligned   */
#define ZARC_GPU_PAD 64         /* readable slack required after the last byte of a device arena   */

typedef struct zarc_gpu zarc_gpu_t;

/* call-level errors (return values) */
enum {
    ZARC_GPU_OK = 0,
    ZARC_GPU_E_DEVICE = -1,      /* HIP error or no device; text via zarc_gpu_last_error()          */
    ZARC_GPU_E_NOMEM = -2,       /* "failed allocating zstd context" analogue (encode.rs:61)        */
    ZARC_GPU_E_PARAM = -3,       /* bad argument / parameter out of bounds                          */
    ZARC_GPU_E_UNSUPPORTED = -4, /* parameter accepted by libzstd but not by this engine            */
    ZARC_GPU_E_DSTSIZE = -5,     /* dst_cap smaller than the sum of zarc_gpu_bound() of the entries */
    ZARC_GPU_E_CHECK = -6        /* pack with ZARC_GPU_PX_CHECK_FRAMES: a frame failed its read-back check; the batch's output is void */
};

/* per-frame status values (status[i]); names follow ZSTD_getErrorName where one exists */
enum {
    ZARC_GPU_FRAME_OK = 0,
    ZARC_GPU_FRAME_CORRUPT = 1,        /* "Data corruption detected"                                */
    ZARC_GPU_FRAME_CHECKSUM = 2,       /* "Restored data doesn't match checksum" (XXH64 mismatch)    */
    ZARC_GPU_FRAME_DIGEST = 3,         /* BLAKE3 != expected: REPORTED, not fatal (unpack.rs:118-120)*/
    ZARC_GPU_FRAME_DSTSIZE = 4,        /* "Destination buffer is too small"                          */
    ZARC_GPU_FRAME_BAD_MAGIC = 5,      /* "Unknown frame descriptor"                                 */
    ZARC_GPU_FRAME_UNSUPPORTED = 6,    /* dictionary id / window beyond the engine limit             */
    ZARC_GPU_FRAME_SRCSIZE = 7,        /* "Src size is incorrect" (frame shorter/longer than given)  */
    ZARC_GPU_FRAME_DUPLICATE = 8       /* pack, hash-first entry points only: content already known to the caller, nothing was compressed
                                          ("frame already exists, skipping", content_frame.rs:30-33); not an error                       */
};

/* Parameter ids are libzstd's ZSTD_cParameter values, which is what zstd_safe::CParameter maps to and
 * what `Encoder::set_zstd_parameter` (encode.rs:84-89) and `--zstd PARAM=VALUE` (zarc-cli/src/pack.rs:
 * 86-217) carry. */
enum {
    ZARC_GPU_P_COMPRESSION_LEVEL = 100,
    ZARC_GPU_P_WINDOW_LOG = 101,
    ZARC_GPU_P_HASH_LOG = 102,
    ZARC_GPU_P_CHAIN_LOG = 103,
    ZARC_GPU_P_SEARCH_LOG = 104,
    ZARC_GPU_P_MIN_MATCH = 105,
    ZARC_GPU_P_TARGET_LENGTH = 106,
    ZARC_GPU_P_STRATEGY = 107,
    ZARC_GPU_P_ENABLE_LDM = 160,
    ZARC_GPU_P_LDM_HASH_LOG = 161,
    ZARC_GPU_P_LDM_MIN_MATCH = 162,
    ZARC_GPU_P_LDM_BUCKET_SIZE_LOG = 163,
    ZARC_GPU_P_LDM_HASH_RATE_LOG = 164,
    ZARC_GPU_P_CONTENT_SIZE_FLAG = 200,
    ZARC_GPU_P_CHECKSUM_FLAG = 201,
    ZARC_GPU_P_DICT_ID_FLAG = 202,
    /* Engine tuning, not libzstd ids: how a batch is cut up, never what bytes come out (frames are identical for every value).
     * The library reads NO environment variable; these are the only switches. */
    ZARC_GPU_PX_SCRATCH_MB = 9001,   /* scratch budget in MiB (0 = encoder: up to 64 GiB / 45 % of free HBM; decoder: what the device has): batches beyond it run as sub-batches */
    ZARC_GPU_PX_STAGE_CHUNK = 9002,  /* host-pointer entry points: content bytes per staged chunk (0 = 2 GiB pack / 4 GiB unpack; >= 4096)         */
    ZARC_GPU_PX_STAGE_THREAD = 9003, /* 1 (default) = a helper thread moves neighbouring chunks over PCIe while the kernels run                     */
    ZARC_GPU_PX_COPY_THREADS = 9004, /* host threads that fill / drain the pinned staging ring (default 8)                                          */
    ZARC_GPU_PX_DEC_GROUPS = 9005,   /* unpack: frames are dealt by descending size into this many groups whose stages overlap (1..4; 0 = by the
                                        batch: 2 when its largest frame has 4 MiB and more and four times the mean size, else 1)                                                    */
    ZARC_GPU_PX_ZERO_COPY = 9006,    /* host-pointer entry points: when every buffer of a chunk is page-locked memory the device can reach (hipHostMalloc /
                                        hipHostRegister by the caller, same HIP runtime) AND the buffers form runs -- contiguous in the caller's memory and in
                                        batch order -- of at least this many KiB on average, the DMA engines move them directly and the staging ring with its
                                        host memcpy pass is skipped.  Default 4096 (a DMA per small scattered buffer is slower than the ring); 0 = always stage.
                                        Ordinary (pageable) buffers are staged either way. */
    /* UNLIKE THE IDS ABOVE THIS ONE CHANGES THE BYTES THAT COME OUT (every frame stays valid Zstandard of the same content). */
    ZARC_GPU_PX_BLOCK_SPLIT = 9007,  /* 0 (default): a block every 64 KiB and nowhere else.  1: a 64 KiB block is cut into up to 16 Zstandard blocks at sequence
                                        boundaries where its literal statistics change, each with its own Huffman table and table modes (what libzstd 1.5 does
                                        inside compress2).  Smaller frames on ELF / machine code / JSON, the same on text; zarc_gpu_bound() holds unchanged (a
                                        block whose pieces would cost more than one raw block goes out as one).  Store mode ignores it.  Other values:
                                        ZARC_GPU_E_PARAM. */
    /* ... and this one changes no byte again, only the time a pack call takes */
    ZARC_GPU_PX_CHECK_FRAMES = 9008, /* 0 (default) / 1; other values ZARC_GPU_E_PARAM.  1: every pack call decodes its own frames again and compares them
                                        with the sources before it returns ("read-back check" below) */
    ZARC_GPU_PX_SEQ_STATES = 9009    /* like ZARC_GPU_PX_DEC_GROUPS it changes no byte.  Pack, frames of several blocks: 1 (default) = the FSE state chains
                                        of the blocks of a 1 MiB group that code their sequences with the same tables run side by side on one wave, in
                                        front of the pass that writes the sequences sections; 0 = every block's wave runs its own chains (as before);
                                        N > 1 = as 1, but only for blocks of fewer than N sequences (for tests and comparisons: the way to reach with small
                                        inputs what a block too large for its state slot does).  Negative: ZARC_GPU_E_PARAM.  Ignored with
                                        ZARC_GPU_PX_BLOCK_SPLIT on. */
};
/* What the engine does with the libzstd ids (pack.rs:86-217 forwards them all):
 *   CompressionLevel  -131072..22 accepted; four finders (zarc_gpu_level_finder says which one a level runs):
 *                     <= 1 (level 1 and the negative levels): the FAST finder -- one LDS table of 2^15 16-bit entries on a 5-byte hash,
 *                     candidates up to 64 KiB back, recent-offset guesses; no far table, no lazy step;
 *                     2..8 (0 = default = 3): the level-3 finder -- the same table plus a 2^16-bucket far table in HBM on a 12-byte hash,
 *                     content-sampled one position in 16, one-byte lazy evaluation, long matches continued in an extension round;
 *                     9..14: the deep finder -- two tagged LDS tables, 4-byte short hash, 2-way far tables on both hashes, a parse that
 *                     tries the live repeat offsets in two more rounds per tile and looks two bytes ahead;
 *                     15..22: the deep finder with four such rounds.  Levels inside one tier give identical frames.
 *   WindowLog         honoured for the frame header / the farthest offset (10..27; default 21, level >= 9: 22).
 *   MinMatch          4..7 honoured (3 is raised to 4); default 5, level >= 9: 4.
 *   HashLog, ChainLog, SearchLog, TargetLength, Strategy
 *                     accepted inside libzstd's bounds (6..30, 6..30, 1..30, 0..131072, 1..9; 0 = default), returned by
 *                     zarc_gpu_get_params, and ADVISORY: table sizes and the search are fixed by the kernels, so the frames are the
 *                     level's frames whatever these say (libzstd would search harder or less hard; the frames are valid either way).
 *   ContentSizeFlag   only 1.  ChecksumFlag honoured.  DictIdFlag accepted (zarc has no dictionaries).
 *   EnableLongDistanceMatching, LdmHashLog, LdmMinMatch, LdmBucketSizeLog, LdmHashRateLog (160-164)
 *                     accepted inside libzstd's bounds and ADVISORY as well: the far tables of the finders are the engine's long-distance
 *                     matcher at every level above 1, whatever these say.
 *   NbWorkers / JobSize / OverlapLog (400-402), experimental ids: ZARC_GPU_E_UNSUPPORTED.
 * zarc_gpu_parameter_advisory(id) tells a caller (the CLI prints a warning) that an id is accepted but changes nothing. */

typedef struct {
    int level;             /* 0 => default 3 (encode.rs:62 init(0))                                  */
    int checksum_flag;     /* the CLI always sets 1 (zarc-cli/src/pack.rs:227)                       */
    int content_size_flag; /* 1: frame content size is always written (one-shot compress2 behaviour) */
    int window_log;        /* 0 => level default (21 at level 3)                                     */
    int hash_log, chain_log, search_log, min_match, target_length, strategy; /* 0 => engine default  */
    int compress;          /* Encoder::enable_compression (encode.rs:95-97); 0 => raw-block frames   */
} zarc_gpu_params;

/* ---- context -------------------------------------------------------------------------------- */
/* CCtx::try_create + init(0) / DCtx::try_create.  device = HIP device ordinal. */
int zarc_gpu_create(zarc_gpu_t **out, int device);
/* Number of usable HIP devices (0 when there is none or the runtime fails): what `--gpus N` is checked against.  Frames are
 * independent, so a caller that wants G devices opens G handles and deals its batch itself. */
int zarc_gpu_device_count(void);
void zarc_gpu_destroy(zarc_gpu_t *h);
/* Sticky across batches, like Encoder::set_zstd_parameter.  Unknown ids -> ZARC_GPU_E_PARAM; ids libzstd knows but the
 * engine cannot honour (NbWorkers, JobSize, OverlapLog, experimental ids) -> ZARC_GPU_E_UNSUPPORTED.  The search-effort
 * and long-distance-matching ids are accepted and ADVISORY (see above; zarc_gpu_parameter_advisory). */
int zarc_gpu_set_parameter(zarc_gpu_t *h, int param_id, int value);
void zarc_gpu_get_params(const zarc_gpu_t *h, zarc_gpu_params *out);
/* Encoder::enable_compression */
void zarc_gpu_enable_compression(zarc_gpu_t *h, int compress);
/* Worst-case frame size for an n-byte entry: n + 3*max(1,ceil(n/65536)) + 18, rounded up to ZARC_GPU_ALIGN.  The formula is
 * the compressing encoder's worst case (every 64 KiB block raw, 3 bytes of header each, with or without
 * ZARC_GPU_PX_BLOCK_SPLIT); store-mode frames have 131 072-byte raw blocks and a 14-byte header, which it covers as well.
 * The reference's Vec capacity rule (lowlevel_frames.rs:21) is smaller than libzstd's own bound; this one never fails. */
size_t zarc_gpu_bound(size_t n);
const char *zarc_gpu_error_name(int code);         /* call-level codes (negative) */
const char *zarc_gpu_frame_status_name(int status); /* per-frame status (>= 0)     */
const char *zarc_gpu_last_error(const zarc_gpu_t *h);
int zarc_gpu_abi_version(void);
/* The level whose finder `level` runs: 1 (level <= 1), 3 (2..8 and 0), 9 (9..14) or 15 (15..22).  `zarc pack --level 19` warns that it packs
 * with the level-15 finder (zarc-cli/src/pack.rs:24-33 accepts -131072..22 and libzstd has a parameter set for each). */
int zarc_gpu_level_finder(int level);
/* 1 = the parameter id is accepted and remembered but ADVISORY (search-effort and long-distance-matching hints, pack.rs:86-217): the
 * frames are the level's frames whatever its value.  0 = honoured, or not accepted at all. */
int zarc_gpu_parameter_advisory(int id);

/* ---- pack: BLAKE3 + Zstandard frame encode (+ XXH64) ------------------------------------------- */
/* Host-memory form (mirrors add_data_frame's `&[u8]` input).  For every entry i the engine writes one
 * complete Zstandard frame at dst + dst_off[i] of dst_len[i] bytes (the value the caller adds to
 * Encoder.offset and stores as Frame.length, content_frame.rs:45-57) and digest[i] (Frame.digest).
 * dst_off[] are slot starts (slot i has room for zarc_gpu_bound(src_len[i])); frames are concatenable in
 * index order.  Dedup (content_frame.rs:30-33) is the caller's: compare digest[], drop later duplicates. */
int zarc_gpu_pack_batch(zarc_gpu_t *h, size_t n, const void *const *src, const size_t *src_len,
                        void *dst, size_t dst_cap, size_t *dst_off, size_t *dst_len,
                        uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status);

/* Device-memory form: d_src_base/d_dst are device pointers, the small per-entry arrays stay on the
 * host.  src_off[i] must be multiples of ZARC_GPU_ALIGN and the arena must extend ZARC_GPU_PAD bytes
 * past the last entry.  Outputs as above (dst_off/dst_len/digest/status are host arrays). */
int zarc_gpu_pack_batch_device(zarc_gpu_t *h, size_t n, const void *d_src_base, const uint64_t *src_off,
                               const uint64_t *src_len, void *d_dst, size_t dst_cap, uint64_t *dst_off,
                               uint64_t *dst_len, uint8_t *digest /* n*32 */, int *status);

/* Hash first, like the reference (content_frame.rs:26-33 hashes, looks the digest up and returns before compressing known content):
 * every entry is digested, then `known(ctx, digest, i)` is called once per entry in index order on the calling thread; a nonzero
 * return skips the entry (status[i] = ZARC_GPU_FRAME_DUPLICATE, dst_len[i] = 0, digest[i] set, nothing compressed).  A callback that
 * returns 0 should remember the digest so that a later copy inside the same batch is skipped too: first occurrence wins.  known == NULL
 * is zarc_gpu_pack_batch.  dst_off[i] is meaningful for compressed entries only.  The digest pass costs about 0.5 ms per GiB where
 * the match finder costs 20: on content that repeats (the reference's own benchmark tree is half duplicates) the saving is the
 * duplicates' whole share. */
typedef int (*zarc_gpu_known_fn)(void *ctx, const uint8_t digest[ZARC_GPU_DIGEST_LEN], size_t index);
int zarc_gpu_pack_batch_dedup(zarc_gpu_t *h, size_t n, const void *const *src, const size_t *src_len,
                              void *dst, size_t dst_cap, size_t *dst_off, size_t *dst_len,
                              uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, zarc_gpu_known_fn known, void *ctx);
int zarc_gpu_pack_batch_device_dedup(zarc_gpu_t *h, size_t n, const void *d_src_base, const uint64_t *src_off,
                                     const uint64_t *src_len, void *d_dst, size_t dst_cap, uint64_t *dst_off,
                                     uint64_t *dst_len, uint8_t *digest /* n*32 */, int *status,
                                     zarc_gpu_known_fn known, void *ctx);

/* Read-back check (ZARC_GPU_PX_CHECK_FRAMES = 1; sticky; all four pack entry points).  Before a pack call returns, while sources and
 * assembled frames are still in HBM, the engine's own decoder decodes every frame of the call (compressed, split-block and store-mode
 * alike; ZARC_GPU_FRAME_DUPLICATE entries have no frame) into scratch of the handle and the decoded bytes are compared with the source
 * bytes, exactly; with the checksum flag the frame's four trailer bytes are compared with the XXH64 of the source as well.  The digest
 * needs no second look: it was computed from the source, and the source was just compared.  Any bad entry: status[i] =
 * ZARC_GPU_FRAME_CORRUPT where status was given, dst_len[i] = 0, zarc_gpu_last_error() names the first bad index of the batch and its
 * first differing byte (or the checksum trailer), and the call returns ZARC_GPU_E_CHECK: treat the batch's output as void.  The
 * decode scratch counts against ZARC_GPU_PX_SCRATCH_MB like verify's.  With the switch off none of this runs and nothing is reserved. */

/* ---- unpack: Zstandard frame decode (+ XXH64 verify) + BLAKE3 verify --------------------------- */
/* frame[i]/frame_len[i] = Frame.offset/.length slice of the archive, raw_len[i] = Frame.uncompressed
 * (crates/zarc/src/directory/frame.rs:17-31), dst[i] = buffer of raw_len[i] bytes.  expect may be NULL;
 * when given, a mismatch sets status[i] = ZARC_GPU_FRAME_DIGEST but the bytes are still delivered
 * (unpack.rs:118-120).  digest[i] always receives the BLAKE3 of what was decoded; a frame that did not decode
 * (any other status than OK / CHECKSUM / DIGEST) has no content and gets an all-zero digest. */
int zarc_gpu_unpack_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len,
                          const size_t *raw_len, void *const *dst,
                          const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN],
                          uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status);

int zarc_gpu_unpack_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off,
                                 const uint64_t *frame_len, void *d_dst_base, const uint64_t *dst_off,
                                 const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */,
                                 uint8_t *digest /* n*32 */, int *status);

/* ---- verify: FrameIterator::verify() for a batch, without the bytes ----------------------------- */
/* What FrameIterator::verify() (crates/zarc/src/decode/frame_iterator.rs:83-88) answers once a frame has been read to its end, and what
 * `zstd --test` does for one file: is this frame good?  Arguments and results as zarc_gpu_unpack_batch minus dst: status[i] and
 * digest[i] are EXACTLY what unpack gives for the same frame (the same decoder, XXH64 / BLAKE3 passes and verdict run; a digest
 * mismatch is ZARC_GPU_FRAME_DIGEST, reported and not fatal, unpack.rs:118-120).  The decoded bytes go to scratch the handle owns
 * and never to the caller: the host form moves only the compressed bytes host-to-device and nothing back but 36 bytes per frame.
 * The scratch counts against ZARC_GPU_PX_SCRATCH_MB: a batch whose decoded bytes (plus decoder scratch) exceed it is verified in
 * parts; a single frame larger than the budget runs alone. */
int zarc_gpu_verify_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                          const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status);
int zarc_gpu_verify_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off,
                                 const uint64_t *frame_len, const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */,
                                 uint8_t *digest /* n*32 */, int *status);

/* ---- repack: one archive's frames into another's, without the content leaving the device ---------------------- */
/* Decoder::read_content_frame joined to Encoder::add_data_frame: every frame is decoded and judged as zarc_gpu_verify_batch does it, and
 * what decoded well is encoded again with the handle's CURRENT parameters, out of the scratch it was decoded into.
 *   - status[i] and digest[i] are EXACTLY what zarc_gpu_verify_batch gives for the same frame and `expect`.  status is required:
 *     dst_len[i] == 0 alone cannot tell an empty result from a refused frame.
 *   - A frame whose status is ZARC_GPU_FRAME_OK is re-encoded: level, checksum flag, window log, min match, enable_compression and
 *     ZARC_GPU_PX_BLOCK_SPLIT are the handle's.  The new frame at dst + dst_off[i], dst_len[i] bytes, is exactly what
 *     zarc_gpu_pack_batch_device writes for the decoded content.
 *   - Every other status -- ZARC_GPU_FRAME_CHECKSUM and ZARC_GPU_FRAME_DIGEST included: content that does not match its address is
 *     never given a new frame -- yields no frame and dst_len[i] = 0.  Its neighbours are unaffected and the call returns ZARC_GPU_OK,
 *     as unpack does.
 *   - dst_off[] are slot starts as in pack; slot i has zarc_gpu_bound(raw_len[i]) bytes; dst_cap below their sum: ZARC_GPU_E_DSTSIZE.
 *     A frame or raw length of 4 GiB or more: ZARC_GPU_E_UNSUPPORTED, checked before any arithmetic.
 *   - ZARC_GPU_PX_CHECK_FRAMES = 1 applies: the new frames are decoded again and compared with the decoded content they were made
 *     from; a failure returns ZARC_GPU_E_CHECK as in pack.
 *   - Neither hash is computed twice: the digest is the decode half's, and the checksum trailer of a new frame is the XXH64 the decoder
 *     computed of what it decoded (it hashes every frame, whether or not the old frame stored a checksum).
 *   - Decoded bytes, decoder scratch and encoder scratch are live together and count together against ZARC_GPU_PX_SCRATCH_MB; a batch
 *     beyond it runs in parts (a single frame alone), with identical results.
 *   - The host form moves the frames host-to-device (sum of frame_len) and the new frames device-to-host (sum of dst_len), and nothing
 *     else of content: zarc_gpu_last_copy_bytes reports exactly these sums, the device form 0.
 *   - zarc_gpu_last_kernel_ms afterwards: T_DECODE, T_DEC_*, T_BLAKE3 and T_XXH64 hold the decode half's times, T_MATCH, T_ENTROPY and
 *     T_ASSEMBLE the encode half's, T_TOTAL the sum of both halves. */
int zarc_gpu_repack_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                          const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, void *dst, size_t dst_cap, size_t *dst_off, size_t *dst_len,
                          uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status);
/* d_frames_base / d_dst are device pointers (frame_off[] need no alignment; d_dst 16-byte aligned), everything else host arrays */
int zarc_gpu_repack_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                 const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, void *d_dst, size_t dst_cap,
                                 uint64_t *dst_off, uint64_t *dst_len, uint8_t *digest /* n*32 */, int *status);

/* ---- search: which frames contain a byte string, without the content leaving the device ------------------------ */
/* What `zstdgrep -c -F` answers per file, for a batch of frames (the reference has no such call: it would unpack everything and scan on
 * the host).  Every frame is decoded and judged as zarc_gpu_verify_batch does it, and a kernel then looks through the decoded bytes where
 * they lie for ONE fixed byte string -- no regular expression -- of 1 .. ZARC_GPU_SEARCH_MAX_PATTERN bytes.
 *   - status[i] and digest[i] are EXACTLY what zarc_gpu_verify_batch gives for the same frame and `expect`.
 *   - count[i] = the number of start positions p with content[p .. p + pattern_len) == pattern (overlapping occurrences count; a match
 *     never crosses a frame's end); first[i] = the lowest such p, or ZARC_GPU_SEARCH_NONE.
 *   - A frame is searched when it decoded: status ZARC_GPU_FRAME_OK, and ZARC_GPU_FRAME_DIGEST as well (content that differs from
 *     `expect` is still delivered by unpack).  Every other status: count 0, first ZARC_GPU_SEARCH_NONE.
 *   - ZARC_GPU_SEARCH_ICASE folds the ASCII letters 'A'..'Z' / 'a'..'z' in pattern and content and NOTHING else: '@' '[' '`' '{' and every
 *     byte >= 0x80 match only themselves.
 *   - pattern == NULL, pattern_len == 0 or above the maximum, unknown flag bits, a missing digest / status / count / first array:
 *     ZARC_GPU_E_PARAM.  n == 0: ZARC_GPU_OK.  A frame or raw length of 4 GiB or more: ZARC_GPU_E_UNSUPPORTED.
 *   - The decoded bytes count against ZARC_GPU_PX_SCRATCH_MB exactly as verify's do; the results are the same for every budget.
 *   - The host form moves the frames host-to-device (sum of frame_len) and no content back: zarc_gpu_last_copy_bytes reports exactly that
 *     (the pattern is not content).  The device form reports 0.
 *   - Cost: one pass over the decoded bytes beside the two hash passes.  The worst case is a pattern whose first four bytes match almost
 *     everywhere (a run of one byte searched for that byte repeated): then every position is compared in full, O(content * pattern_len).
 *   - zarc_gpu_last_kernel_ms: verify's timers, ZARC_GPU_T_SEARCH for the search kernel, ZARC_GPU_T_TOTAL including it. */
#define ZARC_GPU_SEARCH_MAX_PATTERN 256
#define ZARC_GPU_SEARCH_NONE UINT64_MAX           /* first[i] of a frame without a match */
enum { ZARC_GPU_SEARCH_ICASE = 1 };               /* flags; any other bit: ZARC_GPU_E_PARAM */
int zarc_gpu_search_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                          const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, const void *pattern, size_t pattern_len, unsigned flags,
                          uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first);
int zarc_gpu_search_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                 const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, const void *pattern /* HOST pointer */,
                                 size_t pattern_len, unsigned flags, uint8_t *digest /* n*32 */, int *status, uint64_t *count, uint64_t *first);

/* ---- search, lines: the matching lines of a search, gathered on the device ------------------------------------------------------------ */
/* What `grep -n -F` prints per file: zarc_gpu_search_batch, plus the lines that hold a match.  Only those lines' bytes leave the device.
 *   - A LINE is a maximal run of content bytes without 0x0A; it is ended by a 0x0A or by the frame's end; the 0x0A is not part of it (a
 *     0x0D in front of it is).  Content that ends in 0x0A has no extra empty last line; an empty frame has no line.  A line's NUMBER is 1 +
 *     the count of 0x0A bytes in front of its first byte.  A line MATCHES when at least one matching start position (as
 *     zarc_gpu_search_batch defines it, ZARC_GPU_SEARCH_ICASE included) lies in it; a line with several matches is one line.
 *   - The pattern must not contain 0x0A (ZARC_GPU_E_PARAM): a match then never spans two lines.  Nothing crosses a frame's end.
 *   - status, digest, count, first: EXACTLY what zarc_gpu_search_batch gives for the same arguments.  lines[i] = the number of matching
 *     lines of frame i, ALL of them whatever the caps.  Frames that did not decode (status other than OK / DIGEST): 0 lines, no record.
 *   - Delivery, the same for every scratch budget, every chunking, host and device form: go through the frames in batch order; frame i
 *     delivers its first d_i = min(lines[i], max_lines (0 = no limit), rec_cap - sum of d_j, j < i) matching lines in ascending `start`.
 *     Records are therefore ordered by (frame, start); *rec_used = the sum of d_i.  A caller sees truncation by comparing with lines[i].
 *   - text is compact: text_off is the running sum of text_len in record order, *text_used the whole sum.  text_cap < rec_cap * max_line
 *     (or a product that overflows): ZARC_GPU_E_DSTSIZE -- the text can then never run out on its own.  rec_cap == 0 is a counting call:
 *     rec and text may be NULL, both *_used are 0.
 *   - ZARC_GPU_E_PARAM: everything zarc_gpu_search_batch refuses, a missing lines / rec_used / text_used, a NULL rec or text with
 *     rec_cap > 0, max_line outside 1 .. ZARC_GPU_LINES_MAX_LINE, a 0x0A in the pattern.  n == 0: ZARC_GPU_OK, both *_used 0.  A frame or
 *     raw length of 4 GiB or more: ZARC_GPU_E_UNSUPPORTED.
 *   - Host form: `text` is host memory; the frames go up and exactly *text_used bytes of content come back (zarc_gpu_last_copy_bytes:
 *     H2D = sum of frame_len, D2H = *text_used; records, counts and statuses are descriptors).  Device form: frames and `text` are device
 *     memory, `rec` and every per-frame array are host arrays; the counters report 0.
 *   - zarc_gpu_last_kernel_ms: search's timers, ZARC_GPU_T_LINES for the line kernels, ZARC_GPU_T_TOTAL including them. */
#define ZARC_GPU_LINES_MAX_LINE 65536
typedef struct {
    uint64_t frame;    /* index in the batch */
    uint64_t start;    /* offset of the line's first byte in the frame's content */
    uint64_t length;   /* the whole line in bytes, without its 0x0A, however long */
    uint64_t number;   /* 1-based line number */
    uint64_t match;    /* lowest matching start position in the line (offset in the content) */
    uint64_t text_off; /* where the delivered bytes lie in `text` */
    uint64_t text_len; /* min(length, max_line): the line's FIRST text_len bytes */
} zarc_gpu_line;
int zarc_gpu_search_lines_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, const void *pattern, size_t pattern_len, unsigned flags,
                                uint64_t max_lines /* per frame; 0 = no limit */, uint64_t max_line /* 1..65536 */,
                                uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first, uint64_t *lines /* n */,
                                zarc_gpu_line *rec, size_t rec_cap, size_t *rec_used, void *text, size_t text_cap, size_t *text_used);
int zarc_gpu_search_lines_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                       const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, const void *pattern /* HOST pointer */,
                                       size_t pattern_len, unsigned flags, uint64_t max_lines, uint64_t max_line, uint8_t *digest /* n*32 */,
                                       int *status, uint64_t *count, uint64_t *first, uint64_t *lines, zarc_gpu_line *rec /* HOST array */,
                                       size_t rec_cap, size_t *rec_used, void *d_text /* DEVICE pointer */, size_t text_cap, size_t *text_used);

/* ---- search, a set: 1 .. ZARC_GPU_SEARCH_MAX_SET fixed strings in ONE pass ---------------------------------------------------------------- */
/* What `grep -F -f list` answers: the frames are decoded, judged and hashed once and their content is read once, however many patterns the
 * set holds.  A set is `count` patterns, pattern k = bytes[off[k] .. off[k] + len[k]), each of 1 .. ZARC_GPU_SEARCH_MAX_PATTERN bytes; all
 * of it is HOST memory in every form.  Duplicates and patterns that are prefixes of one another are allowed.
 *   - Pattern k MATCHES at p when content[p .. p + len[k]) == pattern k, with p + len[k] <= the frame's length: the frame-end rule is per
 *     pattern (a short one may match where a longer one of the set is cut off).  ZARC_GPU_SEARCH_ICASE folds every pattern and the content
 *     exactly as zarc_gpu_search_batch defines it.
 *   - count[i] = the start positions at which AT LEAST ONE pattern matches (a position counts once, however many match there);
 *     first[i] = the lowest of them, which[i] = the lowest k that matches at first[i]; both ZARC_GPU_SEARCH_NONE without a match.
 *   - hits[k] (may be NULL; count words for the whole call, not per frame) = the sum over all searched frames of the call of the start
 *     positions at which pattern k matches.
 *   - status, digest, which frames are searched: as zarc_gpu_search_batch.  A frame that did not decode: count 0, first and which
 *     ZARC_GPU_SEARCH_NONE, nothing added to hits.  A set of one pattern gives exactly zarc_gpu_search_batch's count and first.
 *   - ZARC_GPU_E_PARAM: everything zarc_gpu_search_batch refuses; a NULL set or member of it; count 0 or above the maximum; a len of 0 or
 *     above ZARC_GPU_SEARCH_MAX_PATTERN; a missing `which`.  n == 0: ZARC_GPU_OK -- the set is validated all the same and hits zeroed.
 *   - The lines forms are zarc_gpu_search_lines_batch* word for word, with "a matching start position" being one of the union: a line with
 *     matches of several patterns is one line, rec.match its lowest matching position.  No pattern may contain 0x0A (ZARC_GPU_E_PARAM).
 *   - Results are the same for every ZARC_GPU_PX_SCRATCH_MB, every chunking, host and device form.  zarc_gpu_last_copy_bytes: as the
 *     one-pattern calls (the compiled set is not content).  zarc_gpu_last_kernel_ms: ZARC_GPU_T_SEARCH covers the set's scan kernels,
 *     ZARC_GPU_T_LINES the line kernels.
 *   - Cost: the pass of zarc_gpu_search_batch with a table lookup per position in place of a compare; the worst case is that call's, times
 *     the patterns that share a position's first bytes. */
#define ZARC_GPU_SEARCH_MAX_SET 1024
typedef struct {
    const void *bytes;     /* the patterns' bytes */
    const uint64_t *off;   /* count offsets into bytes */
    const uint64_t *len;   /* count lengths, 1 .. ZARC_GPU_SEARCH_MAX_PATTERN */
    size_t count;          /* 1 .. ZARC_GPU_SEARCH_MAX_SET */
} zarc_gpu_pattern_set;    /* all HOST memory */
int zarc_gpu_search_set_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                              const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, const zarc_gpu_pattern_set *set, unsigned flags,
                              uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first, uint64_t *which,
                              uint64_t *hits /* set->count words or NULL */);
int zarc_gpu_search_set_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                     const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, const zarc_gpu_pattern_set *set /* HOST */,
                                     unsigned flags, uint8_t *digest /* n*32 */, int *status, uint64_t *count, uint64_t *first, uint64_t *which,
                                     uint64_t *hits /* set->count words or NULL */);
int zarc_gpu_search_set_lines_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                    const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, const zarc_gpu_pattern_set *set, unsigned flags,
                                    uint64_t max_lines /* per frame; 0 = no limit */, uint64_t max_line /* 1..65536 */,
                                    uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first, uint64_t *which,
                                    uint64_t *hits /* or NULL */, uint64_t *lines /* n */, zarc_gpu_line *rec, size_t rec_cap, size_t *rec_used,
                                    void *text, size_t text_cap, size_t *text_used);
int zarc_gpu_search_set_lines_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                           const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, const zarc_gpu_pattern_set *set /* HOST */,
                                           unsigned flags, uint64_t max_lines, uint64_t max_line, uint8_t *digest /* n*32 */, int *status,
                                           uint64_t *count, uint64_t *first, uint64_t *which, uint64_t *hits /* or NULL */, uint64_t *lines,
                                           zarc_gpu_line *rec /* HOST array */, size_t rec_cap, size_t *rec_used, void *d_text /* DEVICE pointer */,
                                           size_t text_cap, size_t *text_used);

/* ---- search, a regular expression: matched on the device, line by line ------------------------------------------------------------------ */
/* What `grep -E` answers: zarc_gpu_search_batch* and zarc_gpu_search_lines_batch* with a regular expression in place of the fixed string.
 * Matching is per LINE (as zarc_gpu_search_lines_batch defines a line) and never crosses a 0x0A or a frame's end; the frame's first byte
 * starts a line and the frame's end ends one, with or without a final 0x0A; a 0x0D in front of a 0x0A is part of the line (`x$` does not
 * match "x\r\n", as in grep).
 *   - Position p is a MATCHING START POSITION of regex R when some non-empty run content[p .. j) inside p's line is in L(R); `^` holds only
 *     at the line's first byte, `$` only behind its last.  Whether a match exists at p does not depend on leftmost-longest or backtracking
 *     order, so POSIX, Python's `re` and this engine agree on it: per line it is {m.start() for m in re.finditer(b"(?=(?:R))", line)}.
 *   - count[i] = the number of matching start positions of frame i, first[i] = the lowest or ZARC_GPU_SEARCH_NONE.  The lines forms are
 *     zarc_gpu_search_lines_batch* word for word with this meaning of "matching start position" (rec.match: the lowest in the line).  A regex
 *     that is one literal string gives exactly the fixed-string call's answers.
 *   - Dialect: bytes, POSIX ERE's operators with Python's escapes.  Literals; `.` (any byte but 0x0A, 0x00 and bytes >= 0x80 included);
 *     `[...]` `[^...]` with ranges (`]` first is the byte); `( )`; `|`; `*` `+` `?` `{n}` `{n,}` `{n,m}` with n <= m <= 255; `^` `$`.
 *     Escapes, outside and inside brackets alike: `\` + punctuation = that byte; \t \r \f \v \0 \xHH; \d \D \w \W \s \S (ASCII).  No class ever
 *     matches 0x0A: negated classes, \s \D \W \S silently lose it.  ZARC_GPU_SEARCH_ICASE folds ASCII letters only, in literals and classes.
 *   - ZARC_GPU_E_PARAM, zarc_gpu_last_error() = "regex: offset N: reason" with N the byte offset in the regex: unbalanced ( ) [; a quantifier
 *     with nothing to repeat or on a quantifier; a `{` that is not a valid bound, {3,2}, {,m}, a bound above 255; [b-a]; an empty regex or
 *     one above ZARC_GPU_REGEX_MAX_PATTERN bytes; any other `\` + letter or digit (\b \1 \A ...: no back-references, word boundaries,
 *     look-around); lazy and possessive quantifiers (*? ++); a literal 0x0A, \n or \x0a; a regex that can match without consuming a content
 *     byte, anchors counted as empty (a*, x|, (), ^$): it would match every line and no position could carry the match.
 *   - ZARC_GPU_E_UNSUPPORTED, the message giving the states needed: the minimised automaton has more than ZARC_GPU_REGEX_MAX_STATES states.
 *     This is inherent to answering "does a match START here": the automaton is that of SIGMA* . reverse(R), read from a line's last byte
 *     to its first, and .{k}a needs 2^(k+1) states (.{4}a fits, .{7}a does not); a literal of m bytes needs m + 1.  Raising the constant is
 *     a known follow-up: the kernels' LDS arrays that scale with it are `delta` (states x 256 bytes) and `tab` (256 threads x states
 *     bytes) of zdec_regex.hip, 16 KiB each at 64; the tables store a state in one byte, which holds up to 256 of them.
 *   - The compiled table (zarc_gpu_regex_compile, public and handle-less so that a caller can refuse a bad expression before it opens
 *     anything): delta[q * 256 + byte] for q < states; start = the state at a line's end; accept[q] bit 0 = a match starts at the byte just
 *     read, bit 1 = a match starts there if it is the line's first byte.  delta[q][0x0A] == start for every q and accept[start] == 0.
 *   - Everything that is not matching is zarc_gpu_search_batch's / zarc_gpu_search_lines_batch's: status, digest, which frames are searched,
 *     the missing-array checks, n == 0 (the regex is validated all the same), the 4 GiB rule, ZARC_GPU_PX_SCRATCH_MB and parts,
 *     zarc_gpu_last_copy_bytes (the compiled table is not content), zarc_gpu_last_kernel_ms (ZARC_GPU_T_SEARCH: zarc_regex_summary,
 *     zarc_regex_carry, zarc_regex_scan; ZARC_GPU_T_LINES: the line kernels).
 *   - Cost: one dependent LDS lookup per content byte per pass (summary and scan; mark and emit for lines).  A 256-byte chunk without a
 *     0x0A (binaries) pays up to `states` lookups per byte for its transition table instead -- slower, but parallel: no lane ever walks
 *     more than its 256 bytes times `states`, whatever the line length. */
#define ZARC_GPU_REGEX_MAX_PATTERN 1024
#define ZARC_GPU_REGEX_MAX_STATES 64
typedef struct { uint32_t states; uint32_t start; uint8_t accept[64]; uint8_t delta[64 * 256]; } zarc_gpu_regex_dfa;
/* 0, ZARC_GPU_E_PARAM or ZARC_GPU_E_UNSUPPORTED; err (may be NULL) receives the text zarc_gpu_last_error would give ("" on success) */
int zarc_gpu_regex_compile(const void *regex, size_t regex_len, unsigned flags, zarc_gpu_regex_dfa *out /* may be NULL */, char *err, size_t err_cap);
int zarc_gpu_search_regex_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, const void *regex, size_t regex_len, unsigned flags,
                                uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first);
int zarc_gpu_search_regex_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                       const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, const void *regex /* HOST pointer */,
                                       size_t regex_len, unsigned flags, uint8_t *digest /* n*32 */, int *status, uint64_t *count, uint64_t *first);
int zarc_gpu_search_regex_lines_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                      const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, const void *regex, size_t regex_len, unsigned flags,
                                      uint64_t max_lines /* per frame; 0 = no limit */, uint64_t max_line /* 1..65536 */,
                                      uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first, uint64_t *lines /* n */,
                                      zarc_gpu_line *rec, size_t rec_cap, size_t *rec_used, void *text, size_t text_cap, size_t *text_used);
int zarc_gpu_search_regex_lines_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                             const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, const void *regex /* HOST pointer */,
                                             size_t regex_len, unsigned flags, uint64_t max_lines, uint64_t max_line, uint8_t *digest /* n*32 */,
                                             int *status, uint64_t *count, uint64_t *first, uint64_t *lines, zarc_gpu_line *rec /* HOST array */,
                                             size_t rec_cap, size_t *rec_used, void *d_text /* DEVICE pointer */, size_t text_cap, size_t *text_used);

/* ---- search, selected lines: the lines a search does NOT match, and the lines around a hit ------------------------------------------------ */
/* What `grep -v` and `grep -A / -B / -C` print: one pair of calls behind all three matchers.  A LINE and a matching start position are
 * defined as in zarc_gpu_search_lines_batch (a set: zarc_gpu_search_set_lines_batch; a regex: zarc_gpu_search_regex_batch).  For frame i
 * with lines 1 .. L:
 *   - M = the lines that hold at least one matching start position.  H, the HIT lines, = M, or {1 .. L} \ M with ZARC_GPU_SELECT_INVERT.
 *     Empty lines exist and never match, so under INVERT they are hits.  Content ending in 0x0A has no extra last line, an empty frame has
 *     no line, "\n" is one empty line.
 *   - S, the SELECTED lines, = { l in 1 .. L : some h in H with h - before <= l <= h + after }.  The arithmetic saturates: before and after
 *     are uint32_t and any value is legal (0xFFFFFFFF: every line of a frame with a hit, none of a frame without).
 *   - status, digest, count, first -- for a set, which and hits as well -- are EXACTLY the matcher's plain search call: INVERT does not
 *     touch them.  lines[i] = |H| and selected[i] = |S|, both whatever the caps.  A frame that did not decode: 0 and 0, no record.
 *   - Delivery is zarc_gpu_search_lines_batch's rule over S: frames in batch order, frame i delivers its first d_i = min(selected[i],
 *     max_lines (0 = no limit), rec_cap - sum of d_j, j < i) lines of S in ascending `start`.  Records are zarc_gpu_line; `match` is the lowest
 *     matching start position in the line, or ZARC_GPU_SEARCH_NONE when the line holds none.  A record is a hit line iff
 *     (match != ZARC_GPU_SEARCH_NONE) != invert; every other record is context.  text, text_cap, max_line and both ZARC_GPU_E_DSTSIZE rules
 *     are zarc_gpu_search_lines_batch's.
 *   - The matcher: kind FIXED (text, text_len = the pattern), SET (set) or REGEX (text, text_len = the expression); flags
 *     (ZARC_GPU_SEARCH_ICASE) and the arguments of that kind exactly as its own lines call takes them.  which and hits may be NULL; non-NULL
 *     with a kind other than SET is ZARC_GPU_E_PARAM.
 *   - Checks, codes and messages: those of the matcher's own lines call, in its order; then, as ZARC_GPU_E_PARAM, an unknown select flag,
 *     reserved != 0, a missing `selected`.  A missing matcher or selection and an unknown kind are ZARC_GPU_E_PARAM as well.
 *   - With flags == 0 && before == 0 && after == 0, lines, selected (== lines) and every record equal the matcher's own lines call byte for
 *     byte.  Results are the same for every ZARC_GPU_PX_SCRATCH_MB, every chunking, host and device form and every number of handles.
 *   - zarc_gpu_last_copy_bytes: as zarc_gpu_search_lines_batch (D2H = *text_used).  zarc_gpu_last_kernel_ms: ZARC_GPU_T_LINES covers
 *     zarc_lines_select_* with zarc_lines_scan and zarc_lines_gather.
 *   - Cost: the content is read by the matcher once to mark and once more, in the slices that deliver, to emit -- as the lines calls.  Under
 *     INVERT or with wide context most slices deliver. */
enum { ZARC_GPU_MATCH_FIXED = 0, ZARC_GPU_MATCH_SET = 1, ZARC_GPU_MATCH_REGEX = 2 };
enum { ZARC_GPU_SELECT_INVERT = 1 };              /* zarc_gpu_line_select.flags; any other bit: ZARC_GPU_E_PARAM */
typedef struct {
    uint32_t kind;                   /* ZARC_GPU_MATCH_* */
    uint32_t flags;                  /* ZARC_GPU_SEARCH_ICASE */
    const void *text;                /* FIXED: the pattern; REGEX: the expression (HOST memory) */
    size_t text_len;
    const zarc_gpu_pattern_set *set; /* SET */
} zarc_gpu_matcher;
typedef struct { uint32_t flags, before, after, reserved; } zarc_gpu_line_select;
int zarc_gpu_select_lines_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, const zarc_gpu_matcher *matcher,
                                const zarc_gpu_line_select *select, uint64_t max_lines /* per frame; 0 = no limit */, uint64_t max_line /* 1..65536 */,
                                uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first, uint64_t *which /* SET, or NULL */,
                                uint64_t *hits /* SET, or NULL */, uint64_t *lines /* n */, uint64_t *selected /* n */, zarc_gpu_line *rec, size_t rec_cap,
                                size_t *rec_used, void *text, size_t text_cap, size_t *text_used);
int zarc_gpu_select_lines_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                       const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, const zarc_gpu_matcher *matcher /* HOST */,
                                       const zarc_gpu_line_select *select, uint64_t max_lines, uint64_t max_line, uint8_t *digest /* n*32 */, int *status,
                                       uint64_t *count, uint64_t *first, uint64_t *which /* SET, or NULL */, uint64_t *hits /* SET, or NULL */,
                                       uint64_t *lines, uint64_t *selected, zarc_gpu_line *rec /* HOST array */, size_t rec_cap, size_t *rec_used,
                                       void *d_text /* DEVICE pointer */, size_t text_cap, size_t *text_used);

/* ---- search, only the matches: every match of a matching line, cut out on the device ------------------------------------------------------- */
/* What `grep -o` prints: not the lines that hold a match but the matches themselves, each with its start, its length and its bytes.  Only
 * the matched bytes leave the device.  A LINE and a MATCHING START POSITION are what the lines calls define, per matcher kind (FIXED:
 * zarc_gpu_search_lines_batch, SET: zarc_gpu_search_set_lines_batch, REGEX: zarc_gpu_search_regex_batch).  Let M be the set of matching
 * start positions of one line [ls, le).
 *   - The END of the match at p in M is E(p):
 *       FIXED  p + pattern_len.
 *       SET    p + max len[k] over the patterns k that match at p, under the per-pattern frame-end rule.  `which` is the lowest k among the
 *              patterns of that length that match at p.
 *       REGEX  the largest j with p < j <= le and content[p .. j) in L(R).  `^` holds only if p == ls, `$` only if j == le.  This is POSIX
 *              leftmost-longest.
 *   - The MATCHES of the line are what `grep -o` prints: c = ls; repeat: p = min{s in M : s >= c}; if there is none, stop; the match is
 *     (p, E(p) - p); then c = E(p).  Matches never overlap.  A regex cannot match without consuming a byte (refused, see
 *     zarc_gpu_regex_compile), so the loop advances.  The first match of a line starts at the line record's `match`.
 *   - The calls take a zarc_gpu_matcher (FIXED, SET or REGEX, with ZARC_GPU_SEARCH_ICASE as that kind takes it) and no zarc_gpu_line_select.
 *   - status, digest, count, first (SET: which, hits; both may be NULL, non-NULL with another kind is ZARC_GPU_E_PARAM) and lines[i] are
 *     EXACTLY the matcher's own lines call's.
 *   - Lines.  Frame i takes part with its first d_i = min(lines[i], max_lines (0 = no limit), line_cap - sum of d_j, j < i) matching lines:
 *     the lines calls' delivery rule with line_cap in rec_cap's place.  Line records are internal and never leave the device.
 *   - matches[i] = the number of matches in those d_i lines, whatever rec_cap.
 *   - Records.  Frame i delivers its first e_i = min(matches[i], rec_cap - sum of e_j, j < i) matches in ascending `start`; a cut may fall
 *     inside a line.  Records are ordered by (frame, start).  *rec_used = the sum of e_i.
 *   - Text.  text_len = min(length, max_line), the match's first bytes; text_off is the running sum in record order, *text_used the whole
 *     sum.  text_cap < rec_cap * max_line (or a product that overflows): ZARC_GPU_E_DSTSIZE.
 *   - line_cap == 0 or rec_cap == 0 is a counting call: rec and text may be NULL, both *_used are 0; matches[i] is what the rules above
 *     give, so 0 when line_cap == 0.
 *   - Checks: the matcher's own lines call's, in its order (with the matches call's rec_cap in the text_cap rule); for a REGEX the forward
 *     table is compiled right behind the backward one and refused as zarc_gpu_regex_compile_ends refuses it; then, as ZARC_GPU_E_PARAM, a
 *     missing matches / rec_used / text_used, or a NULL rec or text with both caps > 0.  A missing matcher and an unknown kind are
 *     ZARC_GPU_E_PARAM as well.  n == 0: ZARC_GPU_OK (the matcher is validated all the same), both *_used 0.
 *   - Host form: the frames go up and exactly *text_used bytes of content come back (zarc_gpu_last_copy_bytes: H2D = sum of frame_len,
 *     D2H = *text_used).  Device form: `rec` and every per-frame array are host arrays, d_text is device memory; the counters report 0.
 *   - Results are the same for every ZARC_GPU_PX_SCRATCH_MB, every ZARC_GPU_PX_STAGE_CHUNK, both forms and every number of handles: the
 *     remainders of line_cap, rec_cap and the text offset are carried from part to part.
 *   - zarc_gpu_last_kernel_ms: ZARC_GPU_T_LINES covers zarc_matches_* as well.
 *   - Cost: everything up to the line records is the matcher's lines call.  Behind it one lane walks one delivered line: a frame that is one
 *     1 MiB line is walked serially, at roughly 50 cycles per dependent LDS lookup (a regex: the line's length, plus for every match the
 *     bytes from its start to where the forward table dies or the line ends); ordinary text is hundreds of lines per workgroup in
 *     parallel.  A call that delivers no line launches nothing new.
 *
 * zarc_gpu_regex_compile_ends (public and handle-less, as zarc_gpu_regex_compile) fills the same struct with the FORWARD table of R alone,
 * without a SIGMA* loop: it reads from a match's first byte towards the line's end.
 *   - delta[q * 256 + byte] for q < states.  DEAD = states - 1: no continuation is in L(R); every byte leads from DEAD to DEAD and a walk
 *     stops there.  An expression that matches nothing (c^) has this one state.
 *   - `start` = the state in front of a match's first byte when that byte is NOT its line's first.  A walk never reads a 0x0A, so that
 *     column is free: delta[start * 256 + 0x0A] = the state in front of a match's first byte when it IS the line's first byte (where `^`
 *     holds).  delta[q * 256 + 0x0A] == DEAD for every other q.  `start` may be DEAD itself: with ^bb a match starts at a line's first byte
 *     or nowhere.
 *   - accept[q] bit 0 = a match may end behind the byte just read; bit 1 = a match may end there if the line ends there (where `$` holds).
 *     accept[start], accept[delta[start * 256 + 0x0A]] are 0 for what R's own acceptance is concerned: R consumes a byte.
 *   - E(p): q = p == ls ? delta[start * 256 + 0x0A] : start; for j = p, p + 1, ... < le: q = delta[q * 256 + content[j]]; stop at DEAD;
 *     accept[q] & 1, or accept[q] & 2 with j + 1 == le: E = j + 1.  The last such E is the match's end.
 *   - Dialect, refusals and messages are zarc_gpu_regex_compile's.  More than ZARC_GPU_REGEX_MAX_STATES forward states (DEAD and the
 *     line-start state included) is ZARC_GPU_E_UNSUPPORTED, the message giving the number needed: an expression that
 *     zarc_gpu_regex_compile -- and so `-E` -- accepts can still be refused here ((a|b)*a(a|b){6} must know which of the last seven bytes were an a: 129 states). */
typedef struct {
    uint64_t frame;      /* index in the batch */
    uint64_t start;      /* offset of the match's first byte in the frame's content */
    uint64_t length;     /* the whole match in bytes, however long */
    uint64_t number;     /* the 1-based number of the line that holds it */
    uint64_t line_start; /* offset of that line's first byte in the frame's content */
    uint64_t which;      /* SET: the pattern that matched (see E(p)); every other kind: ZARC_GPU_SEARCH_NONE */
    uint64_t text_off;   /* where the delivered bytes lie in `text` */
    uint64_t text_len;   /* min(length, max_line): the match's FIRST text_len bytes */
} zarc_gpu_match;
int zarc_gpu_regex_compile_ends(const void *regex, size_t regex_len, unsigned flags, zarc_gpu_regex_dfa *out /* may be NULL */, char *err, size_t err_cap);
int zarc_gpu_search_matches_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                  const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, const zarc_gpu_matcher *matcher,
                                  uint64_t max_lines /* per frame; 0 = no limit */, uint64_t max_line /* 1..65536 */, size_t line_cap,
                                  uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first, uint64_t *which /* SET, or NULL */,
                                  uint64_t *hits /* SET, or NULL */, uint64_t *lines /* n */, uint64_t *matches /* n */, zarc_gpu_match *rec, size_t rec_cap,
                                  size_t *rec_used, void *text, size_t text_cap, size_t *text_used);
int zarc_gpu_search_matches_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                         const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, const zarc_gpu_matcher *matcher /* HOST */,
                                         uint64_t max_lines, uint64_t max_line, size_t line_cap, uint8_t *digest /* n*32 */, int *status, uint64_t *count,
                                         uint64_t *first, uint64_t *which /* SET, or NULL */, uint64_t *hits /* SET, or NULL */, uint64_t *lines,
                                         uint64_t *matches, zarc_gpu_match *rec /* HOST array */, size_t rec_cap, size_t *rec_used,
                                         void *d_text /* DEVICE pointer */, size_t text_cap, size_t *text_used);

/* ---- read ranges: byte and line ranges of frames, cut out on the device ------------------------------------------------------------------ */
/* What `tar -xO file | head -n N` (tail, sed -n 'A,Bp', head -c, tail -c) answers, for a batch of frames: every frame is decoded and judged as
 * zarc_gpu_verify_batch does it, one range of its content is found where the decoded bytes lie, and only that range's bytes leave the
 * device.  range[i] (HOST memory in every form) names the range of frame i in UNITS that tile the frame's content exactly:
 *   - ZARC_GPU_RANGE_BYTES: every byte is a unit; T = raw_len[i].
 *   - ZARC_GPU_RANGE_LINES: a unit is a line together with its 0x0A; T = the number of 0x0A bytes, + 1 if the content is non-empty and its
 *     last byte is not 0x0A.  An empty frame has T = 0, "\n" has T = 1, a 0x0D stays an ordinary byte.  This is the line of
 *     zarc_gpu_search_lines_batch plus its terminator, so consecutive ranges concatenate to the content.
 *   - The range [a, b) of units.  Without ZARC_GPU_RANGE_FROM_END: a = min(skip, T), b = min(a + take, T).  With it: b = T - min(skip, T),
 *     a = b - min(take, b).  Every sum saturates; any skip and take are legal; take == ZARC_GPU_RANGE_ALL means "to the end" without the
 *     flag and "from the beginning" with it.  head -n N: skip 0, take N.  head -n -N: FROM_END, skip N, take ALL.  tail -n N: FROM_END,
 *     skip 0, take N.  tail -n +K: skip K - 1, take ALL.  sed -n 'A,Bp': skip A - 1, take B - A + 1.  head -c / tail -c: the same, BYTES.
 *   - res[i]: units = T, first = a, taken = b - a, start = the offset of unit a's first byte in the content (raw_len[i] when a == T),
 *     length = the bytes of units a .. b - 1 (0 when a == b).  These five are the truth whatever the caps.  reserved = 0.
 *   - status[i] and digest[i] are EXACTLY what zarc_gpu_verify_batch gives for the same frame and `expect`.  A frame takes part when it
 *     decoded: ZARC_GPU_FRAME_OK, and ZARC_GPU_FRAME_DIGEST as well.  Every other status: res[i] all zero and no bytes.
 *   - Delivery, the lines calls' rule with bytes in the place of records: frames in batch order; frame i delivers the first
 *     e_i = min(length, max_bytes (0 = no limit), text_cap - sum of e_j, j < i) bytes of its range to text + text_off, text_off = the running
 *     sum, text_len = e_i, *text_used = the sum of all e_i.  A caller sees a cut by text_len < length and fetches the rest with the BYTES
 *     range {skip = start + text_len, take = length - text_len}.  text_cap == 0 is a counting call: text may be NULL, *text_used is 0.
 *   - The same frame may stand in a batch several times with different ranges.
 *   - Checks: zarc_gpu_verify_batch's first, in its order; then, as ZARC_GPU_E_PARAM, a missing range / res / text_used, an unknown unit, an
 *     unknown flag bit, a NULL text with text_cap > 0.  n == 0: ZARC_GPU_OK, *text_used = 0.  A frame or raw length of 4 GiB or more:
 *     ZARC_GPU_E_UNSUPPORTED.
 *   - res, text and *text_used are identical for every ZARC_GPU_PX_SCRATCH_MB, every ZARC_GPU_PX_STAGE_CHUNK, both forms and every number of
 *     handles a caller deals the batch to: the remainder of text_cap and the text offset are carried from part to part.
 *   - Host form: `text` is host memory; the frames go up and exactly *text_used bytes of content come back (zarc_gpu_last_copy_bytes:
 *     H2D = sum of frame_len, D2H = *text_used).  Device form: frames and d_text are device memory, res and every per-frame array are host
 *     arrays; the counters report 0.
 *   - zarc_gpu_last_kernel_ms: verify's timers, ZARC_GPU_T_RANGE for zarc_range_* summed over the parts of the call, ZARC_GPU_T_TOTAL
 *     including it.
 *   - Cost: decode and both hash passes are verify's and run in full (no early stop inside a frame).  Beside them a BYTES range reads no
 *     content but what it gathers; a LINES range reads the decoded bytes of its frame once to count 0x0A bytes, plus at most two 64 KiB
 *     slices to locate its two boundaries, plus what it gathers. */
enum { ZARC_GPU_RANGE_BYTES = 0, ZARC_GPU_RANGE_LINES = 1 };   /* unit */
enum { ZARC_GPU_RANGE_FROM_END = 1 };                           /* flags; any other bit: ZARC_GPU_E_PARAM */
#define ZARC_GPU_RANGE_ALL UINT64_MAX
typedef struct { uint32_t unit, flags; uint64_t skip, take; } zarc_gpu_range;            /* one per frame, HOST memory */
typedef struct { uint64_t units, first, taken, start, length, text_off, text_len, reserved; } zarc_gpu_range_result;
int zarc_gpu_read_ranges_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                               const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, const zarc_gpu_range *range /* n */,
                               uint64_t max_bytes /* per frame; 0 = no limit */, uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status,
                               zarc_gpu_range_result *res /* n */, void *text, size_t text_cap, size_t *text_used);
int zarc_gpu_read_ranges_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                      const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, const zarc_gpu_range *range /* HOST, n */,
                                      uint64_t max_bytes, uint8_t *digest /* n*32 */, int *status, zarc_gpu_range_result *res /* HOST, n */,
                                      void *d_text /* DEVICE pointer */, size_t text_cap, size_t *text_used);

/* ---- count: lines, words, characters and the longest line of frames, counted on the device -------------------------------------------------- */
/* What `tar -xO file | wc` answers, for a batch of frames: every frame is decoded and judged as zarc_gpu_verify_batch does it, its content
 * is read once more where the decoded bytes lie, and 64 bytes of counts per frame come back.  Arguments, status[i], digest[i] and error
 * returns are EXACTLY those of zarc_gpu_verify_batch* for the same frames and `expect`; res (HOST memory in every form, n records) is the
 * one addition, and a missing res is ZARC_GPU_E_PARAM behind verify's own checks.  n == 0: ZARC_GPU_OK.  A frame or raw length of 4 GiB or
 * more: ZARC_GPU_E_UNSUPPORTED.
 * A frame takes part when it decoded: ZARC_GPU_FRAME_OK, and ZARC_GPU_FRAME_DIGEST as well (the decoded set of the ranges call).  With
 * content d of raw_len[i] bytes:
 *   - lines: the number of 0x0A bytes, as `wc -l` counts.
 *   - words: the number of positions p with !sp(d[p]) && (p == 0 || sp(d[p - 1])), where sp(c) holds for 0x09 .. 0x0D and 0x20: the
 *     maximal runs of other bytes.  It is what `wc -w` gives in the C locale on printable text.
 *   - chars: the number of bytes with (c & 0xC0) != 0x80 -- bytes that are no UTF-8 continuation byte.  For valid UTF-8 it is the number of
 *     code points (`wc -m` under a UTF-8 locale); for any other bytes it is still this definition.
 *   - max_line: the length in BYTES of the longest piece of d split at 0x0A; the unterminated piece behind the last 0x0A counts, the 0x0A
 *     itself does not.  It is NOT GNU `wc -L`, which is a display width that expands tabs and skips non-printable bytes.
 *   - max_line_start: the offset of the first byte of the LOWEST such piece; max_line_no: that piece's 1-based line number -- the 0x0A bytes
 *     in front of it, plus 1 -- the number zarc_gpu_search_lines_batch reports and a ZARC_GPU_RANGE_LINES range with skip = max_line_no - 1
 *     names.
 *   - Empty content: all fields 0.  Every other status: all fields 0.  reserved = 0.
 *   - res is identical for every ZARC_GPU_PX_SCRATCH_MB, every ZARC_GPU_PX_STAGE_CHUNK, both forms and every number of handles a caller
 *     deals the batch to.
 *   - zarc_gpu_last_copy_bytes: H2D = sum of frame_len in the host form, 0 in the device form; D2H = 0 (the 64 bytes a frame are descriptors,
 *     not content, as in verify).
 *   - zarc_gpu_last_kernel_ms: verify's timers, ZARC_GPU_T_WC for zarc_wc_* summed over the parts of the call, ZARC_GPU_T_TOTAL including it.
 *   - Cost: decode and both hash passes are verify's and run in full; beside them the decoded bytes are read once. */
typedef struct { uint64_t lines, words, chars, max_line, max_line_start, max_line_no, reserved[2]; } zarc_gpu_wc;   /* 64 bytes */
int zarc_gpu_count_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                         const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status,
                         zarc_gpu_wc *res /* n */);
int zarc_gpu_count_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, uint8_t *digest /* n*32 */, int *status,
                                zarc_gpu_wc *res /* HOST, n */);

/* ---- compare: frames against other bytes, compared on the device ---------------------------------------------------------------------------- */
/* What `tar --compare` and `cmp` answer, for a batch of pairs: every frame is decoded and judged as zarc_gpu_verify_batch does it, its content
 * is read once more where the decoded bytes lie, next to the other side's bytes, and 64 bytes per pair come back.  Arguments, status[i],
 * digest[i] and error returns are EXACTLY those of zarc_gpu_verify_batch* for the same frames and `expect`; other, other_len and res (HOST
 * memory in every form, n records) are the additions.  A missing res, other or other_len is ZARC_GPU_E_PARAM behind verify's own checks;
 * other[i] may be NULL only where other_len[i] == 0.  n == 0: ZARC_GPU_OK.  A frame, raw or other length of 4 GiB or more:
 * ZARC_GPU_E_UNSUPPORTED.  Device form: other i lies at d_other_base + other_off[i], other_off[i] a multiple of ZARC_GPU_ALIGN (else
 * ZARC_GPU_E_PARAM), with ZARC_GPU_PAD readable bytes behind the arena -- pack's rules for device-resident sources.
 * A frame takes part when it decoded: ZARC_GPU_FRAME_OK, and ZARC_GPU_FRAME_DIGEST as well.  With A the content of raw_len[i] bytes, B the
 * other[i] of other_len[i] bytes and common = min(|A|, |B|):
 *   - differing: the number of p < common with A[p] != B[p] -- what `cmp -l` lists.
 *   - prefix: the lowest such p; common where there is none.
 *   - relation: ZARC_GPU_CMP_DIFFER when differing > 0; otherwise EQUAL, FRAME_IS_PREFIX or OTHER_IS_PREFIX by the lengths.
 *   - line: 1 + the number of 0x0A in A[0 .. prefix) -- the line `cmp` prints.  No exception: for EQUAL it is lines + 1.
 *   - byte_a, byte_b: A[prefix] and B[prefix]; ZARC_GPU_CMP_EOF where that side ends at prefix.
 *   - suffix: the largest s <= common - prefix with A[|A| - s ..] == B[|B| - s ..]: the common tail, which never overlaps the common head.
 *     With |A| == |B| it is the distance from the last differing byte to the end.
 *   - Both sides empty: EQUAL, all counts 0, line 1.  A frame that did not decode: every field 0 (ZARC_GPU_CMP_NONE).  reserved = 0.
 *   - res is identical for every ZARC_GPU_PX_SCRATCH_MB, every ZARC_GPU_PX_STAGE_CHUNK, both forms and every number of handles a caller
 *     deals the batch to.  In the host form the staged other bytes count against the budget and the chunk weight with the frames: chunks
 *     are cut over max(in, out, other).
 *   - zarc_gpu_last_copy_bytes: H2D = sum of frame_len + sum of other_len in the host form, 0 in the device form; D2H = 0.
 *   - zarc_gpu_last_compare_ms: zarc_cmp_* summed over the parts of the call; <= 0 after any other call.  ZARC_GPU_T_TOTAL includes it.
 *     (The timer enum is not extended: ZARC_GPU_T_COUNT stays 14.)
 *   - Cost: decode and both hash passes are verify's and run in full; beside them both sides are read once, and where the lengths differ
 *     the common part of the other side a second time, shifted. */
enum { ZARC_GPU_CMP_NONE = 0,             /* the frame did not decode: every field 0 */
       ZARC_GPU_CMP_EQUAL = 1,            /* same length, same bytes */
       ZARC_GPU_CMP_DIFFER = 2,           /* a byte below min(raw_len, other_len) differs */
       ZARC_GPU_CMP_FRAME_IS_PREFIX = 3,  /* the content is a proper prefix of `other` (cmp: EOF on the archive's side) */
       ZARC_GPU_CMP_OTHER_IS_PREFIX = 4 };/* `other` is a proper prefix of the content */
#define ZARC_GPU_CMP_EOF 256u             /* byte_a / byte_b where that side has no byte at `prefix` */
typedef struct { uint32_t relation, byte_a, byte_b, reserved0;
                 uint64_t prefix, line, differing, suffix, reserved[2]; } zarc_gpu_cmp;   /* 64 bytes */
int zarc_gpu_compare_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                           const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN] /* or NULL */, const void *const *other, const size_t *other_len,
                           uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, zarc_gpu_cmp *res /* n */);
int zarc_gpu_compare_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                  const uint64_t *raw_len, const uint8_t *expect /* n*32 or NULL */, const void *d_other_base,
                                  const uint64_t *other_off, const uint64_t *other_len, uint8_t *digest /* n*32 */, int *status,
                                  zarc_gpu_cmp *res /* HOST, n */);
float zarc_gpu_last_compare_ms(const zarc_gpu_t *h);

/* ---- digest only (DigestType::verify_data, integrity.rs:107-117) ------------------------------- */
int zarc_gpu_blake3_batch(zarc_gpu_t *h, size_t n, const void *const *src, const size_t *len,
                          uint8_t (*digest)[ZARC_GPU_DIGEST_LEN]);
int zarc_gpu_blake3_batch_device(zarc_gpu_t *h, size_t n, const void *d_base, const uint64_t *off,
                                 const uint64_t *len, uint8_t *digest /* n*32 */);
/* XXH64(seed 0) of each entry (what libzstd appends/verifies as the frame checksum). */
int zarc_gpu_xxh64_batch_device(zarc_gpu_t *h, size_t n, const void *d_base, const uint64_t *off,
                                const uint64_t *len, uint64_t *out);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------- */
/* Device time of the kernels of the most recent batch call, measured with HIP events on the engine's
 * own stream.  `which` selects a kernel; returns milliseconds (<0 if not run). */
enum {
    ZARC_GPU_T_BLAKE3 = 0,    /* chunk + tree kernels                  */
    ZARC_GPU_T_XXH64 = 1,
    ZARC_GPU_T_MATCH = 2,     /* encoder: match finder                 */
    ZARC_GPU_T_ENTROPY = 3,   /* encoder: Huffman/FSE block coder      */
    ZARC_GPU_T_ASSEMBLE = 4,  /* encoder: frame assembly               */
    ZARC_GPU_T_DECODE = 5,    /* decoder                               */
    ZARC_GPU_T_TOTAL = 6,     /* pack: setup + match + entropy + assembly (the digest and the checksum run on side streams beside them and
                                 have their own entries); unpack / digest-only calls: first launch .. last launch                       */
    ZARC_GPU_T_DEC_SEQS = 7,  /* decoder stage 2: sequence entropy decoding (zarc_zdec_seqs)             */
    ZARC_GPU_T_DEC_LITS = 8,  /* decoder stage 2: Huffman literals (zarc_zdec_literals, side stream)      */
    ZARC_GPU_T_DEC_FRAMES = 9,/* decoder frame pass (zarc_zstd_frames + the inline decoder for the rest)  */
    ZARC_GPU_T_SEARCH = 10,   /* search: zarc_search_scan (a set: zarc_set_scan and zarc_set_which; a regex: zarc_regex_summary, _carry and _scan), summed over the parts of a call; < 0 or 0 after any other call */
    ZARC_GPU_T_LINES = 11,    /* search_lines: zarc_lines_* (mark, carry, emit, scan, gather; a set or a regex: its twins of mark and emit; select_lines: zarc_lines_select_* in place of mark, carry and emit; search_matches: zarc_matches_* behind emit, in place of scan and gather), summed over the parts of a call; < 0 or 0 after any other call */
    ZARC_GPU_T_RANGE = 12,    /* read_ranges: zarc_range_* (count, carry, locate, gather), summed over the parts of a call; < 0 or 0 after any other call */
    ZARC_GPU_T_WC = 13,       /* count: zarc_wc_* (count, carry), summed over the parts of a call; < 0 or 0 after any other call */
    ZARC_GPU_T_COUNT = 14
};
float zarc_gpu_last_kernel_ms(const zarc_gpu_t *h, int which);
/* Content bytes the most recent batch call moved between host and device (descriptor arrays, statuses, digests not counted).  Every
 * batch call sets them; the device-memory forms report 0.  H2D + D2H == RING + DIRECT. */
enum { ZARC_GPU_C_H2D = 0, ZARC_GPU_C_D2H = 1, ZARC_GPU_C_RING = 2 /* of those, through the pinned staging ring */,
       ZARC_GPU_C_DIRECT = 3 /* of those, DMA straight from/to the caller's page-locked memory */, ZARC_GPU_C_COUNT = 4 };
uint64_t zarc_gpu_last_copy_bytes(const zarc_gpu_t *h, int which);
/* Fill a device buffer with entries of the synthetic corpus; entry i of the
 * call is corpus entry first_index+i, kind = index mod 4 when kind < 0. */
int zarc_gpu_corpus_fill_device(zarc_gpu_t *h, size_t n, void *d_base, const uint64_t *off,
                                const uint64_t *len, uint64_t first_index, int kind);
/* Thin wrappers so that a ctypes-only caller can manage device memory without torch. */
int zarc_gpu_device_malloc(zarc_gpu_t *h, void **d_ptr, size_t bytes);
int zarc_gpu_device_free(zarc_gpu_t *h, void *d_ptr);
int zarc_gpu_memcpy_h2d(zarc_gpu_t *h, void *d_dst, const void *src, size_t bytes);
int zarc_gpu_memcpy_d2h(zarc_gpu_t *h, void *dst, const void *d_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
