// zarc_amd/csrc/zarc_kernels.h -- kernel entry points and the records they exchange through HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// per-frame status values; numerically identical to ZARC_GPU_FRAME_* in include/zarc_gpu.h
enum {
    ZARC_FRAME_OK = 0, ZARC_FRAME_CORRUPT = 1, ZARC_FRAME_CHECKSUM = 2, ZARC_FRAME_DIGEST = 3,
    ZARC_FRAME_DSTSIZE = 4, ZARC_FRAME_BAD_MAGIC = 5, ZARC_FRAME_UNSUPPORTED = 6, ZARC_FRAME_SRCSIZE = 7
};

constexpr uint32_t ZARC_BLOCK_MAX = 128 * 1024;      // Zstandard Block_Maximum_Size: what the decoder must take, what store-mode frames use
// The ENCODER's blocks are 64 KiB (round 4).  A block is the unit of everything that is serial in the format -- one Huffman table for its
// literals, one FSE state chain for its sequences -- so halving it doubles the decoder's parallelism (sequence and literal chains half as
// long) and lets the literal statistics follow the data (libzstd 1.5 splits blocks where they change: its frame of a libtorch slice has
// 112 blocks for 2 MiB).  Model, ours / libzstd -3, 128 -> 64 KiB: ELF tables 1.015 -> 0.999, package.json 1.033 -> 1.022, machine code
// 1.039 -> 1.033, the libtorch string tables 1.067 -> 1.049 (inside the contract), text +0.02 .. 0.1 %, GPU code objects 1.024 -> 1.038;
// 32 KiB: text +0.3 %, code objects 1.07.  The sequence tables are shared by groups of 16 blocks (1 MiB, as before).
constexpr uint32_t ZARC_BLOCK = 64 * 1024;
constexpr uint32_t ZARC_MAX_SEQ = ZARC_BLOCK / 3 + 8; // sequences per block (every match >= 3 bytes)

// ---- encoder tuning (mirrors oracle/zge_model.h zge_params; plain ints so the struct can be passed by value)
struct ZgeParams {
    int level, checksum, window_log, long_log, short_log, short_bytes, tile, sub, cap, min_match, min_rep, rep_search,
        back_cap, lazy, lazy_delta, lit_cost, match_cost, rep_cost, short_window_log, rep_back, tag_bits, seg_log,
        far_log, far_ways, far_step_log, far_res_log, far_short, far_skip, far_back, near16, far_cdc_log, far_min_frame, rep_pass, lazy2_delta, far_cap, cont_cap, ext_cap, live_reps, slot_bytes, dbg;
};
// Encoder scratch of one block slot (sequences, literals, coded block): sized by the largest block of the SUB-BATCH (slot_bytes <=
// ZARC_BLOCK, a multiple of 16) -- a batch of a million 1 KiB entries must not reserve 600 KiB per entry.
__host__ __device__ inline uint64_t zge_seq_stride(uint32_t slot_bytes) { return slot_bytes / 3 + 8; }   // sequences (8 bytes each)
__host__ __device__ inline uint64_t zge_lit_stride(uint32_t slot_bytes) { return (uint64_t)slot_bytes + 64; }
__host__ __device__ inline uint64_t zge_out_stride(uint32_t slot_bytes) { return (uint64_t)slot_bytes + 1024; }
// words of far-table scratch one match-finder workgroup needs (HBM): 2^far_log buckets x ways, once or twice
__host__ __device__ inline size_t zge_far_words(const ZgeParams &P) { return P.far_log ? (((size_t)P.far_ways << P.far_log) * (P.far_short ? 2 : 1)) : 0; }

// Per-block record written by the match finder and completed by the entropy coder.
struct ZgeBlock {
    uint32_t frame;      // entry index
    uint32_t index;      // block index inside the frame
    uint32_t src_len;    // uncompressed bytes in this block
    uint32_t nseq, nlit; // match finder output
    uint32_t type;       // 0 raw, 1 rle, 2 compressed (set by the entropy coder; rle by the match finder)
    uint32_t out_len;    // bytes of block content (without the 3-byte header)
    uint32_t pad;
};
// Sequence-table plan of one block (entropy stage, multi-block frames): written by pass 1 (code histograms, the block's own best table
// per type), settled per group of ZGE_TABLE_GROUP blocks by zarc_zge_plan (one shared table per type where that is cheap: the first
// block describes it, the others say Repeat_Mode), read by pass 2 (model: zstd_enc_model.c, seq_plan / seq_plan_group).
constexpr uint32_t ZGE_TABLE_GROUP = 16;
struct ZgePlanTable {
    int16_t norm[64];   // normalised counts of the table to code with (pass 1: the block's own choice; zarc_zge_plan: the group's)
    uint8_t desc[80];   // its FSE description (mode 2)
    uint32_t count[64]; // histogram of the block's codes of this type (zero beyond the largest code)
    uint32_t cost;      // the own choice's cost in 1/256 bit, description included (modes 0 and 2)
    uint8_t mode, al, nsym, dl, rle, pad[3]; // Symbol_Compression_Mode 0..3, accuracy log, symbols in norm[], description bytes, RLE symbol
};
struct ZgePlan {
    uint32_t active;     // 1 = pass 2 codes this block's sequences section (0: RLE / raw / no sequences: the block record is final)
    uint32_t nseq;       // sequences after joining
    uint32_t lsz;        // bytes of the literals section in front
    uint32_t extra_bits; // bits of all extra-bits fields (for the size bound)
    uint32_t guaranteed; // zarc_zge_plan: an upper bound of the coded size is below the raw size
    uint32_t states;     // zarc_zge_seq_states: 1 = the block's FSE states lie in its literal slot, pass 2 runs no chain (cleared by pass 1)
    uint32_t pad[2];
    ZgePlanTable t[3];   // LL, OF, ML
};
// zarc_zge_seq_states takes the chains of a run of blocks that code with the same tables, if the run has at least this many blocks
constexpr uint32_t ZGE_STATE_MIN_RUN = 4;
static_assert(sizeof(ZgePlanTable) == 476 && sizeof(ZgePlan) == 32 + 3 * 476, "plan record layout");
// Block splitting (ZARC_GPU_PX_BLOCK_SPLIT, off by default; zge_split.hip, model: tests/support/split_model.c).  A 64 KiB parent block
// becomes up to ZGE_SPLIT_K pieces = Zstandard blocks, cut at sequence boundaries where the literal statistics change.  Every parent
// owns ZGE_SPLIT_K piece slots (slot = parent * ZGE_SPLIT_K + k): a ZgeBlock record (type 3 = slot not used; pad of slot 0 = the
// parent's number of pieces), a ZgePiece that places the piece inside its parent's scratch slots, and a ZgePlan.
constexpr uint32_t ZGE_SPLIT_K = 16;          // chunks of a parent a cut can fall between, and so its largest number of pieces
constexpr uint32_t ZGE_SPLIT_PIECE_COST = 192; // bytes the cut rule charges per piece (headers, table descriptions, lost repeat codes)
constexpr uint32_t ZGE_PIECE_UNUSED = 3;      // ZgeBlock.type of an idle piece slot
struct ZgePiece {
    uint32_t seq_first; // first sequence (of the parent's joined ones); the count is the piece record's nseq
    uint32_t lit_first; // first literal; the count is the piece record's nlit
    uint32_t src_off;   // first source byte, relative to the parent; the length is the piece record's src_len
    uint32_t out_off;   // where the coded piece goes inside the parent's output slot ...
    uint32_t out_cap;   // ... and how many bytes it may take there (src_len + 64: whatever does not fit is a raw block anyway)
    uint32_t pad[3];
};
// one sequence: ofv (28 bits) | ll << 28 (18 bits) | ml << 46 (18 bits)
__host__ __device__ inline uint64_t zge_pack_seq(uint32_t ll, uint32_t ml, uint32_t ofv) { return (uint64_t)ofv | ((uint64_t)ll << 28) | ((uint64_t)ml << 46); }
__host__ __device__ inline uint32_t zge_seq_ofv(uint64_t s) { return (uint32_t)(s & 0xFFFFFFFu); }
__host__ __device__ inline uint32_t zge_seq_ll(uint64_t s) { return (uint32_t)((s >> 28) & 0x3FFFFu); }
__host__ __device__ inline uint32_t zge_seq_ml(uint64_t s) { return (uint32_t)((s >> 46) & 0x3FFFFu); }

// Decoder: one slot per block of a frame (the slots of frame f start at slot_prefix[f]); filled by zarc_zdec_scan.
struct ZdecBlock {
    uint32_t frame;    // frame index
    uint32_t type;     // 0 raw, 1 RLE, 2 compressed; 0xFFFFFFFF = slot not used
    uint32_t payload;  // frame offset of the block content (after the 3-byte block header)
    uint32_t size;     // Block_Size field
    uint32_t nseq;     // compressed blocks: Number_of_Sequences
    uint32_t seq_hdr;  // compressed blocks with sequences: frame offset of the Symbol_Compression_Modes byte
    uint32_t state;    // set to 1 by zarc_zdec_seqs once the block's sequences are in the sequence scratch
    uint32_t rep[3];   // repeat-offset history after the block, symbolic (see ZDEC_REP_REF): absolute, or "history slot at block start minus delta"
    uint32_t lit_type; // compressed blocks: Literals_Block_Type (0 raw, 1 RLE, 2 Huffman, 3 treeless)
    uint32_t lit_len;  // regenerated size of the literals
    uint32_t lit_off;  // Huffman literals: frame offset of the section body (tree description, then the streams)
    uint32_t lit_comp; // Huffman literals: bytes of that body
    uint32_t lit_streams; // 1 or 4
    uint32_t pad[3];   // [0] reach: bytes in front of the block its matches read at most (ZDEC_REACH_UNKNOWN: anywhere); [1] bytes the block regenerates
};
static_assert(sizeof(ZdecBlock) == 72, "block slot layout");
constexpr int ZDEC_LDS_LANES = 16;  // active lanes (= block slots) per wave of zarc_zdec_seqs_lds: 16 x 2.5 KiB of tables in LDS
constexpr uint32_t ZDEC_LONG_NSEQ = 768; // a block with at least this many sequences is zarc_zdec_seqs_lds's when the shared-table kernel has not done it
constexpr int ZDEC_LONG_BUCKETS = 16;    // ... listed by sequence count in buckets of 1 024 (the last one: 15 360 and more)
constexpr int ZDEC_LIT_GROUP = 16;  // block slots per wave of zarc_zdec_literals (4 Huffman streams each)
// Fast-path sequences are stored with zge_pack_seq(); the offset field is already resolved against the repeat-offset history
// as far as the block alone allows: bit 17 of the literal-length field set = the offset is (history slot at block start) - delta,
// the offset field then holds slot | delta << 2; otherwise the offset field is the absolute offset.
constexpr uint32_t ZARC_SPLIT_MIN = 4u << 20; // encoder: frames larger than this are searched segment by segment (2 MiB) by different workgroups
constexpr uint32_t ZDEC_LL_REF = 1u << 17;
constexpr uint32_t ZDEC_MAX_DELTA = 1u << 20; // "history slot minus delta": repeated `first history entry - 1` codes add up (libzstd -9 .. -19 on records-like data)
// A run of blocks of one frame that reads nothing in front of its first block: the unit of work of the fast frame pass (engine.hip).
struct ZdecPiece {
    uint32_t frame, first, count; // frame index; first block; number of blocks (a whole frame: first 0, count 0xFFFFFFFF)
    uint32_t rep[3];              // repeat-offset history in front of the first block
    uint64_t out_start, out_len;  // where the piece's output starts inside the frame's, and how many bytes its blocks regenerate
};
constexpr uint32_t ZDEC_REACH_UNKNOWN = 0xFFFFFFFFu; // ZdecBlock.pad[0]: the block's matches may reach anywhere in front of it
constexpr uint32_t ZDEC_REP_REF = 0x80000000u; // same idea for ZdecBlock::rep[]: REF | slot | delta << 2
constexpr int ZDEC_TABLE_CELLS = 1280; // per block slot: LL 512 + ML 512 + OF 256 FSE decode cells (u16)

// ---- kernels -----------------------------------------------------------------------------------
__global__ void zarc_blake3_chunks(const uint8_t *base, const uint64_t *off, const uint64_t *len, const uint64_t *chunk_prefix,
                                   uint32_t n_entries, uint64_t total_chunks, uint32_t *cvs, uint32_t *digests);
__global__ void zarc_blake3_tree(const uint64_t *chunk_prefix, uint32_t n_entries, uint32_t *cvs, uint32_t *tmp, uint32_t *digests);
__global__ void zarc_xxh64(const uint8_t *base, const uint64_t *off, const uint64_t *len, uint32_t n_entries, uint64_t *out);
__global__ void zarc_zstd_decode(const uint8_t *frames_base, const uint64_t *frame_off, const uint64_t *frame_len, uint8_t *dst_base,
                                 const uint64_t *dst_off, const uint64_t *raw_len, const uint32_t *order, uint32_t n_frames,
                                 uint8_t *lit_scratch, int32_t *status, uint32_t *stored_checksum, int dbg, uint32_t *queue,
                                 const uint32_t *fast /* per frame: handled by zarc_zstd_frames; null = take every frame */);
// frame pass of the decoder fast path: frames whose sequences and literals were decoded ahead (fast[f] != 0)
__global__ void zarc_zstd_frames(const uint8_t *frames_base, const uint64_t *frame_off, const uint64_t *frame_len, uint8_t *dst_base,
                                 const uint64_t *dst_off, const uint64_t *raw_len, const ZdecPiece *pieces, uint32_t n_listed /* pieces[] holds this many */,
                                 uint32_t first_unlisted /* behind them: frames first_unlisted .. as one piece each */, uint32_t n_pieces, int32_t *status,
                                 uint32_t *stored_checksum, int dbg, uint32_t *queue, const uint32_t *fast, const uint64_t *slot_prefix,
                                 const ZdecBlock *zblocks, const uint64_t *seq_index, const uint64_t *seqs, const uint64_t *lit_index,
                                 const uint8_t *lits);
__global__ void zarc_gather(const uint8_t *src_base, const uint64_t *src_off, const uint64_t *len, const uint64_t *dense_off, uint32_t n, uint8_t *dst);
__global__ void zarc_zge_store(const uint8_t *src_base, const uint64_t *src_off, const uint64_t *src_len, uint32_t n_frames, uint8_t *dst_base,
                               const uint64_t *dst_off, uint64_t *dst_len);
// exclusive prefix sum of in[i * stride] (at least `floor` each) -> out[0 .. n] and *total; one workgroup of 1024 threads
__global__ void zarc_scan_u32(const uint32_t *in, uint32_t stride, uint32_t floor_, uint64_t n, uint64_t *out, uint64_t *total);
// decoder fast path, stage 1: one LANE per frame walks the block headers (no payload is touched) -> block slots, nseq[], fast[]
__global__ void zarc_zdec_count(const uint8_t *frames_base, const uint64_t *frame_off, const uint64_t *frame_len, const uint64_t *raw_len, uint32_t n_frames,
                                uint32_t *nblocks);
__global__ void zarc_zdec_scan(const uint8_t *frames_base, const uint64_t *frame_off, const uint64_t *frame_len, const uint64_t *raw_len,
                               uint32_t n_frames, const uint64_t *slot_prefix, ZdecBlock *zblocks, uint32_t *counts /* per slot: nseq, Huffman literal bytes */,
                               uint32_t *fast);
// Huffman literals of the fast path: one wave per ZDEC_LIT_GROUP block slots (tables in LDS, one stream per lane) -> lits[]
__global__ void zarc_zdec_literals(const uint8_t *frames_base, const uint64_t *frame_off, uint64_t n_slots, const uint64_t *slot_prefix,
                                   const ZdecBlock *zblocks, const uint64_t *lit_index, uint8_t *lits, uint32_t *fast, uint64_t slot_base);
// stage 2, every lane's own tables in LDS (one wave of ZDEC_LDS_LANES active lanes per workgroup): the compressed blocks of at least
// ZDEC_LONG_NSEQ sequences that zarc_zdec_seqs_shared has not done, from a list ordered by sequence count (zarc_zdec_long_count / _fill);
// zarc_zdec_seqs (split_long) leaves exactly those alone
__global__ void zarc_zdec_long_count(const ZdecBlock *zblocks, uint64_t slot_base, uint64_t n_slots, const uint32_t *wave_flag, uint32_t *counters);
__global__ void zarc_zdec_long_fill(const ZdecBlock *zblocks, uint64_t slot_base, uint64_t n_slots, const uint32_t *wave_flag, uint32_t *counters,
                                    uint32_t *list);
__global__ void zarc_zdec_seqs_lds(const uint8_t *frames_base, const uint64_t *frame_off, uint64_t n_slots, const uint64_t *slot_prefix,
                                   ZdecBlock *zblocks, const uint64_t *seq_index, uint64_t *seqs, uint32_t *fast, uint64_t slot_base,
                                   const uint32_t *counters, const uint32_t *list);
// stage 2: one LANE per block slot entropy-decodes the block's sequences (FSE tables in HBM scratch) into seqs[]; with wave_flag only the
// 64-slot waves zarc_zdec_seqs_shared turned down
__global__ void zarc_zdec_seqs(const uint8_t *frames_base, const uint64_t *frame_off, uint64_t n_slots, const uint64_t *slot_prefix,
                               ZdecBlock *zblocks, const uint64_t *seq_index, uint64_t *seqs, uint16_t *tables, uint32_t *fast, uint64_t slot_base,
                               const uint32_t *wave_flag /* may be null */, const uint16_t *predef /* zarc_zdec_predef's tables, or null */,
                               int split_long /* 1: blocks with a long chain are zarc_zdec_seqs_lds's */);
constexpr int ZDEC_PREDEF_LL = 0, ZDEC_PREDEF_OF = 64, ZDEC_PREDEF_ML = 96, ZDEC_PREDEF_CELLS = 160;
__global__ void zarc_zdec_predef(uint16_t *out);
// stage 2 with the tables shared by a wave's 64 blocks in LDS (Repeat_Mode / equal descriptions); sets wave_flag[wave] where they do not fit
__global__ void zarc_zdec_seqs_shared(const uint8_t *frames_base, const uint64_t *frame_off, uint64_t n_slots, const uint64_t *slot_prefix,
                                      ZdecBlock *zblocks, const uint64_t *seq_index, uint64_t *seqs, uint32_t *fast, uint64_t slot_base,
                                      uint32_t *wave_flag);
// the same with 32 / 16 block slots per workgroup (a flag per workgroup; the launch of zarc_zdec_seqs behind it uses the same width)
__global__ void zarc_zdec_seqs_shared32(const uint8_t *frames_base, const uint64_t *frame_off, uint64_t n_slots, const uint64_t *slot_prefix,
                                        ZdecBlock *zblocks, const uint64_t *seq_index, uint64_t *seqs, uint32_t *fast, uint64_t slot_base,
                                        uint32_t *wave_flag);
__global__ void zarc_zdec_seqs_shared16(const uint8_t *frames_base, const uint64_t *frame_off, uint64_t n_slots, const uint64_t *slot_prefix,
                                        ZdecBlock *zblocks, const uint64_t *seq_index, uint64_t *seqs, uint32_t *fast, uint64_t slot_base,
                                        uint32_t *wave_flag);
// status[i]: keeps decode errors (and clears the digest of such a frame); else CHECKSUM if the stored XXH64 differs; else DIGEST if expect differs
__global__ void zarc_unpack_verdict(uint32_t n, const uint64_t *xxh, const uint32_t *stored_checksum, uint32_t *digests,
                                    const uint32_t *expect /* may be null */, int32_t *status);
// read-back check of a pack call (zge_check.hip): decoded bytes against source bytes, a workgroup per (frame, slice); arrays without a
// note are in the decoder's order, the others are the pack call's own (indexed by entry0 + entry_of[i]).  first_bad[i] (start:
// ZARC_CHECK_CLEAN) receives the lowest differing byte offset, or ZARC_CHECK_TRAILER when only the checksum trailer differs
constexpr uint32_t ZARC_CHECK_SLICE = 65536, ZARC_CHECK_CLEAN = 0xFFFFFFFFu, ZARC_CHECK_TRAILER = 0xFFFFFFFEu;
__global__ void zarc_check_compare(uint32_t n, const uint64_t *slice_prefix, const uint32_t *entry_of, uint32_t entry0, const uint8_t *dec_base,
                                   const uint64_t *dec_off, const int32_t *dec_status, const uint8_t *src_base, const uint64_t *src_off /* pack */,
                                   const uint64_t *src_len /* pack */, const uint8_t *frame_base, const uint64_t *frame_off /* pack */,
                                   const uint64_t *frame_len /* pack */, const uint64_t *xxh /* pack; null = no trailer to look at */, uint32_t *first_bad);
// repack (zge_repack.hip): the decode half's per-frame arrays (decoder order) -> the pack pass's per-entry arrays (entry_of[i] = the entry
// of frame i); a frame whose status is not OK becomes an entry of no bytes
__global__ void zarc_repack_plan(uint32_t n, const uint32_t *entry_of, const int32_t *status, const uint64_t *dec_off, const uint64_t *raw_len,
                                 const uint64_t *dec_xxh, uint64_t *src_off /* pack */, uint64_t *src_len /* pack */, uint64_t *xxh /* pack */);
// search (zdec_search.hip): one byte string of m bytes (1 .. ZARC_SEARCH_MAX_PATTERN; folded by the host when icase) in the decoded bytes of
// every frame whose status is OK or DIGEST, a workgroup per (frame, slice of ZARC_CHECK_SLICE start positions); every array is in the
// decoder's order.  count[i] (start: 0) += matching start positions, first[i] (start: 0xFFFFFFFF) = the lowest of them
constexpr uint32_t ZARC_SEARCH_MAX_PATTERN = 256;
__global__ void zarc_search_scan(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                 const int32_t *status, const uint8_t *pattern, uint32_t m, uint32_t icase, uint32_t *count, uint32_t *first);
// the matching lines of a search (zdec_lines.hip), on the grid of zarc_search_scan; every per-frame array is in the decoder's order.
// ZarcLineSlice: what zarc_lines_mark finds in a slice (positions count from the slice's first byte) and what zarc_lines_carry adds of the
// slices around it (positions count from the frame's first byte)
struct ZarcLineSlice {
    uint32_t nl_count, first_nl, last_nl; // mark: 0x0A bytes of the slice, the first and the last one
    uint32_t nlow;                        // mark: lines that begin behind the slice's first 0x0A and have their lowest match in the slice
    uint32_t flags;                       // mark: 1 = a match in front of the first 0x0A, 2 = behind the last (no 0x0A: anywhere); carry: 4 = the
                                          // line open at the slice's start holds a match in an earlier slice
    uint32_t open_start, nl_base, excl;   // carry: where that line starts; 0x0A bytes and matching lines of the frame in front of the slice
    uint32_t next_end;                    // carry: the first 0x0A behind the slice, or the frame's length
    uint32_t pad;
};
struct ZarcLineRec { uint64_t frame, start, length, number, match, text_off, text_len; }; // zarc_gpu_line; frame: the decoder's index
__global__ void zarc_lines_mark(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                const int32_t *status, const uint8_t *pattern, uint32_t m, uint32_t icase, ZarcLineSlice *slices, uint32_t *lines);
__global__ void zarc_lines_carry(uint32_t n, const uint64_t *slice_prefix, const uint64_t *raw_len, ZarcLineSlice *slices, uint32_t *lines);
// rec_base[i] / deliver[i]: where frame i's records begin in rec[] and how many of its first matching lines get one
__global__ void zarc_lines_emit(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                const uint8_t *pattern, uint32_t m, uint32_t icase, const ZarcLineSlice *slices, const uint64_t *rec_base,
                                const uint32_t *deliver, uint32_t max_line, ZarcLineRec *rec);
__global__ void zarc_lines_scan(uint64_t nrec, ZarcLineRec *rec, uint64_t *total);
__global__ void zarc_lines_gather(uint64_t nrec, const ZarcLineRec *rec, const uint8_t *dec_base, const uint64_t *dec_off, uint8_t *text);
// a set of patterns in one pass (zdec_search_set.hip).  `set` is the blob search_upload_set (engine.hip) compiles: words [0, lds_words) are
// the image a workgroup keeps in LDS -- per length class c (0, 1, 2: patterns of 1, 2, 3 bytes; 3: of 4 bytes and more, keyed by their
// first four) a bit filter of 1 << flog[c] bits at word foff[c] and an exact table of 1 << tlog[c] slots {key, list} at word toff[c]
// (list: a word index into the blob, 0 = an empty slot) -- then the lists {n, n pattern indices}, at word pat_off {first word of the
// bytes, length} per pattern, and the patterns' bytes padded to words.  hits[k] += positions at which pattern k matches (may be null).
constexpr uint32_t ZARC_SEARCH_MAX_SET = 1024;
constexpr uint32_t ZARC_SET_HASH = 0x9E3779B1u; // filter bit and first table slot of a key: the top bits of key * this (one-byte class: the filter bit is the key)
struct ZarcSetDesc {
    uint32_t count, classes;      // patterns; bit c = the set holds patterns of class c
    uint32_t lds_words, min_len;  // words of the LDS image; the shortest pattern
    uint32_t pat_off;
    uint32_t flog[4], tlog[4], foff[4], toff[4];
};
__global__ void zarc_set_scan(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                              const int32_t *status, ZarcSetDesc sd, const uint32_t *set, uint32_t icase, uint32_t *count, uint32_t *first, uint32_t *hits);
__global__ void zarc_set_which(uint32_t n, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len, ZarcSetDesc sd, const uint32_t *set,
                               uint32_t icase, const uint32_t *count, const uint32_t *first, uint32_t *which);
__global__ void zarc_lines_mark_set(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                    const int32_t *status, ZarcSetDesc sd, const uint32_t *set, uint32_t icase, ZarcLineSlice *slices, uint32_t *lines);
__global__ void zarc_lines_emit_set(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                    ZarcSetDesc sd, const uint32_t *set, uint32_t icase, const ZarcLineSlice *slices, const uint64_t *rec_base,
                                    const uint32_t *deliver, uint32_t max_line, ZarcLineRec *rec);
// a regular expression (zdec_regex.hip).  ZarcRegexDfa is zarc_gpu_regex_dfa, the table zre_compile.h makes: it reads a line from its last
// byte to its first.  ZarcRegexSlice: what reading a slice from its last byte to its first does to the state -- a constant when the slice
// holds a 0x0A (the automaton restarts there), else one exit state per entry state.  entry[s] (zarc_regex_carry): the state in front of
// slice s's last byte; slices of frames of one slice have no record and no entry (their entry state is dfa->start).
constexpr uint32_t ZARC_REGEX_MAX_STATES = 64;
struct ZarcRegexDfa { uint32_t states, start; uint8_t accept[ZARC_REGEX_MAX_STATES]; uint8_t delta[ZARC_REGEX_MAX_STATES * 256]; };
struct ZarcRegexSlice { uint8_t constant, value, pad[2]; uint8_t table[ZARC_REGEX_MAX_STATES]; };
__global__ void zarc_regex_summary(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                   const int32_t *status, const ZarcRegexDfa *dfa, ZarcRegexSlice *summary);
__global__ void zarc_regex_carry(uint32_t n, const uint64_t *slice_prefix, const int32_t *status, const ZarcRegexDfa *dfa, const ZarcRegexSlice *summary,
                                 uint8_t *entry);
__global__ void zarc_regex_scan(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                const int32_t *status, const ZarcRegexDfa *dfa, const uint8_t *entry, uint32_t *count, uint32_t *first);
__global__ void zarc_lines_mark_regex(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                      const int32_t *status, const ZarcRegexDfa *dfa, const uint8_t *entry, ZarcLineSlice *slices, uint32_t *lines);
__global__ void zarc_lines_emit_regex(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                      const ZarcRegexDfa *dfa, const uint8_t *entry, const ZarcLineSlice *slices, const uint64_t *rec_base,
                                      const uint32_t *deliver, uint32_t max_line, ZarcLineRec *rec);
// the selected lines of a search (zdec_select.hip): the lines within `before` in front of and `after` behind a hit line -- a matching line,
// with invert a line without a match.  A line belongs to the slice in which it ends.  ZarcSelSlice: what zarc_lines_select_mark* finds in a
// slice and what zarc_lines_select_carry makes of it with the slices around (positions as in ZarcLineSlice; numbers are line numbers)
struct ZarcSelect { uint32_t invert, before, after; };
struct ZarcSelSlice {
    uint32_t nl_count, first_nl, last_nl; // mark: 0x0A bytes of the slice, the first and the last one
    uint32_t flags;                       // mark: 1 = a match in front of the first 0x0A, 2 = behind the last (no 0x0A: anywhere), 8 = the frame's
                                          // unterminated last line ends here; carry: 4 = the line open at the slice's start holds a match in an earlier slice
    uint32_t hits, first_hit, last_hit;   // mark: of the lines that end in the slice, the first one left out: hit lines, the rank (from 1) of the first
                                          // and the last, 0 = none; carry: of all of them, and the NUMBERS of the first and the last
    uint32_t sel;                         // mark: lines ending in the slice that those hits select; carry: that all hits of the frame select
    uint32_t tail_low;                    // mark: the lowest match of the line left open at the slice's end, or 0xFFFFFFFF
    uint32_t open_start, open_low;        // carry: where the line open at the slice's start starts; its lowest match in earlier slices, or 0xFFFFFFFF
    uint32_t nl_base;                     // carry: 0x0A bytes of the frame in front of the slice
    uint32_t prev_hit, next_hit;          // carry: the last hit line ending in front of the slice (0: none), the first ending behind it (0xFFFFFFFF: none)
    uint32_t next_end, sel_excl;          // carry: the first 0x0A behind the slice, or the frame's length; selected lines of the frame in front of the slice
};
__global__ void zarc_lines_select_mark(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                       const int32_t *status, const uint8_t *pattern, uint32_t m, uint32_t icase, ZarcSelect q, ZarcSelSlice *slices);
__global__ void zarc_lines_select_mark_set(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                           const int32_t *status, ZarcSetDesc sd, const uint32_t *set, uint32_t icase, ZarcSelect q, ZarcSelSlice *slices);
__global__ void zarc_lines_select_mark_regex(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                             const int32_t *status, const ZarcRegexDfa *dfa, const uint8_t *entry, ZarcSelect q, ZarcSelSlice *slices);
// lines[i] = the frame's hit lines, selected[i] = its selected lines
__global__ void zarc_lines_select_carry(uint32_t n, const uint64_t *slice_prefix, const uint64_t *raw_len, ZarcSelect q, ZarcSelSlice *slices, uint32_t *lines,
                                        uint32_t *selected);
// rec_base[i] / deliver[i]: where frame i's records begin in rec[] and how many of its first selected lines get one
__global__ void zarc_lines_select_emit(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                       const uint8_t *pattern, uint32_t m, uint32_t icase, ZarcSelect q, const ZarcSelSlice *slices, const uint64_t *rec_base,
                                       const uint32_t *deliver, uint32_t max_line, ZarcLineRec *rec);
__global__ void zarc_lines_select_emit_set(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                           ZarcSetDesc sd, const uint32_t *set, uint32_t icase, ZarcSelect q, const ZarcSelSlice *slices,
                                           const uint64_t *rec_base, const uint32_t *deliver, uint32_t max_line, ZarcLineRec *rec);
__global__ void zarc_lines_select_emit_regex(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                             const ZarcRegexDfa *dfa, const uint8_t *entry, ZarcSelect q, const ZarcSelSlice *slices, const uint64_t *rec_base,
                                             const uint32_t *deliver, uint32_t max_line, ZarcLineRec *rec);
// every match of the delivered matching lines (zdec_matches.hip): a lane per line record of the part (lrec, as zarc_lines_emit* left them).
// ZarcMatchRec is zarc_gpu_match; frame: the decoder's index.  fdfa: the forward table of zarc_gpu_regex_compile_ends.  bits: the lines'
// start bits, record k's from word bit_off[k] on.  prefix[k]: the part's matches in front of line k; matches below `limit` get a record.
struct ZarcMatchRec { uint64_t frame, start, length, number, line_start, which, text_off, text_len; };
__global__ void zarc_matches_count(uint64_t nrec, const ZarcLineRec *lrec, const uint8_t *dec_base, const uint64_t *dec_off, const uint8_t *pattern, uint32_t m,
                                   uint32_t icase, uint32_t *counts);
__global__ void zarc_matches_count_set(uint64_t nrec, const ZarcLineRec *lrec, const uint8_t *dec_base, const uint64_t *dec_off, ZarcSetDesc sd, const uint32_t *set,
                                       uint32_t icase, uint32_t *counts);
__global__ void zarc_matches_count_regex(uint64_t nrec, const ZarcLineRec *lrec, const uint8_t *dec_base, const uint64_t *dec_off, const ZarcRegexDfa *dfa,
                                         const ZarcRegexDfa *fdfa, const uint64_t *bit_off, uint32_t *bits, uint32_t *counts);
__global__ void zarc_matches_emit(uint64_t nrec, const ZarcLineRec *lrec, const uint8_t *dec_base, const uint64_t *dec_off, const uint8_t *pattern, uint32_t m,
                                  uint32_t icase, const uint64_t *prefix, uint64_t limit, uint32_t max_line, ZarcMatchRec *mrec);
__global__ void zarc_matches_emit_set(uint64_t nrec, const ZarcLineRec *lrec, const uint8_t *dec_base, const uint64_t *dec_off, ZarcSetDesc sd, const uint32_t *set,
                                      uint32_t icase, const uint64_t *prefix, uint64_t limit, uint32_t max_line, ZarcMatchRec *mrec);
__global__ void zarc_matches_emit_regex(uint64_t nrec, const ZarcLineRec *lrec, const uint8_t *dec_base, const uint64_t *dec_off, const ZarcRegexDfa *fdfa,
                                        const uint64_t *bit_off, const uint32_t *bits, const uint64_t *prefix, uint64_t limit, uint32_t max_line, ZarcMatchRec *mrec);
// what 0 / 1: out[0 .. nrec] = exclusive sums (and the total) of the lines' bit words / of counts[]; 2: mrec[k].text_off, out[0] = the sum of text_len
__global__ void zarc_matches_scan(uint32_t what, uint64_t nrec, const ZarcLineRec *lrec, const uint32_t *counts, ZarcMatchRec *mrec, uint64_t *out);
__global__ void zarc_matches_gather(uint64_t nrec, const ZarcMatchRec *rec, const uint8_t *dec_base, const uint64_t *dec_off, uint8_t *text);
// byte and line ranges of the decoded frames (zdec_ranges.hip); every per-frame array is in the decoder's order.  ZarcRangeReq is
// zarc_gpu_range.  ZarcRangeFrame: what zarc_range_carry works out -- T, a, b - a, and per boundary (0: unit a, 1: unit b) either its
// byte offset, or the slice of the part's grid that holds its 0x0A and which 0x0A of that slice it is (1-based); zarc_range_locate turns
// the latter into offsets.  open[]: the boundaries (frame * 2 + which) that wait for it, *open_count of them (start: 0).
// ZarcRangeCopy: `len` bytes from `start` of frame `frame` to text + dst; block_prefix counts the 64 KiB blocks of the copies in front.
constexpr uint32_t ZARC_RANGE_BYTES = 0, ZARC_RANGE_LINES = 1, ZARC_RANGE_FROM_END = 1, ZARC_RANGE_NONE = 0xFFFFFFFFu;
struct ZarcRangeReq { uint32_t unit, flags; uint64_t skip, take; };
struct ZarcRangeFrame { uint32_t units, first, taken, pos[2], slice[2], ord[2], decoded; };
struct ZarcRangeCopy { uint64_t dst; uint32_t frame, start, len, pad; };
__global__ void zarc_range_count(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                 const int32_t *status, const ZarcRangeReq *req, uint32_t *cnt);
__global__ void zarc_range_carry(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                                 const int32_t *status, const ZarcRangeReq *req, const uint32_t *cnt, ZarcRangeFrame *out, uint32_t *open,
                                 uint32_t *open_count);
__global__ void zarc_range_locate(const uint32_t *open, const uint32_t *open_count, const uint64_t *slice_prefix, const uint8_t *dec_base,
                                  const uint64_t *dec_off, const uint64_t *raw_len, ZarcRangeFrame *out);
__global__ void zarc_range_gather(uint32_t m, const uint64_t *block_prefix, const ZarcRangeCopy *plan, const uint8_t *dec_base, const uint64_t *dec_off,
                                  uint8_t *text);
// line, word, character and longest-line counts of the decoded frames (zdec_wc.hip); every per-frame array is in the decoder's order.
// ZarcWcSlice: what zarc_wc_count knows of one slice of the part's grid -- its 0x0A bytes, word starts and bytes that are no UTF-8
// continuation byte; its first and last 0x0A (absolute offsets in the frame; ZARC_WC_NONE: none); the longest line between two 0x0A
// bytes of the slice (best_len ZARC_WC_NONE: none), where it starts and how many 0x0A bytes of the slice lie in front of it.
// ZarcWcFrame is zarc_gpu_wc.
constexpr uint32_t ZARC_WC_NONE = 0xFFFFFFFFu;
struct ZarcWcSlice { uint32_t nls, words, chars, first, last, best_len, best_start, best_ord; };
struct ZarcWcFrame { uint64_t lines, words, chars, max_line, max_line_start, max_line_no, reserved[2]; };
__global__ void zarc_wc_count(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                              const int32_t *status, ZarcWcSlice *rec);
__global__ void zarc_wc_carry(uint32_t n, const uint64_t *slice_prefix, const uint64_t *raw_len, const int32_t *status, const ZarcWcSlice *rec,
                              ZarcWcFrame *out);
// the decoded frames against other bytes (zdec_compare.hip); every per-frame array is in the decoder's order.  Frame i's other side lies at
// oth_base + oth_off[i] (16-byte aligned, padding behind it), oth_len[i] bytes.  ZarcCmpSlice: what zarc_cmp_scan knows of one slice of the
// part's grid, over the positions below common = min(raw_len, oth_len) -- its differing bytes, the lowest and the highest of them
// (absolute offsets in the frame; ZARC_CMP_NONE: none), its 0x0A bytes of the frame's side, and those of them in front of `lo`; and, where
// the lengths differ, the highest position of the slice whose byte is not the one that far from the other side's end (`back`).
// ZarcCmpFrame is zarc_gpu_cmp.
constexpr uint32_t ZARC_CMP_NONE = 0xFFFFFFFFu;
constexpr uint32_t ZARC_CMP_R_NONE = 0, ZARC_CMP_R_EQUAL = 1, ZARC_CMP_R_DIFFER = 2, ZARC_CMP_R_FRAME_IS_PREFIX = 3, ZARC_CMP_R_OTHER_IS_PREFIX = 4; // zarc_gpu_cmp.relation
constexpr uint32_t ZARC_CMP_EOF = 256; // ZARC_GPU_CMP_EOF
struct ZarcCmpSlice { uint32_t differing, lo, hi, nls, nl_before, back, pad[2]; };
struct ZarcCmpFrame { uint32_t relation, byte_a, byte_b, reserved0; uint64_t prefix, line, differing, suffix, reserved[2]; };
__global__ void zarc_cmp_scan(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                              const int32_t *status, const uint8_t *oth_base, const uint64_t *oth_off, const uint64_t *oth_len, ZarcCmpSlice *rec);
__global__ void zarc_cmp_carry(uint32_t n, const uint64_t *slice_prefix, const uint8_t *dec_base, const uint64_t *dec_off, const uint64_t *raw_len,
                               const int32_t *status, const uint8_t *oth_base, const uint64_t *oth_off, const uint64_t *oth_len,
                               const ZarcCmpSlice *rec, ZarcCmpFrame *out);
__global__ void zarc_corpus_fill(uint8_t *base, const uint64_t *off, const uint64_t *len, uint32_t n, uint64_t first_index, int kind);

// encoder
__global__ void zarc_zge_match(ZgeParams P, const uint8_t *src_base, const uint64_t *src_off, const uint64_t *src_len,
                               const uint32_t *order, const uint32_t *units /* (queue slot, first block) per 2 MiB segment */, uint32_t n_units, const uint64_t *block_prefix, ZgeBlock *blocks,
                               uint64_t *seq_scratch, uint8_t *lit_scratch, uint32_t *queue, uint32_t *far_scratch);
// the fast finder (level 1 and below): the same near table, no far table, no lazy step, no extension round
__global__ void zarc_zge_match_fast(ZgeParams P, const uint8_t *src_base, const uint64_t *src_off, const uint64_t *src_len,
                                    const uint32_t *order, const uint32_t *units, uint32_t n_units, const uint64_t *block_prefix, ZgeBlock *blocks,
                                    uint64_t *seq_scratch, uint8_t *lit_scratch, uint32_t *queue, uint32_t *far_scratch);
// the same with the ZARC_GPU_DBG switches (diagnostic build only)
__global__ void zarc_zge_match_diag(ZgeParams P, const uint8_t *src_base, const uint64_t *src_off, const uint64_t *src_len,
                               const uint32_t *order, const uint32_t *units /* (queue slot, first block) per 2 MiB segment */, uint32_t n_units, const uint64_t *block_prefix, ZgeBlock *blocks,
                               uint64_t *seq_scratch, uint8_t *lit_scratch, uint32_t *queue, uint32_t *far_scratch);
// the deep finder (level >= 9): same arguments; two tagged tables, 4-byte short hash, two-way far tables, live recent-offset rounds
__global__ void zarc_zge_match_deep(ZgeParams P, const uint8_t *src_base, const uint64_t *src_off, const uint64_t *src_len,
                                    const uint32_t *order, const uint32_t *units /* (queue slot, first block) per 2 MiB segment */, uint32_t n_units, const uint64_t *block_prefix, ZgeBlock *blocks,
                                    uint64_t *seq_scratch, uint8_t *lit_scratch, uint32_t *queue, uint32_t *far_scratch);
#ifdef ZARC_GPU_DIAG
__global__ void zarc_zge_match_deep_diag(ZgeParams P, const uint8_t *src_base, const uint64_t *src_off, const uint64_t *src_len,
                                    const uint32_t *order, const uint32_t *units /* (queue slot, first block) per 2 MiB segment */, uint32_t n_units, const uint64_t *block_prefix, ZgeBlock *blocks,
                                    uint64_t *seq_scratch, uint8_t *lit_scratch, uint32_t *queue, uint32_t *far_scratch);
#endif
// entropy stage, everything in one pass (sub-batches without a multi-block frame: every block chooses its tables alone)
__global__ void zarc_zge_entropy(uint32_t n_blocks, uint32_t slot_bytes, ZgeBlock *blocks, uint64_t *seq_scratch, const uint8_t *lit_scratch,
                                 uint8_t *out_scratch, unsigned long long *prof);
// ... or in two passes around the table plan: literals + sequence pre-pass + histograms + own choices -> plans[]; the plan; sequences
__global__ void zarc_zge_entropy_p1(uint32_t n_blocks, uint32_t slot_bytes, ZgeBlock *blocks, uint64_t *seq_scratch, const uint8_t *lit_scratch,
                                    uint8_t *out_scratch, unsigned long long *prof, ZgePlan *plans);
__global__ void zarc_zge_plan(uint32_t n_blocks, const ZgeBlock *blocks, ZgePlan *plans, const uint32_t *group_start);
// between the plan and pass 2 (ZARC_GPU_PX_SEQ_STATES): a wave per group runs the FSE state chains of the blocks that code with the same
// tables side by side and leaves their states in the blocks' literal slots (`cap_words` of a slot may be used); pass 2 then runs no chain
__global__ void zarc_zge_seq_states(uint32_t n_blocks, uint32_t slot_bytes, const ZgeBlock *blocks, const uint64_t *seq_scratch, uint8_t *lit_scratch,
                                    ZgePlan *plans, const uint32_t *group_start, uint32_t cap_words, unsigned long long *prof);
// (*err |= 1 when a block the plan `guaranteed` to end up compressed did not: its successor may repeat tables the decoder never saw)
__global__ void zarc_zge_entropy_p2(uint32_t n_blocks, uint32_t slot_bytes, ZgeBlock *blocks, uint64_t *seq_scratch, const uint8_t *lit_scratch,
                                    uint8_t *out_scratch, unsigned long long *prof, ZgePlan *plans, uint32_t *err);
__global__ void zarc_zge_assemble(ZgeParams P, const uint8_t *src_base, const uint64_t *src_off, const uint64_t *src_len,
                                  const uint32_t *order, uint32_t n_frames, const uint64_t *block_prefix, const ZgeBlock *blocks, const uint8_t *out_scratch,
                                  const uint64_t *xxh, uint8_t *dst_base, const uint64_t *dst_off, uint64_t *dst_len);
// ---- block splitting on: the cut decision, then the same stages over the parents' pieces (pblocks / plans / pieces: ZGE_SPLIT_K slots per parent)
__global__ void zarc_zge_split(uint32_t n_blocks, uint32_t slot_bytes, const ZgeBlock *blocks, uint64_t *seq_scratch, const uint8_t *lit_scratch,
                               ZgeBlock *pblocks, ZgePiece *pieces);
__global__ void zarc_zge_entropy_split(uint32_t n_blocks, uint32_t slot_bytes, ZgeBlock *pblocks, uint64_t *seq_scratch, const uint8_t *lit_scratch,
                                       uint8_t *out_scratch, unsigned long long *prof, const ZgePiece *pieces);
__global__ void zarc_zge_entropy_p1_split(uint32_t n_blocks, uint32_t slot_bytes, ZgeBlock *pblocks, uint64_t *seq_scratch, const uint8_t *lit_scratch,
                                          uint8_t *out_scratch, unsigned long long *prof, ZgePlan *plans, const ZgePiece *pieces);
__global__ void zarc_zge_plan_split(uint32_t n_blocks, const ZgeBlock *blocks, ZgePlan *plans, const uint32_t *group_start, const ZgeBlock *pblocks);
__global__ void zarc_zge_entropy_p2_split(uint32_t n_blocks, uint32_t slot_bytes, ZgeBlock *pblocks, uint64_t *seq_scratch, const uint8_t *lit_scratch,
                                          uint8_t *out_scratch, unsigned long long *prof, ZgePlan *plans, uint32_t *err, const ZgePiece *pieces);
__global__ void zarc_zge_assemble_split(ZgeParams P, const uint8_t *src_base, const uint64_t *src_off, const uint64_t *src_len,
                                        const uint32_t *order, uint32_t n_frames, const uint64_t *block_prefix, const ZgeBlock *blocks, const uint8_t *out_scratch,
                                        const uint64_t *xxh, uint8_t *dst_base, const uint64_t *dst_off, uint64_t *dst_len, const ZgeBlock *pblocks,
                                        const ZgePiece *pieces);
