// zarc_amd/csrc/engine.hip -- host side of the C ABI declared in include/zarc_gpu.h.
//
// One handle owns its HIP streams on one device (the engine stream plus two side streams for kernels and copies
// that may overlap it) and grow-only workspaces in HBM.  A batch call uploads the small per-entry descriptors,
// launches the kernel chain, times each stage with HIP events recorded on the stream the stage runs on, and copies
// back only per-entry results (lengths, digests, status).  The host-pointer entry points add chunked staging through
// a pinned ring with a few copy threads.  There is no CPU implementation of the codec behind this file: every
// data-path byte is hashed, matched, coded and decoded by the gfx950 kernels.
#include "../../include/zarc_gpu.h"
#include "zarc_kernels.h"
#include "zre_compile.h" // the regular-expression compiler (host code)
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); } // (zarc_gpu_destroy deletes the handle: every scratch buffer goes with it)
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = n + n / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return (T *)p; }
};

} // namespace

struct zarc_gpu {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr; // side stream: independent stage-2 kernels of the decoder run next to each other
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t stream3 = nullptr;
    hipEvent_t ev_fork3 = nullptr, ev_join3 = nullptr;
    // pinned staging ring of the host-pointer entry points (allocated on first use)
    static constexpr int PIN_SLOTS = 8; // slots 0..3: the ring of the way in (H2D); 4..7: the way out (D2H, two alternate) -- the two directions run at once
    static constexpr size_t PIN_PIECE = (size_t)32 << 20;
    uint8_t *pin[PIN_SLOTS] = {};
    hipEvent_t pin_ev[PIN_SLOTS] = {};
    DevBuf d_dense, d_goff, d_glen, d_gdense; // gather of the frames of a chunk before they cross PCIe
    zarc_gpu_params params{};
    std::string last_error;
    std::mutex err_mu; // last_error is also written by the staging helper thread of the host-pointer entry points
    hipStream_t stream_stage = nullptr; // PCIe staging of the host-pointer entry points: its copies never queue behind side kernels
    hipStream_t stream_stage_out = nullptr; // the way out has its own stream (and helper thread): PCIe carries both directions at once
    // descriptors
    DevBuf d_units; // encoder: (queue slot, first block) of every 2 MiB segment
    DevBuf d_pieces; // decoder: ZdecPiece per unit of work of the frame pass
    DevBuf d_off, d_len, d_chunk_prefix, d_block_prefix, d_order, d_dst_off, d_dst_len, d_raw_len, d_frame_off, d_frame_len;
    // hashing
    DevBuf d_cvs, d_cvs_tmp, d_digests, d_xxh, d_expect;
    // encoder
    DevBuf d_blocks, d_seq, d_lit, d_out, d_far, d_plan, d_groups;
    DevBuf d_pblocks, d_zpieces; // block splitting: ZGE_SPLIT_K piece slots per parent block (records, placement)
    DevBuf d_enc_err;           // one word the entropy stage raises when the table plan's size bound did not hold
    int block_split = 0;        // ZARC_GPU_PX_BLOCK_SPLIT
    // decoder
    DevBuf d_declit, d_status, d_stored_ck;
    DevBuf d_slot_prefix, d_zblocks, d_nseq, d_fast, d_seqidx, d_seqs, d_ztables, d_litidx, d_lits, d_seqflag, d_totals, d_predef, d_longlist, d_longcnt; // decoder fast path (sequences decoded ahead)
    DevBuf d_queue; // frame queues of the persistent kernels (one u32 each)
    int num_cus = 1;
    int deep_per_cu = 0; // workgroups of zarc_zge_match_deep a CU holds (0: not asked yet)
    uint64_t blake3_total_chunks = 0;
    hipEvent_t ev_b3[2] = {}; // digest kernels on the side stream (pack)
    // staging arenas for the host-pointer entry points
    DevBuf d_arena_in, d_arena_out;
    hipEvent_t ev[16] = {};
    // decoder groups (zarc_gpu_unpack_batch_device): a pair of streams per group; events: 0/1 sequences, 2/3 literals, 4/5 frame passes, 6/7 checksum,
    // 8/9 digest, 10 literals done (join), 11 both stages ahead done (the host waits for it when it cuts frames into pieces)
    static constexpr int DEC_GROUPS = 4;
    hipStream_t gs[2 * DEC_GROUPS] = {};
    hipEvent_t ev_g[DEC_GROUPS][12] = {};
    int dec_groups = 0;        // ZARC_GPU_PX_DEC_GROUPS: 0 = by the batch's shape
    uint64_t dec_split_above = 0; // unpack: a batch of this many content bytes ran out of device memory; such batches are split at once
    float ms[ZARC_GPU_T_COUNT];
    size_t scratch_budget = 0; // 0 = derive from free memory (ZARC_GPU_PX_SCRATCH_MB)
    uint64_t stage_chunk = 0;  // 0 = default per entry point (ZARC_GPU_PX_STAGE_CHUNK)
    int stage_thread = 1;      // ZARC_GPU_PX_STAGE_THREAD
    int copy_threads = 8;      // ZARC_GPU_PX_COPY_THREADS
    uint8_t *meta_pin = nullptr; // page-locked arena for descriptor uploads (meta_take)
    size_t meta_cap = 0, meta_used = 0;
    int ldm[5] = {0, 0, 0, 0, 0}; // EnableLongDistanceMatching, LdmHashLog, LdmMinMatch, LdmBucketSizeLog, LdmHashRateLog: remembered, advisory
    // verify (zarc_gpu_verify_batch*) and the read-back check of pack (ZARC_GPU_PX_CHECK_FRAMES): the decoder writes into scratch the handle owns
    DevBuf d_vout;              // decoded bytes, 16-byte aligned offsets; counts against scratch_budget
    DevBuf d_chk_off;           // read-back check: the decoder's output offsets (pack keeps d_dst_off for its later sub-batches)
    DevBuf d_chk_order, d_chk_slices, d_chk_bad; // zarc_check_compare: entry of every sorted frame, slice prefix, first differing byte
    int check_frames = 0;       // ZARC_GPU_PX_CHECK_FRAMES
    int seq_states = 1;         // ZARC_GPU_PX_SEQ_STATES: 0 = off, 1 = on, N > 1 = on with at most N state words per block
    size_t chk_index = 0;       // the first entry that failed the check in the most recent pack pass, and where (ZARC_CHECK_TRAILER: its trailer)
    uint32_t chk_at = 0;
    float chk_ms = 0;           // zarc_check_compare of the most recent pack pass (diagnostic build prints it)
    // repack (zarc_gpu_repack_batch*): the decode half leaves its bytes in d_vout and the encode half reads them there
    DevBuf d_vout2;             // read-back check inside a repack pass: d_vout holds the sources, the check decodes into this one
    DevBuf d_rp_order, d_rp_xxh; // zarc_repack_plan: the caller's index of every frame of the decoder's order; XXH64 by entry for frame assembly
    // search (zarc_gpu_search_batch*): zarc_search_scan over d_vout behind the verdict of a verify pass
    DevBuf d_srch_pat, d_srch_slices, d_srch_count, d_srch_first; // the (folded) pattern; slice prefix, matches and lowest match of every frame (decoder order)
    // a set of patterns (zarc_gpu_search_set_*): zarc_set_scan / zarc_set_which in place of zarc_search_scan
    DevBuf d_set, d_set_hits, d_set_which;      // the compiled set (search_upload_set); hits of every pattern in this part; lowest matching pattern of every frame (decoder order)
    ZarcSetDesc set_desc{};                     // where things lie in d_set
    // a regular expression (zarc_gpu_search_regex_*): zarc_regex_* in place of zarc_search_scan
    DevBuf d_regex, d_re_summary, d_re_entry;   // the compiled table (search_prepare); ZarcRegexSlice and entry state of every slice of this part
    // the matching lines of a search (zarc_gpu_search_lines_batch*): zarc_lines_* behind zarc_search_scan, per part
    DevBuf d_ln_slices, d_ln_lines;             // ZarcLineSlice of every slice; matching lines of every frame (decoder order)
    DevBuf d_ln_base, d_ln_deliver;             // what the host decided: first record and number of records of every frame (decoder order)
    DevBuf d_ln_rec, d_ln_total, d_ln_text;     // the part's records, the sum of their text_len, and (host form) their text: sized by what the part delivers
    // the selected lines (zarc_gpu_select_lines_batch*): zarc_lines_select_* in place of zarc_lines_mark / _carry / _emit
    DevBuf d_sel_slices, d_sel_count;           // ZarcSelSlice of every slice; selected lines of every frame (decoder order; the hit lines go to d_ln_lines)
    // every match of the delivered lines (zarc_gpu_search_matches_batch*): zarc_matches_* behind zarc_lines_emit*, over d_ln_rec where it lies
    DevBuf d_regex_fwd;                         // the forward table (search_prepare)
    DevBuf d_mt_bitoff, d_mt_bits;              // a regex: first word of every line record's start bits (and the sum); the bits, at most decoded bytes / 8 + 4 per record
    DevBuf d_mt_counts, d_mt_prefix, d_mt_rec;  // matches of every line record; their exclusive sums (and the total); the part's match records
    // byte and line ranges (zarc_gpu_read_ranges_batch*): zarc_range_* over d_vout behind the verdict of a verify pass, per part
    DevBuf d_rg_slices, d_rg_req, d_rg_cnt;     // slice prefix; the ranges (decoder order); 0x0A bytes of every slice of a LINES frame
    DevBuf d_rg_frames, d_rg_open, d_rg_nopen;  // ZarcRangeFrame of every frame (decoder order); the boundaries that wait for zarc_range_locate, and how many
    DevBuf d_rg_plan, d_rg_blocks, d_rg_text;   // what the host decided: the part's copies and their block prefix; (host form) the part's text
    // line, word, character and longest-line counts (zarc_gpu_count_batch*): zarc_wc_* over d_vout behind the verdict of a verify pass, per part
    DevBuf d_wc_slices, d_wc_rec, d_wc_out;     // slice prefix; ZarcWcSlice of every slice of the part's grid; ZarcWcFrame of every frame (decoder order)
    // frames against other bytes (zarc_gpu_compare_batch*): zarc_cmp_* over d_vout and the other sides behind the verdict of a verify pass, per part
    DevBuf d_cmp_slices, d_cmp_rec, d_cmp_out;  // slice prefix; ZarcCmpSlice of every slice of the part's grid; ZarcCmpFrame of every frame (decoder order)
    DevBuf d_cmp_off, d_cmp_len;                // where every frame's other side lies and how long it is (decoder order)
    float cmp_ms = -1.f;        // zarc_cmp_* of the most recent call, summed over its parts (zarc_gpu_last_compare_ms); the timer enum has no entry for it
    bool vout_busy = false;     // a repack pass is between its halves: d_vout is not the check's to take
    uint64_t dec_scratch = 0;   // decoder scratch (sequences, literals, tables) of the most recent decode, as counted against the budget
    // content bytes the most recent batch call moved (zarc_gpu_last_copy_bytes); the copy helpers run on two helper threads
    std::atomic<uint64_t> copy_bytes[ZARC_GPU_C_COUNT] = {};
    bool nested = false;        // a host-pointer entry point is running: the device forms it calls leave the counters alone
    int zero_copy = 4096;      // ZARC_GPU_PX_ZERO_COPY: page-locked caller memory in runs of this many KiB on average is read / written by the DMA engines directly (0 = never)
};

namespace {

#define ZHIP(call)                                                                                  \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            std::lock_guard<std::mutex> g_(h->err_mu);                                              \
            h->last_error = std::string(#call) + ": " + hipGetErrorString(e_);                      \
            return e_ == hipErrorOutOfMemory ? ZARC_GPU_E_NOMEM : ZARC_GPU_E_DEVICE;                \
        }                                                                                           \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline void set_error(zarc_gpu *h, const char *msg) { std::lock_guard<std::mutex> g(h->err_mu); h->last_error = msg; }

// Timing ablations and kernel-steering switches exist only in the diagnostic build (make DIAG=1 -> libzarc_gpu_diag.so, used by
// tools/): the product library never reads them, so no environment variable can change the bytes it produces.
#ifdef ZARC_GPU_DIAG
inline int diag_env(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
inline double diag_env_f(const char *name, double dflt) { const char *e = getenv(name); return e ? atof(e) : dflt; }
#else
inline int diag_env(const char *, int dflt) { return dflt; }
inline double diag_env_f(const char *, double dflt) { return dflt; }
#endif

ZgeParams derive_params(const zarc_gpu_params &p)
{
    ZgeParams z{};
    int level = p.level == 0 ? 3 : p.level;
    z.level = level;
    z.checksum = p.checksum_flag ? 1 : 0;
    z.window_log = p.window_log ? p.window_log : (level >= 9 ? 22 : 21);
    if (z.window_log < 10) z.window_log = 10;
    if (z.window_log > 27) z.window_log = 27;
    // level >= 9 selects the deep finder (zarc_zge_match_deep): two tagged near tables, a 4-byte short hash, 4-byte matches, a lower
    // match cost, two-way far tables on both hashes, and a parse that tries the live recent offsets (two rounds per tile) with a second
    // lazy step -- within 6 % of libzstd -9 on every real-data item of the test set but one
    const bool deep = level >= 9;
    // levels below 9 (round 3): ONE near table of 2^15 16-bit entries on the 5-byte hash (candidates 1 .. 65536 bytes back), no long table
    z.near16 = deep ? 0 : 1;
    z.long_log = 13; z.short_log = deep ? 13 : 15; z.short_bytes = deep ? 4 : 5; z.tag_bits = 10; z.seg_log = 21; z.rep_back = 256;
    z.tile = 1024; z.sub = 64; z.cap = diag_env("ZARC_GPU_CAP", 256);
    z.min_match = p.min_match >= 4 && p.min_match <= 7 ? p.min_match : (deep ? 4 : 5);
    z.min_rep = 3; z.rep_search = 2; z.back_cap = 8;
    z.lazy = level >= 2 ? 1 : 0; z.lazy_delta = 5; z.lazy2_delta = deep ? 5 : 0;
    // rounds after a tile's first parse: level >= 9 two, with the live recent offsets; below, one that only continues selected matches cut at
    // the cap (ext_cap) and that the kernel runs in tiles that have such a match
    z.rep_pass = deep ? 2 : 1; z.live_reps = deep ? 1 : 0; z.ext_cap = 960;
    z.far_cap = 0; z.cont_cap = deep ? 960 : 0; // level >= 9: continuation guess at a tile's cursor (zge_match.hip: LONG_CAP); far_cap is the model's only
    z.lit_cost = deep ? 6 : 5; z.match_cost = deep ? 10 : 12; z.rep_cost = 9;
    z.short_window_log = 30;
    // far tables in HBM (zge_match.hip).  Level 3: 2^16 buckets, one way on the 12-byte hash, content-defined sampling: the positions
    // whose hash has four given bits zero (one in 16) are inserted and looked up; level >= 9: 2^16 buckets, two ways on both hashes,
    // every 2nd position inserted, all looked up
    z.far_log = 16; z.far_ways = deep ? 2 : 1; z.far_step_log = deep ? 1 : 5; z.far_res_log = deep ? 0 : 2; z.far_short = deep ? 1 : 0;
    z.far_cdc_log = deep ? 0 : 4;
    z.far_min_frame = deep ? 0 : 65536; // smaller frames do without the far table: the near table reaches 64 KiB
    z.far_back = 48; z.far_skip = deep ? 0 : 64;
    if (deep && level >= 15) z.rep_pass = 4; // levels 15 .. 22: two more rounds of the live recent-offset pass (a run-time count: the same kernel)
    if (level <= 1) { // level 1 and the negative levels: the fast finder (zarc_zge_match_fast) -- the near table alone, no lazy step, no extension round
        z.far_log = 0; z.rep_pass = 0; z.lazy = 0;
    }
    z.dbg = diag_env("ZARC_GPU_DBG", 0); // timing-only ablations (outputs invalid when set): diagnostic build only
    return z;
}

inline hipError_t create_low_priority_stream(hipStream_t *s)
{
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return hipStreamCreate(s);
    return hipStreamCreateWithPriority(s, hipStreamDefault, least);
}

// indices 0 .. n-1 by descending len[], equal lengths in index order (what std::stable_sort gives, in O(n): a batch of a million small
// entries spent 80 ms per call in the comparison sort).  Lengths are below 2^32 (larger entries are refused before).
inline std::vector<uint32_t> order_by_size_desc(const uint64_t *len, size_t n)
{
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    if (n < 4096) { std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return len[a] > len[b]; }); return order; }
    // (inverted length << 32 | index) pairs, sorted by the upper half: least significant digit first, 11 bits a pass, the pairs walked in
    // memory order (descending length = ascending inverted key; equal keys keep their order)
    std::vector<uint64_t> a(n), b(n);
    for (size_t i = 0; i < n; i++) a[i] = (uint64_t)(~(uint32_t)len[i]) << 32 | (uint32_t)i;
    for (int pass = 0; pass < 3; pass++) {
        const int shift = 32 + 11 * pass;
        size_t count[2049] = {0};
        for (size_t i = 0; i < n; i++) count[(a[i] >> shift & 2047u) + 1]++;
        for (int d = 0; d < 2048; d++) count[d + 1] += count[d];
        for (size_t i = 0; i < n; i++) b[count[a[i] >> shift & 2047u]++] = a[i];
        a.swap(b);
    }
    for (size_t i = 0; i < n; i++) order[i] = (uint32_t)a[i];
    return order;
}

// The decoder's order: descending content size in steps of 4 KiB (what the groups, the piece lists of large frames and the XXH64 lanes
// want), and among frames of one size step the better compressed first.  The lane-per-block and lane-per-stream kernels of stage 2 work
// on consecutive frames, and a wave lasts as long as its longest lane: neighbours with the same share of matches and literals have
// chains of a length (a batch that alternates text, records and incompressible entries kept half of every wave's lanes waiting).
inline std::vector<uint32_t> order_for_decode(const uint64_t *raw_len, const uint64_t *frame_len, size_t n)
{
    auto key = [&](size_t i) -> uint32_t {
        const uint64_t r = raw_len[i], c = frame_len[i];
        const uint32_t dens = r ? (uint32_t)std::min<uint64_t>(4095, c * 4096 / r) : 4095u; // compressed share, 12 bits
        return (~(uint32_t)(r >> 12) & 0xFFFFFu) << 12 | dens;                               // ascending: larger first, denser matches first
    };
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    if (n < 4096) { std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); }); return order; }
    std::vector<uint64_t> a(n), b(n);
    for (size_t i = 0; i < n; i++) a[i] = (uint64_t)key(i) << 32 | (uint32_t)i;
    for (int pass = 0; pass < 3; pass++) {
        const int shift = 32 + 11 * pass;
        size_t count[2049] = {0};
        for (size_t i = 0; i < n; i++) count[(a[i] >> shift & 2047u) + 1]++;
        for (int d = 0; d < 2048; d++) count[d + 1] += count[d];
        for (size_t i = 0; i < n; i++) b[count[a[i] >> shift & 2047u]++] = a[i];
        a.swap(b);
    }
    for (size_t i = 0; i < n; i++) order[i] = (uint32_t)a[i];
    return order;
}

// encoder scratch: the slot size a sub-batch whose largest frame has first_len bytes works with, and what one block slot of it costs
inline uint32_t enc_slot_of(uint64_t first_len) { return (uint32_t)std::min<uint64_t>(ZARC_BLOCK, std::max<uint64_t>((first_len + 15) / 16 * 16, 1024)); }
inline size_t enc_per_block(bool split, uint32_t slot)
{
    const size_t records = (sizeof(ZgeBlock) + sizeof(ZgePlan)) * (split ? 1 + ZGE_SPLIT_K : 1) + (split ? sizeof(ZgePiece) * ZGE_SPLIT_K : 0);
    return (size_t)(zge_seq_stride(slot) * 8 + zge_lit_stride(slot) + zge_out_stride(slot)) + records;
}
inline uint64_t chunks_of(uint64_t len) { return len == 0 ? 1 : (len + 1023) / 1024; }
inline uint64_t blocks_of(uint64_t len) { return len == 0 ? 1 : (len + ZARC_BLOCK - 1) / ZARC_BLOCK; }

struct Timer {
    zarc_gpu *h;
    int next = 0; // (the read-back check of pack starts at 8: pack's own marks stay valid)
    hipError_t mark(int *idx) { *idx = next; return hipEventRecord(h->ev[next++], h->stream); }
};

// Per-entry descriptor arrays travel through a page-locked arena of the handle: an asynchronous copy out of ordinary memory is staged
// by the runtime at a fraction of the link rate, and a call over half a million entries spent 27 ms in five such copies.  The arena is
// reset where a call begins (every batch call ends with its stream synchronised) and grows to the largest call's needs.
void *meta_take(zarc_gpu *h, size_t bytes)
{
    bytes = (bytes + 63) & ~(size_t)63;
    if (bytes < 65536) return nullptr; // small arrays: the runtime's own staging is as good
    if (h->meta_used + bytes > h->meta_cap) {
        if (h->meta_used) return nullptr; // part of it is in flight: this array goes the ordinary way, the next call starts with more room
        if (h->meta_pin) { (void)hipHostFree(h->meta_pin); h->meta_pin = nullptr; h->meta_cap = 0; }
        const size_t want = std::max<size_t>(bytes * 20, (size_t)16 << 20); // the first array of a call has 8 bytes per entry; an unpack moves about 130
        if (hipHostMalloc((void **)&h->meta_pin, want, 0) != hipSuccess) { (void)hipGetLastError(); h->meta_pin = nullptr; return nullptr; }
        h->meta_cap = want;
    }
    void *p = h->meta_pin + h->meta_used;
    h->meta_used += bytes;
    return p;
}
int upload_bytes(zarc_gpu *h, DevBuf &b, const void *src, size_t bytes)
{
    ZHIP(b.reserve(std::max<size_t>(bytes, 8)));
    if (!bytes) return 0;
    if (void *pin = meta_take(h, bytes)) { memcpy(pin, src, bytes); src = pin; }
    ZHIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, h->stream));
    return 0;
}
int upload_u64(zarc_gpu *h, DevBuf &b, const uint64_t *src, size_t n) { return upload_bytes(h, b, src, n * 8); }
int upload_u32(zarc_gpu *h, DevBuf &b, const uint32_t *src, size_t n) { return upload_bytes(h, b, src, n * 4); }

// BLAKE3 of n entries described by device arrays d_off/d_len (already uploaded); result in h->d_digests
// `side` (pack): the two kernels go to the low-priority side stream behind an event of the engine stream -- the caller launches the
// match finder first: the side stream waits for an event recorded BEHIND that launch, so the digest kernels start when the match finder
// has finished and run beside the entropy stage (low priority) instead of standing in front of the persistent workgroups
int run_blake3(zarc_gpu *h, size_t n, const uint8_t *d_base, const uint64_t *off, const uint64_t *len, const uint64_t *d_off, const uint64_t *d_len,
               bool prepare_only = false, bool launch_only = false, hipStream_t stream = nullptr)
{
    (void)off;
    if (!stream) stream = h->stream;
    if (launch_only) goto launch;
    {
    std::vector<uint64_t> prefix(n + 1);
    prefix[0] = 0;
    for (size_t i = 0; i < n; i++) prefix[i + 1] = prefix[i] + chunks_of(len[i]);
    const uint64_t total = prefix[n];
    int rc = upload_u64(h, h->d_chunk_prefix, prefix.data(), n + 1);
    if (rc) return rc;
    ZHIP(h->d_cvs.reserve(total * 32));
    ZHIP(h->d_cvs_tmp.reserve(total * 32));
    ZHIP(h->d_digests.reserve(std::max<size_t>(n, 1) * 32));
    h->blake3_total_chunks = total;
    }
    if (prepare_only) return 0;
launch:
    {
    const uint64_t total = h->blake3_total_chunks;
    const uint32_t tpb = 256;
    const uint64_t grid = (total + tpb - 1) / tpb;
    hipLaunchKernelGGL(zarc_blake3_chunks, dim3((unsigned)grid), dim3(tpb), 0, stream, d_base, d_off, d_len, h->d_chunk_prefix.as<uint64_t>(),
                       (uint32_t)n, total, h->d_cvs.as<uint32_t>(), h->d_digests.as<uint32_t>());
    const unsigned tgrid = (unsigned)std::min<size_t>(n, 65535);
    hipLaunchKernelGGL(zarc_blake3_tree, dim3(tgrid), dim3(256), 0, stream, h->d_chunk_prefix.as<uint64_t>(), (uint32_t)n,
                       h->d_cvs.as<uint32_t>(), h->d_cvs_tmp.as<uint32_t>(), h->d_digests.as<uint32_t>());
    ZHIP(hipGetLastError());
    }
    return 0;
}

int run_xxh64(zarc_gpu *h, size_t n, const uint8_t *d_base, const uint64_t *d_off, const uint64_t *d_len, hipStream_t stream = nullptr)
{
    if (!stream) stream = h->stream;
    ZHIP(h->d_xxh.reserve(std::max<size_t>(n, 1) * 8));
    const uint32_t tpb = 256;
    const uint64_t threads = (uint64_t)n * 4;
    hipLaunchKernelGGL(zarc_xxh64, dim3((unsigned)((threads + tpb - 1) / tpb)), dim3(tpb), 0, stream, d_base, d_off, d_len, (uint32_t)n,
                       h->d_xxh.as<uint64_t>());
    ZHIP(hipGetLastError());
    return 0;
}

float elapsed(zarc_gpu *h, int a, int b)
{
    float ms = -1.f;
    if (hipEventElapsedTime(&ms, h->ev[a], h->ev[b]) != hipSuccess) return -1.f;
    return ms;
}

int check_common(zarc_gpu *h, size_t n)
{
    if (!h) return ZARC_GPU_E_PARAM;
    if (n > 0x7FFFFFFFu) { set_error(h, "batch too large"); return ZARC_GPU_E_PARAM; }
    ZHIP(hipSetDevice(h->device));
    for (int i = 0; i < ZARC_GPU_T_COUNT; i++) h->ms[i] = -1.f;
    h->cmp_ms = -1.f;
    h->meta_used = 0; // every batch call ends with its stream synchronised: what the arena held has been copied
    if (!h->nested) for (auto &c : h->copy_bytes) c.store(0, std::memory_order_relaxed);
    return 0;
}

// the host-pointer entry points call the device forms per chunk: those must not reset what the call has counted so far
struct NestedCall {
    zarc_gpu *h;
    explicit NestedCall(zarc_gpu *h_) : h(h_) { h->nested = true; }
    ~NestedCall() { h->nested = false; }
};

} // namespace

extern "C" {

int zarc_gpu_abi_version(void) { return ZARC_GPU_ABI_VERSION; }

int zarc_gpu_device_count(void)
{
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess && count > 0 ? count : 0;
}

int zarc_gpu_create(zarc_gpu_t **out, int device)
{
    if (!out) return ZARC_GPU_E_PARAM;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return ZARC_GPU_E_DEVICE;
    zarc_gpu *h = new (std::nothrow) zarc_gpu();
    if (!h) return ZARC_GPU_E_NOMEM;
    h->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&h->stream) != hipSuccess || hipStreamCreate(&h->stream2) != hipSuccess || create_low_priority_stream(&h->stream3) != hipSuccess || hipStreamCreate(&h->stream_stage) != hipSuccess || hipStreamCreate(&h->stream_stage_out) != hipSuccess ||
        hipEventCreate(&h->ev_fork3) != hipSuccess || hipEventCreate(&h->ev_join3) != hipSuccess ||
        hipEventCreate(&h->ev_fork) != hipSuccess || hipEventCreate(&h->ev_join) != hipSuccess) { delete h; return ZARC_GPU_E_DEVICE; }
    for (auto &e : h->ev)
        if (hipEventCreate(&e) != hipSuccess) { delete h; return ZARC_GPU_E_DEVICE; }
    for (int i = 0; i < 2 * zarc_gpu::DEC_GROUPS; i++) { // the first group holds the largest frames, whose chains are the critical path: its streams go first
        int least = 0, greatest = 0;
        const bool prio = i < 2 && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least;
        if ((prio ? hipStreamCreateWithPriority(&h->gs[i], hipStreamDefault, greatest) : hipStreamCreate(&h->gs[i])) != hipSuccess) { delete h; return ZARC_GPU_E_DEVICE; }
    }
    for (auto &row : h->ev_g)
        for (auto &e : row)
            if (hipEventCreate(&e) != hipSuccess) { delete h; return ZARC_GPU_E_DEVICE; }
    for (auto &e : h->ev_b3)
        if (hipEventCreate(&e) != hipSuccess) { delete h; return ZARC_GPU_E_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->num_cus = prop.multiProcessorCount;
    h->params.level = 0;          // CCtx::init(0): default level (crates/zarc/src/encode.rs:62)
    h->params.checksum_flag = 0;  // libzstd default; the zarc CLI switches it on (pack.rs:227)
    h->params.content_size_flag = 1;
    h->params.compress = 1;
    for (int i = 0; i < ZARC_GPU_T_COUNT; i++) h->ms[i] = -1.f;
    *out = h;
    return ZARC_GPU_OK;
}

void zarc_gpu_destroy(zarc_gpu_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    DevBuf *all[] = {&h->d_off, &h->d_len, &h->d_chunk_prefix, &h->d_block_prefix, &h->d_order, &h->d_dst_off, &h->d_dst_len, &h->d_raw_len,
                     &h->d_frame_off, &h->d_frame_len, &h->d_cvs, &h->d_cvs_tmp, &h->d_digests, &h->d_xxh, &h->d_expect, &h->d_blocks, &h->d_seq,
                     &h->d_lit, &h->d_out, &h->d_far, &h->d_declit, &h->d_status, &h->d_stored_ck, &h->d_arena_in, &h->d_arena_out, &h->d_queue,
                     &h->d_units, &h->d_pieces, &h->d_slot_prefix, &h->d_zblocks, &h->d_nseq, &h->d_fast, &h->d_seqidx, &h->d_seqs, &h->d_ztables, &h->d_litidx, &h->d_lits};
    for (DevBuf *b : all) b->release();
    for (auto &e : h->ev) if (e) (void)hipEventDestroy(e);
    for (auto &row : h->ev_g) for (auto &e : row) if (e) (void)hipEventDestroy(e);
    for (auto &st : h->gs) if (st) (void)hipStreamDestroy(st);
    for (auto &e : h->ev_b3) if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    if (h->stream3) (void)hipStreamDestroy(h->stream3);
    if (h->stream_stage) (void)hipStreamDestroy(h->stream_stage);
    if (h->stream_stage_out) (void)hipStreamDestroy(h->stream_stage_out);
    if (h->ev_fork3) (void)hipEventDestroy(h->ev_fork3);
    if (h->ev_join3) (void)hipEventDestroy(h->ev_join3);
    for (int i = 0; i < zarc_gpu::PIN_SLOTS; i++) { if (h->pin[i]) (void)hipHostFree(h->pin[i]); if (h->pin_ev[i]) (void)hipEventDestroy(h->pin_ev[i]); }
    h->d_dense.release(); h->d_goff.release(); h->d_glen.release(); h->d_gdense.release();
    h->d_vout.release(); h->d_vout2.release(); h->d_rp_order.release(); h->d_rp_xxh.release(); h->d_chk_off.release(); h->d_chk_order.release(); h->d_chk_slices.release(); h->d_chk_bad.release();
    if (h->meta_pin) (void)hipHostFree(h->meta_pin);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    delete h;
}

int zarc_gpu_set_parameter(zarc_gpu_t *h, int id, int value)
{
    if (!h) return ZARC_GPU_E_PARAM;
    switch (id) {
    case ZARC_GPU_P_COMPRESSION_LEVEL:
        if (value < -131072 || value > 22) return ZARC_GPU_E_PARAM; // same bounds as --level (zarc-cli/src/pack.rs:28-33) / libzstd
        h->params.level = value; return ZARC_GPU_OK;
    case ZARC_GPU_P_WINDOW_LOG:
        if (value != 0 && (value < 10 || value > 27)) return ZARC_GPU_E_PARAM;
        h->params.window_log = value; return ZARC_GPU_OK;
    // Search-effort hints: libzstd accepts them inside its bounds and the reference forwards whatever the user gives (pack.rs:86-217), so
    // `zarc pack --zstd Strategy=btopt` has to work.  They are range-checked as libzstd does (ZSTD_cParam_getBounds), remembered (get_params
    // returns them) and ADVISORY: table sizes, search depth and strategy are fixed by the kernels, the frames are the level's frames.
    case ZARC_GPU_P_HASH_LOG: if (value != 0 && (value < 6 || value > 30)) return ZARC_GPU_E_PARAM; h->params.hash_log = value; return ZARC_GPU_OK;
    case ZARC_GPU_P_CHAIN_LOG: if (value != 0 && (value < 6 || value > 30)) return ZARC_GPU_E_PARAM; h->params.chain_log = value; return ZARC_GPU_OK;
    case ZARC_GPU_P_SEARCH_LOG: if (value != 0 && (value < 1 || value > 30)) return ZARC_GPU_E_PARAM; h->params.search_log = value; return ZARC_GPU_OK;
    case ZARC_GPU_P_TARGET_LENGTH: if (value < 0 || value > 131072) return ZARC_GPU_E_PARAM; h->params.target_length = value; return ZARC_GPU_OK;
    case ZARC_GPU_P_STRATEGY: if (value < 0 || value > 9) return ZARC_GPU_E_PARAM; h->params.strategy = value; return ZARC_GPU_OK;
    case ZARC_GPU_P_MIN_MATCH:
        if (value != 0 && (value < 3 || value > 7)) return ZARC_GPU_E_PARAM;
        h->params.min_match = value; return ZARC_GPU_OK;
    case ZARC_GPU_PX_SCRATCH_MB:
        if (value < 0) return ZARC_GPU_E_PARAM;
        h->scratch_budget = (size_t)value << 20; return ZARC_GPU_OK;
    case ZARC_GPU_PX_STAGE_CHUNK:
        if (value != 0 && value < 4096) return ZARC_GPU_E_PARAM;
        h->stage_chunk = (uint64_t)value; return ZARC_GPU_OK;
    case ZARC_GPU_PX_STAGE_THREAD: h->stage_thread = value ? 1 : 0; return ZARC_GPU_OK;
    case ZARC_GPU_PX_COPY_THREADS:
        if (value < 1 || value > 64) return ZARC_GPU_E_PARAM;
        h->copy_threads = value; return ZARC_GPU_OK;
    case ZARC_GPU_PX_DEC_GROUPS:
        if (value < 0 || value > zarc_gpu::DEC_GROUPS) return ZARC_GPU_E_PARAM;
        h->dec_groups = value; return ZARC_GPU_OK;
    case ZARC_GPU_PX_ZERO_COPY: if (value < 0 || value > (1 << 20)) return ZARC_GPU_E_PARAM; h->zero_copy = value; return ZARC_GPU_OK;
    case ZARC_GPU_PX_BLOCK_SPLIT: if (value != 0 && value != 1) return ZARC_GPU_E_PARAM; h->block_split = value; return ZARC_GPU_OK;
    case ZARC_GPU_PX_CHECK_FRAMES: if (value != 0 && value != 1) return ZARC_GPU_E_PARAM; h->check_frames = value; return ZARC_GPU_OK;
    case ZARC_GPU_PX_SEQ_STATES: if (value < 0) return ZARC_GPU_E_PARAM; h->seq_states = value; return ZARC_GPU_OK;
    case ZARC_GPU_P_CONTENT_SIZE_FLAG:
        if (value != 1) return ZARC_GPU_E_UNSUPPORTED; // frames always carry their content size
        return ZARC_GPU_OK;
    case ZARC_GPU_P_CHECKSUM_FLAG: h->params.checksum_flag = value ? 1 : 0; return ZARC_GPU_OK;
    case ZARC_GPU_P_DICT_ID_FLAG: return ZARC_GPU_OK; // no dictionaries in zarc
    // Long-distance matching (pack.rs:89-109 forwards these; libzstd accepts them single-threaded): accepted inside libzstd's bounds and
    // ADVISORY like the search-effort hints -- the finders' far tables in HBM ARE a long-distance matcher, at every level above 1
    case ZARC_GPU_P_ENABLE_LDM: if (value < 0 || value > 2) return ZARC_GPU_E_PARAM; h->ldm[0] = value; return ZARC_GPU_OK;
    case ZARC_GPU_P_LDM_HASH_LOG: if (value != 0 && (value < 6 || value > 30)) return ZARC_GPU_E_PARAM; h->ldm[1] = value; return ZARC_GPU_OK;
    case ZARC_GPU_P_LDM_MIN_MATCH: if (value != 0 && (value < 4 || value > 4096)) return ZARC_GPU_E_PARAM; h->ldm[2] = value; return ZARC_GPU_OK;
    case ZARC_GPU_P_LDM_BUCKET_SIZE_LOG: if (value != 0 && (value < 1 || value > 8)) return ZARC_GPU_E_PARAM; h->ldm[3] = value; return ZARC_GPU_OK;
    case ZARC_GPU_P_LDM_HASH_RATE_LOG: if (value < 0 || value > 25) return ZARC_GPU_E_PARAM; h->ldm[4] = value; return ZARC_GPU_OK;
    default:
        // nbWorkers/jobSize/overlapLog (400-402) and the experimental ids
        if ((id >= 400 && id <= 402) || (id >= 500 && id <= 1020)) return ZARC_GPU_E_UNSUPPORTED;
        return ZARC_GPU_E_PARAM;
    }
}

void zarc_gpu_get_params(const zarc_gpu_t *h, zarc_gpu_params *out) { if (h && out) *out = h->params; }

int zarc_gpu_level_finder(int level)
{
    if (level == 0) level = 3; // encode.rs:62: init(0) = the default level
    return level <= 1 ? 1 : (level < 9 ? 3 : (level < 15 ? 9 : 15));
}

int zarc_gpu_parameter_advisory(int id)
{
    switch (id) {
    case ZARC_GPU_P_HASH_LOG: case ZARC_GPU_P_CHAIN_LOG: case ZARC_GPU_P_SEARCH_LOG: case ZARC_GPU_P_TARGET_LENGTH: case ZARC_GPU_P_STRATEGY:
    case ZARC_GPU_P_ENABLE_LDM: case ZARC_GPU_P_LDM_HASH_LOG: case ZARC_GPU_P_LDM_MIN_MATCH: case ZARC_GPU_P_LDM_BUCKET_SIZE_LOG: case ZARC_GPU_P_LDM_HASH_RATE_LOG:
        return 1;
    default: return 0;
    }
}
void zarc_gpu_enable_compression(zarc_gpu_t *h, int compress) { if (h) h->params.compress = compress ? 1 : 0; }

size_t zarc_gpu_bound(size_t n)
{
    size_t blocks = (n + ZARC_BLOCK - 1) / ZARC_BLOCK;
    if (blocks == 0) blocks = 1;
    return align_up(n + 3 * blocks + 18, ZARC_GPU_ALIGN);
}

const char *zarc_gpu_error_name(int code)
{
    switch (code) {
    case ZARC_GPU_OK: return "No error detected";
    case ZARC_GPU_E_DEVICE: return "HIP device error";
    case ZARC_GPU_E_NOMEM: return "Allocation error : not enough memory";
    case ZARC_GPU_E_PARAM: return "Parameter is out of bound";
    case ZARC_GPU_E_UNSUPPORTED: return "Unsupported parameter";
    case ZARC_GPU_E_DSTSIZE: return "Destination buffer is too small";
    case ZARC_GPU_E_CHECK: return "Frame failed its read-back check";
    default: return "Unspecified error code";
    }
}
const char *zarc_gpu_frame_status_name(int s)
{
    switch (s) {
    case ZARC_GPU_FRAME_OK: return "No error detected";
    case ZARC_GPU_FRAME_CORRUPT: return "Data corruption detected";
    case ZARC_GPU_FRAME_CHECKSUM: return "Restored data doesn't match checksum";
    case ZARC_GPU_FRAME_DIGEST: return "BLAKE3 digest mismatch";
    case ZARC_GPU_FRAME_DSTSIZE: return "Destination buffer is too small";
    case ZARC_GPU_FRAME_BAD_MAGIC: return "Unknown frame descriptor";
    case ZARC_GPU_FRAME_UNSUPPORTED: return "Unsupported frame parameter";
    case ZARC_GPU_FRAME_SRCSIZE: return "Src size is incorrect";
    case ZARC_GPU_FRAME_DUPLICATE: return "frame already exists, skipping";
    default: return "Unspecified error code";
    }
}
const char *zarc_gpu_last_error(const zarc_gpu_t *h) { return h ? h->last_error.c_str() : "null handle"; }
uint64_t zarc_gpu_last_copy_bytes(const zarc_gpu_t *h, int which) { return (h && which >= 0 && which < ZARC_GPU_C_COUNT) ? h->copy_bytes[which].load(std::memory_order_relaxed) : 0; }
float zarc_gpu_last_kernel_ms(const zarc_gpu_t *h, int which) { return (h && which >= 0 && which < ZARC_GPU_T_COUNT) ? h->ms[which] : -1.f; }
float zarc_gpu_last_compare_ms(const zarc_gpu_t *h) { return h ? h->cmp_ms : -1.f; }

// ---------------------------------------------------------------------------------------------------
int zarc_gpu_blake3_batch_device(zarc_gpu_t *h, size_t n, const void *d_base, const uint64_t *off, const uint64_t *len, uint8_t *digest)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!d_base || !off || !len || !digest) return ZARC_GPU_E_PARAM;
    for (size_t i = 0; i < n; i++) if (off[i] % ZARC_GPU_ALIGN) { set_error(h, "entry offset not 16-byte aligned"); return ZARC_GPU_E_PARAM; }
    if ((rc = upload_u64(h, h->d_off, off, n))) return rc;
    if ((rc = upload_u64(h, h->d_len, len, n))) return rc;
    Timer t{h};
    int a, b;
    ZHIP(t.mark(&a));
    if ((rc = run_blake3(h, n, (const uint8_t *)d_base, off, len, h->d_off.as<uint64_t>(), h->d_len.as<uint64_t>()))) return rc;
    ZHIP(t.mark(&b));
    ZHIP(hipMemcpyAsync(digest, h->d_digests.p, n * 32, hipMemcpyDeviceToHost, h->stream));
    ZHIP(hipStreamSynchronize(h->stream));
    h->ms[ZARC_GPU_T_BLAKE3] = h->ms[ZARC_GPU_T_TOTAL] = elapsed(h, a, b);
    return ZARC_GPU_OK;
}

int zarc_gpu_xxh64_batch_device(zarc_gpu_t *h, size_t n, const void *d_base, const uint64_t *off, const uint64_t *len, uint64_t *out)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!d_base || !off || !len || !out) return ZARC_GPU_E_PARAM;
    for (size_t i = 0; i < n; i++) if (off[i] % ZARC_GPU_ALIGN) { set_error(h, "entry offset not 16-byte aligned"); return ZARC_GPU_E_PARAM; }
    if ((rc = upload_u64(h, h->d_off, off, n))) return rc;
    if ((rc = upload_u64(h, h->d_len, len, n))) return rc;
    Timer t{h};
    int a, b;
    ZHIP(t.mark(&a));
    if ((rc = run_xxh64(h, n, (const uint8_t *)d_base, h->d_off.as<uint64_t>(), h->d_len.as<uint64_t>()))) return rc;
    ZHIP(t.mark(&b));
    ZHIP(hipMemcpyAsync(out, h->d_xxh.p, n * 8, hipMemcpyDeviceToHost, h->stream));
    ZHIP(hipStreamSynchronize(h->stream));
    h->ms[ZARC_GPU_T_XXH64] = h->ms[ZARC_GPU_T_TOTAL] = elapsed(h, a, b);
    return ZARC_GPU_OK;
}

} // extern "C"
namespace {
// Read-back check of a pack pass (ZARC_GPU_PX_CHECK_FRAMES): the decoder runs DECODE-ONLY -- no hash passes, no verdict, nothing written to
// h->ms -- and zarc_check_compare takes their place.  Pack's own buffers stay as they are: the decoder leaves d_off / d_len / d_dst_len /
// d_xxh / d_digests alone in this mode, puts its output offsets into d_chk_off instead of d_dst_off, and takes its timing events from
// the upper half of the pool (pack's e0 .. e2 and the sub-batch marks live in the lower one).
struct PackCheck {
    const uint8_t *src_base;   // the pack pass's sources (offsets / lengths: h->d_off, h->d_len, by entry)
    bool trailer;              // frames carry the checksum trailer: compare it with h->d_xxh
    uint32_t entry0;           // the decoder's frame 0 is this entry of the pack pass (parts of a split batch)
    uint32_t *first_bad;       // host, by entry from entry0 on: ZARC_CHECK_CLEAN, a byte offset, or ZARC_CHECK_TRAILER
    float *ms;                 // += device time of zarc_check_compare
    const uint32_t *entry_map; // host, or null: the decoder's frame j is entry entry_map[j] of the pack pass (a pass with skipped entries; entry0 is 0)
    const uint64_t *xxh;       // device, by entry, or null = h->d_xxh: where the pack pass took its checksums from
};
// A pack pass whose per-entry arrays were made on the device (zarc_repack_plan): h->d_off / h->d_len are in place, digests and checksums
// exist already.  No hash kernel runs; entries whose status is not OK are left out of the size order, so no launch sees them.
struct PackPlanned {
    const uint64_t *d_xxh;     // device, by entry: XXH64 of every entry, for frame assembly and the read-back check
    int *status;               // host, by entry: only ZARC_GPU_FRAME_OK entries are packed; the read-back check marks its failures here
    size_t budget;             // encoder scratch budget of this pass (0 = the handle's)
};

// A verify pass that also searches what it decoded (zarc_gpu_search_batch*): zarc_search_scan runs behind the verdict, per part, while that
// part's bytes are in d_vout
// ... and gathers the matching lines (zarc_gpu_search_lines_batch*).  The parts of a call -- chunks of the host form, halves of
// unpack_device_split -- are contiguous ranges of the caller's frames processed in the caller's order, so the running remainder of rec_cap in
// `run` gives every frame the same records however the call is cut.
struct LinesRun { size_t rec_used = 0; uint64_t text_used = 0; float ms = 0; size_t match_used = 0; }; // one per call (matches: rec_used counts the lines that took part, match_used the records)
// zarc_gpu_search_matches_batch*: the lines of `ln` stay on the device (ln.rec_cap is the call's line_cap) and their matches are delivered
struct MatchesReq {
    bool on;
    uint64_t *matches;         // host, in the caller's order, this part's first frame first
    zarc_gpu_match *rec;       // host: the call's records
    size_t rec_cap;
    const ZarcRegexDfa *d_fwd; // REGEX; device: the forward table
};
struct LinesReq {
    uint64_t max_lines;        // per frame; 0 = no limit
    uint32_t max_line;
    uint64_t *lines;           // host, in the caller's order, this part's first frame first
    uint64_t frame0;           // the caller's index of this part's first frame
    zarc_gpu_line *rec;        // host: the call's records
    size_t rec_cap;
    uint8_t *d_text;           // device form: the caller's text buffer
    uint8_t *h_text;           // host form: the caller's text buffer (the part's text is gathered into scratch of the handle first)
    LinesRun *run;
    bool select;               // zarc_gpu_select_lines_batch* with an ACTIVE selection: deliver the selected lines `sel` describes; lines[] counts the hit lines
    ZarcSelect sel;
    uint64_t *selected;        // zarc_gpu_select_lines_batch*; host, as lines (an inactive selection: the plain kernels run, selected == lines)
    MatchesReq mt;
};
// What to search for, as search_prepare has put it on the device: one of three kinds, each with the fields its kernels take
struct Matcher {
    enum Kind { PATTERN, SET, REGEX } kind;
    uint32_t icase;
    struct Pattern { const uint8_t *d_bytes; uint32_t m; };
    union {
        Pattern pattern;              // device: the pattern, folded when icase (zarc_search_scan, zarc_lines_*)
        const ZarcSetDesc *set;       // the handle's set_desc; the blob is h->d_set, the hits of a part h->d_set_hits (zarc_set_*)
        const ZarcRegexDfa *d_regex;  // device: the handle's table (zarc_regex_*)
    };
};
struct SearchReq {
    Matcher match;
    uint64_t *count, *first;   // host, in the caller's order: matching start positions; the lowest, or ZARC_GPU_SEARCH_NONE
    uint64_t *which;           // SET; host, in the caller's order: the lowest pattern that matches at first[i], or ZARC_GPU_SEARCH_NONE
    uint64_t *hits;            // SET; host, per pattern, or null: every part ADDS the positions at which the pattern matches in its frames
    bool lines;                // gather the matching lines as well, as `ln` says
    LinesReq ln;
};
// the request of the part of a call that starts at the caller's frame a
SearchReq part_of(SearchReq r, size_t a)
{
    r.count += a; r.first += a;
    if (r.which) r.which += a;
    if (r.lines) { r.ln.lines += a; r.ln.frame0 += a; if (r.ln.selected) r.ln.selected += a; if (r.ln.mt.on) r.ln.mt.matches += a; }
    return r;
}
// A verify pass that cuts a range out of what it decoded (zarc_gpu_read_ranges_batch*): zarc_range_* run behind the verdict, per part, while
// that part's bytes are in d_vout.  The parts of a call are ranges of the caller's frames in the caller's order, so the running sum in `run`
// gives every frame the same text offset and the same remainder of text_cap however the call is cut.
struct RangeRun { uint64_t text_used = 0; };
struct RangeReq {
    const zarc_gpu_range *range;   // host, in the caller's order, this part's first frame first
    zarc_gpu_range_result *res;    // host, likewise
    uint64_t max_bytes;            // per frame; 0 = no limit
    uint64_t text_cap;             // the call's
    uint8_t *d_text;               // device form: the caller's text buffer
    uint8_t *h_text;               // host form: the caller's text buffer (the part's text is gathered into scratch of the handle first)
    RangeRun *run;
};
RangeReq part_of(RangeReq r, size_t a) { r.range += a; r.res += a; return r; }
// A verify pass that counts what it decoded (zarc_gpu_count_batch*): zarc_wc_* run behind the verdict, per part, while that part's bytes
// are in d_vout.  Every frame's answer is its own, so the parts of a call share nothing.
struct WcReq { zarc_gpu_wc *res; }; // host, in the caller's order, this part's first frame first
WcReq part_of(WcReq r, size_t a) { r.res += a; return r; }
// what the count kernels keep in the handle's scratch for a part of n frames and `raw` decoded bytes (counted against the budget)
uint64_t wc_scratch(size_t n, uint64_t raw) { return (raw / ZARC_CHECK_SLICE + n) * sizeof(ZarcWcSlice) + n * sizeof(ZarcWcFrame); }
// A verify pass that compares what it decoded with other bytes (zarc_gpu_compare_batch*): zarc_cmp_* run behind the verdict, per part, while
// that part's bytes are in d_vout.  Every pair's answer is its own, so the parts of a call share nothing.
struct CmpReq {
    const uint8_t *d_other;               // device: frame i's other side at d_other + other_off[i] (16-byte aligned, padding behind the arena)
    const uint64_t *other_off, *other_len; // host, in the caller's order, this part's first frame first
    zarc_gpu_cmp *res;                    // host, the same order
    bool staged;                          // the host form: the other sides were staged by this call and count against the budget
};
struct CmpHost { const void *const *other; const size_t *other_len; zarc_gpu_cmp *res; }; // the host form's request: caller memory, the caller's order
CmpReq part_of(CmpReq r, size_t a) { r.other_off += a; r.other_len += a; r.res += a; return r; }
// what the compare kernels keep in the handle's scratch for a part of n frames and `raw` decoded bytes (counted against the budget)
uint64_t cmp_scratch(size_t n, uint64_t raw) { return (raw / ZARC_CHECK_SLICE + n) * sizeof(ZarcCmpSlice) + n * (sizeof(ZarcCmpFrame) + 16); }
int lines_text_out(zarc_gpu_t *h, uint8_t *host, const uint8_t *dev, uint64_t bytes);
static_assert(sizeof(ZarcCmpFrame) == sizeof(zarc_gpu_cmp) && sizeof(zarc_gpu_cmp) == 64 && sizeof(ZarcCmpSlice) == 32, "the device's record is the caller's");
static_assert(offsetof(ZarcCmpFrame, prefix) == offsetof(zarc_gpu_cmp, prefix) && offsetof(zarc_gpu_cmp, suffix) == 40, "the device's record is the caller's");
static_assert(ZARC_CMP_R_OTHER_IS_PREFIX == ZARC_GPU_CMP_OTHER_IS_PREFIX && ZARC_CMP_R_DIFFER == ZARC_GPU_CMP_DIFFER && ZARC_CMP_EOF == ZARC_GPU_CMP_EOF, "the device's constants are the caller's");
static_assert(sizeof(ZarcWcFrame) == sizeof(zarc_gpu_wc) && sizeof(zarc_gpu_wc) == 64, "the device's record is the caller's");
static_assert(sizeof(ZarcRangeReq) == sizeof(zarc_gpu_range), "the device's range is the caller's");
static_assert(sizeof(ZarcLineRec) == sizeof(zarc_gpu_line), "the device's record is the caller's");
static_assert(sizeof(ZarcMatchRec) == sizeof(zarc_gpu_match), "the device's record is the caller's");

int unpack_device_split(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len, void *d_dst_base,
                        const uint64_t *dst_off, const uint64_t *raw_len, const uint8_t *expect, uint8_t *digest, int *status, const PackCheck *chk,
                        const SearchReq *srch = nullptr, const RangeReq *rng = nullptr, const WcReq *wc = nullptr, const CmpReq *cmp = nullptr);
int check_pack(zarc_gpu_t *h, size_t n, const void *d_src_base, const uint64_t *src_len, void *d_dst, const uint64_t *dst_off, uint64_t *dst_len,
               int *status, bool trailer, const PackPlanned *pl = nullptr);
void check_message(zarc_gpu_t *h, size_t index);

// have_digests: the caller has hashed the entries already (hash-first dedup): no digest kernels, `digest` is not written
// pl (repack): see PackPlanned; src_off is not looked at (the offsets are on the device), `status` is left alone
int pack_device_impl(zarc_gpu_t *h, size_t n, const void *d_src_base, const uint64_t *src_off, const uint64_t *src_len, void *d_dst,
                     size_t dst_cap, uint64_t *dst_off, uint64_t *dst_len, uint8_t *digest, int *status, bool have_digests,
                     const PackPlanned *pl = nullptr)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!d_src_base || (!src_off && !pl) || !src_len || !d_dst || !dst_off || !dst_len || (!digest && !have_digests)) return ZARC_GPU_E_PARAM;
    ZgeParams P = derive_params(h->params); // (slot_bytes is set per sub-batch below)
#ifdef ZARC_GPU_DIAG
    // host-side phase clock of this call (ZARC_GPU_DBG & 512): where a call over a million entries spends its time outside the kernels
    double hp[8] = {0};
    auto hnow = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double hlast = hnow();
#define HOST_PHASE(i) do { const double n_ = hnow(); hp[i] += n_ - hlast; hlast = n_; } while (0)
#else
#define HOST_PHASE(i) do { } while (0)
#endif
    // the match finder has these compiled in (zge_match.hip: F_*)
    const bool dp = P.level >= 9; // the deep finder (zarc_zge_match_deep)
    const bool fp = P.level <= 1; // the fast finder (zarc_zge_match_fast): the level-3 finder's near table without everything behind it
    if (P.rep_back != 256 || P.back_cap != 8 || P.lazy_delta != 5 || P.min_rep != 3 || P.rep_search != 2 || P.seg_log != 21 || P.short_window_log < 30 ||
        P.lit_cost != (dp ? 6 : 5) || P.rep_cost != 9 || P.tag_bits != 10 || P.far_log != (fp ? 0 : 16) || P.match_cost != (dp ? 10 : 12) || P.far_ways != (dp ? 2 : 1) ||
        P.far_step_log != (dp ? 1 : 5) || P.far_res_log != (dp ? 0 : 2) || (P.far_short != 0) != dp || P.long_log != 13 ||
        P.near16 != (dp ? 0 : 1) || P.short_log != (dp ? 13 : 15) || P.far_cdc_log != (dp ? 0 : 4) || P.lazy2_delta != (dp ? 5 : 0) ||
        P.rep_pass != (dp ? (P.level >= 15 ? 4 : 2) : (fp ? 0 : 1)) || P.live_reps != (dp ? 1 : 0) || P.ext_cap != 960 || P.far_cap != 0 || P.cont_cap != (dp ? 960 : 0) ||
        P.far_back != 48 || P.far_skip != (dp ? 0 : 64) || (fp && P.lazy)) { set_error(h, "internal: encoder parameters differ from the compiled-in ones"); return ZARC_GPU_E_PARAM; }
    uint64_t need = 0;
    for (size_t i = 0; i < n; i++) {
        if (!pl && src_off[i] % ZARC_GPU_ALIGN) { set_error(h, "entry offset not 16-byte aligned"); return ZARC_GPU_E_PARAM; }
        if (src_len[i] >= 0xFFFFFFF0ull) { set_error(h, "entries of 4 GiB or more are not supported"); return ZARC_GPU_E_UNSUPPORTED; }
        dst_off[i] = need;
        need += zarc_gpu_bound((size_t)src_len[i]);
    }
    if (need > dst_cap) return ZARC_GPU_E_DSTSIZE;
    if (!pl) {
        if ((rc = upload_u64(h, h->d_off, src_off, n))) return rc;
        if ((rc = upload_u64(h, h->d_len, src_len, n))) return rc;
    }
    if ((rc = upload_u64(h, h->d_dst_off, dst_off, n))) return rc;
    ZHIP(h->d_dst_len.reserve(n * 8));
    const uint8_t *base = (const uint8_t *)d_src_base;
    const uint64_t *d_off = h->d_off.as<uint64_t>(), *d_len = h->d_len.as<uint64_t>();
    Timer t{h};
    int e0, e1, e2;
    ZHIP(t.mark(&e0));
    if (h->params.compress && !pl) {
        // the frame checksum is a chain of 64-bit multiplies per entry (few waves, latency-bound): it runs on a side stream from the
        // start and is only waited for by the first frame assembly
        ZHIP(hipEventRecord(h->ev_fork, h->stream));
        ZHIP(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
        ZHIP(hipEventRecord(h->ev[14], h->stream2));
        if ((rc = run_xxh64(h, n, base, d_off, d_len, h->stream2))) return rc;
        ZHIP(hipEventRecord(h->ev[15], h->stream2));
        ZHIP(hipEventRecord(h->ev_join, h->stream2));
    }
    // the digest: in store mode right here; otherwise its kernels are queued on the low-priority side stream right behind the first
    // match-finder launch (below): they start when it ends, run beside the entropy stage, and are joined before the digests travel back
    if (!have_digests && (rc = run_blake3(h, n, base, src_off, src_len, d_off, d_len, /*prepare_only=*/h->params.compress != 0))) return rc;
    ZHIP(t.mark(&e1));
    bool digest_queued = have_digests; // nothing to queue
    if (!h->params.compress) {
        // store mode (Encoder::enable_compression(false)): raw-block frames, no checksum (lowlevel_frames.rs:47-84)
        hipLaunchKernelGGL(zarc_zge_store, dim3((unsigned)n), dim3(256), 0, h->stream, base, d_off, d_len, (uint32_t)n, (uint8_t *)d_dst,
                           h->d_dst_off.as<uint64_t>(), h->d_dst_len.as<uint64_t>());
        ZHIP(hipGetLastError());
        ZHIP(t.mark(&e2));
        ZHIP(hipMemcpyAsync(dst_len, h->d_dst_len.p, n * 8, hipMemcpyDeviceToHost, h->stream));
        if (!have_digests) ZHIP(hipMemcpyAsync(digest, h->d_digests.p, n * 32, hipMemcpyDeviceToHost, h->stream));
        ZHIP(hipStreamSynchronize(h->stream));
        if (status) for (size_t i = 0; i < n; i++) status[i] = ZARC_GPU_FRAME_OK;
        h->ms[ZARC_GPU_T_BLAKE3] = elapsed(h, e0, e1);
        h->ms[ZARC_GPU_T_XXH64] = 0;
        h->ms[ZARC_GPU_T_MATCH] = 0;
        h->ms[ZARC_GPU_T_ENTROPY] = 0;
        h->ms[ZARC_GPU_T_ASSEMBLE] = elapsed(h, e1, e2);
        h->ms[ZARC_GPU_T_TOTAL] = h->ms[ZARC_GPU_T_BLAKE3] + h->ms[ZARC_GPU_T_ASSEMBLE];
        if (h->check_frames) return check_pack(h, n, d_src_base, src_len, d_dst, dst_off, dst_len, pl ? pl->status : status, /*trailer=*/false, pl);
        return ZARC_GPU_OK;
    }
    ZHIP(t.mark(&e2));
    bool xxh_joined = pl != nullptr; // (nothing was forked)

    // ---- encoder: frames sorted by size (largest first), processed in sub-batches that fit the scratch budget ----
    HOST_PHASE(0); // checks, descriptor uploads, checksum + digest set-up
    std::vector<uint32_t> order = order_by_size_desc(src_len, n);
    if (pl) order.erase(std::remove_if(order.begin(), order.end(), [pl](uint32_t e) { return pl->status[e] != ZARC_GPU_FRAME_OK; }), order.end());
    const size_t n_ord = order.size(); // entries that get a frame (all of them unless the pass is a planned one)
    HOST_PHASE(1); // size ordering
    const bool split = h->block_split != 0; // blocks cut where their statistics change (zge_split.hip): ZGE_SPLIT_K piece slots per block
    auto per_block_of = [split](uint32_t slot) { return enc_per_block(split, slot); };
    ZHIP(h->d_enc_err.reserve(16));
    ZHIP(hipMemsetAsync(h->d_enc_err.p, 0, 4, h->stream));
    size_t budget = pl && pl->budget ? pl->budget : h->scratch_budget;
    if (!budget) {
        // up to 64 GiB of scratch (BASELINE configs[1] needs 46 GiB to run as ONE launch per kernel), at most 45 % of what is free
        size_t free_b = 0, total_b = 0;
        budget = (size_t)64 << 30;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b / 100 * 45 < budget) budget = free_b / 100 * 45;
        if (budget < ((size_t)1 << 30)) budget = (size_t)1 << 30;
    }
    float ms_match = 0, ms_ent = 0, ms_asm = 0;
    size_t start = 0;
    std::vector<uint64_t> bp;
    while (start < n_ord) {
        // Scratch slots are sized by the largest block of the sub-batch (frames come in descending size): slot_bytes.  A sub-batch also
        // ends where the frames have become four times smaller than its slots, so that a batch of a few large and a million small
        // entries does not give every small one a large slot.
        const uint64_t first_len = src_len[order[start]];
        const uint32_t slot = enc_slot_of(first_len);
        P.slot_bytes = (int)slot;
        const size_t max_blocks = std::max<size_t>(budget / per_block_of(slot), 1);
        size_t end = start, nb = 0;
        while (end < n_ord) {
            const size_t b = (size_t)blocks_of(src_len[order[end]]);
            if (end > start && nb + b > max_blocks) break;
            if (end > start + 4096 && slot > 1024 && src_len[order[end]] * 4 <= slot) break;
            nb += b;
            end++;
        }
        const size_t m = end - start;
        bp.assign(m + 1, 0);
        for (size_t j = 0; j < m; j++) bp[j + 1] = bp[j] + blocks_of(src_len[order[start + j]]);
        if ((rc = upload_u64(h, h->d_block_prefix, bp.data(), m + 1))) return rc;
        if ((rc = upload_u32(h, h->d_order, order.data() + start, m))) return rc;
        ZHIP(h->d_blocks.reserve(nb * sizeof(ZgeBlock)));
        ZHIP(h->d_seq.reserve(nb * (size_t)zge_seq_stride(slot) * 8));
        ZHIP(h->d_lit.reserve(nb * (size_t)zge_lit_stride(slot)));
        ZHIP(h->d_out.reserve(nb * (size_t)zge_out_stride(slot)));
        if (split) {
            ZHIP(h->d_pblocks.reserve(nb * ZGE_SPLIT_K * sizeof(ZgeBlock)));
            ZHIP(h->d_zpieces.reserve(nb * ZGE_SPLIT_K * sizeof(ZgePiece)));
        }
        ZHIP(h->d_queue.reserve(256));
        int a, b, c, d;
        ZHIP(t.mark(&a));
        ZHIP(hipMemsetAsync(h->d_queue.p, 0, 256, h->stream));
        const bool deep = P.level >= 9;
        // the match finder's units of work: the 2^seg_log segments (16 blocks) of every frame, largest frames first
        std::vector<uint32_t> units;
        {
            const uint32_t seg_blocks = (1u << P.seg_log) / ZARC_BLOCK;
            // longest unit first (the queue is a longest-processing-time-first schedule): an unsplit frame of 8 MiB is a longer piece of
            // work than a 2 MiB segment of a split one and has to start before them; the segments of split frames are interleaved frame
            // by frame (equal size: the stable sort keeps that order)
            struct U { uint64_t bytes; uint32_t slot, b0; };
            std::vector<U> us;
            size_t n_split = 0;
            uint64_t max_blocks = 0;
            while (n_split < m && src_len[order[start + n_split]] > ZARC_SPLIT_MIN) { max_blocks = std::max<uint64_t>(max_blocks, bp[n_split + 1] - bp[n_split]); n_split++; }
            for (uint64_t b0 = 0; b0 < max_blocks; b0 += seg_blocks)
                for (size_t j = 0; j < n_split; j++)
                    if (b0 < bp[j + 1] - bp[j]) {
                        const uint64_t len = src_len[order[start + j]], at = b0 * (uint64_t)ZARC_BLOCK;
                        us.push_back(U{std::min<uint64_t>(len - at, (uint64_t)seg_blocks * ZARC_BLOCK), (uint32_t)j, (uint32_t)b0});
                    }
            if (n_split == 0) { // every frame is one unit (zge_match.hip) and the list is in `order` already: longest first
                units.resize(2 * m);
                for (size_t j = 0; j < m; j++) { units[2 * j] = (uint32_t)j; units[2 * j + 1] = 0u; }
            } else {
                for (size_t j = n_split; j < m; j++) us.push_back(U{src_len[order[start + j]], (uint32_t)j, 0u});
                std::stable_sort(us.begin(), us.end(), [](const U &x, const U &y) { return x.bytes > y.bytes; });
                units.reserve(us.size() * 2);
                for (const U &u : us) { units.push_back(u.slot); units.push_back(u.b0); }
            }
        }
        const size_t n_units = units.size() / 2;
        if ((rc = upload_u32(h, h->d_units, units.data(), units.size()))) return rc;
        HOST_PHASE(2); // sub-batch lists + uploads
        auto match_kernel = deep ? zarc_zge_match_deep : (P.level <= 1 ? zarc_zge_match_fast : zarc_zge_match);
#ifdef ZARC_GPU_DIAG
        if (P.dbg) match_kernel = deep ? zarc_zge_match_deep_diag : zarc_zge_match_diag;
#endif
        // persistent workgroups: as many as the chip holds at once -- two of 80 KiB of LDS and 128 registers per thread on a CU; the
        // deep finder's register count decides whether it is one or two (asked once)
        if (deep && h->deep_per_cu == 0) {
            int per_cu = 0;
            ZHIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, match_kernel, 512, 0));
            h->deep_per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);
        }
        const size_t match_grid = std::min<size_t>(n_units, (size_t)h->num_cus * (size_t)(deep ? h->deep_per_cu : 2));
        ZHIP(h->d_far.reserve(match_grid * zge_far_words(P) * 4 + 16)); // one far-table slab per resident workgroup (cleared by the kernel per frame)
        // The digest kernels (low-priority stream, queued behind the FIRST sub-batch's match launch) must be off the chip before another
        // match launch: measured on the configs[4] shape, a second launch that found the last 4 ms of them still running took 326 ms
        // instead of 209 (kernel trace in gpurun_out/trace_dpp.txt) -- the persistent workgroups keep whatever uneven placement the
        // launch moment gave them.
        if (digest_queued && !have_digests) ZHIP(hipStreamWaitEvent(h->stream, h->ev_join3, 0));
        hipLaunchKernelGGL(match_kernel, dim3((unsigned)match_grid), dim3(512), 0, h->stream, P, base, d_off, d_len, h->d_order.as<uint32_t>(), h->d_units.as<uint32_t>(), (uint32_t)n_units,
                           h->d_block_prefix.as<uint64_t>(), h->d_blocks.as<ZgeBlock>(), h->d_seq.as<uint64_t>(), h->d_lit.as<uint8_t>(),
                           h->d_queue.as<uint32_t>(), h->d_far.as<uint32_t>());
        ZHIP(hipGetLastError());
        if (!digest_queued) {
            ZHIP(hipEventRecord(h->ev_fork3, h->stream)); // orders the side stream behind the descriptor uploads (and this launch)
            ZHIP(hipStreamWaitEvent(h->stream3, h->ev_fork3, 0));
            ZHIP(hipEventRecord(h->ev_b3[0], h->stream3));
            if ((rc = run_blake3(h, n, base, src_off, src_len, d_off, d_len, false, /*launch_only=*/true, h->stream3))) return rc;
            ZHIP(hipEventRecord(h->ev_b3[1], h->stream3));
            ZHIP(hipEventRecord(h->ev_join3, h->stream3));
            digest_queued = true;
        }
        ZHIP(t.mark(&b));
        {
            unsigned long long *const eprof = (P.dbg & 1024) ? (unsigned long long *)((char *)h->d_queue.p + 128) : (unsigned long long *)nullptr;
            if (split) {
                // block splitting: the cut decision, then the same stage with a wave per parent that codes the parent's pieces one after
                // the other; frames of one block keep the one-pass kernel, their pieces choose their tables alone
                const size_t ns = nb * ZGE_SPLIT_K; // piece slots
                hipLaunchKernelGGL(zarc_zge_split, dim3((unsigned)nb), dim3(64), 0, h->stream, (uint32_t)nb, slot, h->d_blocks.as<ZgeBlock>(), h->d_seq.as<uint64_t>(),
                                   h->d_lit.as<uint8_t>(), h->d_pblocks.as<ZgeBlock>(), h->d_zpieces.as<ZgePiece>());
                if (bp[1] - bp[0] > 1) {
                    ZHIP(h->d_plan.reserve(ns * sizeof(ZgePlan)));
                    std::vector<uint32_t> groups;
                    for (size_t j = 0; j < m && bp[j + 1] - bp[j] > 1; j++)
                        for (uint64_t g0 = bp[j]; g0 < bp[j + 1]; g0 += ZGE_TABLE_GROUP) groups.push_back((uint32_t)g0);
                    if ((rc = upload_u32(h, h->d_groups, groups.data(), groups.size()))) return rc;
                    hipLaunchKernelGGL(zarc_zge_entropy_p1_split, dim3((unsigned)nb), dim3(64), 0, h->stream, (uint32_t)nb, slot, h->d_pblocks.as<ZgeBlock>(),
                                       h->d_seq.as<uint64_t>(), h->d_lit.as<uint8_t>(), h->d_out.as<uint8_t>(), eprof, h->d_plan.as<ZgePlan>(), h->d_zpieces.as<ZgePiece>());
                    hipLaunchKernelGGL(zarc_zge_plan_split, dim3((unsigned)groups.size()), dim3(64), 0, h->stream, (uint32_t)nb, h->d_blocks.as<ZgeBlock>(),
                                       h->d_plan.as<ZgePlan>(), h->d_groups.as<uint32_t>(), h->d_pblocks.as<ZgeBlock>());
                    hipLaunchKernelGGL(zarc_zge_entropy_p2_split, dim3((unsigned)nb), dim3(64), 0, h->stream, (uint32_t)nb, slot, h->d_pblocks.as<ZgeBlock>(),
                                       h->d_seq.as<uint64_t>(), h->d_lit.as<uint8_t>(), h->d_out.as<uint8_t>(), eprof, h->d_plan.as<ZgePlan>(),
                                       h->d_enc_err.as<uint32_t>(), h->d_zpieces.as<ZgePiece>());
                } else
                    hipLaunchKernelGGL(zarc_zge_entropy_split, dim3((unsigned)nb), dim3(64), 0, h->stream, (uint32_t)nb, slot, h->d_pblocks.as<ZgeBlock>(),
                                       h->d_seq.as<uint64_t>(), h->d_lit.as<uint8_t>(), h->d_out.as<uint8_t>(), eprof, h->d_zpieces.as<ZgePiece>());
            } else if (bp[1] - bp[0] > 1) {
                // the sub-batch holds frames of several blocks (the largest comes first): the entropy stage runs in two passes around the
                // table plan, which lets the blocks of a group share their sequence tables (zge_entropy.hip: zarc_zge_plan).  (Neither
                // running pass 1 of one half of the blocks beside pass 2 of the other nor moving the digest kernels beside pass 2 gave any
                // time back: tools/r4_ab5.sh, r4_ab7.sh, EXPERIMENTS.md.  What pass 2 spends is the latency of its FSE state chains, three
                // lanes of a wave: 9.0 of its 13.0 ms at configs[1] go when they are taken out, 9.5 with the table build, EXPERIMENTS.md
                // round 18.  With ZARC_GPU_PX_SEQ_STATES on, zarc_zge_seq_states runs the chains of the blocks of a group that share their
                // tables on one wave in front of pass 2, which then has neither chain nor table build for those blocks.)
                ZHIP(h->d_plan.reserve(nb * sizeof(ZgePlan)));
                std::vector<uint32_t> groups; // first block slot of every group of a frame with more than one block (frames come largest first)
                for (size_t j = 0; j < m && bp[j + 1] - bp[j] > 1; j++)
                    for (uint64_t g0 = bp[j]; g0 < bp[j + 1]; g0 += ZGE_TABLE_GROUP) groups.push_back((uint32_t)g0);
                if ((rc = upload_u32(h, h->d_groups, groups.data(), groups.size()))) return rc;
                hipLaunchKernelGGL(zarc_zge_entropy_p1, dim3((unsigned)nb), dim3(64), 0, h->stream, (uint32_t)nb, slot, h->d_blocks.as<ZgeBlock>(),
                                   h->d_seq.as<uint64_t>(), h->d_lit.as<uint8_t>(), h->d_out.as<uint8_t>(), eprof, h->d_plan.as<ZgePlan>());
                hipLaunchKernelGGL(zarc_zge_plan, dim3((unsigned)groups.size()), dim3(64), 0, h->stream, (uint32_t)nb, h->d_blocks.as<ZgeBlock>(), h->d_plan.as<ZgePlan>(),
                                   h->d_groups.as<uint32_t>());
                if (h->seq_states) { // the literal slots are free from here on: a block's states go where its literals were
                    uint32_t cap_words = (uint32_t)(zge_lit_stride(slot) / 4);
                    if (h->seq_states > 1) cap_words = std::min<uint32_t>(cap_words, (uint32_t)h->seq_states);
                    hipLaunchKernelGGL(zarc_zge_seq_states, dim3((unsigned)groups.size()), dim3(64), 0, h->stream, (uint32_t)nb, slot, h->d_blocks.as<ZgeBlock>(),
                                       h->d_seq.as<uint64_t>(), h->d_lit.as<uint8_t>(), h->d_plan.as<ZgePlan>(), h->d_groups.as<uint32_t>(), cap_words, eprof);
                }
                hipLaunchKernelGGL(zarc_zge_entropy_p2, dim3((unsigned)nb), dim3(64), 0, h->stream, (uint32_t)nb, slot, h->d_blocks.as<ZgeBlock>(),
                                   h->d_seq.as<uint64_t>(), h->d_lit.as<uint8_t>(), h->d_out.as<uint8_t>(), eprof, h->d_plan.as<ZgePlan>(), h->d_enc_err.as<uint32_t>());
            } else
                hipLaunchKernelGGL(zarc_zge_entropy, dim3((unsigned)nb), dim3(64), 0, h->stream, (uint32_t)nb, slot, h->d_blocks.as<ZgeBlock>(),
                                   h->d_seq.as<uint64_t>(), h->d_lit.as<uint8_t>(), h->d_out.as<uint8_t>(), eprof);
        }
        ZHIP(hipGetLastError());
        ZHIP(t.mark(&c));
        if (!xxh_joined) { ZHIP(hipStreamWaitEvent(h->stream, h->ev_join, 0)); xxh_joined = true; }
        const uint64_t *const d_xxh = pl ? pl->d_xxh : h->d_xxh.as<uint64_t>();
        if (split)
            hipLaunchKernelGGL(zarc_zge_assemble_split, dim3((unsigned)m), dim3(256), 0, h->stream, P, base, d_off, d_len, h->d_order.as<uint32_t>(), (uint32_t)m,
                               h->d_block_prefix.as<uint64_t>(), h->d_blocks.as<ZgeBlock>(), h->d_out.as<uint8_t>(), d_xxh,
                               (uint8_t *)d_dst, h->d_dst_off.as<uint64_t>(), h->d_dst_len.as<uint64_t>(), h->d_pblocks.as<ZgeBlock>(), h->d_zpieces.as<ZgePiece>());
        else
            hipLaunchKernelGGL(zarc_zge_assemble, dim3((unsigned)m), dim3(256), 0, h->stream, P, base, d_off, d_len, h->d_order.as<uint32_t>(), (uint32_t)m,
                               h->d_block_prefix.as<uint64_t>(), h->d_blocks.as<ZgeBlock>(), h->d_out.as<uint8_t>(), d_xxh,
                               (uint8_t *)d_dst, h->d_dst_off.as<uint64_t>(), h->d_dst_len.as<uint64_t>());
        ZHIP(hipGetLastError());
        ZHIP(t.mark(&d));
        HOST_PHASE(3); // launches
        ZHIP(hipStreamSynchronize(h->stream)); // the scratch is reused by the next sub-batch; also bounds the event pool
        HOST_PHASE(4); // waiting for the kernels
        if (P.dbg & 1024) { // stage timing of the match finder (diagnostics)
            unsigned long long prof[15];
            ZHIP(hipMemcpy(prof, (const char *)h->d_queue.p + 8, sizeof prof, hipMemcpyDeviceToHost));
            unsigned long long tot = 0;
            for (int i = 0; i < 15; i++) tot += prof[i];
            fprintf(stderr, "zge_match stage ticks (%% of %llu):", tot);
            for (int i = 0; i < 15; i++) fprintf(stderr, " %d:%.1f", i, tot ? 100.0 * (double)prof[i] / (double)tot : 0.0);
            fprintf(stderr, "\n");
            ZHIP(hipMemcpy(prof, (const char *)h->d_queue.p + 128, 8 * 8, hipMemcpyDeviceToHost)); // [6]: zarc_zge_seq_states, all of a wave's ticks; [7]: blocks it took
            tot = 0;
            for (int i = 0; i < 7; i++) tot += prof[i];
            fprintf(stderr, "zge_entropy stage ticks (%% of %llu): hist %.1f huf-build %.1f lit-encode %.1f seq-prepass %.1f seq-tables %.1f seq-encode %.1f seq-states %.1f; seq-states blocks %llu\n", tot,
                    100.0 * prof[0] / tot, 100.0 * prof[1] / tot, 100.0 * prof[2] / tot, 100.0 * prof[3] / tot, 100.0 * prof[4] / tot, 100.0 * prof[5] / tot,
                    100.0 * prof[6] / tot, prof[7]);
        }
        ms_match += elapsed(h, a, b);
        ms_ent += elapsed(h, b, c);
        ms_asm += elapsed(h, c, d);
        t.next = 3;
        start = end;
    }
    if (!have_digests) ZHIP(hipStreamWaitEvent(h->stream, h->ev_join3, 0)); // the digests are done
    ZHIP(hipMemcpyAsync(dst_len, h->d_dst_len.p, n * 8, hipMemcpyDeviceToHost, h->stream));
    if (!have_digests) ZHIP(hipMemcpyAsync(digest, h->d_digests.p, n * 32, hipMemcpyDeviceToHost, h->stream));
    uint32_t enc_err = 0;
    ZHIP(hipMemcpyAsync(&enc_err, h->d_enc_err.p, 4, hipMemcpyDeviceToHost, h->stream));
    ZHIP(hipStreamSynchronize(h->stream));
    if (enc_err) { set_error(h, "internal: a block the table plan guaranteed to end up compressed did not (its successor may repeat tables the decoder never saw)"); return ZARC_GPU_E_DEVICE; }
    if (status) for (size_t i = 0; i < n; i++) status[i] = ZARC_GPU_FRAME_OK;
    HOST_PHASE(5); // results back
#ifdef ZARC_GPU_DIAG
    if (P.dbg & 512) fprintf(stderr, "pack host phases (ms): setup %.2f order %.2f lists %.2f launch %.2f wait %.2f results %.2f\n", hp[0], hp[1], hp[2], hp[3], hp[4], hp[5]);
#endif
    if (have_digests) h->ms[ZARC_GPU_T_BLAKE3] = 0;
    else { float ms = -1.f; if (hipEventElapsedTime(&ms, h->ev_b3[0], h->ev_b3[1]) == hipSuccess) h->ms[ZARC_GPU_T_BLAKE3] = ms; } // side stream: queue wait + kernels
    h->ms[ZARC_GPU_T_XXH64] = pl ? 0 : elapsed(h, 14, 15); // side stream: overlaps the match finder, not part of the total
    h->ms[ZARC_GPU_T_MATCH] = ms_match;
    h->ms[ZARC_GPU_T_ENTROPY] = ms_ent;
    h->ms[ZARC_GPU_T_ASSEMBLE] = ms_asm;
    h->ms[ZARC_GPU_T_TOTAL] = elapsed(h, e0, e1) + ms_match + ms_ent + ms_asm; // the digest and the checksum run beside these
    // read-back check: pack has taken its results off the buffers it shares with the decoder; sources and frames are still resident
    if (h->check_frames) return check_pack(h, n, d_src_base, src_len, d_dst, dst_off, dst_len, pl ? pl->status : status, P.checksum != 0, pl);
    return ZARC_GPU_OK;
}

// ZARC_GPU_PX_CHECK_FRAMES: decode the frames this pass has assembled (decode-only, into the handle's scratch) and compare the bytes with
// the sources (zarc_check_compare).  The decoder's timers stay out of h->ms: the call reports pack's.
// pl (repack): only the entries the pass has packed (status OK) have a frame to check
int check_pack(zarc_gpu_t *h, size_t n, const void *d_src_base, const uint64_t *src_len, void *d_dst, const uint64_t *dst_off, uint64_t *dst_len,
               int *status, bool trailer, const PackPlanned *pl)
{
#ifdef ZARC_GPU_DIAG
    // fault injection (diagnostic build only): one byte of one assembled frame, between assembly and the check.  The decoder is built to
    // distrust what it reads; this shows the check failing, which it otherwise never would
    for (int tail = 0; tail < 2; tail++) {
        const int idx = diag_env(tail ? "ZARC_GPU_CHECK_FLIP_TAIL" : "ZARC_GPU_CHECK_FLIP_BODY", -1);
        if (idx < 0 || (size_t)idx >= n || (pl && pl->status[idx] != ZARC_GPU_FRAME_OK) || dst_len[idx] == 0) continue;
        uint8_t *at = (uint8_t *)d_dst + dst_off[idx] + (tail ? dst_len[idx] - 1 : dst_len[idx] / 2), v = 0;
        ZHIP(hipMemcpy(&v, at, 1, hipMemcpyDeviceToHost));
        v ^= 0xFF;
        ZHIP(hipMemcpy(at, &v, 1, hipMemcpyHostToDevice));
    }
#endif
    std::vector<uint32_t> first_bad(n, ZARC_CHECK_CLEAN);
    h->chk_ms = 0;
    int rc;
    if (pl) {
        std::vector<uint32_t> keep, bad;
        std::vector<uint64_t> off, len, raw;
        for (size_t i = 0; i < n; i++)
            if (pl->status[i] == ZARC_GPU_FRAME_OK) { keep.push_back((uint32_t)i); off.push_back(dst_off[i]); len.push_back(dst_len[i]); raw.push_back(src_len[i]); }
        if (keep.empty()) return ZARC_GPU_OK;
        bad.assign(keep.size(), ZARC_CHECK_CLEAN);
        const PackCheck chk{(const uint8_t *)d_src_base, trailer, 0u, bad.data(), &h->chk_ms, keep.data(), pl->d_xxh};
        rc = unpack_device_split(h, keep.size(), d_dst, off.data(), len.data(), nullptr, nullptr, raw.data(), nullptr, nullptr, nullptr, &chk);
        for (size_t j = 0; j < keep.size(); j++) first_bad[keep[j]] = bad[j];
    } else {
        const PackCheck chk{(const uint8_t *)d_src_base, trailer, 0u, first_bad.data(), &h->chk_ms, nullptr, nullptr};
        rc = unpack_device_split(h, n, d_dst, dst_off, dst_len, nullptr, nullptr, src_len, nullptr, nullptr, nullptr, &chk);
    }
    if (rc) return rc;
#ifdef ZARC_GPU_DIAG
    if (diag_env("ZARC_GPU_CHECK_STATS", 0)) fprintf(stderr, "zarc_check_compare: %.3f ms\n", h->chk_ms);
#endif
    bool any = false;
    for (size_t i = 0; i < n; i++) {
        if (first_bad[i] == ZARC_CHECK_CLEAN) continue;
        if (!any) { any = true; h->chk_index = i; h->chk_at = first_bad[i]; }
        if (status) status[i] = ZARC_GPU_FRAME_CORRUPT;
        dst_len[i] = 0;
    }
    if (!any) return ZARC_GPU_OK;
    check_message(h, h->chk_index);
    return ZARC_GPU_E_CHECK;
}

// (the callers above pack_device_impl know an entry by another index: they say it again with theirs)
void check_message(zarc_gpu_t *h, size_t index)
{
    char msg[160];
    if (h->chk_at == ZARC_CHECK_TRAILER) snprintf(msg, sizeof msg, "read-back check: entry %zu: checksum trailer differs from the XXH64 of its source", index);
    else snprintf(msg, sizeof msg, "read-back check: entry %zu decodes to other bytes than its source, first at byte %u", index, h->chk_at);
    h->chk_index = index;
    set_error(h, msg);
}

// Hash first (content_frame.rs:26-33): digest every entry, ask the caller which digests it has a frame for already, compress the rest.
// `known(ctx, digest, i)` is called once per entry in index order on the calling thread; nonzero = skip this entry
// (status ZARC_GPU_FRAME_DUPLICATE, dst_len 0).  A caller that returns 0 is expected to remember the digest, so that a later copy
// inside the same batch is skipped as well (first occurrence wins).
int pack_device_dedup_impl(zarc_gpu_t *h, size_t n, const void *d_src_base, const uint64_t *src_off, const uint64_t *src_len, void *d_dst,
                           size_t dst_cap, uint64_t *dst_off, uint64_t *dst_len, uint8_t *digest, int *status, zarc_gpu_known_fn known, void *ctx)
{
    if (!known) return pack_device_impl(h, n, d_src_base, src_off, src_len, d_dst, dst_cap, dst_off, dst_len, digest, status, false);
    if (!status) return ZARC_GPU_E_PARAM;
    int rc = zarc_gpu_blake3_batch_device(h, n, d_src_base, src_off, src_len, digest);
    if (rc) return rc;
    const float ms_b3 = h->ms[ZARC_GPU_T_BLAKE3];
    std::vector<size_t> keep;
    for (size_t i = 0; i < n; i++) {
        dst_off[i] = 0; dst_len[i] = 0;
        if (known(ctx, digest + i * 32, i)) status[i] = ZARC_GPU_FRAME_DUPLICATE;
        else keep.push_back(i);
    }
    if (keep.empty()) { for (int t = 0; t < ZARC_GPU_T_COUNT; t++) if (t != ZARC_GPU_T_BLAKE3 && t != ZARC_GPU_T_TOTAL) h->ms[t] = 0; return ZARC_GPU_OK; }
    const size_t m = keep.size();
    std::vector<uint64_t> off(m), len(m), doff(m), dlen(m);
    std::vector<int> st(m);
    for (size_t j = 0; j < m; j++) { off[j] = src_off[keep[j]]; len[j] = src_len[keep[j]]; }
    rc = pack_device_impl(h, m, d_src_base, off.data(), len.data(), d_dst, dst_cap, doff.data(), dlen.data(), nullptr, st.data(), true);
    if (rc && rc != ZARC_GPU_E_CHECK) return rc;
    for (size_t j = 0; j < m; j++) { dst_off[keep[j]] = doff[j]; dst_len[keep[j]] = dlen[j]; status[keep[j]] = st[j]; }
    if (rc) { check_message(h, keep[h->chk_index]); return rc; }
    h->ms[ZARC_GPU_T_BLAKE3] = ms_b3;
    h->ms[ZARC_GPU_T_TOTAL] += ms_b3;
    return ZARC_GPU_OK;
}
} // namespace
extern "C" {

int zarc_gpu_pack_batch_device(zarc_gpu_t *h, size_t n, const void *d_src_base, const uint64_t *src_off, const uint64_t *src_len, void *d_dst,
                               size_t dst_cap, uint64_t *dst_off, uint64_t *dst_len, uint8_t *digest, int *status)
{
    return pack_device_impl(h, n, d_src_base, src_off, src_len, d_dst, dst_cap, dst_off, dst_len, digest, status, false);
}

int zarc_gpu_pack_batch_device_dedup(zarc_gpu_t *h, size_t n, const void *d_src_base, const uint64_t *src_off, const uint64_t *src_len, void *d_dst,
                                     size_t dst_cap, uint64_t *dst_off, uint64_t *dst_len, uint8_t *digest, int *status, zarc_gpu_known_fn known, void *ctx)
{
    if (n && (!digest || !dst_off || !dst_len)) return ZARC_GPU_E_PARAM;
    return pack_device_dedup_impl(h, n, d_src_base, src_off, src_len, d_dst, dst_cap, dst_off, dst_len, digest, status, known, ctx);
}

// The decoder's stages (sequences + literals ahead, frame pass, checksum + digest) of ONE frame are a chain, and a large frame's chain
// is long whatever runs beside it (one wave walks its blocks; XXH64 is serial by construction).  Frames are therefore taken in
// descending size and dealt into up to DEC_GROUPS groups of equal bytes, each group with its own pair of streams: the frame pass and
// the hashes of the large frames start as soon as THEIR sequences and literals are decoded and run beside the earlier stages of the
// groups behind them.  Per-frame arrays are uploaded in that order (group = index range = slot range); results go back in the caller's.
} // extern "C"
namespace {
constexpr int UNPACK_SPLIT = -1000; // internal: the decoder's scratch for this batch exceeds the budget, run it in two parts

// ---- the stages behind the decoder: the read-back check of pack, or the search of a verify pass ----
// What they see of the part unpack_device_once has just decoded.  Every per-frame array, on the host and on the device, is in the decoder's
// order; the stages queue their work on the engine stream and none of them waits for it but where it says so.
struct DecodedPart {
    zarc_gpu *h;
    size_t n;
    const std::vector<uint32_t> &order;   // the caller's index of the decoder's frame i
    const std::vector<uint64_t> &raw_len;
    const uint8_t *d_base;                // the decoded bytes: frame i at d_base + d_off[i]
    const uint64_t *d_off;
    const int32_t *d_status;
    Timer &t;
};
// slice prefix of the part's frames (a slice is ZARC_CHECK_SLICE bytes; every frame has one at least) -> buf; *total: slices in all
int upload_slices(const DecodedPart &p, DevBuf &buf, const char *too_large, uint64_t *total)
{
    zarc_gpu *const h = p.h;
    std::vector<uint64_t> slices(p.n + 1, 0);
    for (size_t i = 0; i < p.n; i++) slices[i + 1] = slices[i] + std::max<uint64_t>(1, (p.raw_len[i] + ZARC_CHECK_SLICE - 1) / ZARC_CHECK_SLICE);
    if (slices[p.n] > 0x7FFFFFFFull) { set_error(h, too_large); return ZARC_GPU_E_PARAM; }
    *total = slices[p.n];
    return upload_u64(h, buf, slices.data(), p.n + 1);
}

// read-back check: decoded bytes against the pack pass's sources (the frame passes are joined; with one group they ran on the engine
// stream).  Waits for the result.
int readback_compare(const DecodedPart &p, const PackCheck &chk, const void *d_frames_base)
{
    zarc_gpu *const h = p.h;
    const size_t n = p.n;
    int rc, e3, e4;
    uint64_t slices = 0;
    if ((rc = upload_slices(p, h->d_chk_slices, "read-back check: batch too large", &slices))) return rc;
    if (chk.entry_map) { // a pass with skipped entries: the frames are a subset of its entries
        std::vector<uint32_t> mapped(n);
        for (size_t i = 0; i < n; i++) mapped[i] = chk.entry_map[p.order[i]];
        if ((rc = upload_u32(h, h->d_chk_order, mapped.data(), n))) return rc;
    } else if ((rc = upload_u32(h, h->d_chk_order, p.order.data(), n))) return rc;
    ZHIP(h->d_chk_bad.reserve(n * 4));
    ZHIP(hipMemsetAsync(h->d_chk_bad.p, 0xFF, n * 4, h->stream));
    ZHIP(p.t.mark(&e3));
    hipLaunchKernelGGL(zarc_check_compare, dim3((unsigned)slices), dim3(256), 0, h->stream, (uint32_t)n, h->d_chk_slices.as<uint64_t>(), h->d_chk_order.as<uint32_t>(),
                       chk.entry0, p.d_base, p.d_off, p.d_status, chk.src_base, h->d_off.as<uint64_t>(),
                       h->d_len.as<uint64_t>(), (const uint8_t *)d_frames_base, h->d_dst_off.as<uint64_t>(), h->d_dst_len.as<uint64_t>(),
                       chk.trailer ? (chk.xxh ? chk.xxh : h->d_xxh.as<uint64_t>()) : (const uint64_t *)nullptr, h->d_chk_bad.as<uint32_t>());
    ZHIP(hipGetLastError());
    ZHIP(p.t.mark(&e4));
    std::vector<uint32_t> bad(n);
    ZHIP(hipMemcpyAsync(bad.data(), h->d_chk_bad.p, n * 4, hipMemcpyDeviceToHost, h->stream));
    ZHIP(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; i++) chk.first_bad[p.order[i]] = bad[i];
    *chk.ms += elapsed(h, e3, e4);
    return ZARC_GPU_OK;
}

// what a part's search carries from one of its stages to the next
struct SearchPart {
    uint64_t slices = 0;               // of all the part's frames
    size_t set_lds = 0;                // SET: bytes of the set's image in LDS
    int e5 = -1, e6 = -1, e7 = -1;     // timer marks: in front of the scan, behind it, behind the first half of the lines
    float lines_ms2 = 0;               // the second half of the lines
    std::vector<uint32_t> count, first, which, hits, lines, selected; // what search_collect asked back (decoder order), for search_scatter
};

// search: the decoded bytes are judged; look through those of the frames that decoded, where they lie
int search_launch(const DecodedPart &p, const SearchReq &srch, SearchPart &sp)
{
    zarc_gpu *const h = p.h;
    const Matcher &mt = srch.match;
    const uint32_t n = (uint32_t)p.n;
    int rc;
    if ((rc = upload_slices(p, h->d_srch_slices, "search: batch too large", &sp.slices))) return rc;
    const dim3 per_slice((unsigned)sp.slices), per_frame((unsigned)((p.n + 255) / 256)), per_4((unsigned)((p.n + 3) / 4));
    const uint64_t *const d_slices = h->d_srch_slices.as<uint64_t>(), *const d_raw = h->d_raw_len.as<uint64_t>();
    ZHIP(h->d_srch_count.reserve(p.n * 4));
    ZHIP(h->d_srch_first.reserve(p.n * 4));
    ZHIP(hipMemsetAsync(h->d_srch_count.p, 0, p.n * 4, h->stream));
    ZHIP(hipMemsetAsync(h->d_srch_first.p, 0xFF, p.n * 4, h->stream));
    uint32_t *const d_count = h->d_srch_count.as<uint32_t>(), *const d_first = h->d_srch_first.as<uint32_t>();
    switch (mt.kind) {
    case Matcher::PATTERN:
        ZHIP(p.t.mark(&sp.e5));
        hipLaunchKernelGGL(zarc_search_scan, per_slice, dim3(256), 0, h->stream, n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, mt.pattern.d_bytes, mt.pattern.m,
                           mt.icase, d_count, d_first);
        break;
    case Matcher::SET:
        sp.set_lds = (size_t)mt.set->lds_words * 4;
        ZHIP(h->d_set_which.reserve(p.n * 4));
        if (srch.hits) ZHIP(hipMemsetAsync(h->d_set_hits.p, 0, (size_t)mt.set->count * 4, h->stream)); // (reserved by search_upload_set)
        ZHIP(p.t.mark(&sp.e5));
        hipLaunchKernelGGL(zarc_set_scan, per_slice, dim3(256), sp.set_lds, h->stream, n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, *mt.set, h->d_set.as<uint32_t>(),
                           mt.icase, d_count, d_first, srch.hits ? h->d_set_hits.as<uint32_t>() : (uint32_t *)nullptr);
        hipLaunchKernelGGL(zarc_set_which, per_frame, dim3(256), 0, h->stream, n, p.d_base, p.d_off, d_raw, *mt.set, h->d_set.as<uint32_t>(), mt.icase,
                           d_count, d_first, h->d_set_which.as<uint32_t>());
        break;
    case Matcher::REGEX: // what every slice does to the state, every slice's entry state from the frame's end down, then the scan
        ZHIP(h->d_re_summary.reserve(sp.slices * sizeof(ZarcRegexSlice)));
        ZHIP(h->d_re_entry.reserve(sp.slices));
        ZHIP(p.t.mark(&sp.e5));
        hipLaunchKernelGGL(zarc_regex_summary, per_slice, dim3(256), 0, h->stream, n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, mt.d_regex,
                           h->d_re_summary.as<ZarcRegexSlice>());
        hipLaunchKernelGGL(zarc_regex_carry, per_4, dim3(256), 0, h->stream, n, d_slices, p.d_status, mt.d_regex, h->d_re_summary.as<ZarcRegexSlice>(),
                           h->d_re_entry.as<uint8_t>());
        hipLaunchKernelGGL(zarc_regex_scan, per_slice, dim3(256), 0, h->stream, n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, mt.d_regex,
                           h->d_re_entry.as<uint8_t>(), d_count, d_first);
        break;
    }
    ZHIP(hipGetLastError());
    ZHIP(p.t.mark(&sp.e6));
    return ZARC_GPU_OK;
}

// lines, first half: what every slice holds, what every slice must know of its neighbours, lines[] of every frame
int lines_mark(const DecodedPart &p, const SearchReq &srch, SearchPart &sp)
{
    zarc_gpu *const h = p.h;
    const Matcher &mt = srch.match;
    const uint32_t n = (uint32_t)p.n;
    const dim3 per_slice((unsigned)sp.slices);
    const uint64_t *const d_slices = h->d_srch_slices.as<uint64_t>(), *const d_raw = h->d_raw_len.as<uint64_t>();
    ZHIP(h->d_ln_slices.reserve(sp.slices * sizeof(ZarcLineSlice)));
    ZHIP(h->d_ln_lines.reserve(p.n * 4));
    ZarcLineSlice *const d_ln = h->d_ln_slices.as<ZarcLineSlice>();
    uint32_t *const d_lines = h->d_ln_lines.as<uint32_t>();
    if (srch.ln.select) { // the selected lines: a line belongs to the slice in which it ends, the carry counts hits and selected lines
        const ZarcSelect q = srch.ln.sel;
        ZHIP(h->d_sel_slices.reserve(sp.slices * sizeof(ZarcSelSlice)));
        ZHIP(h->d_sel_count.reserve(p.n * 4));
        ZarcSelSlice *const d_sel = h->d_sel_slices.as<ZarcSelSlice>();
        switch (mt.kind) {
        case Matcher::PATTERN:
            hipLaunchKernelGGL(zarc_lines_select_mark, per_slice, dim3(256), 0, h->stream, n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, mt.pattern.d_bytes,
                               mt.pattern.m, mt.icase, q, d_sel);
            break;
        case Matcher::SET:
            hipLaunchKernelGGL(zarc_lines_select_mark_set, per_slice, dim3(256), sp.set_lds, h->stream, n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, *mt.set,
                               h->d_set.as<uint32_t>(), mt.icase, q, d_sel);
            break;
        case Matcher::REGEX:
            hipLaunchKernelGGL(zarc_lines_select_mark_regex, per_slice, dim3(256), 0, h->stream, n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, mt.d_regex,
                               h->d_re_entry.as<uint8_t>(), q, d_sel);
            break;
        }
        hipLaunchKernelGGL(zarc_lines_select_carry, dim3((unsigned)((p.n + 3) / 4)), dim3(256), 0, h->stream, n, d_slices, d_raw, q, d_sel, d_lines,
                           h->d_sel_count.as<uint32_t>());
        ZHIP(hipGetLastError());
        ZHIP(p.t.mark(&sp.e7));
        return ZARC_GPU_OK;
    }
    switch (mt.kind) {
    case Matcher::PATTERN:
        hipLaunchKernelGGL(zarc_lines_mark, per_slice, dim3(256), 0, h->stream, n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, mt.pattern.d_bytes, mt.pattern.m,
                           mt.icase, d_ln, d_lines);
        break;
    case Matcher::SET:
        hipLaunchKernelGGL(zarc_lines_mark_set, per_slice, dim3(256), sp.set_lds, h->stream, n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, *mt.set,
                           h->d_set.as<uint32_t>(), mt.icase, d_ln, d_lines);
        break;
    case Matcher::REGEX:
        hipLaunchKernelGGL(zarc_lines_mark_regex, per_slice, dim3(256), 0, h->stream, n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, mt.d_regex,
                           h->d_re_entry.as<uint8_t>(), d_ln, d_lines);
        break;
    }
    hipLaunchKernelGGL(zarc_lines_carry, dim3((unsigned)((p.n + 3) / 4)), dim3(256), 0, h->stream, n, d_slices, d_raw, d_ln, d_lines);
    ZHIP(hipGetLastError());
    ZHIP(p.t.mark(&sp.e7));
    return ZARC_GPU_OK;
}

// The search's per-frame results are asked back here and are on the host behind the caller's next synchronize -- the one the part's statuses
// and digests wait for as well -- where search_scatter takes them to the caller's order.
int search_collect(const DecodedPart &p, const SearchReq &srch, SearchPart &sp)
{
    zarc_gpu *const h = p.h;
    const size_t n = p.n;
    sp.count.resize(n); sp.first.resize(n);
    ZHIP(hipMemcpyAsync(sp.count.data(), h->d_srch_count.p, n * 4, hipMemcpyDeviceToHost, h->stream));
    ZHIP(hipMemcpyAsync(sp.first.data(), h->d_srch_first.p, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (srch.match.kind == Matcher::SET) {
        sp.which.resize(n);
        ZHIP(hipMemcpyAsync(sp.which.data(), h->d_set_which.p, n * 4, hipMemcpyDeviceToHost, h->stream));
        if (srch.hits) { sp.hits.resize(srch.match.set->count); ZHIP(hipMemcpyAsync(sp.hits.data(), h->d_set_hits.p, sp.hits.size() * 4, hipMemcpyDeviceToHost, h->stream)); }
    }
    if (srch.lines) { sp.lines.resize(n); ZHIP(hipMemcpyAsync(sp.lines.data(), h->d_ln_lines.p, n * 4, hipMemcpyDeviceToHost, h->stream)); }
    if (srch.lines && srch.ln.select) { sp.selected.resize(n); ZHIP(hipMemcpyAsync(sp.selected.data(), h->d_sel_count.p, n * 4, hipMemcpyDeviceToHost, h->stream)); }
    return ZARC_GPU_OK;
}
void search_scatter(const DecodedPart &p, const SearchReq &srch, const SearchPart &sp)
{
    auto none = [](uint32_t v) -> uint64_t { return v == 0xFFFFFFFFu ? ZARC_GPU_SEARCH_NONE : v; };
    for (size_t i = 0; i < p.n; i++) { srch.count[p.order[i]] = sp.count[i]; srch.first[p.order[i]] = none(sp.first[i]); }
    for (size_t i = 0; i < sp.which.size(); i++) srch.which[p.order[i]] = none(sp.which[i]);
    for (size_t k = 0; k < sp.hits.size(); k++) srch.hits[k] += sp.hits[k]; // (32-bit per part, 64-bit over the call)
}

// matches: the lines' delivery rule with line_cap, the line records of this part (they stay on the device), the matches of every one of them,
// the record rule over their sums, then records and text of the matches this part delivers.  Waits three times: for the sums, for the
// records (their text is sized by them) and for the text.
int matches_deliver(const DecodedPart &p, const SearchReq &srch, SearchPart &sp)
{
    zarc_gpu *const h = p.h;
    const Matcher &mt = srch.match;
    const size_t n = p.n;
    const LinesReq &ln = srch.ln;
    const MatchesReq &mq = ln.mt;
    LinesRun &run = *ln.run;
    int rc;
    std::vector<uint32_t> where(n); // the decoder's index of the caller's frame
    for (size_t i = 0; i < n; i++) where[p.order[i]] = (uint32_t)i;
    std::vector<uint64_t> base(n);
    std::vector<uint32_t> deliver(n);
    uint64_t nrec = 0;
    for (size_t c = 0; c < n; c++) {
        const uint32_t i = where[c];
        ln.lines[c] = sp.lines[i];
        mq.matches[c] = 0;
        uint64_t d = sp.lines[i];
        if (ln.max_lines && d > ln.max_lines) d = ln.max_lines;
        d = std::min<uint64_t>(d, ln.rec_cap - run.rec_used - nrec);
        base[i] = nrec; deliver[i] = (uint32_t)d;
        nrec += d;
    }
    if (!nrec) return ZARC_GPU_OK;
    if ((rc = upload_u64(h, h->d_ln_base, base.data(), n))) return rc;
    if ((rc = upload_u32(h, h->d_ln_deliver, deliver.data(), n))) return rc;
    ZHIP(h->d_ln_rec.reserve(nrec * sizeof(ZarcLineRec)));
    ZHIP(h->d_ln_total.reserve(8));
    ZHIP(h->d_mt_counts.reserve(nrec * 4));
    ZHIP(h->d_mt_prefix.reserve((nrec + 1) * 8));
    ZHIP(hipMemsetAsync(h->d_ln_rec.p, 0, nrec * sizeof(ZarcLineRec), h->stream)); // (a record nobody wrote is an empty line of frame 0: no match)
    ZHIP(hipMemsetAsync(h->d_mt_counts.p, 0, nrec * 4, h->stream));
    int e8, e9;
    ZHIP(p.t.mark(&e8));
    const dim3 per_slice((unsigned)sp.slices), per_line((unsigned)((nrec + 255) / 256));
    const uint64_t *const d_slices = h->d_srch_slices.as<uint64_t>(), *const d_raw = h->d_raw_len.as<uint64_t>(), *const d_rbase = h->d_ln_base.as<uint64_t>();
    const ZarcLineSlice *const d_ln = h->d_ln_slices.as<ZarcLineSlice>();
    const uint32_t *const d_deliver = h->d_ln_deliver.as<uint32_t>();
    ZarcLineRec *const d_lrec = h->d_ln_rec.as<ZarcLineRec>();
    uint32_t *const d_counts = h->d_mt_counts.as<uint32_t>();
    uint64_t *const d_prefix = h->d_mt_prefix.as<uint64_t>();
    switch (mt.kind) {
    case Matcher::PATTERN:
        hipLaunchKernelGGL(zarc_lines_emit, per_slice, dim3(256), 0, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, mt.pattern.d_bytes, mt.pattern.m, mt.icase,
                           d_ln, d_rbase, d_deliver, ln.max_line, d_lrec);
        hipLaunchKernelGGL(zarc_matches_count, per_line, dim3(256), 0, h->stream, nrec, d_lrec, p.d_base, p.d_off, mt.pattern.d_bytes, mt.pattern.m, mt.icase, d_counts);
        break;
    case Matcher::SET:
        hipLaunchKernelGGL(zarc_lines_emit_set, per_slice, dim3(256), sp.set_lds, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, *mt.set, h->d_set.as<uint32_t>(),
                           mt.icase, d_ln, d_rbase, d_deliver, ln.max_line, d_lrec);
        hipLaunchKernelGGL(zarc_matches_count_set, per_line, dim3(256), sp.set_lds, h->stream, nrec, d_lrec, p.d_base, p.d_off, *mt.set, h->d_set.as<uint32_t>(), mt.icase,
                           d_counts);
        break;
    case Matcher::REGEX: {
        hipLaunchKernelGGL(zarc_lines_emit_regex, per_slice, dim3(256), 0, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, mt.d_regex, h->d_re_entry.as<uint8_t>(),
                           d_ln, d_rbase, d_deliver, ln.max_line, d_lrec);
        // the lines' start bits: a bit per byte of every delivered line, rounded up to words per line
        uint64_t total_raw = 0;
        for (size_t i = 0; i < n; i++) total_raw += p.raw_len[i];
        ZHIP(h->d_mt_bitoff.reserve((nrec + 1) * 8));
        ZHIP(h->d_mt_bits.reserve(total_raw / 8 + nrec * 4 + 8));
        hipLaunchKernelGGL(zarc_matches_scan, dim3(1), dim3(256), 0, h->stream, 0u, nrec, d_lrec, (const uint32_t *)nullptr, (ZarcMatchRec *)nullptr, h->d_mt_bitoff.as<uint64_t>());
        hipLaunchKernelGGL(zarc_matches_count_regex, per_line, dim3(256), 0, h->stream, nrec, d_lrec, p.d_base, p.d_off, mt.d_regex, mq.d_fwd, h->d_mt_bitoff.as<uint64_t>(),
                           h->d_mt_bits.as<uint32_t>(), d_counts);
        break; }
    }
    hipLaunchKernelGGL(zarc_matches_scan, dim3(1), dim3(256), 0, h->stream, 1u, nrec, d_lrec, d_counts, (ZarcMatchRec *)nullptr, d_prefix);
    ZHIP(hipGetLastError());
    std::vector<uint64_t> prefix(nrec + 1);
    ZHIP(hipMemcpyAsync(prefix.data(), d_prefix, (nrec + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    ZHIP(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; i++) mq.matches[p.order[i]] = prefix[base[i] + deliver[i]] - prefix[base[i]];
    run.rec_used += nrec;
    const uint64_t nm = std::min<uint64_t>(prefix[nrec], mq.rec_cap - run.match_used); // records are in (frame, start) order: the part's first nm matches
    if (!nm) { ZHIP(p.t.mark(&e9)); sp.lines_ms2 = elapsed(h, e8, e9); return ZARC_GPU_OK; }
    ZHIP(h->d_mt_rec.reserve(nm * sizeof(ZarcMatchRec)));
    ZHIP(hipMemsetAsync(h->d_mt_rec.p, 0, nm * sizeof(ZarcMatchRec), h->stream));
    ZarcMatchRec *const d_mrec = h->d_mt_rec.as<ZarcMatchRec>();
    switch (mt.kind) {
    case Matcher::PATTERN:
        hipLaunchKernelGGL(zarc_matches_emit, per_line, dim3(256), 0, h->stream, nrec, d_lrec, p.d_base, p.d_off, mt.pattern.d_bytes, mt.pattern.m, mt.icase, d_prefix, nm,
                           ln.max_line, d_mrec);
        break;
    case Matcher::SET:
        hipLaunchKernelGGL(zarc_matches_emit_set, per_line, dim3(256), sp.set_lds, h->stream, nrec, d_lrec, p.d_base, p.d_off, *mt.set, h->d_set.as<uint32_t>(), mt.icase,
                           d_prefix, nm, ln.max_line, d_mrec);
        break;
    case Matcher::REGEX:
        hipLaunchKernelGGL(zarc_matches_emit_regex, per_line, dim3(256), 0, h->stream, nrec, d_lrec, p.d_base, p.d_off, mq.d_fwd, h->d_mt_bitoff.as<uint64_t>(),
                           h->d_mt_bits.as<uint32_t>(), d_prefix, nm, ln.max_line, d_mrec);
        break;
    }
    hipLaunchKernelGGL(zarc_matches_scan, dim3(1), dim3(256), 0, h->stream, 2u, nm, d_lrec, (const uint32_t *)nullptr, d_mrec, h->d_ln_total.as<uint64_t>());
    ZHIP(hipGetLastError());
    uint64_t text_bytes = 0;
    std::vector<ZarcMatchRec> recs(nm);
    ZHIP(hipMemcpyAsync(recs.data(), d_mrec, nm * sizeof(ZarcMatchRec), hipMemcpyDeviceToHost, h->stream));
    ZHIP(hipMemcpyAsync(&text_bytes, h->d_ln_total.p, 8, hipMemcpyDeviceToHost, h->stream));
    ZHIP(hipStreamSynchronize(h->stream));
    uint8_t *d_text = ln.d_text ? ln.d_text + run.text_used : nullptr;
    if (!d_text) { ZHIP(h->d_ln_text.reserve(text_bytes + 16)); d_text = h->d_ln_text.as<uint8_t>(); } // (host form: sized by what came of the scan)
    hipLaunchKernelGGL(zarc_matches_gather, dim3((unsigned)((nm + 3) / 4)), dim3(256), 0, h->stream, nm, d_mrec, p.d_base, p.d_off, d_text);
    ZHIP(hipGetLastError());
    ZHIP(p.t.mark(&e9));
    if (ln.h_text && text_bytes && (rc = lines_text_out(h, ln.h_text + run.text_used, d_text, text_bytes))) return rc;
    ZHIP(hipStreamSynchronize(h->stream));
    for (uint64_t k = 0; k < nm; k++) {
        zarc_gpu_match &r = mq.rec[run.match_used + k];
        memcpy(&r, &recs[k], sizeof r);
        r.frame = ln.frame0 + p.order[recs[k].frame];
        r.text_off += run.text_used;
    }
    run.match_used += nm; run.text_used += text_bytes;
    sp.lines_ms2 = elapsed(h, e8, e9);
    return ZARC_GPU_OK;
}

// lines, second half: the delivery rule in the caller's order, then records and text of what this part delivers.  Waits twice: for the
// records (their text is sized by them) and for the text.
int lines_deliver(const DecodedPart &p, const SearchReq &srch, SearchPart &sp)
{
    zarc_gpu *const h = p.h;
    const Matcher &mt = srch.match;
    const size_t n = p.n;
    const LinesReq &ln = srch.ln;
    if (ln.mt.on) return matches_deliver(p, srch, sp);
    LinesRun &run = *ln.run;
    int rc;
    std::vector<uint32_t> where(n); // the decoder's index of the caller's frame
    for (size_t i = 0; i < n; i++) where[p.order[i]] = (uint32_t)i;
    std::vector<uint64_t> base(n);
    std::vector<uint32_t> deliver(n);
    uint64_t nrec = 0;
    for (size_t c = 0; c < n; c++) {
        const uint32_t i = where[c];
        ln.lines[c] = sp.lines[i];
        if (ln.selected) ln.selected[c] = ln.select ? sp.selected[i] : sp.lines[i];
        uint64_t d = ln.select ? sp.selected[i] : sp.lines[i];
        if (ln.max_lines && d > ln.max_lines) d = ln.max_lines;
        d = std::min<uint64_t>(d, ln.rec_cap - run.rec_used - nrec);
        base[i] = nrec; deliver[i] = (uint32_t)d;
        nrec += d;
    }
    if (!nrec) return ZARC_GPU_OK;
    if ((rc = upload_u64(h, h->d_ln_base, base.data(), n))) return rc;
    if ((rc = upload_u32(h, h->d_ln_deliver, deliver.data(), n))) return rc;
    ZHIP(h->d_ln_rec.reserve(nrec * sizeof(ZarcLineRec)));
    ZHIP(h->d_ln_total.reserve(8));
    ZHIP(hipMemsetAsync(h->d_ln_rec.p, 0, nrec * sizeof(ZarcLineRec), h->stream)); // (a record nobody wrote would name no frame and no text)
    int e8, e9;
    ZHIP(p.t.mark(&e8));
    const dim3 per_slice((unsigned)sp.slices);
    const uint64_t *const d_slices = h->d_srch_slices.as<uint64_t>(), *const d_raw = h->d_raw_len.as<uint64_t>(), *const d_rbase = h->d_ln_base.as<uint64_t>();
    const ZarcLineSlice *const d_ln = h->d_ln_slices.as<ZarcLineSlice>();
    const uint32_t *const d_deliver = h->d_ln_deliver.as<uint32_t>();
    ZarcLineRec *const d_rec = h->d_ln_rec.as<ZarcLineRec>();
    if (ln.select) {
        const ZarcSelSlice *const d_sel = h->d_sel_slices.as<ZarcSelSlice>();
        switch (mt.kind) {
        case Matcher::PATTERN:
            hipLaunchKernelGGL(zarc_lines_select_emit, per_slice, dim3(256), 0, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, mt.pattern.d_bytes,
                               mt.pattern.m, mt.icase, ln.sel, d_sel, d_rbase, d_deliver, ln.max_line, d_rec);
            break;
        case Matcher::SET:
            hipLaunchKernelGGL(zarc_lines_select_emit_set, per_slice, dim3(256), sp.set_lds, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, *mt.set,
                               h->d_set.as<uint32_t>(), mt.icase, ln.sel, d_sel, d_rbase, d_deliver, ln.max_line, d_rec);
            break;
        case Matcher::REGEX:
            hipLaunchKernelGGL(zarc_lines_select_emit_regex, per_slice, dim3(256), 0, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, mt.d_regex,
                               h->d_re_entry.as<uint8_t>(), ln.sel, d_sel, d_rbase, d_deliver, ln.max_line, d_rec);
            break;
        }
    } else
    switch (mt.kind) {
    case Matcher::PATTERN:
        hipLaunchKernelGGL(zarc_lines_emit, per_slice, dim3(256), 0, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, mt.pattern.d_bytes, mt.pattern.m, mt.icase,
                           d_ln, d_rbase, d_deliver, ln.max_line, d_rec);
        break;
    case Matcher::SET:
        hipLaunchKernelGGL(zarc_lines_emit_set, per_slice, dim3(256), sp.set_lds, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, *mt.set, h->d_set.as<uint32_t>(),
                           mt.icase, d_ln, d_rbase, d_deliver, ln.max_line, d_rec);
        break;
    case Matcher::REGEX:
        hipLaunchKernelGGL(zarc_lines_emit_regex, per_slice, dim3(256), 0, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, mt.d_regex, h->d_re_entry.as<uint8_t>(),
                           d_ln, d_rbase, d_deliver, ln.max_line, d_rec);
        break;
    }
    hipLaunchKernelGGL(zarc_lines_scan, dim3(1), dim3(256), 0, h->stream, nrec, d_rec, h->d_ln_total.as<uint64_t>());
    ZHIP(hipGetLastError());
    uint64_t text_bytes = 0;
    std::vector<ZarcLineRec> recs(nrec);
    ZHIP(hipMemcpyAsync(recs.data(), h->d_ln_rec.p, nrec * sizeof(ZarcLineRec), hipMemcpyDeviceToHost, h->stream));
    ZHIP(hipMemcpyAsync(&text_bytes, h->d_ln_total.p, 8, hipMemcpyDeviceToHost, h->stream));
    ZHIP(hipStreamSynchronize(h->stream));
    uint8_t *d_text = ln.d_text ? ln.d_text + run.text_used : nullptr;
    if (!d_text) { ZHIP(h->d_ln_text.reserve(text_bytes + 16)); d_text = h->d_ln_text.as<uint8_t>(); } // (host form: sized by what came of the scan)
    hipLaunchKernelGGL(zarc_lines_gather, dim3((unsigned)((nrec + 3) / 4)), dim3(256), 0, h->stream, nrec, d_rec, p.d_base, p.d_off, d_text);
    ZHIP(hipGetLastError());
    ZHIP(p.t.mark(&e9));
    if (ln.h_text && text_bytes && (rc = lines_text_out(h, ln.h_text + run.text_used, d_text, text_bytes))) return rc;
    ZHIP(hipStreamSynchronize(h->stream));
    for (uint64_t k = 0; k < nrec; k++) {
        zarc_gpu_line &r = ln.rec[run.rec_used + k];
        memcpy(&r, &recs[k], sizeof r);
        r.frame = ln.frame0 + p.order[recs[k].frame];
        r.text_off += run.text_used;
    }
    run.rec_used += nrec; run.text_used += text_bytes;
    sp.lines_ms2 = elapsed(h, e8, e9);
    return ZARC_GPU_OK;
}

// what a part's ranges carry from one of their stages to the next
struct RangePart {
    int r0 = -1, r1 = -1;               // timer marks: in front of the count, behind the locate
    float ms2 = 0;                      // the gather
    std::vector<ZarcRangeFrame> frames; // what range_launch asked back (decoder order)
};

// ranges, first half: the frames are judged; count the line feeds of the frames that are asked for lines, work out T, a and b of every frame
// and the byte offsets of both boundaries.  The descriptors are asked back here and are on the host behind the part's one wait.
int range_launch(const DecodedPart &p, const RangeReq &rng, RangePart &rp)
{
    zarc_gpu *const h = p.h;
    const size_t n = p.n;
    int rc;
    uint64_t slices = 0;
    if ((rc = upload_slices(p, h->d_rg_slices, "read_ranges: batch too large", &slices))) return rc;
    std::vector<ZarcRangeReq> req(n);
    bool any_lines = false;
    for (size_t i = 0; i < n; i++) {
        const zarc_gpu_range &r = rng.range[p.order[i]];
        req[i] = ZarcRangeReq{r.unit, r.flags, r.skip, r.take};
        any_lines = any_lines || r.unit == ZARC_GPU_RANGE_LINES;
    }
    if ((rc = upload_bytes(h, h->d_rg_req, req.data(), n * sizeof(ZarcRangeReq)))) return rc;
    ZHIP(h->d_rg_cnt.reserve(slices * 4));
    ZHIP(h->d_rg_frames.reserve(n * sizeof(ZarcRangeFrame)));
    ZHIP(h->d_rg_open.reserve(n * 8));
    ZHIP(h->d_rg_nopen.reserve(8));
    ZHIP(hipMemsetAsync(h->d_rg_nopen.p, 0, 8, h->stream));
    const uint64_t *const d_slices = h->d_rg_slices.as<uint64_t>(), *const d_raw = h->d_raw_len.as<uint64_t>();
    const ZarcRangeReq *const d_req = h->d_rg_req.as<ZarcRangeReq>();
    ZarcRangeFrame *const d_frames = h->d_rg_frames.as<ZarcRangeFrame>();
    ZHIP(p.t.mark(&rp.r0));
    if (any_lines)
        hipLaunchKernelGGL(zarc_range_count, dim3((unsigned)slices), dim3(256), 0, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, d_req,
                           h->d_rg_cnt.as<uint32_t>());
    hipLaunchKernelGGL(zarc_range_carry, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, p.d_status, d_req,
                       h->d_rg_cnt.as<uint32_t>(), d_frames, h->d_rg_open.as<uint32_t>(), h->d_rg_nopen.as<uint32_t>());
    if (any_lines) // a fixed grid walks the list of open boundaries: its length is known on the device only
        hipLaunchKernelGGL(zarc_range_locate, dim3((unsigned)std::min<size_t>(2 * n, (size_t)h->num_cus * 8)), dim3(256), 0, h->stream, h->d_rg_open.as<uint32_t>(),
                           h->d_rg_nopen.as<uint32_t>(), d_slices, p.d_base, p.d_off, d_raw, d_frames);
    ZHIP(hipGetLastError());
    ZHIP(p.t.mark(&rp.r1));
    rp.frames.resize(n);
    ZHIP(hipMemcpyAsync(rp.frames.data(), h->d_rg_frames.p, n * sizeof(ZarcRangeFrame), hipMemcpyDeviceToHost, h->stream));
    return ZARC_GPU_OK;
}

// ranges, second half: res[] and the delivery rule in the caller's order, then the bytes this part delivers.  Waits once, for the text.
int range_deliver(const DecodedPart &p, const RangeReq &rng, RangePart &rp)
{
    zarc_gpu *const h = p.h;
    const size_t n = p.n;
    RangeRun &run = *rng.run;
    int rc;
    std::vector<uint32_t> where(n); // the decoder's index of the caller's frame
    for (size_t i = 0; i < n; i++) where[p.order[i]] = (uint32_t)i;
    std::vector<ZarcRangeCopy> plan;
    std::vector<uint64_t> blocks(1, 0);
    uint64_t bytes = 0; // of this part
    for (size_t c = 0; c < n; c++) {
        const ZarcRangeFrame &F = rp.frames[where[c]];
        zarc_gpu_range_result &r = rng.res[c];
        memset(&r, 0, sizeof r);
        if (!F.decoded) continue;
        r.units = F.units; r.first = F.first; r.taken = F.taken; r.start = F.pos[0]; r.length = F.pos[1] - F.pos[0];
        uint64_t e = r.length;
        if (rng.max_bytes && e > rng.max_bytes) e = rng.max_bytes;
        e = std::min<uint64_t>(e, rng.text_cap - run.text_used - bytes);
        r.text_off = run.text_used + bytes; r.text_len = e;
        if (!e) continue;
        plan.push_back(ZarcRangeCopy{bytes, where[c], F.pos[0], (uint32_t)e, 0u});
        blocks.push_back(blocks.back() + (e + ZARC_CHECK_SLICE - 1) / ZARC_CHECK_SLICE);
        bytes += e;
    }
    if (!bytes) return ZARC_GPU_OK;
    if (blocks.back() > 0x7FFFFFFFull) { set_error(h, "read_ranges: batch too large"); return ZARC_GPU_E_PARAM; }
    if ((rc = upload_bytes(h, h->d_rg_plan, plan.data(), plan.size() * sizeof(ZarcRangeCopy)))) return rc;
    if ((rc = upload_u64(h, h->d_rg_blocks, blocks.data(), blocks.size()))) return rc;
    uint8_t *d_text = rng.d_text ? rng.d_text + run.text_used : nullptr;
    if (!d_text) { ZHIP(h->d_rg_text.reserve(bytes + 16)); d_text = h->d_rg_text.as<uint8_t>(); } // (host form: sized by what the part delivers)
    int r2, r3;
    ZHIP(p.t.mark(&r2));
    hipLaunchKernelGGL(zarc_range_gather, dim3((unsigned)blocks.back()), dim3(256), 0, h->stream, (uint32_t)plan.size(), h->d_rg_blocks.as<uint64_t>(),
                       h->d_rg_plan.as<ZarcRangeCopy>(), p.d_base, p.d_off, d_text);
    ZHIP(hipGetLastError());
    ZHIP(p.t.mark(&r3));
    if (rng.h_text && (rc = lines_text_out(h, rng.h_text + run.text_used, d_text, bytes))) return rc;
    ZHIP(hipStreamSynchronize(h->stream));
    run.text_used += bytes;
    rp.ms2 = elapsed(h, r2, r3);
    return ZARC_GPU_OK;
}

// what a part's counts carry from their launch to their delivery
struct WcPart {
    int w0 = -1, w1 = -1;           // timer marks: in front of the count, behind the carry
    std::vector<ZarcWcFrame> out;   // what wc_launch asked back (decoder order)
};

// counts, first half: the frames are judged; one record per slice, then one zarc_gpu_wc per frame.  The answers are asked back here and are
// on the host behind the part's one wait.
int wc_launch(const DecodedPart &p, WcPart &wp)
{
    zarc_gpu *const h = p.h;
    const size_t n = p.n;
    int rc;
    uint64_t slices = 0;
    if ((rc = upload_slices(p, h->d_wc_slices, "count: batch too large", &slices))) return rc;
    ZHIP(h->d_wc_rec.reserve(slices * sizeof(ZarcWcSlice)));
    ZHIP(h->d_wc_out.reserve(n * sizeof(ZarcWcFrame)));
    const uint64_t *const d_slices = h->d_wc_slices.as<uint64_t>(), *const d_raw = h->d_raw_len.as<uint64_t>();
    ZHIP(p.t.mark(&wp.w0));
    hipLaunchKernelGGL(zarc_wc_count, dim3((unsigned)slices), dim3(256), 0, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, p.d_status,
                       h->d_wc_rec.as<ZarcWcSlice>());
    hipLaunchKernelGGL(zarc_wc_carry, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (uint32_t)n, d_slices, d_raw, p.d_status,
                       h->d_wc_rec.as<ZarcWcSlice>(), h->d_wc_out.as<ZarcWcFrame>());
    ZHIP(hipGetLastError());
    ZHIP(p.t.mark(&wp.w1));
    wp.out.resize(n);
    ZHIP(hipMemcpyAsync(wp.out.data(), h->d_wc_out.p, n * sizeof(ZarcWcFrame), hipMemcpyDeviceToHost, h->stream));
    return ZARC_GPU_OK;
}

// counts, second half: to the caller's order
void wc_deliver(const DecodedPart &p, const WcReq &wc, const WcPart &wp)
{
    for (size_t i = 0; i < p.n; i++) memcpy(&wc.res[p.order[i]], &wp.out[i], sizeof(zarc_gpu_wc));
}

// what a part's comparison carries from its launch to its delivery
struct CmpPart {
    int c0 = -1, c1 = -1;           // timer marks: in front of the scan, behind the carry
    std::vector<ZarcCmpFrame> out;  // what cmp_launch asked back (decoder order)
};

// comparison, first half: the frames are judged; one record per slice, then one zarc_gpu_cmp per frame.  The answers are asked back here and
// are on the host behind the part's one wait.
int cmp_launch(const DecodedPart &p, const CmpReq &cmp, CmpPart &cp)
{
    zarc_gpu *const h = p.h;
    const size_t n = p.n;
    int rc;
    uint64_t slices = 0;
    if ((rc = upload_slices(p, h->d_cmp_slices, "compare: batch too large", &slices))) return rc;
    std::vector<uint64_t> off(n), len(n);
    for (size_t i = 0; i < n; i++) { off[i] = cmp.other_off[p.order[i]]; len[i] = cmp.other_len[p.order[i]]; }
    if ((rc = upload_u64(h, h->d_cmp_off, off.data(), n))) return rc;
    if ((rc = upload_u64(h, h->d_cmp_len, len.data(), n))) return rc;
    ZHIP(h->d_cmp_rec.reserve(slices * sizeof(ZarcCmpSlice)));
    ZHIP(h->d_cmp_out.reserve(n * sizeof(ZarcCmpFrame)));
    const uint64_t *const d_slices = h->d_cmp_slices.as<uint64_t>(), *const d_raw = h->d_raw_len.as<uint64_t>();
    const uint64_t *const d_ooff = h->d_cmp_off.as<uint64_t>(), *const d_olen = h->d_cmp_len.as<uint64_t>();
    ZHIP(p.t.mark(&cp.c0));
    hipLaunchKernelGGL(zarc_cmp_scan, dim3((unsigned)slices), dim3(256), 0, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw, p.d_status,
                       cmp.d_other, d_ooff, d_olen, h->d_cmp_rec.as<ZarcCmpSlice>());
    hipLaunchKernelGGL(zarc_cmp_carry, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (uint32_t)n, d_slices, p.d_base, p.d_off, d_raw,
                       p.d_status, cmp.d_other, d_ooff, d_olen, h->d_cmp_rec.as<ZarcCmpSlice>(), h->d_cmp_out.as<ZarcCmpFrame>());
    ZHIP(hipGetLastError());
    ZHIP(p.t.mark(&cp.c1));
    cp.out.resize(n);
    ZHIP(hipMemcpyAsync(cp.out.data(), h->d_cmp_out.p, n * sizeof(ZarcCmpFrame), hipMemcpyDeviceToHost, h->stream));
    return ZARC_GPU_OK;
}

// comparison, second half: to the caller's order
void cmp_deliver(const DecodedPart &p, const CmpReq &cmp, const CmpPart &cp)
{
    for (size_t i = 0; i < p.n; i++) memcpy(&cmp.res[p.order[i]], &cp.out[i], sizeof(zarc_gpu_cmp));
}

// own_out: bytes of engine-owned output scratch this call decodes into (verify, read-back check); they count against the budget
int unpack_device_once(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off_in, const uint64_t *frame_len_in,
                       void *d_dst_base, const uint64_t *dst_off_in, const uint64_t *raw_len_in, const uint8_t *expect_in, uint8_t *digest,
                       int *status, uint64_t own_out = 0, const PackCheck *chk = nullptr, DevBuf *order_out = nullptr, const SearchReq *srch = nullptr,
                       const RangeReq *rng = nullptr, const WcReq *wc = nullptr, const CmpReq *cmp = nullptr)
{
    int rc = 0;
    h->dec_scratch = 0;
    DevBuf &b_dst_off = chk ? h->d_chk_off : h->d_dst_off;
    uint64_t total_raw = 0;
    for (size_t i = 0; i < n; i++) {
        if (dst_off_in && dst_off_in[i] % ZARC_GPU_ALIGN) { set_error(h, "output offset not 16-byte aligned"); return ZARC_GPU_E_PARAM; }
        if (frame_len_in[i] >= 0xFFFFFFF0ull || raw_len_in[i] >= 0xFFFFFFF0ull) { set_error(h, "frames of 4 GiB or more are not supported"); return ZARC_GPU_E_UNSUPPORTED; }
        total_raw += raw_len_in[i];
    }
    const std::vector<uint32_t> order = diag_env("ZARC_GPU_DEC_DENSITY", 1) ? order_for_decode(raw_len_in, frame_len_in, n) : order_by_size_desc(raw_len_in, n);
    std::vector<uint64_t> frame_off(n), frame_len(n), dst_off(n), raw_len(n);
    if (dst_off_in)
        for (size_t i = 0; i < n; i++) { const uint32_t f = order[i]; frame_off[i] = frame_off_in[f]; frame_len[i] = frame_len_in[f]; dst_off[i] = dst_off_in[f]; raw_len[i] = raw_len_in[f]; }
    else { // engine-owned output (verify, read-back check): laid out right here, in the decoder's own order, 16-byte aligned -- own_out bytes in all
        uint64_t at = 0;
        for (size_t i = 0; i < n; i++) { const uint32_t f = order[i]; frame_off[i] = frame_off_in[f]; frame_len[i] = frame_len_in[f]; dst_off[i] = at; raw_len[i] = raw_len_in[f]; at += align_up((size_t)raw_len[i], ZARC_GPU_ALIGN); }
    }
    if ((rc = upload_u64(h, h->d_frame_off, frame_off.data(), n))) return rc;
    if ((rc = upload_u64(h, h->d_frame_len, frame_len.data(), n))) return rc;
    if ((rc = upload_u64(h, b_dst_off, dst_off.data(), n))) return rc;
    if ((rc = upload_u64(h, h->d_raw_len, raw_len.data(), n))) return rc;
    { std::vector<uint32_t> ident(n); std::iota(ident.begin(), ident.end(), 0u); if ((rc = upload_u32(h, h->d_order, ident.data(), n))) return rc; } // the queues walk the (sorted) indices
    if (order_out && (rc = upload_u32(h, *order_out, order.data(), n))) return rc; // repack: zarc_repack_plan takes the results back to the caller's order
    const size_t dec_grid = std::min<size_t>(n, (size_t)h->num_cus * 16); // 4 waves per SIMD (launch bounds of the frame kernels: 128 VGPRs, no spills)
    ZHIP(h->d_declit.reserve(dec_grid * (size_t)(ZARC_BLOCK_MAX + 64)));
    ZHIP(h->d_queue.reserve(256));
    ZHIP(h->d_status.reserve(n * 4));
    ZHIP(h->d_stored_ck.reserve(n * 8));
    std::vector<uint8_t> expect;
    if (expect_in) { // reordered straight into the page-locked descriptor arena when it has room (32 bytes per frame: the largest array of the call)
        uint8_t *ex = (uint8_t *)meta_take(h, n * 32);
        if (!ex) { expect.resize(n * 32); ex = expect.data(); }
        for (size_t i = 0; i < n; i++) memcpy(ex + i * 32, expect_in + (size_t)order[i] * 32, 32);
        ZHIP(h->d_expect.reserve(n * 32));
        ZHIP(hipMemcpyAsync(h->d_expect.p, ex, n * 32, hipMemcpyHostToDevice, h->stream));
    }
    Timer t{h, chk ? 8 : 0};
    int e0, e1, e3;
    ZHIP(t.mark(&e0));
    // ---- fast path: block scan (lane per frame), then sequence entropy decoding with one lane per block ----
    bool fastpath = diag_env("ZARC_GPU_DEC_FAST", 1) != 0;
    // slots of the fast path: one per block, counted on the device first (a frame the count turns down keeps one slot and goes to the
    // general decoder)
    // Lean sizing (round 4): a batch without large frames needs nothing on the host but three totals -- no frame is cut into pieces, there
    // is one group -- so the slot / sequence / literal offsets are prefix sums made on the device (zarc_scan_u32) and stay there.  With
    // large frames (4 MiB and more) the host needs the per-block summaries anyway and takes the arrays as before.
    size_t n_large = 0; // frames of 4 MiB and more (sorted order: a prefix): the ones the host may cut into pieces
    while (n_large < n && raw_len[n_large] >= ((uint64_t)4 << 20)) n_large++;
    bool lean = fastpath && (n_large == 0 || n_large * 64 <= n) && diag_env("ZARC_GPU_DEC_LEAN", 1) != 0;
    uint64_t lean_totals[3] = {0, 0, 0};
    std::vector<uint64_t> slot_prefix(n + 1, 0); // lean: only the entries the host needs are filled in (the large frames', the groups' bounds, [n])
    if (fastpath) {
        ZHIP(h->d_fast.reserve(n * 4));
        hipLaunchKernelGGL(zarc_zdec_count, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, (const uint8_t *)d_frames_base, h->d_frame_off.as<uint64_t>(),
                           h->d_frame_len.as<uint64_t>(), h->d_raw_len.as<uint64_t>(), (uint32_t)n, h->d_fast.as<uint32_t>());
        ZHIP(hipGetLastError());
        if (lean) {
            ZHIP(h->d_slot_prefix.reserve((n + 1) * 8));
            ZHIP(h->d_totals.reserve(64));
            hipLaunchKernelGGL(zarc_scan_u32, dim3(1), dim3(1024), 0, h->stream, h->d_fast.as<uint32_t>(), 1u, 1u, (uint64_t)n, h->d_slot_prefix.as<uint64_t>(),
                               h->d_totals.as<uint64_t>());
            ZHIP(hipGetLastError());
            ZHIP(hipMemcpyAsync(lean_totals, h->d_totals.p, 8, hipMemcpyDeviceToHost, h->stream));
            if (n_large) ZHIP(hipMemcpyAsync(slot_prefix.data(), h->d_slot_prefix.p, (n_large + 1) * 8, hipMemcpyDeviceToHost, h->stream));
            ZHIP(hipStreamSynchronize(h->stream));
            slot_prefix[n] = lean_totals[0];
        } else {
            std::vector<uint32_t> nblk(n);
            ZHIP(hipMemcpyAsync(nblk.data(), h->d_fast.p, n * 4, hipMemcpyDeviceToHost, h->stream));
            ZHIP(hipStreamSynchronize(h->stream));
            for (size_t i = 0; i < n; i++) slot_prefix[i + 1] = slot_prefix[i] + std::max<uint32_t>(nblk[i], 1u);
        }
    } else
        for (size_t i = 0; i < n; i++) slot_prefix[i + 1] = slot_prefix[i] + 1;
    const size_t nslots = (size_t)slot_prefix[n];
    if (nslots * (size_t)ZDEC_TABLE_CELLS * 2 > ((size_t)8 << 30)) { fastpath = false; if (lean) { lean = false; for (size_t i = 0; i < n; i++) slot_prefix[i + 1] = i + 1; } } // table scratch out of proportion (millions of tiny frames)
    // groups: [gf[g], gf[g+1]) in sorted order, equal shares of the bytes.  One group (the stages simply follow each other) unless the
    // batch holds frames large enough for their chains to matter.
    int groups = h->dec_groups;
    // Measured (tools/ab_groups.sh): overlapped stages slow each other down (they all live on memory latency), so equal-sized frames are
    // best served by one group (configs[1]: 64 / 82 / 117 ms with 1 / 2 / 4 groups); a batch whose largest frames are several times the
    // mean gains from two (configs[4] shape: 227 / 203 / 285 ms) -- the large half's frame pass and XXH64 chains run beside the small
    // half's sequence stage instead of after it.
    if (groups <= 0) groups = (fastpath && n >= 16 && raw_len[0] >= ((uint64_t)4 << 20) && raw_len[0] * (uint64_t)n >= 4 * total_raw) ? 2 : 1;
    if (!fastpath) groups = 1;
    if (groups > zarc_gpu::DEC_GROUPS) groups = zarc_gpu::DEC_GROUPS;
    if ((size_t)groups > n) groups = (int)n;
    std::vector<size_t> gf(groups + 1, n);
    gf[0] = 0;
    { uint64_t acc = 0; int g = 1;
      for (size_t i = 0; i < n && g < groups; i++) {
          acc += raw_len[i];
          if (acc * (uint64_t)groups >= total_raw * (uint64_t)g && i + 1 + (size_t)(groups - g) <= n) gf[g++] = i + 1; // every group keeps a frame
      }
      for (; g < groups; g++) gf[g] = std::max(gf[g - 1] + 1, n - (size_t)(groups - g)); }
    if (lean && fastpath && groups > 1) { // the slot at which every group starts (lean: the prefix sums live on the device)
        for (int g = 1; g < groups; g++) ZHIP(hipMemcpyAsync(&slot_prefix[gf[g]], h->d_slot_prefix.as<uint64_t>() + gf[g], 8, hipMemcpyDeviceToHost, h->stream));
        ZHIP(hipStreamSynchronize(h->stream));
    }
    // digest descriptors: per group, chunk prefixes rebased to the group's first chunk (the kernels take sub-ranges by pointer)
    std::vector<uint64_t> cprefix(n + (size_t)groups), gchunk0(groups + 1, 0);
    { uint64_t c = 0;
      for (int g = 0; g < groups; g++) {
          gchunk0[g] = c;
          uint64_t r = 0;
          for (size_t i = gf[g]; i < gf[g + 1]; i++) { cprefix[i + (size_t)g] = r; r += chunks_of(raw_len[i]); }
          cprefix[gf[g + 1] + (size_t)g] = r;
          c += r;
      }
      gchunk0[groups] = c; }
    if (!chk) {
        if ((rc = upload_u64(h, h->d_chunk_prefix, cprefix.data(), cprefix.size()))) return rc;
        ZHIP(h->d_cvs.reserve(gchunk0[groups] * 32));
        ZHIP(h->d_cvs_tmp.reserve(gchunk0[groups] * 32));
        ZHIP(h->d_digests.reserve(n * 32));
        ZHIP(h->d_xxh.reserve(n * 8));
    }
    std::vector<uint64_t> seqidx, litidx;
    uint64_t total_seqs = 0, total_lits = 0;
    uint64_t g_seq_at[zarc_gpu::DEC_GROUPS + 1] = {}, g_lit_at[zarc_gpu::DEC_GROUPS + 1] = {}; // lean: the groups' first sequence / literal
    if (fastpath) {
        if (!lean && (rc = upload_u64(h, h->d_slot_prefix, slot_prefix.data(), n + 1))) return rc;
        ZHIP(h->d_zblocks.reserve(nslots * sizeof(ZdecBlock)));
        ZHIP(h->d_nseq.reserve(nslots * 8));
        ZHIP(h->d_fast.reserve(n * 4));
        ZHIP(h->d_seqidx.reserve((nslots + 1) * 8));
        ZHIP(h->d_litidx.reserve((nslots + 1) * 8));
        ZHIP(h->d_ztables.reserve(nslots * (size_t)ZDEC_TABLE_CELLS * 2));
        if (!h->d_predef.p) { // the predefined tables: once per handle
            ZHIP(h->d_predef.reserve(ZDEC_PREDEF_CELLS * 2));
            hipLaunchKernelGGL(zarc_zdec_predef, dim3(1), dim3(64), 0, h->stream, h->d_predef.as<uint16_t>());
            ZHIP(hipGetLastError());
        }
        ZHIP(h->d_seqflag.reserve((nslots / 16 + (size_t)zarc_gpu::DEC_GROUPS + 2) * 4));
        ZHIP(h->d_longlist.reserve((nslots + 64) * 4));                                   // zarc_zdec_seqs_lds: the blocks with long chains, per group
        ZHIP(h->d_longcnt.reserve((size_t)zarc_gpu::DEC_GROUPS * 64 * 4));                // ... and their counters (2 x ZDEC_LONG_BUCKETS + 1 words per group)
        ZHIP(hipMemsetAsync(h->d_zblocks.p, 0xFF, nslots * sizeof(ZdecBlock), h->stream));
        ZHIP(hipMemsetAsync(h->d_nseq.p, 0, nslots * 8, h->stream));
        hipLaunchKernelGGL(zarc_zdec_scan, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, (const uint8_t *)d_frames_base, h->d_frame_off.as<uint64_t>(),
                           h->d_frame_len.as<uint64_t>(), h->d_raw_len.as<uint64_t>(), (uint32_t)n, h->d_slot_prefix.as<uint64_t>(), h->d_zblocks.as<ZdecBlock>(),
                           h->d_nseq.as<uint32_t>(), h->d_fast.as<uint32_t>());
        ZHIP(hipGetLastError());
        if (lean) { // the sequence / literal scratch is sized exactly: sums of the blocks' counts, made where the counts are
            hipLaunchKernelGGL(zarc_scan_u32, dim3(1), dim3(1024), 0, h->stream, h->d_nseq.as<uint32_t>(), 2u, 0u, (uint64_t)nslots, h->d_seqidx.as<uint64_t>(),
                               h->d_totals.as<uint64_t>() + 1);
            hipLaunchKernelGGL(zarc_scan_u32, dim3(1), dim3(1024), 0, h->stream, h->d_nseq.as<uint32_t>() + 1, 2u, 0u, (uint64_t)nslots, h->d_litidx.as<uint64_t>(),
                               h->d_totals.as<uint64_t>() + 2);
            ZHIP(hipGetLastError());
            ZHIP(hipMemcpyAsync(lean_totals + 1, h->d_totals.as<uint64_t>() + 1, 16, hipMemcpyDeviceToHost, h->stream));
            for (int g = 1; g < groups; g++) { // where every group's sequences / literals start
                ZHIP(hipMemcpyAsync(&g_seq_at[g], h->d_seqidx.as<uint64_t>() + slot_prefix[gf[g]], 8, hipMemcpyDeviceToHost, h->stream));
                ZHIP(hipMemcpyAsync(&g_lit_at[g], h->d_litidx.as<uint64_t>() + slot_prefix[gf[g]], 8, hipMemcpyDeviceToHost, h->stream));
            }
            ZHIP(hipStreamSynchronize(h->stream));
            total_seqs = lean_totals[1]; total_lits = lean_totals[2];
            g_seq_at[groups] = total_seqs; g_lit_at[groups] = total_lits;
        } else {
            std::vector<uint32_t> counts(nslots * 2);
            ZHIP(hipMemcpyAsync(counts.data(), h->d_nseq.p, nslots * 8, hipMemcpyDeviceToHost, h->stream));
            ZHIP(hipStreamSynchronize(h->stream)); // the sequence / literal scratch is sized exactly: sums of the blocks' counts
            seqidx.resize(nslots + 1); litidx.resize(nslots + 1);
            uint64_t total = 0, lit_total = 0;
            for (size_t i = 0; i < nslots; i++) { seqidx[i] = total; total += counts[2 * i]; litidx[i] = lit_total; lit_total += counts[2 * i + 1]; }
            seqidx[nslots] = total; litidx[nslots] = lit_total;
            total_seqs = total; total_lits = lit_total;
        }
        h->dec_scratch = total_seqs * 8 + total_lits + nslots * (uint64_t)(ZDEC_TABLE_CELLS * 2 + sizeof(ZdecBlock) + 32);
        if (wc) h->dec_scratch += wc_scratch(n, total_raw); // the slices' records lie in the handle's scratch beside the decoder's
        if (cmp) { // ... and so do the other sides the host form staged for this part
            h->dec_scratch += cmp_scratch(n, total_raw);
            if (cmp->staged) for (size_t i = 0; i < n; i++) h->dec_scratch += align_up((size_t)cmp->other_len[i], ZARC_GPU_ALIGN);
        }
        if (h->scratch_budget && n > 1 && own_out + h->dec_scratch > h->scratch_budget) return UNPACK_SPLIT;
        if (!lean) {
            if ((rc = upload_u64(h, h->d_seqidx, seqidx.data(), nslots))) return rc;
            if ((rc = upload_u64(h, h->d_litidx, litidx.data(), nslots))) return rc;
        }
        ZHIP(h->d_seqs.reserve(std::max<uint64_t>(total_seqs, 1) * 8));
        ZHIP(h->d_lits.reserve(std::max<uint64_t>(total_lits, 1) + 64));
    }
    ZHIP(hipMemsetAsync(h->d_queue.p, 0, 256, h->stream)); // two queues per group: the fast frame pass and the general decoder each walk the group's frames
    ZHIP(hipMemsetAsync(h->d_status.p, 0, n * 4, h->stream)); // the pieces of a frame raise its status with atomicMax
    ZHIP(hipEventRecord(h->ev_fork, h->stream)); // descriptors are in place
    const int dec_dbg = diag_env("ZARC_GPU_DBG_DEC", 0);
    const bool side = diag_env("ZARC_GPU_DEC_SIDE", 1) != 0;
    int seq_lanes = diag_env("ZARC_GPU_SEQ_LANES", 64);
    if (seq_lanes != 8 && seq_lanes != 16 && seq_lanes != 32 && seq_lanes != 64) seq_lanes = 64;
    bool have_seq_t[zarc_gpu::DEC_GROUPS] = {}, have_lit_t[zarc_gpu::DEC_GROUPS] = {};
    std::vector<uint32_t> nblk_of(lean ? n_large : n); // blocks per frame (sorted order; lean: of the large frames only)
    for (size_t i = 0; i < nblk_of.size(); i++) nblk_of[i] = (uint32_t)(slot_prefix[i + 1] - slot_prefix[i]);
    std::vector<ZdecPiece> pieces[zarc_gpu::DEC_GROUPS];
    std::vector<ZdecBlock> hblocks;
    std::vector<uint32_t> hfast;
    ZHIP(h->d_pieces.reserve(lean ? (size_t)(slot_prefix[n_large] / 8 + n_large + 16) * sizeof(ZdecPiece) : (nslots / 8 + n + 16) * sizeof(ZdecPiece)));
    size_t piece_base = 0;
    // phase 0 queues the stages ahead of every group, phase 1 the frame passes and hashes: in between the host may have to look at what
    // stage 2 found out about a group's blocks (pieces, below), and the next group's stages ahead must be running by then
    for (int phase = 0; phase < 2; phase++)
    for (int g = 0; g < groups; g++) {
        // The stages ahead (sequences, literals) of all groups follow each other on the engine's two streams -- several sequence kernels side
        // by side were measured and only slow each other down (they live on MALL / fabric latency) -- while the frame pass and the hashes
        // of a group run on the group's own pair of streams beside the next group's stages ahead.
        hipStream_t pa = h->stream, pb = h->stream2;
        hipStream_t sa = groups == 1 ? h->stream : h->gs[2 * g], sb = groups == 1 ? h->stream2 : h->gs[2 * g + 1];
        hipEvent_t *ev = h->ev_g[g];
        const size_t f0 = gf[g], f1 = gf[g + 1], ng = f1 - f0;
        if (phase == 0 && g == 0) ZHIP(hipStreamWaitEvent(pb, h->ev_fork, 0));
        if (phase == 0 && fastpath) {
            hipStream_t sa_post = sa, sb_post = sb;
            sa = pa; sb = pb; // this block launches the stages ahead
            const uint64_t s0 = slot_prefix[f0], s1 = slot_prefix[f1];
            const uint64_t g_seqs = lean ? g_seq_at[g + 1] - g_seq_at[g] : seqidx[s1] - seqidx[s0], g_lits = lean ? g_lit_at[g + 1] - g_lit_at[g] : litidx[s1] - litidx[s0];
            // the literal and the sequence kernels are independent and neither fills the chip: they run side by side
            hipStream_t sl = side ? sb : sa;
            // the shared-table sequence kernel needs 23 KiB of LDS per wave: launched first it gets its place on every CU at once and the
            // literal waves (12.5 KiB each) fill what is left; behind them it would wait for LDS (diagnostic switch: ZARC_GPU_LIT_FIRST)
            const bool lit_first = diag_env("ZARC_GPU_LIT_FIRST", 0) != 0;
            auto launch_literals = [&]() -> int {
            if (g_lits) {
                ZHIP(hipEventRecord(ev[2], sl));
                hipLaunchKernelGGL(zarc_zdec_literals, dim3((unsigned)((s1 - s0 + ZDEC_LIT_GROUP - 1) / ZDEC_LIT_GROUP)), dim3(64), 0, sl, (const uint8_t *)d_frames_base,
                                   h->d_frame_off.as<uint64_t>(), s1, h->d_slot_prefix.as<uint64_t>(), h->d_zblocks.as<ZdecBlock>(), h->d_litidx.as<uint64_t>(),
                                   h->d_lits.as<uint8_t>(), h->d_fast.as<uint32_t>(), s0);
                ZHIP(hipGetLastError());
                ZHIP(hipEventRecord(ev[3], sl));
                have_lit_t[g] = true;
            }
            return ZARC_GPU_OK; };
            if (lit_first && (rc = launch_literals())) return rc;
            if (g_seqs) {
                ZHIP(hipEventRecord(ev[0], sa));
                {
                    // Waves whose 64 blocks share their tables (the engine's own frames: one table set per group of sixteen 64 KiB blocks; libzstd's
                    // Repeat_Mode blocks) decode with the tables in LDS; the others raise their flag and are done by the launches behind it: blocks
                    // with a long chain by zarc_zdec_seqs_lds (every lane's own tables in LDS, on a side stream, from a list ordered by sequence count),
                    // the rest by zarc_zdec_seqs with a table set per block in HBM scratch.
                    // (a batch of small frames -- fewer than four blocks per frame on average -- has nothing to share: a workgroup's 64 blocks
                    // would belong to a dozen frames with a dozen table sets, and every workgroup would hand its blocks on after looking)
                    const bool shared = diag_env("ZARC_GPU_SEQ_SHARED", 1) != 0 && (s1 - s0) >= 4 * (uint64_t)ng;
                    // block slots per workgroup of the shared-table kernel.  Round 4, 128 KiB blocks and a table per 8: 64 -> 27.3 ms, 32 -> 23.7, 16 -> 27.3
                    // (tools/r4_ab4.sh); with the straight-line step, 64 KiB blocks and a table per 16: 64 lanes with 8 sets 13.1 ms alone, 32 lanes with
                    // 5 sets 14.9, and side by side with the literals the smaller LDS share is what counts (tools/r4_sets.sh)
                    int sw = diag_env("ZARC_GPU_SEQ_WIDTH", 64);
                    if (sw != 16 && sw != 32 && sw != 64) sw = 64;
                    if (!shared) sw = seq_lanes;
                    const size_t waves = (size_t)((s1 - s0 + (uint64_t)sw - 1) / (uint64_t)sw);
                    const bool split_long = diag_env("ZARC_GPU_SEQ_LONG", 1) != 0 && (shared ? sw == 64 : sw % ZDEC_LDS_LANES == 0);
                    uint32_t *flags = nullptr;
                    if (shared) {
                        flags = h->d_seqflag.as<uint32_t>() + (size_t)(s0 / 16) + (size_t)g; // (a group's slots need not start at a multiple of the width)
                        ZHIP(hipMemsetAsync(flags, 0, waves * 4, sa));
                        auto kern = sw == 64 ? zarc_zdec_seqs_shared : (sw == 32 ? zarc_zdec_seqs_shared32 : zarc_zdec_seqs_shared16);
                        hipLaunchKernelGGL(kern, dim3((unsigned)waves), dim3(sw), 0, sa, (const uint8_t *)d_frames_base, h->d_frame_off.as<uint64_t>(),
                                           s1, h->d_slot_prefix.as<uint64_t>(), h->d_zblocks.as<ZdecBlock>(), h->d_seqidx.as<uint64_t>(), h->d_seqs.as<uint64_t>(),
                                           h->d_fast.as<uint32_t>(), s0, flags);
                    }
                    if (split_long) {
                        static_assert(2 * ZDEC_LONG_BUCKETS + 1 <= 64, "counter words per group");
                        uint32_t *cnt = h->d_longcnt.as<uint32_t>() + (size_t)g * 64, *list = h->d_longlist.as<uint32_t>() + (size_t)s0;
                        const unsigned w64 = (unsigned)((s1 - s0 + 63) / 64);
                        ZHIP(hipEventRecord(h->ev_fork3, sa));
                        ZHIP(hipStreamWaitEvent(h->stream3, h->ev_fork3, 0));
                        ZHIP(hipMemsetAsync(cnt, 0, 64 * 4, h->stream3));
                        hipLaunchKernelGGL(zarc_zdec_long_count, dim3(w64), dim3(64), 0, h->stream3, (const ZdecBlock *)h->d_zblocks.as<ZdecBlock>(), s0, s1,
                                           (const uint32_t *)flags, cnt);
                        hipLaunchKernelGGL(zarc_zdec_long_fill, dim3(w64), dim3(64), 0, h->stream3, (const ZdecBlock *)h->d_zblocks.as<ZdecBlock>(), s0, s1,
                                           (const uint32_t *)flags, cnt, list);
                        hipLaunchKernelGGL(zarc_zdec_seqs_lds, dim3((unsigned)((s1 - s0 + ZDEC_LDS_LANES - 1) / ZDEC_LDS_LANES)), dim3(ZDEC_LDS_LANES), 0, h->stream3,
                                           (const uint8_t *)d_frames_base, h->d_frame_off.as<uint64_t>(), s1, h->d_slot_prefix.as<uint64_t>(),
                                           h->d_zblocks.as<ZdecBlock>(), h->d_seqidx.as<uint64_t>(), h->d_seqs.as<uint64_t>(), h->d_fast.as<uint32_t>(), s0,
                                           (const uint32_t *)cnt, (const uint32_t *)list);
                        ZHIP(hipGetLastError());
                        ZHIP(hipEventRecord(h->ev_join3, h->stream3));
                    }
                    hipLaunchKernelGGL(zarc_zdec_seqs, dim3((unsigned)waves), dim3(sw), 0, sa, (const uint8_t *)d_frames_base,
                                       h->d_frame_off.as<uint64_t>(), s1, h->d_slot_prefix.as<uint64_t>(), h->d_zblocks.as<ZdecBlock>(), h->d_seqidx.as<uint64_t>(),
                                       h->d_seqs.as<uint64_t>(), h->d_ztables.as<uint16_t>(), h->d_fast.as<uint32_t>(), s0, (const uint32_t *)flags,
                                       h->d_predef.as<uint16_t>(), split_long ? 1 : 0);
                    if (split_long) ZHIP(hipStreamWaitEvent(sa, h->ev_join3, 0));
                }
                ZHIP(hipGetLastError());
                ZHIP(hipEventRecord(ev[1], sa));
                have_seq_t[g] = true;
            }
            if (!lit_first && (rc = launch_literals())) return rc;
            sa = sa_post; sb = sb_post;
            if (groups > 1) { ZHIP(hipEventRecord(ev[1], pa)); ZHIP(hipStreamWaitEvent(sa, ev[1], 0)); } // (re-recorded when the group has no sequences: it still orders the group behind the descriptors)
            if (g_lits && side) { ZHIP(hipEventRecord(ev[10], pb)); ZHIP(hipStreamWaitEvent(sa, ev[10], 0)); }
            ZHIP(hipEventRecord(ev[11], sa));
        }
        if (phase == 0) continue;
        // ---- pieces: the units of work of the frame pass.  A frame is a chain for one wave (its matches read what its earlier blocks
        // wrote) -- unless stage 2's summaries show that from some block on nothing in front of that block is read: the engine's own
        // frames are made of independent 2 MiB segments (zge_match.hip), libzstd's multi-threaded ones of independent jobs.  The host
        // cuts such frames (4 MiB and more) at those blocks, gives every piece its output position and repeat-offset history, and the
        // pieces decode side by side.
        const size_t fl = lean ? std::max(f0, std::min(f1, n_large)) : f1; // lean: frames [f0, fl) get a piece list, [fl, f1) are one piece each (no list)
        if (fastpath) {
            const uint64_t s0 = slot_prefix[f0], s1 = slot_prefix[fl];
            bool large = false;
            for (size_t i = f0; i < fl && !large; i++) large = nblk_of[i] >= 32;
            if (large) {
                ZHIP(hipEventSynchronize(ev[11]));
                hblocks.resize(s1 - s0); hfast.resize(fl - f0);
                ZHIP(hipMemcpyAsync(hblocks.data(), h->d_zblocks.as<ZdecBlock>() + s0, (s1 - s0) * sizeof(ZdecBlock), hipMemcpyDeviceToHost, sa));
                ZHIP(hipMemcpyAsync(hfast.data(), h->d_fast.as<uint32_t>() + f0, (fl - f0) * 4, hipMemcpyDeviceToHost, sa));
                ZHIP(hipStreamSynchronize(sa));
            }
            std::vector<ZdecPiece> &pc = pieces[g];
            std::vector<uint64_t> start, need;
            for (size_t i = f0; i < fl; i++) {
                const uint32_t nb = nblk_of[i];
                ZdecPiece whole{(uint32_t)i, 0u, 0xFFFFFFFFu, {1u, 4u, 8u}, 0ull, raw_len[i]};
                if (!large || nb < 32 || !hfast[i - f0]) { pc.push_back(whole); continue; }
                const ZdecBlock *zb = hblocks.data() + (slot_prefix[i] - s0);
                // where every block's output starts, and the lowest position it reads
                start.assign(nb + 1, 0); need.assign(nb + 1, ~0ull);
                bool usable = true;
                for (uint32_t j = 0; j < nb && usable; j++) {
                    if (zb[j].type > 2 || (zb[j].type == 2 && zb[j].nseq && zb[j].state != 1)) usable = false;
                    start[j + 1] = start[j] + zb[j].pad[1];
                    need[j] = (zb[j].pad[0] == ZDEC_REACH_UNKNOWN || zb[j].pad[0] > start[j]) ? 0 : start[j] - zb[j].pad[0];
                }
                if (!usable || start[nb] != raw_len[i]) { pc.push_back(whole); continue; }
                for (uint32_t j = nb; j-- > 0;) need[j] = std::min(need[j], need[j + 1]); // lowest position read by block j or any later one
                uint32_t r[3] = {1u, 4u, 8u}, first = 0, rfirst[3] = {1u, 4u, 8u};
                bool rep_ok = true;
                for (uint32_t j = 0; j <= nb; j++) {
                    const bool cut = j == nb || (j > first && j - first >= 8 && nb - j >= 8 && need[j] >= start[j] && rep_ok);
                    if (cut) {
                        pc.push_back(ZdecPiece{(uint32_t)i, first, j == nb ? 0xFFFFFFFFu : j - first, {rfirst[0], rfirst[1], rfirst[2]}, start[first], start[j] - start[first]});
                        first = j; rfirst[0] = r[0]; rfirst[1] = r[1]; rfirst[2] = r[2];
                    }
                    if (j == nb) break;
                    if (zb[j].type == 2 && zb[j].nseq) { // history after the block, from its symbolic summary
                        uint32_t nr[3];
                        for (int k = 0; k < 3; k++) {
                            const uint32_t e = zb[j].rep[k];
                            if (e & ZDEC_REP_REF) {
                                const uint32_t slot = e & 3, delta = (e & ~ZDEC_REP_REF) >> 2, hv = slot < 3 ? r[slot] : 0u;
                                if (hv <= delta) { rep_ok = false; nr[k] = 1; } else nr[k] = hv - delta; // (no cut behind a history the frame pass would reject)
                            }
                            else nr[k] = e;
                        }
                        r[0] = nr[0]; r[1] = nr[1]; r[2] = nr[2];
                    }
                }
            }
            std::stable_sort(pc.begin(), pc.end(), [](const ZdecPiece &x, const ZdecPiece &y) { return x.out_len > y.out_len; }); // longest first
            if (!pc.empty()) ZHIP(hipMemcpyAsync(h->d_pieces.as<ZdecPiece>() + piece_base, pc.data(), pc.size() * sizeof(ZdecPiece), hipMemcpyHostToDevice, sa));
        }
        ZHIP(hipEventRecord(ev[4], sa));
        const size_t grid_g = std::max<size_t>(1, std::min<size_t>(ng, dec_grid / (size_t)groups));
        if (fastpath) {
            const size_t listed = pieces[g].size(), np = listed + (f1 - fl); // behind the list: frames [fl, f1), one piece each, made up by the kernel
            hipLaunchKernelGGL(zarc_zstd_frames, dim3((unsigned)std::min<size_t>(np, (size_t)h->num_cus * 16)), dim3(64), 0, sa, (const uint8_t *)d_frames_base, h->d_frame_off.as<uint64_t>(),
                               h->d_frame_len.as<uint64_t>(), (uint8_t *)d_dst_base, b_dst_off.as<uint64_t>(), h->d_raw_len.as<uint64_t>(),
                               h->d_pieces.as<ZdecPiece>() + piece_base, (uint32_t)listed, (uint32_t)fl, (uint32_t)np, h->d_status.as<int32_t>(), h->d_stored_ck.as<uint32_t>(), dec_dbg, h->d_queue.as<uint32_t>() + 2 * g,
                               h->d_fast.as<uint32_t>(), h->d_slot_prefix.as<uint64_t>(), h->d_zblocks.as<ZdecBlock>(), h->d_seqidx.as<uint64_t>(),
                               h->d_seqs.as<uint64_t>(), h->d_litidx.as<uint64_t>(), h->d_lits.as<uint8_t>());
            ZHIP(hipGetLastError());
        }
        // frames the fast path turned down (or all of them when it is off) are decoded inline; with nothing to do every wave leaves at once.
        // Each group's launch has its own slice of the per-wave literal scratch.
        hipLaunchKernelGGL(zarc_zstd_decode, dim3((unsigned)grid_g), dim3(64), (size_t)diag_env("ZARC_GPU_DEC_PADLDS", 0), sa,
                           (const uint8_t *)d_frames_base, h->d_frame_off.as<uint64_t>(), h->d_frame_len.as<uint64_t>(), (uint8_t *)d_dst_base,
                           b_dst_off.as<uint64_t>(), h->d_raw_len.as<uint64_t>(), h->d_order.as<uint32_t>() + f0, (uint32_t)ng,
                           h->d_declit.as<uint8_t>() + (size_t)g * (dec_grid / (size_t)groups) * (size_t)(ZARC_BLOCK_MAX + 64),
                           h->d_status.as<int32_t>(), h->d_stored_ck.as<uint32_t>(), dec_dbg, h->d_queue.as<uint32_t>() + 2 * g + 1,
                           fastpath ? h->d_fast.as<uint32_t>() : (const uint32_t *)nullptr);
        ZHIP(hipGetLastError());
        ZHIP(hipEventRecord(ev[5], sa));
        if (chk) { piece_base += pieces[g].size(); continue; } // decode-only: zarc_check_compare judges the bytes
        // verification passes over the decoded bytes (K2 + XXH64 inside libzstd in the reference): checksum (side stream) and digest
        // next to each other
        ZHIP(hipStreamWaitEvent(sb, ev[5], 0));
        ZHIP(hipEventRecord(ev[6], sb));
        hipLaunchKernelGGL(zarc_xxh64, dim3((unsigned)((ng * 4 + 255) / 256)), dim3(256), 0, sb, (const uint8_t *)d_dst_base, b_dst_off.as<uint64_t>() + f0,
                           h->d_raw_len.as<uint64_t>() + f0, (uint32_t)ng, h->d_xxh.as<uint64_t>() + f0);
        ZHIP(hipGetLastError());
        ZHIP(hipEventRecord(ev[7], sb));
        ZHIP(hipEventRecord(ev[8], sa));
        {
            const uint64_t chunks = gchunk0[g + 1] - gchunk0[g];
            hipLaunchKernelGGL(zarc_blake3_chunks, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, sa, (const uint8_t *)d_dst_base, b_dst_off.as<uint64_t>() + f0,
                               h->d_raw_len.as<uint64_t>() + f0, h->d_chunk_prefix.as<uint64_t>() + f0 + (size_t)g, (uint32_t)ng, chunks,
                               h->d_cvs.as<uint32_t>() + gchunk0[g] * 8, h->d_digests.as<uint32_t>() + f0 * 8);
            hipLaunchKernelGGL(zarc_blake3_tree, dim3((unsigned)std::min<size_t>(ng, 65535)), dim3(256), 0, sa, h->d_chunk_prefix.as<uint64_t>() + f0 + (size_t)g, (uint32_t)ng,
                               h->d_cvs.as<uint32_t>() + gchunk0[g] * 8, h->d_cvs_tmp.as<uint32_t>() + gchunk0[g] * 8, h->d_digests.as<uint32_t>() + f0 * 8);
            ZHIP(hipGetLastError());
        }
        ZHIP(hipEventRecord(ev[9], sa));
        piece_base += pieces[g].size();
    }
    // join: the decode time ends with the last group's frame pass, the whole call with the last hash
    for (int g = 0; g < groups; g++) if (groups > 1) ZHIP(hipStreamWaitEvent(h->stream, h->ev_g[g][5], 0));
    ZHIP(t.mark(&e1));
    const DecodedPart part{h, n, order, raw_len, (const uint8_t *)d_dst_base, b_dst_off.as<uint64_t>(), h->d_status.as<int32_t>(), t};
    if (chk) return readback_compare(part, *chk, d_frames_base);
    for (int g = 0; g < groups; g++) {
        ZHIP(hipStreamWaitEvent(h->stream, h->ev_g[g][7], 0));
        if (groups > 1) ZHIP(hipStreamWaitEvent(h->stream, h->ev_g[g][9], 0));
    }
    ZHIP(t.mark(&e3));
    hipLaunchKernelGGL(zarc_unpack_verdict, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (uint32_t)n, h->d_xxh.as<uint64_t>(),
                       h->d_stored_ck.as<uint32_t>(), h->d_digests.as<uint32_t>(), expect_in ? h->d_expect.as<uint32_t>() : (const uint32_t *)nullptr,
                       h->d_status.as<int32_t>());
    ZHIP(hipGetLastError());
    SearchPart sp;
    if (srch && (rc = search_launch(part, *srch, sp))) return rc;
    if (srch && srch->lines && (rc = lines_mark(part, *srch, sp))) return rc;
    RangePart rp;
    if (rng && (rc = range_launch(part, *rng, rp))) return rc;
    WcPart wp;
    if (wc && (rc = wc_launch(part, wp))) return rc;
    CmpPart cp;
    if (cmp && (rc = cmp_launch(part, *cmp, cp))) return rc;
    std::vector<int32_t> st_v;
    std::vector<uint8_t> dg_v;
    int32_t *st = (int32_t *)meta_take(h, n * 4); // results come back through the page-locked arena too, then go to the caller's order
    uint8_t *dg = (uint8_t *)meta_take(h, n * 32);
    if (!st) { st_v.resize(n); st = st_v.data(); }
    if (!dg) { dg_v.resize(n * 32); dg = dg_v.data(); }
    ZHIP(hipMemcpyAsync(st, h->d_status.p, n * 4, hipMemcpyDeviceToHost, h->stream));
    ZHIP(hipMemcpyAsync(dg, h->d_digests.p, n * 32, hipMemcpyDeviceToHost, h->stream));
    if (srch && (rc = search_collect(part, *srch, sp))) return rc;
    ZHIP(hipStreamSynchronize(h->stream)); // the one wait of a part for its per-frame results: the verdict's and the search's
    for (size_t i = 0; i < n; i++) { status[order[i]] = st[i]; memcpy(digest + (size_t)order[i] * 32, dg + i * 32, 32); }
    if (srch) search_scatter(part, *srch, sp);
    if (srch && srch->lines && (rc = lines_deliver(part, *srch, sp))) return rc;
    if (rng && (rc = range_deliver(part, *rng, rp))) return rc;
    if (wc) wc_deliver(part, *wc, wp);
    if (cmp) cmp_deliver(part, *cmp, cp);
    if (fastpath && diag_env("ZARC_GPU_DEC_STATS", 0)) { // diagnostics: how many frames had their sequences decoded ahead
        std::vector<uint32_t> fl(n);
        ZHIP(hipMemcpy(fl.data(), h->d_fast.p, n * 4, hipMemcpyDeviceToHost));
        size_t nf = 0;
        for (uint32_t v : fl) nf += v != 0;
        size_t np = 0;
        for (int g = 0; g < groups; g++) np += pieces[g].size();
        fprintf(stderr, "zstd_decode: %zu of %zu frames on the fast path, %d group(s), %zu piece(s)\n", nf, n, groups, np);
        if (h->d_seqflag.p) {
            std::vector<uint32_t> wf(nslots / 16 + 1);
            ZHIP(hipMemcpy(wf.data(), h->d_seqflag.p, wf.size() * 4, hipMemcpyDeviceToHost));
            size_t nw = 0;
            for (uint32_t v : wf) nw += v != 0;
            fprintf(stderr, "zdec_seqs: %zu of %zu 64-slot waves workgroups turned down by the shared-table kernel (of at most that many; one group: exact)\n", nw, wf.size());
        }
    }
    h->ms[ZARC_GPU_T_DECODE] = elapsed(h, e0, e1);
    // per-kernel times: sums over the groups (with several groups the kernels of different groups overlap, so the sums exceed T_DECODE)
    float t_seq = 0, t_lit = 0, t_frm = 0, t_xxh = 0, t_b3 = 0;
    for (int g = 0; g < groups; g++) {
        float ms = 0;
        hipEvent_t *ev = h->ev_g[g];
        if (have_seq_t[g] && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) t_seq += ms;
        if (have_lit_t[g] && hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) t_lit += ms;
        if (hipEventElapsedTime(&ms, ev[4], ev[5]) == hipSuccess) t_frm += ms;
        if (hipEventElapsedTime(&ms, ev[6], ev[7]) == hipSuccess) t_xxh += ms;
        if (hipEventElapsedTime(&ms, ev[8], ev[9]) == hipSuccess) t_b3 += ms;
    }
    h->ms[ZARC_GPU_T_DEC_SEQS] = t_seq; h->ms[ZARC_GPU_T_DEC_LITS] = t_lit; h->ms[ZARC_GPU_T_DEC_FRAMES] = t_frm;
    h->ms[ZARC_GPU_T_XXH64] = t_xxh; // side stream: overlaps the digest pass
    h->ms[ZARC_GPU_T_BLAKE3] = t_b3;
    h->ms[ZARC_GPU_T_TOTAL] = elapsed(h, e0, e3);
    if (srch) { h->ms[ZARC_GPU_T_SEARCH] = elapsed(h, sp.e5, sp.e6); h->ms[ZARC_GPU_T_TOTAL] = elapsed(h, e0, sp.e6); }
    if (srch && srch->lines) { h->ms[ZARC_GPU_T_LINES] = elapsed(h, sp.e6, sp.e7) + sp.lines_ms2; h->ms[ZARC_GPU_T_TOTAL] = elapsed(h, e0, sp.e7) + sp.lines_ms2; }
    if (rng) { h->ms[ZARC_GPU_T_RANGE] = elapsed(h, rp.r0, rp.r1) + rp.ms2; h->ms[ZARC_GPU_T_TOTAL] = elapsed(h, e0, rp.r1) + rp.ms2; }
    if (wc) { h->ms[ZARC_GPU_T_WC] = elapsed(h, wp.w0, wp.w1); h->ms[ZARC_GPU_T_TOTAL] = elapsed(h, e0, wp.w1); }
    if (cmp) { h->cmp_ms = elapsed(h, cp.c0, cp.c1); h->ms[ZARC_GPU_T_TOTAL] = elapsed(h, e0, cp.c1); }
    return ZARC_GPU_OK;
}

// A batch whose decoder scratch (sequences and literals decoded ahead, tables) does not fit -- the budget of ZARC_GPU_PX_SCRATCH_MB, or
// the device itself -- is unpacked in two halves, each of which may split again; the scratch is reused between them.  Frames are
// independent, so nothing changes but the time.
// d_dst_base == nullptr (verify, the read-back check of pack): the decoded bytes go to scratch the handle owns (d_vout, offsets 16-byte
// aligned in the decoder's order, made by unpack_device_once: no per-frame array of the caller's is involved) and count against the same budget: a batch whose decoded bytes exceed it is halved before it is tried, one
// that does not fit the device is halved after; a single frame runs alone whatever its size.
int unpack_device_split(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                        void *d_dst_base, const uint64_t *dst_off, const uint64_t *raw_len, const uint8_t *expect, uint8_t *digest, int *status,
                        const PackCheck *chk = nullptr, const SearchReq *srch, const RangeReq *rng, const WcReq *wc, const CmpReq *cmp)
{
    const bool own = d_dst_base == nullptr;
    DevBuf &vout = h->vout_busy ? h->d_vout2 : h->d_vout; // (the read-back check inside a repack pass: d_vout holds what it compares with)
    uint64_t total = 0, acc = 0, own_bytes = 0;
    for (size_t i = 0; i < n; i++) { total += raw_len[i]; own_bytes += (raw_len[i] + (ZARC_GPU_ALIGN - 1)) & ~(uint64_t)(ZARC_GPU_ALIGN - 1); }
    if (!own) own_bytes = 0;
    int rc = UNPACK_SPLIT;
    bool attempt = !(n >= 2 && h->dec_split_above && total >= h->dec_split_above); // (a batch of this size ran out of device memory before: do not try again)
    if (own && attempt) {
        if (n >= 2 && h->scratch_budget && own_bytes > h->scratch_budget) attempt = false;
        else {
            const hipError_t e = vout.reserve(own_bytes + ZARC_GPU_PAD + 256);
            if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); rc = ZARC_GPU_E_NOMEM; attempt = false; }
            else ZHIP(e);
        }
    }
    if (attempt)
        rc = unpack_device_once(h, n, d_frames_base, frame_off, frame_len, own ? vout.p : d_dst_base, own ? nullptr : dst_off, raw_len, expect, digest,
                                status, own_bytes, chk, nullptr, srch, rng, wc, cmp);
    if ((rc != UNPACK_SPLIT && rc != ZARC_GPU_E_NOMEM) || n < 2) return rc == UNPACK_SPLIT ? ZARC_GPU_E_NOMEM : rc;
    (void)hipStreamSynchronize(h->stream);
    if (rc == ZARC_GPU_E_NOMEM) {
        DevBuf *big[] = {&h->d_seqs, &h->d_lits, &h->d_ztables, &h->d_zblocks, &h->d_seqidx, &h->d_litidx, &h->d_nseq, &vout};
        for (DevBuf *b : big) b->release();
        if (!chk) { h->d_cvs.release(); h->d_cvs_tmp.release(); }
        if (!h->dec_split_above || total < h->dec_split_above) h->dec_split_above = total;
    }
    size_t k = 0;
    while (k + 1 < n && (acc + raw_len[k]) * 2 <= total) acc += raw_len[k++];
    if (k == 0) k = 1;
    float ms[ZARC_GPU_T_COUNT], cmp_ms = 0;
    const size_t part[3] = {0, k, n};
    for (int i = 0; i < ZARC_GPU_T_COUNT; i++) ms[i] = 0;
    for (int p = 0; p < 2; p++) {
        const size_t a = part[p], m = part[p + 1] - a;
        PackCheck sub{};
        if (chk) { sub = *chk; sub.first_bad += a; if (chk->entry_map) sub.entry_map += a; else sub.entry0 += (uint32_t)a; }
        const SearchReq ssub = srch ? part_of(*srch, a) : SearchReq{};
        const RangeReq rsub = rng ? part_of(*rng, a) : RangeReq{};
        const WcReq wsub = wc ? part_of(*wc, a) : WcReq{};
        const CmpReq csub = cmp ? part_of(*cmp, a) : CmpReq{};
        rc = unpack_device_split(h, m, d_frames_base, frame_off + a, frame_len + a, d_dst_base, own ? nullptr : dst_off + a, raw_len + a, expect ? expect + a * 32 : nullptr,
                                 digest ? digest + a * 32 : nullptr, status ? status + a : nullptr, chk ? &sub : nullptr, srch ? &ssub : nullptr, rng ? &rsub : nullptr,
                                 wc ? &wsub : nullptr, cmp ? &csub : nullptr);
        if (rc) return rc;
        for (int i = 0; i < ZARC_GPU_T_COUNT; i++) ms[i] += h->ms[i];
        if (cmp) cmp_ms += h->cmp_ms;
    }
    if (!chk) for (int i = 0; i < ZARC_GPU_T_COUNT; i++) h->ms[i] = ms[i];
    if (cmp) h->cmp_ms = cmp_ms;
    return ZARC_GPU_OK;
}
} // namespace
extern "C" {

int zarc_gpu_unpack_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                 void *d_dst_base, const uint64_t *dst_off, const uint64_t *raw_len, const uint8_t *expect, uint8_t *digest,
                                 int *status)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!d_frames_base || !frame_off || !frame_len || !d_dst_base || !dst_off || !raw_len || !digest || !status) return ZARC_GPU_E_PARAM;
    return unpack_device_split(h, n, d_frames_base, frame_off, frame_len, d_dst_base, dst_off, raw_len, expect, digest, status);
}

// FrameIterator::verify() without the bytes: the same decoder, hash passes and verdict as unpack, the output in scratch of the handle
int zarc_gpu_verify_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                 const uint64_t *raw_len, const uint8_t *expect, uint8_t *digest, int *status)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!d_frames_base || !frame_off || !frame_len || !raw_len || !digest || !status) return ZARC_GPU_E_PARAM;
    return unpack_device_split(h, n, d_frames_base, frame_off, frame_len, nullptr, nullptr, raw_len, expect, digest, status);
}

} // extern "C"
namespace {
// Frames of 4 GiB and more are refused before any size arithmetic or staging.  frame (host forms): every frame with bytes has an address.
template <typename Len> // (uint64_t in the device forms, size_t in the host forms)
int check_frame_sizes(zarc_gpu_t *h, size_t n, const Len *frame_len, const Len *raw_len, const void *const *frame = nullptr)
{
    for (size_t i = 0; i < n; i++) {
        if (frame && frame_len[i] && !frame[i]) return ZARC_GPU_E_PARAM;
        if ((uint64_t)frame_len[i] >= 0xFFFFFFF0ull || (uint64_t)raw_len[i] >= 0xFFFFFFF0ull) { set_error(h, "frames of 4 GiB or more are not supported"); return ZARC_GPU_E_UNSUPPORTED; }
    }
    return 0;
}

// ---- search (zarc_gpu_search_*): a verify pass that looks through what it decoded, per part, while that part's bytes are in d_vout ----
uint32_t ceil_log2(uint32_t v) { uint32_t l = 0; while ((1u << l) < v) l++; return l; }
// The set goes up once per call, compiled into what zdec_search_set.hip reads (the layout is described there and at ZarcSetDesc) and folded
// here when the text is folded there.  Filters and tables are sized from the number of distinct keys of each length class.
int search_upload_set(zarc_gpu_t *h, const zarc_gpu_pattern_set *set, unsigned flags)
{
    const uint32_t K = (uint32_t)set->count;
    const bool fold = (flags & ZARC_GPU_SEARCH_ICASE) != 0;
    std::map<uint32_t, std::vector<uint32_t>> keys[4]; // per class: the patterns that share a key, ascending
    std::vector<uint32_t> pat(2 * (size_t)K), bytes;
    ZarcSetDesc sd{};
    sd.count = K; sd.min_len = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < K; k++) {
        const uint8_t *src = (const uint8_t *)set->bytes + set->off[k];
        const uint32_t len = (uint32_t)set->len[k], w0 = (uint32_t)bytes.size();
        bytes.resize(w0 + (len + 3) / 4, 0);
        for (uint32_t b = 0; b < len; b++) {
            uint8_t v = src[b];
            if (fold && v >= 'A' && v <= 'Z') v |= 0x20;
            bytes[w0 + b / 4] |= (uint32_t)v << (8 * (b & 3));
        }
        pat[2 * k] = w0; pat[2 * k + 1] = len;
        const uint32_t c = std::min(len, 4u) - 1; // (the word's unused bytes are 0: the word of a short pattern is its key)
        keys[c][bytes[w0]].push_back(k);
        sd.min_len = std::min(sd.min_len, len);
    }
    uint32_t cur = 0;
    for (uint32_t c = 0; c < 4; c++) {
        if (keys[c].empty()) continue;
        const uint32_t nk = (uint32_t)keys[c].size();
        sd.classes |= 1u << c;
        sd.flog[c] = c == 0 ? 8 : std::max(6u, ceil_log2(16 * nk));
        sd.tlog[c] = std::max(1u, ceil_log2(2 * nk));
        sd.foff[c] = cur; cur += (1u << sd.flog[c]) / 32;
        sd.toff[c] = cur; cur += 2u << sd.tlog[c];
    }
    sd.lds_words = cur;
    if ((size_t)cur * 4 > 40960) { set_error(h, "search_set: the compiled set is too large"); return ZARC_GPU_E_PARAM; } // (cannot happen with 1024 patterns: 9 words per key at the most)
    std::vector<uint32_t> blob(cur, 0);
    for (uint32_t c = 0; c < 4; c++)
        for (const auto &kv : keys[c]) {
            const uint32_t key = kv.first, hash = key * ZARC_SET_HASH;
            const uint32_t bit = c == 0 ? key : hash >> (32 - sd.flog[c]);
            blob[sd.foff[c] + bit / 32] |= 1u << (bit & 31);
            uint32_t slot = hash >> (32 - sd.tlog[c]);
            while (blob[sd.toff[c] + 2 * slot + 1]) slot = (slot + 1) & ((1u << sd.tlog[c]) - 1);
            blob[sd.toff[c] + 2 * slot] = key;
            blob[sd.toff[c] + 2 * slot + 1] = (uint32_t)blob.size(); // (never 0: the image lies in front)
            blob.push_back((uint32_t)kv.second.size());
            blob.insert(blob.end(), kv.second.begin(), kv.second.end());
        }
    sd.pat_off = (uint32_t)blob.size();
    const uint32_t bytes_off = sd.pat_off + 2 * K;
    for (uint32_t k = 0; k < K; k++) { blob.push_back(bytes_off + pat[2 * k]); blob.push_back(pat[2 * k + 1]); }
    blob.insert(blob.end(), bytes.begin(), bytes.end());
    ZHIP(h->d_set.reserve(blob.size() * 4));
    ZHIP(h->d_set_hits.reserve((size_t)K * 4));
    ZHIP(hipMemcpy(h->d_set.p, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
    h->set_desc = sd;
    return 0;
}
static_assert(sizeof(ZarcRegexDfa) == sizeof(zarc_gpu_regex_dfa) && offsetof(ZarcRegexDfa, delta) == offsetof(zarc_gpu_regex_dfa, delta), "the device's table is the caller's");

// What the twelve entry points are called with, beside the frames: what to search for, where the results go, and (lines) what to gather
struct MatcherArgs {
    Matcher::Kind kind;
    const void *text;                 // PATTERN: its bytes; REGEX: the expression
    size_t text_len;
    const zarc_gpu_pattern_set *set;  // SET
    unsigned flags;
};
struct SearchOut { uint8_t *digest; int *status; uint64_t *count, *first, *which /* SET */, *hits /* SET, or null */; };
struct LinesArgs {
    uint64_t max_lines, max_line;
    uint64_t *lines;
    zarc_gpu_line *rec;
    size_t rec_cap, *rec_used;
    void *text;                       // device form: on the device; host form: the caller's memory
    size_t text_cap, *text_used;
    const zarc_gpu_line_select *select = nullptr; // zarc_gpu_select_lines_batch*
    uint64_t *selected = nullptr;
    // zarc_gpu_search_matches_batch*: rec_cap, rec_used, text* above are the MATCH records' (rec itself stays null); the lines have line_cap
    bool only_matches = false;
    size_t line_cap = 0;
    uint64_t *matches = nullptr;
    zarc_gpu_match *match_rec = nullptr;
};

// Every check of a search call that does not look at the frames, in the order the callers are promised (the matcher, the flags, the result
// arrays, then the lines arguments), the zeroing of what the call adds to, the call's request, and -- unless the call is empty -- the matcher's
// way to the device: once per call, whatever the call is cut into.  A bad expression is refused whatever n is.
// host_text: the lines' text goes to the caller's memory (host form), not to the device
int search_prepare(zarc_gpu_t *h, size_t n, const MatcherArgs &a, const SearchOut &out, const LinesArgs *la, bool host_text, LinesRun *run, SearchReq *req)
{
    const unsigned unknown = a.flags & ~(unsigned)ZARC_GPU_SEARCH_ICASE;
    const bool no_out = !out.digest || !out.status || !out.count || !out.first;
    zarc_gpu_regex_dfa dfa, fwd; // REGEX: compiled by the checks, uploaded below (fwd: the matches calls' forward table)
    switch (a.kind) {
    case Matcher::PATTERN:
        if (!a.text || a.text_len == 0 || a.text_len > ZARC_GPU_SEARCH_MAX_PATTERN) { set_error(h, "search: the pattern has 1 to 256 bytes"); return ZARC_GPU_E_PARAM; }
        if (unknown) { set_error(h, "search: unknown flag"); return ZARC_GPU_E_PARAM; }
        if (no_out) return ZARC_GPU_E_PARAM;
        break;
    case Matcher::SET:
        if (!a.set || !a.set->bytes || !a.set->off || !a.set->len) { set_error(h, "search_set: a set and its members are needed"); return ZARC_GPU_E_PARAM; }
        if (a.set->count == 0 || a.set->count > ZARC_GPU_SEARCH_MAX_SET) { set_error(h, "search_set: a set has 1 to 1024 patterns"); return ZARC_GPU_E_PARAM; }
        for (size_t k = 0; k < a.set->count; k++) {
            if (a.set->len[k] == 0 || a.set->len[k] > ZARC_GPU_SEARCH_MAX_PATTERN) { set_error(h, "search_set: a pattern has 1 to 256 bytes"); return ZARC_GPU_E_PARAM; }
            if (la && memchr((const uint8_t *)a.set->bytes + a.set->off[k], 0x0A, a.set->len[k])) { set_error(h, "search_set_lines: a pattern must not contain a newline"); return ZARC_GPU_E_PARAM; }
        }
        if (unknown) { set_error(h, "search: unknown flag"); return ZARC_GPU_E_PARAM; }
        if (no_out || !out.which) return ZARC_GPU_E_PARAM;
        break;
    case Matcher::REGEX: {
        if (unknown) { set_error(h, "search: unknown flag"); return ZARC_GPU_E_PARAM; }
        std::string err;
        const int rc = zre::compile(a.text, a.text_len, a.flags, &dfa, err);
        if (rc) { set_error(h, err.c_str()); return rc; }
        if (la && la->only_matches) {
            const int rc2 = zre::compile(a.text, a.text_len, a.flags, &fwd, err, /*ends=*/true);
            if (rc2) { set_error(h, err.c_str()); return rc2; }
        }
        if (no_out) return ZARC_GPU_E_PARAM;
        break; }
    }
    if (la) { // -> ZARC_GPU_E_PARAM or ZARC_GPU_E_DSTSIZE
        if (!la->lines || !la->rec_used || !la->text_used) return ZARC_GPU_E_PARAM;
        if (!la->only_matches && la->rec_cap && (!la->rec || !la->text)) return ZARC_GPU_E_PARAM;
        if (la->max_line < 1 || la->max_line > ZARC_GPU_LINES_MAX_LINE) { set_error(h, "search_lines: max_line is 1 to 65536"); return ZARC_GPU_E_PARAM; }
        if (a.kind == Matcher::PATTERN && memchr(a.text, 0x0A, a.text_len)) { set_error(h, "search_lines: the pattern must not contain a newline"); return ZARC_GPU_E_PARAM; }
        if (la->rec_cap > SIZE_MAX / (size_t)la->max_line || la->text_cap < la->rec_cap * (size_t)la->max_line) { set_error(h, "search_lines: text_cap is below rec_cap * max_line"); return ZARC_GPU_E_DSTSIZE; }
        if (la->select) {
            if (la->select->flags & ~(uint32_t)ZARC_GPU_SELECT_INVERT) { set_error(h, "select_lines: unknown select flag"); return ZARC_GPU_E_PARAM; }
            if (la->select->reserved) { set_error(h, "select_lines: reserved must be 0"); return ZARC_GPU_E_PARAM; }
            if (!la->selected) return ZARC_GPU_E_PARAM;
        }
        if (la->only_matches && (!la->matches || (la->line_cap && la->rec_cap && (!la->match_rec || !la->text)))) return ZARC_GPU_E_PARAM;
        *la->rec_used = 0; *la->text_used = 0;
    }
    if (a.kind == Matcher::SET && out.hits) memset(out.hits, 0, a.set->count * sizeof *out.hits); // (every part adds to them)
    *req = SearchReq{Matcher{a.kind, a.flags & ZARC_GPU_SEARCH_ICASE ? 1u : 0u, {}}, out.count, out.first, out.which, out.hits, la != nullptr, LinesReq{}};
    if (la) req->ln = LinesReq{la->max_lines, (uint32_t)la->max_line, la->lines, 0, la->rec, la->rec_cap, host_text ? nullptr : (uint8_t *)la->text,
                               host_text ? (uint8_t *)la->text : nullptr, run, false, ZarcSelect{0, 0, 0}, nullptr};
    if (la && la->only_matches) { // the line records stay on the device: their cap is line_cap
        req->ln.rec = nullptr; req->ln.rec_cap = la->line_cap;
        req->ln.mt = MatchesReq{true, la->matches, la->match_rec, la->rec_cap, nullptr};
    }
    if (la && la->select) {
        req->ln.select = la->select->flags || la->select->before || la->select->after;
        req->ln.sel = ZarcSelect{la->select->flags & ZARC_GPU_SELECT_INVERT ? 1u : 0u, la->select->before, la->select->after};
        req->ln.selected = la->selected;
    }
    if (n == 0) return 0;
    switch (a.kind) {
    case Matcher::PATTERN: { // folded here when the text is folded there ('A'..'Z' only)
        uint8_t pat[ZARC_GPU_SEARCH_MAX_PATTERN] = {0};
        memcpy(pat, a.text, a.text_len);
        if (req->match.icase) for (size_t k = 0; k < a.text_len; k++) if (pat[k] >= 'A' && pat[k] <= 'Z') pat[k] |= 0x20;
        ZHIP(h->d_srch_pat.reserve(sizeof pat));
        ZHIP(hipMemcpy(h->d_srch_pat.p, pat, sizeof pat, hipMemcpyHostToDevice));
        req->match.pattern = Matcher::Pattern{h->d_srch_pat.as<uint8_t>(), (uint32_t)a.text_len};
        return 0; }
    case Matcher::SET:
        req->match.set = &h->set_desc;
        return search_upload_set(h, a.set, a.flags);
    case Matcher::REGEX:
        ZHIP(h->d_regex.reserve(sizeof dfa));
        ZHIP(hipMemcpy(h->d_regex.p, &dfa, sizeof dfa, hipMemcpyHostToDevice));
        req->match.d_regex = h->d_regex.as<ZarcRegexDfa>();
        if (la && la->only_matches) {
            ZHIP(h->d_regex_fwd.reserve(sizeof fwd));
            ZHIP(hipMemcpy(h->d_regex_fwd.p, &fwd, sizeof fwd, hipMemcpyHostToDevice));
            req->ln.mt.d_fwd = h->d_regex_fwd.as<ZarcRegexDfa>();
        }
        return 0;
    }
    return 0;
}

// zarc_gpu_select_lines_batch*: the matcher description as the arguments of that kind's own lines call
// ... and zarc_gpu_search_matches_batch*: the matcher alone
int matches_matcher(zarc_gpu_t *h, const zarc_gpu_matcher *m, const uint64_t *which, const uint64_t *hits, MatcherArgs *a)
{
    if (!m) { set_error(h, "search_matches: a matcher is needed"); return ZARC_GPU_E_PARAM; }
    switch (m->kind) {
    case ZARC_GPU_MATCH_FIXED: *a = MatcherArgs{Matcher::PATTERN, m->text, m->text_len, nullptr, m->flags}; break;
    case ZARC_GPU_MATCH_SET: *a = MatcherArgs{Matcher::SET, nullptr, 0, m->set, m->flags}; break;
    case ZARC_GPU_MATCH_REGEX: *a = MatcherArgs{Matcher::REGEX, m->text, m->text_len, nullptr, m->flags}; break;
    default: set_error(h, "search_matches: unknown matcher kind"); return ZARC_GPU_E_PARAM;
    }
    if (m->kind != ZARC_GPU_MATCH_SET && (which || hits)) { set_error(h, "search_matches: which and hits belong to a set"); return ZARC_GPU_E_PARAM; }
    return 0;
}
int select_matcher(zarc_gpu_t *h, const zarc_gpu_matcher *m, const zarc_gpu_line_select *select, const uint64_t *which, const uint64_t *hits, MatcherArgs *a)
{
    if (!m || !select) { set_error(h, "select_lines: a matcher and a selection are needed"); return ZARC_GPU_E_PARAM; }
    switch (m->kind) {
    case ZARC_GPU_MATCH_FIXED: *a = MatcherArgs{Matcher::PATTERN, m->text, m->text_len, nullptr, m->flags}; break;
    case ZARC_GPU_MATCH_SET: *a = MatcherArgs{Matcher::SET, nullptr, 0, m->set, m->flags}; break;
    case ZARC_GPU_MATCH_REGEX: *a = MatcherArgs{Matcher::REGEX, m->text, m->text_len, nullptr, m->flags}; break;
    default: set_error(h, "select_lines: unknown matcher kind"); return ZARC_GPU_E_PARAM;
    }
    if (m->kind != ZARC_GPU_MATCH_SET && (which || hits)) { set_error(h, "select_lines: which and hits belong to a set"); return ZARC_GPU_E_PARAM; }
    return 0;
}

// The six device forms: zarc_gpu_verify_batch_device with the matcher's kernels behind the verdict of every part (and the line kernels
// behind those)
int search_call_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len, const uint64_t *raw_len,
                       const uint8_t *expect, const MatcherArgs &a, const LinesArgs *la, const SearchOut &out)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    SearchReq req;
    LinesRun run;
    if ((rc = search_prepare(h, n, a, out, la, /*host_text=*/false, &run, &req))) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!d_frames_base || !frame_off || !frame_len || !raw_len) return ZARC_GPU_E_PARAM;
    if ((rc = check_frame_sizes(h, n, frame_len, raw_len))) return rc;
    rc = unpack_device_split(h, n, d_frames_base, frame_off, frame_len, nullptr, nullptr, raw_len, expect, out.digest, out.status, nullptr, &req);
    if (la) { *la->rec_used = la->only_matches ? run.match_used : run.rec_used; *la->text_used = (size_t)run.text_used; }
    return rc;
}

// ---- read ranges (zarc_gpu_read_ranges_batch*): a verify pass that cuts a byte or line range out of what it decoded, per part ----
// Every check of the call that is not verify's, and the call's request
int range_prepare(zarc_gpu_t *h, size_t n, const zarc_gpu_range *range, uint64_t max_bytes, zarc_gpu_range_result *res, void *text, size_t text_cap,
                  size_t *text_used, bool host_text, RangeRun *run, RangeReq *req)
{
    if (!range || !res || !text_used) { set_error(h, "read_ranges: range, res and text_used are needed"); return ZARC_GPU_E_PARAM; }
    for (size_t i = 0; i < n; i++) {
        if (range[i].unit != ZARC_GPU_RANGE_BYTES && range[i].unit != ZARC_GPU_RANGE_LINES) { set_error(h, "read_ranges: unknown unit"); return ZARC_GPU_E_PARAM; }
        if (range[i].flags & ~(uint32_t)ZARC_GPU_RANGE_FROM_END) { set_error(h, "read_ranges: unknown flag"); return ZARC_GPU_E_PARAM; }
    }
    if (text_cap && !text) { set_error(h, "read_ranges: text_cap without a text buffer"); return ZARC_GPU_E_PARAM; }
    *text_used = 0;
    *req = RangeReq{range, res, max_bytes, text_cap, host_text ? nullptr : (uint8_t *)text, host_text ? (uint8_t *)text : nullptr, run};
    return 0;
}
} // namespace
extern "C" {

int zarc_gpu_read_ranges_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                      const uint64_t *raw_len, const uint8_t *expect, const zarc_gpu_range *range, uint64_t max_bytes, uint8_t *digest,
                                      int *status, zarc_gpu_range_result *res, void *d_text, size_t text_cap, size_t *text_used)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) { if (text_used) *text_used = 0; return ZARC_GPU_OK; }
    if (!d_frames_base || !frame_off || !frame_len || !raw_len || !digest || !status) return ZARC_GPU_E_PARAM;
    RangeReq req;
    RangeRun run;
    if ((rc = range_prepare(h, n, range, max_bytes, res, d_text, text_cap, text_used, /*host_text=*/false, &run, &req))) return rc;
    if ((rc = check_frame_sizes(h, n, frame_len, raw_len))) return rc;
    rc = unpack_device_split(h, n, d_frames_base, frame_off, frame_len, nullptr, nullptr, raw_len, expect, digest, status, nullptr, nullptr, &req);
    *text_used = (size_t)run.text_used;
    return rc;
}

// verify_batch_device with the count kernels behind every part's verdict
int zarc_gpu_count_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                const uint64_t *raw_len, const uint8_t *expect, uint8_t *digest, int *status, zarc_gpu_wc *res)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!d_frames_base || !frame_off || !frame_len || !raw_len || !digest || !status) return ZARC_GPU_E_PARAM;
    if (!res) { set_error(h, "count: res is needed"); return ZARC_GPU_E_PARAM; }
    const WcReq req{res};
    return unpack_device_split(h, n, d_frames_base, frame_off, frame_len, nullptr, nullptr, raw_len, expect, digest, status, nullptr, nullptr, nullptr, &req);
}

// verify_batch_device with the compare kernels behind every part's verdict; the other sides are where the caller put them
int zarc_gpu_compare_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                  const uint64_t *raw_len, const uint8_t *expect, const void *d_other_base, const uint64_t *other_off,
                                  const uint64_t *other_len, uint8_t *digest, int *status, zarc_gpu_cmp *res)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!d_frames_base || !frame_off || !frame_len || !raw_len || !digest || !status) return ZARC_GPU_E_PARAM;
    if ((rc = check_frame_sizes(h, n, frame_len, raw_len))) return rc;
    if (!res || !d_other_base || !other_off || !other_len) { set_error(h, "compare: res, the other sides, their offsets and lengths are needed"); return ZARC_GPU_E_PARAM; }
    for (size_t i = 0; i < n; i++) {
        if (other_len[i] >= 0xFFFFFFF0ull) { set_error(h, "compare: other sides of 4 GiB or more are not supported"); return ZARC_GPU_E_UNSUPPORTED; }
        if (other_off[i] % ZARC_GPU_ALIGN) { set_error(h, "compare: other offset not 16-byte aligned"); return ZARC_GPU_E_PARAM; }
    }
    const CmpReq req{(const uint8_t *)d_other_base, other_off, other_len, res, false};
    return unpack_device_split(h, n, d_frames_base, frame_off, frame_len, nullptr, nullptr, raw_len, expect, digest, status, nullptr, nullptr, nullptr, nullptr, &req);
}

int zarc_gpu_search_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                 const uint64_t *raw_len, const uint8_t *expect, const void *pattern, size_t pattern_len, unsigned flags,
                                 uint8_t *digest, int *status, uint64_t *count, uint64_t *first)
{
    return search_call_device(h, n, d_frames_base, frame_off, frame_len, raw_len, expect, MatcherArgs{Matcher::PATTERN, pattern, pattern_len, nullptr, flags}, nullptr,
                              SearchOut{digest, status, count, first, nullptr, nullptr});
}
int zarc_gpu_search_lines_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                       const uint64_t *raw_len, const uint8_t *expect, const void *pattern, size_t pattern_len, unsigned flags,
                                       uint64_t max_lines, uint64_t max_line, uint8_t *digest, int *status, uint64_t *count, uint64_t *first, uint64_t *lines,
                                       zarc_gpu_line *rec, size_t rec_cap, size_t *rec_used, void *d_text, size_t text_cap, size_t *text_used)
{
    const LinesArgs la{max_lines, max_line, lines, rec, rec_cap, rec_used, d_text, text_cap, text_used};
    return search_call_device(h, n, d_frames_base, frame_off, frame_len, raw_len, expect, MatcherArgs{Matcher::PATTERN, pattern, pattern_len, nullptr, flags}, &la,
                              SearchOut{digest, status, count, first, nullptr, nullptr});
}
int zarc_gpu_search_set_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                     const uint64_t *raw_len, const uint8_t *expect, const zarc_gpu_pattern_set *set, unsigned flags,
                                     uint8_t *digest, int *status, uint64_t *count, uint64_t *first, uint64_t *which, uint64_t *hits)
{
    return search_call_device(h, n, d_frames_base, frame_off, frame_len, raw_len, expect, MatcherArgs{Matcher::SET, nullptr, 0, set, flags}, nullptr,
                              SearchOut{digest, status, count, first, which, hits});
}
int zarc_gpu_search_set_lines_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                           const uint64_t *raw_len, const uint8_t *expect, const zarc_gpu_pattern_set *set, unsigned flags,
                                           uint64_t max_lines, uint64_t max_line, uint8_t *digest, int *status, uint64_t *count, uint64_t *first,
                                           uint64_t *which, uint64_t *hits, uint64_t *lines, zarc_gpu_line *rec, size_t rec_cap, size_t *rec_used,
                                           void *d_text, size_t text_cap, size_t *text_used)
{
    const LinesArgs la{max_lines, max_line, lines, rec, rec_cap, rec_used, d_text, text_cap, text_used};
    return search_call_device(h, n, d_frames_base, frame_off, frame_len, raw_len, expect, MatcherArgs{Matcher::SET, nullptr, 0, set, flags}, &la,
                              SearchOut{digest, status, count, first, which, hits});
}
int zarc_gpu_search_regex_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                       const uint64_t *raw_len, const uint8_t *expect, const void *regex, size_t regex_len, unsigned flags,
                                       uint8_t *digest, int *status, uint64_t *count, uint64_t *first)
{
    return search_call_device(h, n, d_frames_base, frame_off, frame_len, raw_len, expect, MatcherArgs{Matcher::REGEX, regex, regex_len, nullptr, flags}, nullptr,
                              SearchOut{digest, status, count, first, nullptr, nullptr});
}
int zarc_gpu_search_regex_lines_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                             const uint64_t *raw_len, const uint8_t *expect, const void *regex, size_t regex_len, unsigned flags,
                                             uint64_t max_lines, uint64_t max_line, uint8_t *digest, int *status, uint64_t *count, uint64_t *first,
                                             uint64_t *lines, zarc_gpu_line *rec, size_t rec_cap, size_t *rec_used, void *d_text, size_t text_cap,
                                             size_t *text_used)
{
    const LinesArgs la{max_lines, max_line, lines, rec, rec_cap, rec_used, d_text, text_cap, text_used};
    return search_call_device(h, n, d_frames_base, frame_off, frame_len, raw_len, expect, MatcherArgs{Matcher::REGEX, regex, regex_len, nullptr, flags}, &la,
                              SearchOut{digest, status, count, first, nullptr, nullptr});
}

int zarc_gpu_select_lines_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                       const uint64_t *raw_len, const uint8_t *expect, const zarc_gpu_matcher *matcher, const zarc_gpu_line_select *select,
                                       uint64_t max_lines, uint64_t max_line, uint8_t *digest, int *status, uint64_t *count, uint64_t *first, uint64_t *which,
                                       uint64_t *hits, uint64_t *lines, uint64_t *selected, zarc_gpu_line *rec, size_t rec_cap, size_t *rec_used, void *d_text,
                                       size_t text_cap, size_t *text_used)
{
    MatcherArgs a;
    int rc = check_common(h, n);
    if (rc || (rc = select_matcher(h, matcher, select, which, hits, &a))) return rc;
    LinesArgs la{max_lines, max_line, lines, rec, rec_cap, rec_used, d_text, text_cap, text_used};
    la.select = select; la.selected = selected;
    std::vector<uint64_t> own_which; // a set without `which`: the search still computes it
    if (a.kind == Matcher::SET && !which) { own_which.resize(n + 1); which = own_which.data(); }
    return search_call_device(h, n, d_frames_base, frame_off, frame_len, raw_len, expect, a, &la, SearchOut{digest, status, count, first, which, hits});
}

int zarc_gpu_regex_compile(const void *regex, size_t regex_len, unsigned flags, zarc_gpu_regex_dfa *out, char *err, size_t err_cap)
{
    std::string msg;
    const int rc = zre::compile(regex, regex_len, flags, out, msg);
    if (err && err_cap) { const size_t k = std::min(msg.size(), err_cap - 1); memcpy(err, msg.data(), k); err[k] = 0; }
    return rc;
}
int zarc_gpu_regex_compile_ends(const void *regex, size_t regex_len, unsigned flags, zarc_gpu_regex_dfa *out, char *err, size_t err_cap)
{
    std::string msg;
    const int rc = zre::compile(regex, regex_len, flags, out, msg, /*ends=*/true);
    if (err && err_cap) { const size_t k = std::min(msg.size(), err_cap - 1); memcpy(err, msg.data(), k); err[k] = 0; }
    return rc;
}

int zarc_gpu_search_matches_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                         const uint64_t *raw_len, const uint8_t *expect, const zarc_gpu_matcher *matcher, uint64_t max_lines, uint64_t max_line,
                                         size_t line_cap, uint8_t *digest, int *status, uint64_t *count, uint64_t *first, uint64_t *which, uint64_t *hits,
                                         uint64_t *lines, uint64_t *matches, zarc_gpu_match *rec, size_t rec_cap, size_t *rec_used, void *d_text, size_t text_cap,
                                         size_t *text_used)
{
    MatcherArgs a;
    int rc = check_common(h, n);
    if (rc || (rc = matches_matcher(h, matcher, which, hits, &a))) return rc;
    LinesArgs la{max_lines, max_line, lines, nullptr, rec_cap, rec_used, d_text, text_cap, text_used};
    la.only_matches = true; la.line_cap = line_cap; la.matches = matches; la.match_rec = rec;
    std::vector<uint64_t> own_which; // a set without `which`: the search still computes it
    if (a.kind == Matcher::SET && !which) { own_which.resize(n + 1); which = own_which.data(); }
    return search_call_device(h, n, d_frames_base, frame_off, frame_len, raw_len, expect, a, &la, SearchOut{digest, status, count, first, which, hits});
}


// ---- repack: Decoder::read_content_frame joined to Encoder::add_data_frame without the bytes leaving HBM --------------------------
// One pass = the decode half of verify (unpack_device_once into d_vout: the same decoder, hash passes and verdict), zarc_repack_plan, the
// encode half (pack_device_impl over d_vout, planned: no hash kernel runs, entries without an OK verdict are in no launch).  d_vout is laid
// out by the decoder -- 16-byte aligned entries, ZARC_GPU_PAD and more readable behind the last -- which is what pack asks of an arena.
} // extern "C"
namespace {
// encoder scratch a pass needs at the very least: its largest frame packed alone (store mode: none)
uint64_t enc_scratch_min(const zarc_gpu *h, uint64_t max_len)
{
    return h->params.compress ? (uint64_t)enc_per_block(h->block_split != 0, enc_slot_of(max_len)) * blocks_of(max_len) : 0;
}

int repack_device_once(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len, const uint64_t *raw_len,
                       const uint8_t *expect, uint8_t *d_slots, size_t slots_cap, uint64_t *dst_off, uint64_t *dst_len, uint8_t *digest, int *status,
                       uint64_t own_bytes, uint64_t enc_min)
{
    // what the plan kernel writes is reserved in front of the decode half: nothing is reallocated between that kernel and its readers
    ZHIP(h->d_off.reserve(n * 8));
    ZHIP(h->d_len.reserve(n * 8));
    ZHIP(h->d_rp_xxh.reserve(n * 8));
    int rc = unpack_device_once(h, n, d_frames_base, frame_off, frame_len, h->d_vout.p, nullptr, raw_len, expect, digest, status, own_bytes + enc_min, nullptr,
                                &h->d_rp_order);
    if (rc) return rc;
    float dec_ms[ZARC_GPU_T_COUNT];
    for (int t = 0; t < ZARC_GPU_T_COUNT; t++) dec_ms[t] = h->ms[t];
    // the decoder's arrays (its own order) -> pack's (the caller's order).  The decoder hashes every frame it decodes, with or without a
    // stored checksum, so the XXH64 of every good entry exists: the encode half computes none
    hipLaunchKernelGGL(zarc_repack_plan, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, (uint32_t)n, h->d_rp_order.as<uint32_t>(), h->d_status.as<int32_t>(),
                       h->d_dst_off.as<uint64_t>(), h->d_raw_len.as<uint64_t>(), h->d_xxh.as<uint64_t>(), h->d_off.as<uint64_t>(), h->d_len.as<uint64_t>(),
                       h->d_rp_xxh.as<uint64_t>());
    ZHIP(hipGetLastError());
    // decoded bytes and decoder scratch stay live beside the encoder's scratch: it gets what they leave of the budget, and never less than
    // its largest frame needs (repack_device_split has halved the batch for that where it could)
    size_t enc_budget = 0;
    if (h->scratch_budget) {
        const uint64_t used = own_bytes + h->dec_scratch;
        enc_budget = (size_t)std::max<uint64_t>(std::max<uint64_t>(enc_min, 1), h->scratch_budget > used ? h->scratch_budget - used : 0);
    }
    const PackPlanned pl{h->d_rp_xxh.as<uint64_t>(), status, enc_budget};
    h->vout_busy = true;
    rc = pack_device_impl(h, n, h->d_vout.p, nullptr, raw_len, d_slots, slots_cap, dst_off, dst_len, nullptr, nullptr, /*have_digests=*/true, &pl);
    h->vout_busy = false;
    if (rc && rc != ZARC_GPU_E_CHECK) return rc;
    for (size_t i = 0; i < n; i++) if (status[i] != ZARC_GPU_FRAME_OK) dst_len[i] = 0; // no frame (a store-mode pass has written an empty one into the slot)
    const float enc_total = h->ms[ZARC_GPU_T_TOTAL];
    for (int t : {ZARC_GPU_T_BLAKE3, ZARC_GPU_T_XXH64, ZARC_GPU_T_DECODE, ZARC_GPU_T_DEC_SEQS, ZARC_GPU_T_DEC_LITS, ZARC_GPU_T_DEC_FRAMES}) h->ms[t] = dec_ms[t];
    h->ms[ZARC_GPU_T_TOTAL] = dec_ms[ZARC_GPU_T_TOTAL] + enc_total;
    return rc;
}

// A pass that does not fit -- the budget of ZARC_GPU_PX_SCRATCH_MB or the device -- runs as two, each of which may split again, the way
// unpack_device_split treats verify: halved before it is tried when decoded bytes plus the least encoder scratch exceed the budget, after
// the decoder's sizing kernels when its scratch does not fit either, after an allocation failure.  A single frame runs alone.  Frames are
// independent on both sides, so the output is the same for every budget.  slot_base: where this part's slots start in d_dst.
int repack_device_split(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len, const uint64_t *raw_len,
                        const uint8_t *expect, uint8_t *d_dst, uint64_t slot_base, uint64_t *dst_off, uint64_t *dst_len, uint8_t *digest, int *status)
{
    uint64_t total = 0, acc = 0, own_bytes = 0, max_len = 0, slots = 0;
    for (size_t i = 0; i < n; i++) {
        total += raw_len[i]; own_bytes += align_up((size_t)raw_len[i], ZARC_GPU_ALIGN); max_len = std::max(max_len, raw_len[i]); slots += zarc_gpu_bound((size_t)raw_len[i]);
    }
    const uint64_t enc_min = enc_scratch_min(h, max_len);
    int rc = UNPACK_SPLIT;
    bool attempt = !(n >= 2 && h->dec_split_above && total >= h->dec_split_above);
    if (attempt) {
        if (n >= 2 && h->scratch_budget && own_bytes + enc_min > h->scratch_budget) attempt = false;
        else {
            const hipError_t e = h->d_vout.reserve(own_bytes + ZARC_GPU_PAD + 256);
            if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); rc = ZARC_GPU_E_NOMEM; attempt = false; }
            else ZHIP(e);
        }
    }
    if (attempt) {
        rc = repack_device_once(h, n, d_frames_base, frame_off, frame_len, raw_len, expect, d_dst + slot_base, (size_t)slots, dst_off, dst_len, digest, status, own_bytes, enc_min);
        if (rc == ZARC_GPU_OK || rc == ZARC_GPU_E_CHECK) for (size_t i = 0; i < n; i++) dst_off[i] += slot_base;
    }
    if ((rc != UNPACK_SPLIT && rc != ZARC_GPU_E_NOMEM) || n < 2) return rc == UNPACK_SPLIT ? ZARC_GPU_E_NOMEM : rc;
    (void)hipStreamSynchronize(h->stream);
    if (rc == ZARC_GPU_E_NOMEM) {
        DevBuf *big[] = {&h->d_seqs, &h->d_lits, &h->d_ztables, &h->d_zblocks, &h->d_seqidx, &h->d_litidx, &h->d_nseq, &h->d_vout, &h->d_vout2, &h->d_cvs, &h->d_cvs_tmp,
                         &h->d_seq, &h->d_lit, &h->d_out, &h->d_blocks, &h->d_plan, &h->d_pblocks, &h->d_zpieces};
        for (DevBuf *b : big) b->release();
        if (!h->dec_split_above || total < h->dec_split_above) h->dec_split_above = total;
    }
    size_t k = 0;
    while (k + 1 < n && (acc + raw_len[k]) * 2 <= total) acc += raw_len[k++];
    if (k == 0) k = 1;
    float ms[ZARC_GPU_T_COUNT];
    const size_t part[3] = {0, k, n};
    for (int i = 0; i < ZARC_GPU_T_COUNT; i++) ms[i] = 0;
    for (int p = 0; p < 2; p++) {
        const size_t a = part[p], m = part[p + 1] - a;
        rc = repack_device_split(h, m, d_frames_base, frame_off + a, frame_len + a, raw_len + a, expect ? expect + a * 32 : nullptr, d_dst, slot_base, dst_off + a,
                                 dst_len + a, digest + a * 32, status + a);
        if (rc == ZARC_GPU_E_CHECK) check_message(h, a + h->chk_index);
        if (rc) return rc;
        for (size_t i = a; i < a + m; i++) slot_base += zarc_gpu_bound((size_t)raw_len[i]);
        for (int i = 0; i < ZARC_GPU_T_COUNT; i++) ms[i] += h->ms[i] > 0 ? h->ms[i] : 0;
    }
    for (int i = 0; i < ZARC_GPU_T_COUNT; i++) h->ms[i] = ms[i];
    return ZARC_GPU_OK;
}
} // namespace
extern "C" {

int zarc_gpu_repack_batch_device(zarc_gpu_t *h, size_t n, const void *d_frames_base, const uint64_t *frame_off, const uint64_t *frame_len,
                                 const uint64_t *raw_len, const uint8_t *expect, void *d_dst, size_t dst_cap, uint64_t *dst_off, uint64_t *dst_len,
                                 uint8_t *digest, int *status)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!d_frames_base || !frame_off || !frame_len || !raw_len || !d_dst || !dst_off || !dst_len || !digest || !status) return ZARC_GPU_E_PARAM;
    if ((rc = check_frame_sizes(h, n, frame_len, raw_len))) return rc;
    uint64_t need = 0;
    for (size_t i = 0; i < n; i++) need += zarc_gpu_bound((size_t)raw_len[i]);
    if (need > dst_cap) return ZARC_GPU_E_DSTSIZE;
    return repack_device_split(h, n, d_frames_base, frame_off, frame_len, raw_len, expect, (uint8_t *)d_dst, 0, dst_off, dst_len, digest, status);
}

// ---- host-memory entry points: stage through engine-owned arenas -----------------------------------
// ---- host-pointer entry points: chunked, with the PCIe copies of neighbouring chunks overlapped -----------------------
// The caller's buffers are ordinary pageable memory, so hipMemcpyAsync blocks the calling thread while it stages the
// bytes.  A helper thread therefore moves chunk c+1 in and chunk c-1 out (side stream) while this thread runs the
// kernels of chunk c (engine stream); arenas are double-buffered, which also bounds the staging memory of huge batches.
// Chunks are large (2 GiB of content for pack, 4 GiB for unpack): the kernels need thousands of frames in flight to fill the
// chip (a 1 MiB frame is a ~10 ms serial chain for one workgroup / wave), measured: 256 MiB chunks halve the throughput.
// SURVEY.md 8 row f4.
} // extern "C"
namespace {

// A byte range of the caller's memory and where it sits in a flat device range
struct Seg { uint8_t *host; uint64_t dev; uint64_t len; };

int pin_ring(zarc_gpu *h)
{
    for (int i = 0; i < zarc_gpu::PIN_SLOTS; i++) {
        if (!h->pin[i] && hipHostMalloc((void **)&h->pin[i], zarc_gpu::PIN_PIECE, 0) != hipSuccess) { h->pin[i] = nullptr; return ZARC_GPU_E_NOMEM; }
        if (!h->pin_ev[i] && hipEventCreate(&h->pin_ev[i]) != hipSuccess) return ZARC_GPU_E_DEVICE;
    }
    return 0;
}

// copy the parts of `segs` (sorted by .dev, non-overlapping) that fall into device range [lo, hi) between the caller's memory
// and `pinned` (which mirrors [lo, hi)), with several threads: the single-thread memcpy rate is far below PCIe
void piece_copy(const std::vector<Seg> &segs, size_t first_seg, uint64_t lo, uint64_t hi, uint8_t *pinned, bool to_pinned, unsigned want)
{
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 2 ? 1 : (nt > want ? want : nt);
    if (hi - lo < ((uint64_t)1 << 20)) nt = 1;
    auto work = [&](uint64_t a, uint64_t b) {
        for (size_t k = first_seg; k < segs.size() && segs[k].dev < b; k++) {
            const uint64_t s0 = std::max(segs[k].dev, a), s1 = std::min(segs[k].dev + segs[k].len, b);
            if (s0 >= s1) continue;
            if (to_pinned) memcpy(pinned + (s0 - lo), segs[k].host + (s0 - segs[k].dev), s1 - s0);
            else memcpy(segs[k].host + (s0 - segs[k].dev), pinned + (s0 - lo), s1 - s0);
        }
    };
    if (nt == 1) { work(lo, hi); return; }
    std::vector<std::thread> th;
    const uint64_t step = (hi - lo + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) {
        const uint64_t a = lo + t * step, b = std::min(hi, a + step);
        if (a < b) th.emplace_back(work, a, b);
    }
    for (auto &x : th) x.join();
}

// Is every byte of every segment page-locked host memory the device can reach (hipHostMalloc / hipHostRegister)?  Then the DMA engines
// can read and write the caller's buffers themselves and the staging ring -- one more pass of host memcpy over every byte, which is
// what bounds the pageable path at about half the link rate -- is skipped.  One attribute query per segment boundary: segments that
// follow each other in host memory share the answer of the byte between them.
bool segs_pinned(const std::vector<Seg> &segs, uint64_t min_run)
{
    if (segs.empty()) return false;
    { // A DMA per small scattered buffer loses to one pass through the ring (measured: 8192 frames of 0.5 MiB each into separate slots,
      // 26 GiB/s direct against 31 staged): go direct only when the runs that are contiguous on both sides average 4 MiB
        uint64_t bytes = 0, runs = 0;
        for (size_t k = 0; k < segs.size(); k++) {
            bytes += segs[k].len;
            if (k == 0 || segs[k].host != segs[k - 1].host + segs[k - 1].len || segs[k].dev != segs[k - 1].dev + segs[k - 1].len) runs++;
        }
        if (bytes / runs < min_run) return false;
    }
    auto pinned = [](const uint8_t *p) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; } // ordinary memory: an error, which must not stay behind as the "last error"
        return a.type == hipMemoryTypeHost;
    };
    const uint8_t *verified_end = nullptr; // one past a byte known to be pinned
    for (const Seg &sg : segs) {
        if (sg.host != verified_end && !pinned(sg.host)) return false;
        if (!pinned(sg.host + sg.len - 1)) return false;
        verified_end = sg.host + sg.len;
    }
    return true;
}

// content bytes a copy helper has moved (zarc_gpu_last_copy_bytes): the segments' own lengths, not the padding between them
inline void count_copy(zarc_gpu *h, const std::vector<Seg> &segs, bool to_device, bool direct)
{
    uint64_t bytes = 0;
    for (const Seg &sg : segs) bytes += sg.len;
    h->copy_bytes[to_device ? ZARC_GPU_C_H2D : ZARC_GPU_C_D2H].fetch_add(bytes, std::memory_order_relaxed);
    h->copy_bytes[direct ? ZARC_GPU_C_DIRECT : ZARC_GPU_C_RING].fetch_add(bytes, std::memory_order_relaxed);
}

// pinned caller memory <-> device range at `dev_base`: one asynchronous copy per run of segments that are contiguous on both sides
int direct_copy(zarc_gpu *h, hipStream_t stream, const std::vector<Seg> &segs, uint8_t *dev_base, bool to_device)
{
    size_t k = 0;
    while (k < segs.size()) {
        size_t e = k + 1;
        uint64_t len = segs[k].len;
        while (e < segs.size() && segs[e].host == segs[k].host + len && segs[e].dev == segs[k].dev + len && len + segs[e].len < ((uint64_t)1 << 31)) { len += segs[e].len; e++; }
        // A run may span two page-locked allocations that happen to be adjacent, or a buffer with an unpinned hole (segs_pinned looks at
        // the first and the last byte of a segment): the runtime may refuse such a copy.  That is no device error: the caller falls
        // back to the staging ring, which redoes the whole range (copies already queued here move the same bytes).
        const hipError_t e_ = to_device ? hipMemcpyAsync(dev_base + segs[k].dev, segs[k].host, len, hipMemcpyHostToDevice, stream)
                                        : hipMemcpyAsync(segs[k].host, dev_base + segs[k].dev, len, hipMemcpyDeviceToHost, stream);
        if (e_ != hipSuccess) { (void)hipGetLastError(); return 1; }
        k = e;
    }
    count_copy(h, segs, to_device, /*direct=*/true); // (a refused run returns above: the ring redoes the range and counts it)
    return 0;
}

// caller memory -> device range [0, total) at `dev_base`, through the pinned ring on `stream` (or straight from pinned caller memory)
int staged_h2d(zarc_gpu *h, hipStream_t stream, const std::vector<Seg> &segs, uint8_t *dev_base, uint64_t total)
{
    if (h->zero_copy && segs_pinned(segs, (uint64_t)h->zero_copy << 10) && direct_copy(h, stream, segs, dev_base, true) == 0) return 0;
    int rc = pin_ring(h);
    if (rc) return rc;
    size_t first = 0;
    int slot = 0;
    for (uint64_t lo = 0; lo < total; lo += zarc_gpu::PIN_PIECE, slot = (slot + 1) % 4) { // slots 0..3
        const uint64_t hi = std::min<uint64_t>(total, lo + zarc_gpu::PIN_PIECE);
        while (first < segs.size() && segs[first].dev + segs[first].len <= lo) first++;
        ZHIP(hipEventSynchronize(h->pin_ev[slot])); // the transfer that last used this slot is over
        piece_copy(segs, first, lo, hi, h->pin[slot], true, (unsigned)h->copy_threads);
        ZHIP(hipMemcpyAsync(dev_base + lo, h->pin[slot], hi - lo, hipMemcpyHostToDevice, stream));
        ZHIP(hipEventRecord(h->pin_ev[slot], stream));
    }
    count_copy(h, segs, true, /*direct=*/false);
    return 0;
}

// device range [0, total) at `dev_base` -> caller memory; the scatter of piece p overlaps the transfer of piece p+1
int staged_d2h(zarc_gpu *h, hipStream_t stream, const std::vector<Seg> &segs, const uint8_t *dev_base, uint64_t total)
{
    if (h->zero_copy && segs_pinned(segs, (uint64_t)h->zero_copy << 10)) { // the callers synchronise the stream before they hand the buffers back
        if (direct_copy(h, stream, segs, (uint8_t *)dev_base, false) == 0) {
            ZHIP(hipStreamSynchronize(stream));
            return 0;
        }
    }
    int rc = pin_ring(h);
    if (rc) return rc;
    struct Piece { uint64_t lo, hi; int slot; size_t first; };
    size_t first = 0;
    int slot = 4;
    bool have_prev = false;
    Piece prev{};
    for (uint64_t lo = 0; lo < total; lo += zarc_gpu::PIN_PIECE, slot = 4 + ((slot - 3) & 1)) { // slots 4 and 5 alternate
        const uint64_t hi = std::min<uint64_t>(total, lo + zarc_gpu::PIN_PIECE);
        while (first < segs.size() && segs[first].dev + segs[first].len <= lo) first++;
        ZHIP(hipMemcpyAsync(h->pin[slot], dev_base + lo, hi - lo, hipMemcpyDeviceToHost, stream));
        ZHIP(hipEventRecord(h->pin_ev[slot], stream));
        if (have_prev) { ZHIP(hipEventSynchronize(h->pin_ev[prev.slot])); piece_copy(segs, prev.first, prev.lo, prev.hi, h->pin[prev.slot], false, (unsigned)h->copy_threads); }
        prev = Piece{lo, hi, slot, first};
        have_prev = true;
    }
    if (have_prev) { ZHIP(hipEventSynchronize(h->pin_ev[prev.slot])); piece_copy(segs, prev.first, prev.lo, prev.hi, h->pin[prev.slot], false, (unsigned)h->copy_threads); }
    count_copy(h, segs, false, /*direct=*/false);
    return 0;
}

// the text of a part's matching lines, device -> the caller's host buffer (content: counted)
int lines_text_out(zarc_gpu_t *h, uint8_t *host, const uint8_t *dev, uint64_t bytes)
{
    const std::vector<Seg> segs{Seg{host, 0, bytes}};
    return staged_d2h(h, h->stream, segs, dev, bytes);
}

struct Chunk { size_t i0, i1; uint64_t in_bytes, out_bytes; };

// cut [0, n) into chunks of about STAGE_CHUNK content bytes (at least one entry each)
std::vector<Chunk> make_chunks(size_t n, const std::vector<uint64_t> &in_sz, const std::vector<uint64_t> &out_sz, const std::vector<uint64_t> &weight,
                               uint64_t STAGE_CHUNK, bool ramp = false)
{
    // ramp: the first chunk's way in and the last chunk's way out overlap nothing, so a batch of several chunks starts and ends with a
    // quarter-sized one (the kernels lose efficiency on it, the pipeline fills and drains four times sooner)
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) total += weight[i];
    ramp = ramp && total >= 3 * STAGE_CHUNK;
    const uint64_t small = STAGE_CHUNK / 4;
    std::vector<Chunk> cs;
    size_t i = 0;
    uint64_t left = total;
    while (i < n) {
        Chunk c{i, i, 0, 0};
        uint64_t w = 0, target = STAGE_CHUNK;
        if (ramp) {
            if (cs.empty()) target = small;
            else if (left <= small + small / 2) target = left;                       // the last, small chunk
            else if (left <= STAGE_CHUNK + small) target = left - small;             // the one before it leaves a quarter behind
        }
        while (c.i1 < n && (c.i1 == c.i0 || w + weight[c.i1] <= target)) { w += weight[c.i1]; c.in_bytes += in_sz[c.i1]; c.out_bytes += out_sz[c.i1]; c.i1++; }
        cs.push_back(c);
        i = c.i1;
        left -= w;
    }
    return cs;
}

} // namespace
extern "C" {

int zarc_gpu_blake3_batch(zarc_gpu_t *h, size_t n, const void *const *src, const size_t *len, uint8_t (*digest)[ZARC_GPU_DIGEST_LEN])
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!src || !len || !digest) return ZARC_GPU_E_PARAM;
    std::vector<uint64_t> off(n), l64(n);
    std::vector<Seg> segs;
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
        if (len[i] && !src[i]) return ZARC_GPU_E_PARAM;
        off[i] = total; l64[i] = len[i];
        if (len[i]) segs.push_back(Seg{(uint8_t *)src[i], total, len[i]});
        total += align_up(len[i], ZARC_GPU_ALIGN);
    }
    ZHIP(h->d_arena_in.reserve(total + ZARC_GPU_PAD + 256));
    NestedCall nested(h);
    if ((rc = staged_h2d(h, h->stream, segs, h->d_arena_in.as<uint8_t>(), total))) return rc;
    return zarc_gpu_blake3_batch_device(h, n, h->d_arena_in.p, off.data(), l64.data(), (uint8_t *)digest);
}

int zarc_gpu_pack_batch(zarc_gpu_t *h, size_t n, const void *const *src, const size_t *src_len, void *dst, size_t dst_cap, size_t *dst_off,
                        size_t *dst_len, uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status)
{
    return zarc_gpu_pack_batch_dedup(h, n, src, src_len, dst, dst_cap, dst_off, dst_len, digest, status, nullptr, nullptr);
}

int zarc_gpu_pack_batch_dedup(zarc_gpu_t *h, size_t n, const void *const *src, const size_t *src_len, void *dst, size_t dst_cap, size_t *dst_off,
                              size_t *dst_len, uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, zarc_gpu_known_fn known, void *ctx)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!src || !src_len || !dst || !dst_off || !dst_len || !digest || (known && !status)) return ZARC_GPU_E_PARAM;
    NestedCall nested(h);
    std::vector<uint64_t> in_sz(n), out_sz(n), l64(n);
    uint64_t need = 0;
    for (size_t i = 0; i < n; i++) {
        if (src_len[i] && !src[i]) return ZARC_GPU_E_PARAM;
        if ((uint64_t)src_len[i] >= 0xFFFFFFF0ull) { set_error(h, "entries of 4 GiB or more are not supported"); return ZARC_GPU_E_UNSUPPORTED; } // before any size arithmetic or staging
        l64[i] = src_len[i];
        in_sz[i] = align_up(src_len[i], ZARC_GPU_ALIGN);
        out_sz[i] = zarc_gpu_bound(src_len[i]);
        dst_off[i] = (size_t)need; // the caller's buffer uses the same slot layout as the device arena
        need += out_sz[i];
    }
    if (need > dst_cap) return ZARC_GPU_E_DSTSIZE;
    const std::vector<Chunk> cs = make_chunks(n, in_sz, out_sz, in_sz, h->stage_chunk ? h->stage_chunk : (uint64_t)2 << 30, /*ramp=*/true); // measured: 1-2 GiB chunks pack fastest (27 vs 23 GiB/s at 4 GiB)
    uint64_t max_in = 0, max_out = 0;
    for (const Chunk &c : cs) { max_in = std::max(max_in, c.in_bytes); max_out = std::max(max_out, c.out_bytes); }
    const uint64_t in_half = align_up(max_in + ZARC_GPU_PAD + 256, 256), out_half = align_up(max_out + ZARC_GPU_PAD, 256);
    ZHIP(h->d_arena_in.reserve(2 * in_half));
    ZHIP(h->d_arena_out.reserve(2 * out_half));
    uint8_t *const ain = h->d_arena_in.as<uint8_t>(), *const aout = h->d_arena_out.as<uint8_t>();
    const int device = h->device;
    hipStream_t side = h->stream_stage, side_out = h->stream_stage_out;
    std::vector<uint64_t> doff(n), dlen(n);
    auto copy_in = [&](size_t c) -> int { // entries of chunk c -> input half c & 1
        std::vector<Seg> segs;
        uint64_t at = 0;
        for (size_t i = cs[c].i0; i < cs[c].i1; i++) { if (src_len[i]) segs.push_back(Seg{(uint8_t *)src[i], at, src_len[i]}); at += in_sz[i]; }
        return staged_h2d(h, side, segs, ain + (c & 1) * in_half, at);
    };
    auto copy_out = [&](size_t c) -> int { // frames of chunk c (lengths known): packed back to back on the device, then to the caller's slots
        const size_t m = cs[c].i1 - cs[c].i0, i0 = cs[c].i0;
        std::vector<uint64_t> dense(m);
        std::vector<Seg> segs;
        uint64_t at = 0;
        for (size_t k = 0; k < m; k++) { dense[k] = at; if (dlen[i0 + k]) segs.push_back(Seg{(uint8_t *)dst + dst_off[i0 + k], at, dlen[i0 + k]}); at += dlen[i0 + k]; }
        if (h->d_dense.reserve(at + 256) != hipSuccess || h->d_goff.reserve(m * 8) != hipSuccess || h->d_glen.reserve(m * 8) != hipSuccess ||
            h->d_gdense.reserve(m * 8) != hipSuccess) return ZARC_GPU_E_NOMEM;
        if (hipMemcpyAsync(h->d_goff.p, doff.data() + i0, m * 8, hipMemcpyHostToDevice, side_out) != hipSuccess ||
            hipMemcpyAsync(h->d_glen.p, dlen.data() + i0, m * 8, hipMemcpyHostToDevice, side_out) != hipSuccess ||
            hipMemcpyAsync(h->d_gdense.p, dense.data(), m * 8, hipMemcpyHostToDevice, side_out) != hipSuccess) return ZARC_GPU_E_DEVICE;
        hipLaunchKernelGGL(zarc_gather, dim3((unsigned)m), dim3(256), 0, side_out, aout + (c & 1) * out_half, h->d_goff.as<uint64_t>(), h->d_glen.as<uint64_t>(),
                           h->d_gdense.as<uint64_t>(), (uint32_t)m, h->d_dense.as<uint8_t>());
        if (hipGetLastError() != hipSuccess) return ZARC_GPU_E_DEVICE;
        const int r = staged_d2h(h, side_out, segs, h->d_dense.as<uint8_t>(), at);
        if (hipStreamSynchronize(side_out) != hipSuccess) return ZARC_GPU_E_DEVICE; // `dense` is read by an async copy above
        return r;
    };
    float sum[ZARC_GPU_T_COUNT] = {};
    if ((rc = copy_in(0))) return rc;
    ZHIP(hipStreamSynchronize(side));
    for (size_t c = 0; c < cs.size(); c++) {
        // chunk c+1 comes in and chunk c-1 goes out while chunk c is worked on: one helper thread and one stream per direction
        int helper_rc = 0, helper_rc_out = 0;
        auto move_in = [&] {
            (void)hipSetDevice(device);
            if (c + 1 < cs.size()) helper_rc = copy_in(c + 1);
            if (hipStreamSynchronize(side) != hipSuccess) helper_rc = ZARC_GPU_E_DEVICE;
        };
        auto move_out = [&] {
            (void)hipSetDevice(device);
            if (c > 0) helper_rc_out = copy_out(c - 1);
            if (hipStreamSynchronize(side_out) != hipSuccess) helper_rc_out = ZARC_GPU_E_DEVICE;
        };
        std::thread helper, helper_out;
        if (h->stage_thread) { helper = std::thread(move_in); helper_out = std::thread(move_out); } else { move_in(); move_out(); }
        const size_t m = cs[c].i1 - cs[c].i0, i0 = cs[c].i0;
        std::vector<uint64_t> off(m);
        uint64_t at = 0;
        for (size_t k = 0; k < m; k++) { off[k] = at; at += in_sz[i0 + k]; }
        // hash first when the caller can tell known content (the chunk is resident: the digest pass costs 0.5 ms per GiB): the callback sees
        // indices of the whole batch
        struct Shift { zarc_gpu_known_fn fn; void *ctx; size_t base; } shift{known, ctx, i0};
        auto shifted = [](void *c, const uint8_t *d, size_t i) -> int { Shift *s = (Shift *)c; return s->fn(s->ctx, d, s->base + i); };
        rc = pack_device_dedup_impl(h, m, ain + (c & 1) * in_half, off.data(), l64.data() + i0, aout + (c & 1) * out_half, cs[c].out_bytes, doff.data() + i0,
                                    dlen.data() + i0, (uint8_t *)digest[i0], status ? status + i0 : nullptr, known ? (zarc_gpu_known_fn)shifted : nullptr, &shift);
        if (helper.joinable()) helper.join();
        if (helper_out.joinable()) helper_out.join();
        if (rc == ZARC_GPU_E_CHECK) { // the batch's output is void: say which entry of the batch it was
            for (size_t k = 0; k < m; k++) dst_len[i0 + k] = (size_t)dlen[i0 + k];
            check_message(h, i0 + h->chk_index);
        }
        if (rc) return rc;
        if (helper_rc) return helper_rc;
        if (helper_rc_out) return helper_rc_out;
        for (size_t k = 0; k < m; k++) dst_len[i0 + k] = (size_t)dlen[i0 + k];
        for (int t = 0; t < ZARC_GPU_T_COUNT; t++) sum[t] += h->ms[t] > 0 ? h->ms[t] : 0;
    }
    if ((rc = copy_out(cs.size() - 1))) return rc;
    ZHIP(hipStreamSynchronize(side_out));
    for (int t = 0; t < ZARC_GPU_T_COUNT; t++) h->ms[t] = sum[t];
    return ZARC_GPU_OK;
}

int zarc_gpu_unpack_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len, void *const *dst,
                          const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!frame || !frame_len || !raw_len || !dst || !digest || !status) return ZARC_GPU_E_PARAM;
    NestedCall nested(h);
    std::vector<uint64_t> in_sz(n), out_sz(n), weight(n), flen(n), rlen(n);
    for (size_t i = 0; i < n; i++) {
        if ((frame_len[i] && !frame[i]) || (raw_len[i] && !dst[i])) return ZARC_GPU_E_PARAM;
        if ((uint64_t)frame_len[i] >= 0xFFFFFFF0ull || (uint64_t)raw_len[i] >= 0xFFFFFFF0ull) { set_error(h, "frames of 4 GiB or more are not supported"); return ZARC_GPU_E_UNSUPPORTED; } // before any size arithmetic or staging
        flen[i] = frame_len[i]; rlen[i] = raw_len[i];
        in_sz[i] = align_up(frame_len[i], ZARC_GPU_ALIGN);
        out_sz[i] = align_up(raw_len[i], ZARC_GPU_ALIGN);
        weight[i] = std::max(in_sz[i], out_sz[i]);
    }
    const std::vector<Chunk> cs = make_chunks(n, in_sz, out_sz, weight, h->stage_chunk ? h->stage_chunk : (uint64_t)4 << 30); // the decoder's lane-per-block stage wants many frames at once
    uint64_t max_in = 0, max_out = 0;
    for (const Chunk &c : cs) { max_in = std::max(max_in, c.in_bytes); max_out = std::max(max_out, c.out_bytes); }
    const uint64_t in_half = align_up(max_in + ZARC_GPU_PAD + 256, 256), out_half = align_up(max_out + ZARC_GPU_PAD + 256, 256);
    ZHIP(h->d_arena_in.reserve(2 * in_half));
    ZHIP(h->d_arena_out.reserve(2 * out_half));
    uint8_t *const ain = h->d_arena_in.as<uint8_t>(), *const aout = h->d_arena_out.as<uint8_t>();
    const int device = h->device;
    hipStream_t side = h->stream_stage, side_out = h->stream_stage_out;
    auto copy_in = [&](size_t c) -> int {
        std::vector<Seg> segs;
        uint64_t at = 0;
        for (size_t i = cs[c].i0; i < cs[c].i1; i++) { if (frame_len[i]) segs.push_back(Seg{(uint8_t *)frame[i], at, frame_len[i]}); at += in_sz[i]; }
        return staged_h2d(h, side, segs, ain + (c & 1) * in_half, at);
    };
    auto copy_out = [&](size_t c) -> int {
        std::vector<Seg> segs;
        uint64_t at = 0;
        for (size_t i = cs[c].i0; i < cs[c].i1; i++) {
            // like the reference, bytes are delivered unless the frame itself failed to decode
            const bool decoded = status[i] == ZARC_GPU_FRAME_OK || status[i] == ZARC_GPU_FRAME_DIGEST || status[i] == ZARC_GPU_FRAME_CHECKSUM;
            if (decoded && raw_len[i]) segs.push_back(Seg{(uint8_t *)dst[i], at, raw_len[i]});
            at += out_sz[i];
        }
        return staged_d2h(h, side_out, segs, aout + (c & 1) * out_half, at);
    };
    float sum[ZARC_GPU_T_COUNT] = {};
    if ((rc = copy_in(0))) return rc;
    ZHIP(hipStreamSynchronize(side));
    for (size_t c = 0; c < cs.size(); c++) {
        // chunk c+1 comes in and chunk c-1 goes out while chunk c is worked on: one helper thread and one stream per direction
        int helper_rc = 0, helper_rc_out = 0;
        auto move_in = [&] {
            (void)hipSetDevice(device);
            if (c + 1 < cs.size()) helper_rc = copy_in(c + 1);
            if (hipStreamSynchronize(side) != hipSuccess) helper_rc = ZARC_GPU_E_DEVICE;
        };
        auto move_out = [&] {
            (void)hipSetDevice(device);
            if (c > 0) helper_rc_out = copy_out(c - 1);
            if (hipStreamSynchronize(side_out) != hipSuccess) helper_rc_out = ZARC_GPU_E_DEVICE;
        };
        std::thread helper, helper_out;
        if (h->stage_thread) { helper = std::thread(move_in); helper_out = std::thread(move_out); } else { move_in(); move_out(); }
        const size_t m = cs[c].i1 - cs[c].i0, i0 = cs[c].i0;
        std::vector<uint64_t> foff(m), doff(m);
        uint64_t fa = 0, da = 0;
        for (size_t k = 0; k < m; k++) { foff[k] = fa; fa += in_sz[i0 + k]; doff[k] = da; da += out_sz[i0 + k]; }
        rc = zarc_gpu_unpack_batch_device(h, m, ain + (c & 1) * in_half, foff.data(), flen.data() + i0, aout + (c & 1) * out_half, doff.data(), rlen.data() + i0,
                                          expect ? (const uint8_t *)expect[i0] : nullptr, (uint8_t *)digest[i0], status + i0);
        if (helper.joinable()) helper.join();
        if (helper_out.joinable()) helper_out.join();
        if (rc) return rc;
        if (helper_rc) return helper_rc;
        if (helper_rc_out) return helper_rc_out;
        for (int t = 0; t < ZARC_GPU_T_COUNT; t++) sum[t] += h->ms[t] > 0 ? h->ms[t] : 0;
    }
    if ((rc = copy_out(cs.size() - 1))) return rc;
    ZHIP(hipStreamSynchronize(side_out));
    for (int t = 0; t < ZARC_GPU_T_COUNT; t++) h->ms[t] = sum[t];
    return ZARC_GPU_OK;
}

// The chunk loop of zarc_gpu_unpack_batch without its outbound half: chunk c+1's frames come in while chunk c is decoded and judged;
// nothing but statuses and digests goes back.  A chunk's decoded bytes live in the handle's scratch (unpack_device_split), so the
// chunks are cut by the same weight as unpack's.
// With a search request every chunk is searched as well (the matcher is on the device already: search_prepare), its results go back too,
// and a set's chunks add to the call's hits.
} // extern "C"
namespace {
int verify_host_impl(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                     const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, const SearchReq *srch, const RangeReq *rng = nullptr,
                     const WcReq *wc = nullptr, const CmpHost *cmp = nullptr)
{
    int rc = 0;
    if (!frame || !frame_len || !raw_len || !digest || !status) return ZARC_GPU_E_PARAM;
    NestedCall nested(h);
    if ((rc = check_frame_sizes(h, n, frame_len, raw_len, frame))) return rc;
    std::vector<uint64_t> in_sz(n), out_sz(n), weight(n), flen(n), rlen(n), olen, oth_sz, up_sz;
    for (size_t i = 0; i < n; i++) {
        flen[i] = frame_len[i]; rlen[i] = raw_len[i];
        in_sz[i] = align_up(frame_len[i], ZARC_GPU_ALIGN);
        out_sz[i] = align_up(raw_len[i], ZARC_GPU_ALIGN);
        weight[i] = std::max(in_sz[i], out_sz[i]);
    }
    if (cmp) { // the second staged stream: a chunk's other sides lie in the input arena behind the chunk's frames
        olen.resize(n); oth_sz.resize(n); up_sz.resize(n);
        for (size_t i = 0; i < n; i++) {
            olen[i] = cmp->other_len[i];
            oth_sz[i] = align_up(cmp->other_len[i], ZARC_GPU_ALIGN);
            up_sz[i] = in_sz[i] + oth_sz[i];
            weight[i] = std::max(weight[i], oth_sz[i]);
        }
    }
    const std::vector<Chunk> cs = make_chunks(n, cmp ? up_sz : in_sz, out_sz, weight, h->stage_chunk ? h->stage_chunk : (uint64_t)4 << 30);
    uint64_t max_in = 0;
    for (const Chunk &c : cs) max_in = std::max(max_in, c.in_bytes);
    const uint64_t in_half = align_up(max_in + ZARC_GPU_PAD + 256, 256);
    ZHIP(h->d_arena_in.reserve(2 * in_half));
    uint8_t *const ain = h->d_arena_in.as<uint8_t>();
    const int device = h->device;
    hipStream_t side = h->stream_stage;
    auto copy_in = [&](size_t c) -> int {
        std::vector<Seg> segs;
        uint64_t at = 0;
        for (size_t i = cs[c].i0; i < cs[c].i1; i++) { if (frame_len[i]) segs.push_back(Seg{(uint8_t *)frame[i], at, frame_len[i]}); at += in_sz[i]; }
        if (cmp) for (size_t i = cs[c].i0; i < cs[c].i1; i++) { if (olen[i]) segs.push_back(Seg{(uint8_t *)cmp->other[i], at, olen[i]}); at += oth_sz[i]; }
        return staged_h2d(h, side, segs, ain + (c & 1) * in_half, at);
    };
    float sum[ZARC_GPU_T_COUNT] = {}, cmp_sum = 0;
    if ((rc = copy_in(0))) return rc;
    ZHIP(hipStreamSynchronize(side));
    for (size_t c = 0; c < cs.size(); c++) {
        int helper_rc = 0;
        auto move_in = [&] {
            (void)hipSetDevice(device);
            if (c + 1 < cs.size()) helper_rc = copy_in(c + 1);
            if (hipStreamSynchronize(side) != hipSuccess) helper_rc = ZARC_GPU_E_DEVICE;
        };
        std::thread helper;
        if (h->stage_thread) helper = std::thread(move_in); else move_in();
        const size_t m = cs[c].i1 - cs[c].i0, i0 = cs[c].i0;
        std::vector<uint64_t> foff(m);
        uint64_t fa = 0;
        for (size_t k = 0; k < m; k++) { foff[k] = fa; fa += in_sz[i0 + k]; }
        // every chunk is a batch call of its own to the clocks and the descriptor arena; the copy counters are the whole call's (NestedCall).
        // The chunks are ranges of the caller's frames in the caller's order: the running remainder of rec_cap goes from one to the next
        const SearchReq sub = srch ? part_of(*srch, i0) : SearchReq{};
        const RangeReq rsub = rng ? part_of(*rng, i0) : RangeReq{};
        const WcReq wsub = wc ? part_of(*wc, i0) : WcReq{};
        std::vector<uint64_t> ooff;
        CmpReq csub{};
        if (cmp) { // (fa: where the chunk's frames end)
            ooff.resize(m);
            for (size_t k = 0; k < m; k++) { ooff[k] = fa; fa += oth_sz[i0 + k]; }
            csub = CmpReq{ain + (c & 1) * in_half, ooff.data(), olen.data() + i0, cmp->res + i0, true};
        }
        if (!(rc = check_common(h, m)))
            rc = unpack_device_split(h, m, ain + (c & 1) * in_half, foff.data(), flen.data() + i0, nullptr, nullptr, rlen.data() + i0,
                                     expect ? (const uint8_t *)expect[i0] : nullptr, (uint8_t *)digest[i0], status + i0, nullptr, srch ? &sub : nullptr, rng ? &rsub : nullptr,
                                     wc ? &wsub : nullptr, cmp ? &csub : nullptr);
        if (helper.joinable()) helper.join();
        if (rc) return rc;
        if (helper_rc) return helper_rc;
        for (int t = 0; t < ZARC_GPU_T_COUNT; t++) sum[t] += h->ms[t] > 0 ? h->ms[t] : 0;
        cmp_sum += h->cmp_ms > 0 ? h->cmp_ms : 0;
    }
    for (int t = 0; t < ZARC_GPU_T_COUNT; t++) h->ms[t] = sum[t];
    if (cmp) h->cmp_ms = cmp_sum;
    return ZARC_GPU_OK;
}

// The six host forms: verify's chunk loop with the search behind every chunk's verdict.  The compressed bytes go up; 52 bytes per frame come
// back (a set: 60, and the hits), and with lines the matching lines' bytes.
int search_call_host(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len, const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN],
                     const MatcherArgs &a, const LinesArgs *la, const SearchOut &out)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    SearchReq req;
    LinesRun run;
    if ((rc = search_prepare(h, n, a, out, la, /*host_text=*/true, &run, &req))) return rc;
    if (n == 0) return ZARC_GPU_OK;
    rc = verify_host_impl(h, n, frame, frame_len, raw_len, expect, (uint8_t (*)[ZARC_GPU_DIGEST_LEN])out.digest, out.status, &req);
    if (la) { *la->rec_used = la->only_matches ? run.match_used : run.rec_used; *la->text_used = (size_t)run.text_used; }
    return rc;
}
} // namespace
extern "C" {

int zarc_gpu_verify_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                          const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    return verify_host_impl(h, n, frame, frame_len, raw_len, expect, digest, status, nullptr);
}
// verify's chunk loop with the range kernels behind every chunk's verdict: the compressed bytes go up, the ranges' bytes come back
int zarc_gpu_read_ranges_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                               const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], const zarc_gpu_range *range, uint64_t max_bytes,
                               uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, zarc_gpu_range_result *res, void *text, size_t text_cap, size_t *text_used)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) { if (text_used) *text_used = 0; return ZARC_GPU_OK; }
    if (!frame || !frame_len || !raw_len || !digest || !status) return ZARC_GPU_E_PARAM;
    RangeReq req;
    RangeRun run;
    if ((rc = range_prepare(h, n, range, max_bytes, res, text, text_cap, text_used, /*host_text=*/true, &run, &req))) return rc;
    rc = verify_host_impl(h, n, frame, frame_len, raw_len, expect, digest, status, nullptr, &req);
    *text_used = (size_t)run.text_used;
    return rc;
}
// verify's chunk loop with the count kernels behind every chunk's verdict: the compressed bytes go up, 64 bytes a frame come back
int zarc_gpu_count_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                         const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, zarc_gpu_wc *res)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!frame || !frame_len || !raw_len || !digest || !status) return ZARC_GPU_E_PARAM;
    if (!res) { set_error(h, "count: res is needed"); return ZARC_GPU_E_PARAM; }
    const WcReq req{res};
    return verify_host_impl(h, n, frame, frame_len, raw_len, expect, digest, status, nullptr, nullptr, &req);
}
// verify's chunk loop with the compare kernels behind every chunk's verdict: the compressed bytes and the other sides go up, 64 bytes a
// pair come back
int zarc_gpu_compare_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                           const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], const void *const *other, const size_t *other_len,
                           uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, zarc_gpu_cmp *res)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!frame || !frame_len || !raw_len || !digest || !status) return ZARC_GPU_E_PARAM;
    if ((rc = check_frame_sizes(h, n, frame_len, raw_len, frame))) return rc;
    if (!res || !other || !other_len) { set_error(h, "compare: res, other and other_len are needed"); return ZARC_GPU_E_PARAM; }
    for (size_t i = 0; i < n; i++) {
        if (other_len[i] && !other[i]) { set_error(h, "compare: an other side with bytes has no address"); return ZARC_GPU_E_PARAM; }
        if ((uint64_t)other_len[i] >= 0xFFFFFFF0ull) { set_error(h, "compare: other sides of 4 GiB or more are not supported"); return ZARC_GPU_E_UNSUPPORTED; }
    }
    const CmpHost req{other, other_len, res};
    return verify_host_impl(h, n, frame, frame_len, raw_len, expect, digest, status, nullptr, nullptr, nullptr, &req);
}
int zarc_gpu_search_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                          const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], const void *pattern, size_t pattern_len, unsigned flags,
                          uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first)
{
    return search_call_host(h, n, frame, frame_len, raw_len, expect, MatcherArgs{Matcher::PATTERN, pattern, pattern_len, nullptr, flags}, nullptr,
                            SearchOut{(uint8_t *)digest, status, count, first, nullptr, nullptr});
}
int zarc_gpu_search_lines_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], const void *pattern, size_t pattern_len, unsigned flags, uint64_t max_lines,
                                uint64_t max_line, uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first, uint64_t *lines,
                                zarc_gpu_line *rec, size_t rec_cap, size_t *rec_used, void *text, size_t text_cap, size_t *text_used)
{
    const LinesArgs la{max_lines, max_line, lines, rec, rec_cap, rec_used, text, text_cap, text_used};
    return search_call_host(h, n, frame, frame_len, raw_len, expect, MatcherArgs{Matcher::PATTERN, pattern, pattern_len, nullptr, flags}, &la,
                            SearchOut{(uint8_t *)digest, status, count, first, nullptr, nullptr});
}
int zarc_gpu_search_set_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                              const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], const zarc_gpu_pattern_set *set, unsigned flags,
                              uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first, uint64_t *which, uint64_t *hits)
{
    return search_call_host(h, n, frame, frame_len, raw_len, expect, MatcherArgs{Matcher::SET, nullptr, 0, set, flags}, nullptr,
                            SearchOut{(uint8_t *)digest, status, count, first, which, hits});
}
int zarc_gpu_search_set_lines_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                    const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], const zarc_gpu_pattern_set *set, unsigned flags, uint64_t max_lines,
                                    uint64_t max_line, uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first,
                                    uint64_t *which, uint64_t *hits, uint64_t *lines, zarc_gpu_line *rec, size_t rec_cap, size_t *rec_used, void *text,
                                    size_t text_cap, size_t *text_used)
{
    const LinesArgs la{max_lines, max_line, lines, rec, rec_cap, rec_used, text, text_cap, text_used};
    return search_call_host(h, n, frame, frame_len, raw_len, expect, MatcherArgs{Matcher::SET, nullptr, 0, set, flags}, &la,
                            SearchOut{(uint8_t *)digest, status, count, first, which, hits});
}
int zarc_gpu_search_regex_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], const void *regex, size_t regex_len, unsigned flags,
                                uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first)
{
    return search_call_host(h, n, frame, frame_len, raw_len, expect, MatcherArgs{Matcher::REGEX, regex, regex_len, nullptr, flags}, nullptr,
                            SearchOut{(uint8_t *)digest, status, count, first, nullptr, nullptr});
}
int zarc_gpu_search_regex_lines_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                      const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], const void *regex, size_t regex_len, unsigned flags, uint64_t max_lines,
                                      uint64_t max_line, uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first,
                                      uint64_t *lines, zarc_gpu_line *rec, size_t rec_cap, size_t *rec_used, void *text, size_t text_cap, size_t *text_used)
{
    const LinesArgs la{max_lines, max_line, lines, rec, rec_cap, rec_used, text, text_cap, text_used};
    return search_call_host(h, n, frame, frame_len, raw_len, expect, MatcherArgs{Matcher::REGEX, regex, regex_len, nullptr, flags}, &la,
                            SearchOut{(uint8_t *)digest, status, count, first, nullptr, nullptr});
}

int zarc_gpu_select_lines_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], const zarc_gpu_matcher *matcher, const zarc_gpu_line_select *select,
                                uint64_t max_lines, uint64_t max_line, uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first,
                                uint64_t *which, uint64_t *hits, uint64_t *lines, uint64_t *selected, zarc_gpu_line *rec, size_t rec_cap, size_t *rec_used,
                                void *text, size_t text_cap, size_t *text_used)
{
    MatcherArgs a;
    int rc = check_common(h, n);
    if (rc || (rc = select_matcher(h, matcher, select, which, hits, &a))) return rc;
    LinesArgs la{max_lines, max_line, lines, rec, rec_cap, rec_used, text, text_cap, text_used};
    la.select = select; la.selected = selected;
    std::vector<uint64_t> own_which; // a set without `which`: the search still computes it
    if (a.kind == Matcher::SET && !which) { own_which.resize(n + 1); which = own_which.data(); }
    return search_call_host(h, n, frame, frame_len, raw_len, expect, a, &la, SearchOut{(uint8_t *)digest, status, count, first, which, hits});
}

int zarc_gpu_search_matches_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                                  const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], const zarc_gpu_matcher *matcher, uint64_t max_lines, uint64_t max_line, size_t line_cap,
                                  uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status, uint64_t *count, uint64_t *first, uint64_t *which, uint64_t *hits,
                                  uint64_t *lines, uint64_t *matches, zarc_gpu_match *rec, size_t rec_cap, size_t *rec_used, void *text, size_t text_cap,
                                  size_t *text_used)
{
    MatcherArgs a;
    int rc = check_common(h, n);
    if (rc || (rc = matches_matcher(h, matcher, which, hits, &a))) return rc;
    LinesArgs la{max_lines, max_line, lines, nullptr, rec_cap, rec_used, text, text_cap, text_used};
    la.only_matches = true; la.line_cap = line_cap; la.matches = matches; la.match_rec = rec;
    std::vector<uint64_t> own_which; // a set without `which`: the search still computes it
    if (a.kind == Matcher::SET && !which) { own_which.resize(n + 1); which = own_which.data(); }
    return search_call_host(h, n, frame, frame_len, raw_len, expect, a, &la, SearchOut{(uint8_t *)digest, status, count, first, which, hits});
}

// verify's way in and pack's way out around zarc_gpu_repack_batch_device, per staged chunk: chunk c+1's frames come in and chunk c-1's
// new frames go out while chunk c is decoded and encoded.  Nothing else of content moves: the decoded bytes stay in the handle's scratch.
int zarc_gpu_repack_batch(zarc_gpu_t *h, size_t n, const void *const *frame, const size_t *frame_len, const size_t *raw_len,
                          const uint8_t (*expect)[ZARC_GPU_DIGEST_LEN], void *dst, size_t dst_cap, size_t *dst_off, size_t *dst_len,
                          uint8_t (*digest)[ZARC_GPU_DIGEST_LEN], int *status)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!frame || !frame_len || !raw_len || !dst || !dst_off || !dst_len || !digest || !status) return ZARC_GPU_E_PARAM;
    NestedCall nested(h);
    if ((rc = check_frame_sizes(h, n, frame_len, raw_len, frame))) return rc;
    std::vector<uint64_t> in_sz(n), out_sz(n), weight(n), flen(n), rlen(n);
    uint64_t need = 0;
    for (size_t i = 0; i < n; i++) {
        flen[i] = frame_len[i]; rlen[i] = raw_len[i];
        in_sz[i] = align_up(frame_len[i], ZARC_GPU_ALIGN);
        out_sz[i] = zarc_gpu_bound(raw_len[i]);
        weight[i] = std::max<uint64_t>(in_sz[i], align_up(raw_len[i], ZARC_GPU_ALIGN)); // a chunk is cut by what the kernels work on: the decoded bytes
        dst_off[i] = (size_t)need; // the caller's buffer uses the same slot layout as the device arena
        need += out_sz[i];
    }
    if (need > dst_cap) return ZARC_GPU_E_DSTSIZE;
    const std::vector<Chunk> cs = make_chunks(n, in_sz, out_sz, weight, h->stage_chunk ? h->stage_chunk : (uint64_t)2 << 30, /*ramp=*/true); // the encode half is the slow one: pack's chunks
    uint64_t max_in = 0, max_out = 0;
    for (const Chunk &c : cs) { max_in = std::max(max_in, c.in_bytes); max_out = std::max(max_out, c.out_bytes); }
    const uint64_t in_half = align_up(max_in + ZARC_GPU_PAD + 256, 256), out_half = align_up(max_out + ZARC_GPU_PAD, 256);
    ZHIP(h->d_arena_in.reserve(2 * in_half));
    ZHIP(h->d_arena_out.reserve(2 * out_half));
    uint8_t *const ain = h->d_arena_in.as<uint8_t>(), *const aout = h->d_arena_out.as<uint8_t>();
    const int device = h->device;
    hipStream_t side = h->stream_stage, side_out = h->stream_stage_out;
    std::vector<uint64_t> doff(n), dlen(n);
    auto copy_in = [&](size_t c) -> int {
        std::vector<Seg> segs;
        uint64_t at = 0;
        for (size_t i = cs[c].i0; i < cs[c].i1; i++) { if (frame_len[i]) segs.push_back(Seg{(uint8_t *)frame[i], at, frame_len[i]}); at += in_sz[i]; }
        return staged_h2d(h, side, segs, ain + (c & 1) * in_half, at);
    };
    auto copy_out = [&](size_t c) -> int { // new frames of chunk c (lengths known): packed back to back on the device, then to the caller's slots
        const size_t m = cs[c].i1 - cs[c].i0, i0 = cs[c].i0;
        std::vector<uint64_t> dense(m);
        std::vector<Seg> segs;
        uint64_t at = 0;
        for (size_t k = 0; k < m; k++) { dense[k] = at; if (dlen[i0 + k]) segs.push_back(Seg{(uint8_t *)dst + dst_off[i0 + k], at, dlen[i0 + k]}); at += dlen[i0 + k]; }
        if (h->d_dense.reserve(at + 256) != hipSuccess || h->d_goff.reserve(m * 8) != hipSuccess || h->d_glen.reserve(m * 8) != hipSuccess ||
            h->d_gdense.reserve(m * 8) != hipSuccess) return ZARC_GPU_E_NOMEM;
        if (hipMemcpyAsync(h->d_goff.p, doff.data() + i0, m * 8, hipMemcpyHostToDevice, side_out) != hipSuccess ||
            hipMemcpyAsync(h->d_glen.p, dlen.data() + i0, m * 8, hipMemcpyHostToDevice, side_out) != hipSuccess ||
            hipMemcpyAsync(h->d_gdense.p, dense.data(), m * 8, hipMemcpyHostToDevice, side_out) != hipSuccess) return ZARC_GPU_E_DEVICE;
        hipLaunchKernelGGL(zarc_gather, dim3((unsigned)m), dim3(256), 0, side_out, aout + (c & 1) * out_half, h->d_goff.as<uint64_t>(), h->d_glen.as<uint64_t>(),
                           h->d_gdense.as<uint64_t>(), (uint32_t)m, h->d_dense.as<uint8_t>());
        if (hipGetLastError() != hipSuccess) return ZARC_GPU_E_DEVICE;
        const int r = staged_d2h(h, side_out, segs, h->d_dense.as<uint8_t>(), at);
        if (hipStreamSynchronize(side_out) != hipSuccess) return ZARC_GPU_E_DEVICE; // `dense` is read by an async copy above
        return r;
    };
    float sum[ZARC_GPU_T_COUNT] = {};
    if ((rc = copy_in(0))) return rc;
    ZHIP(hipStreamSynchronize(side));
    for (size_t c = 0; c < cs.size(); c++) {
        int helper_rc = 0, helper_rc_out = 0;
        auto move_in = [&] {
            (void)hipSetDevice(device);
            if (c + 1 < cs.size()) helper_rc = copy_in(c + 1);
            if (hipStreamSynchronize(side) != hipSuccess) helper_rc = ZARC_GPU_E_DEVICE;
        };
        auto move_out = [&] {
            (void)hipSetDevice(device);
            if (c > 0) helper_rc_out = copy_out(c - 1);
            if (hipStreamSynchronize(side_out) != hipSuccess) helper_rc_out = ZARC_GPU_E_DEVICE;
        };
        std::thread helper, helper_out;
        if (h->stage_thread) { helper = std::thread(move_in); helper_out = std::thread(move_out); } else { move_in(); move_out(); }
        const size_t m = cs[c].i1 - cs[c].i0, i0 = cs[c].i0;
        std::vector<uint64_t> foff(m);
        uint64_t fa = 0;
        for (size_t k = 0; k < m; k++) { foff[k] = fa; fa += in_sz[i0 + k]; }
        rc = zarc_gpu_repack_batch_device(h, m, ain + (c & 1) * in_half, foff.data(), flen.data() + i0, rlen.data() + i0, expect ? (const uint8_t *)expect[i0] : nullptr,
                                          aout + (c & 1) * out_half, cs[c].out_bytes, doff.data() + i0, dlen.data() + i0, (uint8_t *)digest[i0], status + i0);
        if (helper.joinable()) helper.join();
        if (helper_out.joinable()) helper_out.join();
        if (rc == ZARC_GPU_E_CHECK) { // the batch's output is void: say which frame of the batch it was
            for (size_t k = 0; k < m; k++) dst_len[i0 + k] = (size_t)dlen[i0 + k];
            check_message(h, i0 + h->chk_index);
        }
        if (rc) return rc;
        if (helper_rc) return helper_rc;
        if (helper_rc_out) return helper_rc_out;
        for (size_t k = 0; k < m; k++) dst_len[i0 + k] = (size_t)dlen[i0 + k];
        for (int t = 0; t < ZARC_GPU_T_COUNT; t++) sum[t] += h->ms[t] > 0 ? h->ms[t] : 0;
    }
    if ((rc = copy_out(cs.size() - 1))) return rc;
    ZHIP(hipStreamSynchronize(side_out));
    for (int t = 0; t < ZARC_GPU_T_COUNT; t++) h->ms[t] = sum[t];
    return ZARC_GPU_OK;
}

// ---- bench / test utilities ---------------------------------------------------------------------------
int zarc_gpu_corpus_fill_device(zarc_gpu_t *h, size_t n, void *d_base, const uint64_t *off, const uint64_t *len, uint64_t first_index, int kind)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (n == 0) return ZARC_GPU_OK;
    if (!d_base || !off || !len) return ZARC_GPU_E_PARAM;
    if ((rc = upload_u64(h, h->d_off, off, n))) return rc;
    if ((rc = upload_u64(h, h->d_len, len, n))) return rc;
    hipLaunchKernelGGL(zarc_corpus_fill, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, (uint8_t *)d_base, h->d_off.as<uint64_t>(),
                       h->d_len.as<uint64_t>(), (uint32_t)n, first_index, kind);
    ZHIP(hipGetLastError());
    ZHIP(hipStreamSynchronize(h->stream));
    return ZARC_GPU_OK;
}
int zarc_gpu_device_malloc(zarc_gpu_t *h, void **d_ptr, size_t bytes)
{
    if (!h || !d_ptr) return ZARC_GPU_E_PARAM;
    ZHIP(hipSetDevice(h->device));
    ZHIP(hipMalloc(d_ptr, bytes ? bytes : 1));
    return ZARC_GPU_OK;
}
int zarc_gpu_device_free(zarc_gpu_t *h, void *d_ptr)
{
    if (!h) return ZARC_GPU_E_PARAM;
    ZHIP(hipSetDevice(h->device));
    ZHIP(hipFree(d_ptr));
    return ZARC_GPU_OK;
}
int zarc_gpu_memcpy_h2d(zarc_gpu_t *h, void *d_dst, const void *src, size_t bytes)
{
    if (!h) return ZARC_GPU_E_PARAM;
    ZHIP(hipSetDevice(h->device));
    ZHIP(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return ZARC_GPU_OK;
}
int zarc_gpu_memcpy_d2h(zarc_gpu_t *h, void *dst, const void *d_src, size_t bytes)
{
    if (!h) return ZARC_GPU_E_PARAM;
    ZHIP(hipSetDevice(h->device));
    ZHIP(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return ZARC_GPU_OK;
}

} // extern "C"
