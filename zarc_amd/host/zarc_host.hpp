// zarc_amd/host/zarc_host.hpp -- host-side mirror of the reference's library API for the content path,
// written above the C ABI (include/zarc_gpu.h).  The reference is Rust (no rustc/cargo on the build image), so
// this is the C++ stand-in for what a patched `crates/zarc` would do around the FFI calls; names, argument
// meaning and error behaviour follow the reference:
//
//   zarc::Encoder            crates/zarc/src/encode.rs:27-97 (struct + new/set_zstd_parameter/enable_compression)
//   Encoder::add_data_frame  crates/zarc/src/encode/content_frame.rs:20-60 (hash + compress -> dedup -> Frame record)
//   zarc::Frame              crates/zarc/src/directory/frame.rs:10-32
//   zarc::Digest             crates/zarc/src/integrity.rs:14-36 (constant-time equality :17-22)
//   zarc::FrameReader        crates/zarc/src/decode/frame_iterator.rs:14-104 (read_content_frame + verify)
//   Encoder::repack_frames   read_content_frame joined to add_data_frame on the device (zarc_gpu_repack_batch): the frames of another
//                            archive become frames of this one without their content passing through host memory
//
// What differs, on purpose: the engine is batched, so `add_data_frames` takes many entries at once (frames
// are independent: a fresh session per frame, content_frame.rs:37-39).  Call order is preserved: frame order
// = call order, first occurrence of a digest wins, later duplicates write nothing (content_frame.rs:30-33),
// offsets are running sums starting at 12 (encode.rs:65,75).  Unlike the reference, writes use write-all
// semantics (the reference's `writer.write` can short-write, lowlevel_frames.rs:38 -- SURVEY quirk 1).
// The archive directory / trailer (`add_file_entry`, `finalise`, `open`) live in zarc_container.hpp.
//
// Several GPUs: frames are independent, so an Encoder constructed with G devices deals the entries of a
// batch to G engine handles (`shard_assign`: index mod G when all sizes are equal, largest-first onto the least loaded device
// otherwise), packs the shares concurrently (one host thread per handle, no collective, nothing crosses between devices) and
// then does in ORIGINAL index order exactly what the single-device path does: running offsets and first-wins dedup.  The
// archive is byte-identical to the single-device one.
#pragma once
#include "../../include/zarc_gpu.h"
#include <cstdlib>
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <optional>
#include <ostream>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace zarc {

// header.rs:35-40: skippable-frame magic 0x184D2A50, length 4, ZARC_MAGIC 65 AA DC, version 1
static const uint8_t FILE_MAGIC[12] = {0x50, 0x2A, 0x4D, 0x18, 0x04, 0x00, 0x00, 0x00, 0x65, 0xAA, 0xDC, 0x01};

struct Digest {
    std::array<uint8_t, 32> bytes{};
    // constant-time equality (integrity.rs:17-22 uses subtle::ConstantTimeEq)
    bool operator==(const Digest &o) const
    {
        uint8_t d = 0;
        for (size_t i = 0; i < 32; i++) d |= (uint8_t)(bytes[i] ^ o.bytes[i]);
        return d == 0;
    }
    bool operator<(const Digest &o) const { return std::memcmp(bytes.data(), o.bytes.data(), 32) < 0; } // map key only
};

struct Frame { // directory/frame.rs:12-32
    uint16_t edition = 1;
    uint64_t offset = 0;
    Digest digest;
    uint64_t length = 0;       // compressed bytes in the archive
    uint64_t uncompressed = 0;
};

struct Error : std::runtime_error { // lib.rs:27-30: io::Error::other(ZSTD_getErrorName(code))
    int code;
    Error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

class Engine { // CCtx/DCtx analogue: one per Encoder / reader (encode.rs:60-62, zstd_iterator.rs:29)
  public:
    explicit Engine(int device = 0)
    {
        int rc = zarc_gpu_create(&h_, device);
        if (rc != ZARC_GPU_OK) throw Error(rc, "failed allocating zstd context"); // encode.rs:61 / ErrorKind::ZstdInit
    }
    ~Engine() { zarc_gpu_destroy(h_); }
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;
    zarc_gpu_t *get() const { return h_; }
    void check(int rc) const
    {
        if (rc != ZARC_GPU_OK) throw Error(rc, std::string(zarc_gpu_error_name(rc)) + ": " + zarc_gpu_last_error(h_));
    }

  private:
    zarc_gpu_t *h_ = nullptr;
};

// Which device packs which entry.  Equal sizes: entry i goes to device i mod G.  Mixed sizes (BASELINE
// configs[4]): largest first onto the least loaded device by bytes (ties: the lower device), each share then back in index
// order.  Deterministic; zarc_amd/shard.py is the same function for bench.py and the tests.
inline std::vector<std::vector<size_t>> shard_assign(const size_t *len, size_t n, size_t g)
{
    std::vector<std::vector<size_t>> out(g ? g : 1);
    if (g <= 1) { out[0].resize(n); std::iota(out[0].begin(), out[0].end(), (size_t)0); return out; }
    bool equal = true;
    for (size_t i = 1; i < n; i++) equal = equal && len[i] == len[0];
    if (equal) { for (size_t i = 0; i < n; i++) out[i % g].push_back(i); return out; }
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return len[a] > len[b]; });
    std::vector<uint64_t> load(g, 0);
    for (size_t i : order) {
        size_t best = 0;
        for (size_t d = 1; d < g; d++) if (load[d] < load[best]) best = d;
        out[best].push_back(i);
        load[best] += len[i];
    }
    for (auto &v : out) std::sort(v.begin(), v.end());
    return out;
}

// Host-thread budget of G handles working at once (`--gpus G`): every handle's host-pointer entry points fill / drain their pinned
// staging ring with ZARC_GPU_PX_COPY_THREADS threads (default 8) beside two helper threads and the caller's own.  Eight handles at the
// default would be 64 copy threads on one host for a PCIe complex that 16 saturate: the total is capped at 16 (at least 2 per handle).
inline void cap_copy_threads(const std::vector<std::unique_ptr<Engine>> &engines)
{
    const size_t g = engines.size();
    if (g <= 2) return;
    const int per = (int)std::max<size_t>(2, 16 / g);
    for (auto &e : engines) e->check(zarc_gpu_set_parameter(e->get(), ZARC_GPU_PX_COPY_THREADS, per));
}

// Directory records come out of an archive and are untrusted: no u64 wrap-around, no frame beyond the file, no allocation the engine
// would refuse anyway (FrameReader and Encoder::repack_frames look at them before anything is sized by them)
inline void check_frame_records(size_t archive_len, const std::vector<Frame> &wanted)
{
    for (const Frame &f : wanted) {
        if (f.length > archive_len || f.offset > archive_len - f.length) throw Error(ZARC_GPU_E_PARAM, "frame outside the archive");
        if (f.uncompressed >= 0xFFFFFFF0ull || f.length >= 0xFFFFFFF0ull) throw Error(ZARC_GPU_E_UNSUPPORTED, "frames of 4 GiB or more are not supported");
        // Zstandard cannot expand a frame by more than a factor of ~(128 KiB block from a 4-byte RLE block): a larger claim is corrupt
        if (f.uncompressed > (f.length + 16) * (uint64_t)65536) throw Error(ZARC_GPU_E_PARAM, "frame claims an impossible uncompressed size");
    }
}

class Encoder {
  public:
    // Encoder::new: creates the context and writes the 12-byte header (encode.rs:58-78)
    explicit Encoder(std::ostream &writer, int device = 0) : Encoder(writer, std::vector<int>{device}) {}
    // ... on several devices: one engine handle each (`zarc pack --gpus N`)
    Encoder(std::ostream &writer, const std::vector<int> &devices) : writer_(writer)
    {
        if (devices.empty()) throw Error(ZARC_GPU_E_PARAM, "no device");
        for (int d : devices) engines_.emplace_back(new Engine(d));
        cap_copy_threads(engines_);
        writer_.write((const char *)FILE_MAGIC, sizeof FILE_MAGIC);
        offset_ = sizeof FILE_MAGIC;
    }
    size_t devices() const { return engines_.size(); }
    // Encoder::set_zstd_parameter -- sticky for future frames (encode.rs:84-89); id = ZSTD_cParameter value
    void set_zstd_parameter(int id, int value) { for (auto &e : engines_) e->check(zarc_gpu_set_parameter(e->get(), id, value)); }
    // Encoder::enable_compression (encode.rs:95-97)
    void enable_compression(bool compress) { for (auto &e : engines_) zarc_gpu_enable_compression(e->get(), compress ? 1 : 0); }
    // Engine extension (`zarc pack --split-blocks`): 64 KiB blocks are cut where their literal statistics change
    // (ZARC_GPU_PX_BLOCK_SPLIT).  Set on every handle, so several devices write the archive one would.
    void split_blocks(bool on) { set_zstd_parameter(ZARC_GPU_PX_BLOCK_SPLIT, on ? 1 : 0); }
    // Engine extension (`zarc pack --check`): every frame is decoded again and compared with its source before the batch call returns
    // (ZARC_GPU_PX_CHECK_FRAMES); a frame that fails makes add_data_frames throw Error(ZARC_GPU_E_CHECK) and nothing of the batch is written
    void check_frames(bool on) { set_zstd_parameter(ZARC_GPU_PX_CHECK_FRAMES, on ? 1 : 0); }

    // Encoder::add_data_frame for one entry (content_frame.rs:20)
    Digest add_data_frame(const uint8_t *content, size_t len)
    {
        const void *p = content;
        return add_data_frames(&p, &len, 1)[0];
    }

    // Batched add_data_frame: returns the digest of every entry in call order.
    // Hash first, like the reference (content_frame.rs:26-33): the engine digests the batch, asks `claim` below for every entry, and
    // compresses only content that neither an earlier call nor an earlier entry of this batch has brought -- on the reference's own
    // benchmark tree (half of the bytes are duplicates) that halves the work.  With several devices the claims of one digest may come
    // in any order; whichever device compresses it, the bytes are the same (the encoder is deterministic), and they are written where
    // the FIRST entry with that digest stands in call order.
    std::vector<Digest> add_data_frames(const void *const *content, const size_t *len, size_t n)
    {
        std::vector<Digest> digests(n);
        check_failed_.reset();
        if (n == 0) return digests;
        // 1. one fresh session per frame (reset(SessionOnly), content_frame.rs:37-39) == one independent frame each.  The batch
        //    is dealt to the devices; every device packs its share into its own buffer, concurrently, with no exchange.
        const size_t g = engines_.size();
        const auto share = shard_assign(len, n, g);
        std::vector<std::vector<uint8_t>> buffers(g);
        std::vector<int> status(n, ZARC_GPU_FRAME_OK);
        std::vector<int> rc(g, ZARC_GPU_OK);
        struct Made { const uint8_t *at; size_t len; };
        std::map<Digest, Made> made;   // digest -> the frame some device compressed in this call
        struct Claims { std::mutex mu; std::map<Digest, int> taken; const std::map<Digest, Frame> *written; } claims;
        claims.written = &frames_;
        auto claim = [](void *ctx, const uint8_t *d, size_t) -> int { // "frame already exists, skipping" (content_frame.rs:30-33)
            Claims *c = (Claims *)ctx;
            Digest dg;
            std::memcpy(dg.bytes.data(), d, 32);
            std::lock_guard<std::mutex> lk(c->mu);
            if (c->written->count(dg)) return 1;
            return c->taken.emplace(dg, 1).second ? 0 : 1;
        };
        std::mutex made_mu;
        auto pack_share = [&](size_t d) {
            const std::vector<size_t> &idx = share[d];
            const size_t m = idx.size();
            if (m == 0) return;
            std::vector<const void *> src(m);
            std::vector<size_t> l(m), off(m), out_len(m);
            std::vector<Digest> dig(m);
            std::vector<int> st(m);
            size_t cap = 0;
            for (size_t j = 0; j < m; j++) { src[j] = content[idx[j]]; l[j] = len[idx[j]]; cap += zarc_gpu_bound(l[j]); }
            buffers[d].resize(cap);
            rc[d] = zarc_gpu_pack_batch_dedup(engines_[d]->get(), m, src.data(), l.data(), buffers[d].data(), cap, off.data(), out_len.data(),
                                              (uint8_t(*)[32])dig.data(), st.data(), hash_first_ ? (zarc_gpu_known_fn)claim : nullptr, &claims);
            if (rc[d] == ZARC_GPU_E_CHECK) { // which entry of the CALL it was (the engine's message counts inside this device's share)
                std::lock_guard<std::mutex> lk(made_mu);
                for (size_t j = 0; j < m; j++) if (st[j] == ZARC_GPU_FRAME_CORRUPT && (!check_failed_ || idx[j] < *check_failed_)) check_failed_ = idx[j];
            }
            if (rc[d] != ZARC_GPU_OK) return;
            std::lock_guard<std::mutex> lk(made_mu);
            for (size_t j = 0; j < m; j++) {
                digests[idx[j]] = dig[j];
                status[idx[j]] = st[j];
                if (st[j] == ZARC_GPU_FRAME_OK) made.emplace(dig[j], Made{buffers[d].data() + off[j], out_len[j]}); // (without hash-first: the first copy inserted stays, all copies are equal)
            }
        };
        if (g == 1) pack_share(0);
        else {
            std::vector<std::thread> th;
            for (size_t d = 0; d < g; d++) th.emplace_back(pack_share, d);
            for (auto &t : th) t.join();
        }
        for (size_t d = 0; d < g; d++) engines_[d]->check(rc[d]);
        // 2. append in call order -- whichever device made the frame; first occurrence wins -- against frames already written and
        //    inside this batch, across devices -- later duplicates write nothing; offsets are the running sum of the lengths of
        //    what was written (content_frame.rs:22,45-57)
        for (size_t k = 0; k < n; k++) {
            if (status[k] != ZARC_GPU_FRAME_OK && status[k] != ZARC_GPU_FRAME_DUPLICATE) throw Error(status[k], zarc_gpu_frame_status_name(status[k]));
            if (frames_.count(digests[k])) continue; // "frame already exists, skipping"
            const auto it = made.find(digests[k]);
            if (it == made.end()) throw Error(ZARC_GPU_E_DEVICE, "internal: no frame was made for a new digest");
            Frame f;
            f.edition = edition_;
            f.offset = offset_;
            f.digest = digests[k];
            f.length = it->second.len;
            f.uncompressed = len[k];
            writer_.write((const char *)it->second.at, (std::streamsize)it->second.len);
            if (!writer_) throw Error(ZARC_GPU_E_DEVICE, "write failed");
            offset_ += it->second.len;
            frames_.emplace(f.digest, f);
            order_.push_back(f.digest);
        }
        return digests;
    }
    // What became of one frame handed to repack_frames
    struct Repacked {
        int status = ZARC_GPU_FRAME_OK; // FrameIterator::verify()'s answer for the OLD frame (zarc_gpu_verify_batch's status); ZARC_GPU_FRAME_CORRUPT
                                        // with check_frames(true): the NEW frame failed its read-back check.  Only OK frames are written
        Digest digest;                  // BLAKE3 of what the old frame decoded to
        uint64_t old_length = 0, new_length = 0; // new_length: what was written (the old length for a kept frame, 0 for a refused one)
        bool kept = false;              // keep_smaller: the new frame was not smaller, the old bytes were copied
    };
    // Decoder::read_content_frame joined to add_data_frame for a batch: `wanted` are directory records of the archive image `archive`
    // (offset / length / uncompressed / digest).  Every frame is judged as FrameReader::check_content_frames judges it, and the good ones
    // are encoded again with THIS encoder's parameters -- on the device, out of the scratch they were decoded into -- and appended in the
    // order of `wanted` with new records (offset, length, this edition; digest and uncompressed size unchanged).  The batch is dealt to
    // the devices by uncompressed bytes with shard_assign and the results are appended in the caller's order: G devices write the bytes
    // one would.  A digest this encoder has a frame for already is skipped, as in add_data_frames.  Frames that are not good are
    // reported and not written; it is the caller's to give up the archive.  keep_smaller: a new frame that is not smaller than the old
    // one is dropped and the old bytes are copied.
    std::vector<Repacked> repack_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted, bool keep_smaller = false)
    {
        const size_t n = wanted.size();
        std::vector<Repacked> out(n);
        check_frame_records(archive_len, wanted);
        if (n == 0) return out;
        std::vector<size_t> rl(n);
        for (size_t i = 0; i < n; i++) rl[i] = (size_t)wanted[i].uncompressed;
        const size_t g = engines_.size();
        const auto share = shard_assign(rl.data(), n, g);
        std::vector<std::vector<uint8_t>> buffers(g);
        std::vector<const uint8_t *> made(n, nullptr);
        std::vector<int> rc(g, ZARC_GPU_OK);
        auto repack_share = [&](size_t d) {
            const std::vector<size_t> &idx = share[d];
            const size_t m = idx.size();
            if (m == 0) return;
            std::vector<const void *> fp(m);
            std::vector<size_t> fl(m), ul(m), off(m), out_len(m);
            std::vector<Digest> expect(m), got(m);
            std::vector<int> status(m);
            size_t cap = 0;
            for (size_t j = 0; j < m; j++) {
                const Frame &f = wanted[idx[j]];
                fp[j] = archive + f.offset; fl[j] = (size_t)f.length; ul[j] = (size_t)f.uncompressed; expect[j] = f.digest; cap += zarc_gpu_bound(ul[j]);
            }
            buffers[d].resize(cap);
            rc[d] = zarc_gpu_repack_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(), buffers[d].data(), cap,
                                          off.data(), out_len.data(), (uint8_t(*)[32])got.data(), status.data());
            if (rc[d] != ZARC_GPU_OK && rc[d] != ZARC_GPU_E_CHECK) return;
            for (size_t j = 0; j < m; j++) { // (every share writes its own entries of out / made)
                Repacked &r = out[idx[j]];
                r.status = status[j]; r.digest = got[j]; r.old_length = fl[j]; r.new_length = out_len[j];
                made[idx[j]] = buffers[d].data() + off[j];
            }
        };
        if (g == 1) repack_share(0);
        else {
            std::vector<std::thread> th;
            for (size_t d = 0; d < g; d++) th.emplace_back(repack_share, d);
            for (auto &t : th) t.join();
        }
        bool check_failed = false;
        for (size_t d = 0; d < g; d++) { if (rc[d] == ZARC_GPU_E_CHECK) check_failed = true; else engines_[d]->check(rc[d]); }
        for (size_t k = 0; k < n; k++) {
            Repacked &r = out[k];
            if (r.status != ZARC_GPU_FRAME_OK || check_failed) { r.new_length = 0; continue; } // (a failed read-back check voids the whole call)
            if (frames_.count(wanted[k].digest)) { r.new_length = frames_.at(wanted[k].digest).length; continue; } // "frame already exists, skipping"
            const uint8_t *at = made[k];
            if (keep_smaller && r.new_length >= r.old_length) { r.kept = true; r.new_length = r.old_length; at = archive + wanted[k].offset; }
            Frame f;
            f.edition = edition_;
            f.offset = offset_;
            f.digest = wanted[k].digest;
            f.length = r.new_length;
            f.uncompressed = wanted[k].uncompressed;
            writer_.write((const char *)at, (std::streamsize)f.length);
            if (!writer_) throw Error(ZARC_GPU_E_DEVICE, "write failed");
            offset_ += f.length;
            frames_.emplace(f.digest, f);
            order_.push_back(f.digest);
        }
        return out;
    }

    // hash-first dedup (default on; off = every entry is compressed and duplicates are dropped afterwards: same archive, more work)
    void set_hash_first(bool on) { hash_first_ = on; }

    // after add_data_frames threw Error(ZARC_GPU_E_CHECK): the first entry of that call whose frame failed its read-back check
    std::optional<size_t> check_failed() const { return check_failed_; }
    const std::map<Digest, Frame> &frames() const { return frames_; }
    const std::vector<Digest> &frame_order() const { return order_; } // insertion order (the reference uses a HashMap)
    uint64_t offset() const { return offset_; }

  protected: // ArchiveWriter (zarc_container.hpp) adds add_file_entry / finalise on top
    std::ostream &writer_;
    std::vector<std::unique_ptr<Engine>> engines_; // one per device; engines_[0] also serves the directory frame / digest
    Engine &engine0() { return *engines_[0]; }
    uint16_t edition_ = 1;
    bool hash_first_ = true;
    std::optional<size_t> check_failed_;
    std::map<Digest, Frame> frames_;
    std::vector<Digest> order_;
    uint64_t offset_ = 0;
};

// Which lines a lines call delivers (zarc_gpu_line_select): the hit lines -- the matching lines, with `invert` the others -- and `before`
// lines in front of and `after` lines behind each.  The default selects the matching lines: the call is then the plain lines call.
struct LineSelect {
    bool invert = false;
    uint32_t before = 0, after = 0;
    bool active() const { return invert || before || after; }
};

// What a matches call searches for (zarc_gpu_matcher): one fixed string or one regular expression (text), or a set of fixed strings
struct MatchWhat {
    int kind = ZARC_GPU_MATCH_FIXED; // ZARC_GPU_MATCH_*
    std::string text;
    std::vector<std::string> set;
};

// Decoder::read_content_frame + FrameIterator for a batch of frames of one archive image held in memory.
// The reference's read side is a serial loop over frames that each get a fresh reader and DCtx (zarc-cli/src/unpack.rs:62-88,
// decode/zstd_iterator.rs:28-29): frames are as independent on the way out as on the way in.  A FrameReader constructed with G
// devices deals the wanted frames with the same `shard_assign` as the Encoder -- by UNCOMPRESSED bytes, what the decoder's work
// is proportional to -- decodes the shares concurrently (one host thread per handle, no collective) and returns the results in the
// caller's order; statuses, digests and bytes are identical to the single-device ones.
class FrameReader {
  public:
    struct Result {
        std::vector<uint8_t> data;       // the concatenation of what FrameIterator::next would yield
        Digest digest;                   // FrameIterator::digest() once the frame is done
        std::optional<bool> verify;      // FrameIterator::verify(): None if the frame did not decode
        int status = ZARC_GPU_FRAME_OK;  // Error::Zstd analogue (decode/error.rs:35-38) via zarc_gpu_frame_status_name
        uint64_t count = 0;              // search_content_frames: start positions at which the pattern occurs (0 for a frame that did not decode)
        std::optional<uint64_t> first;   // ... and the lowest of them
        std::optional<uint64_t> which;   // search_set_content_frames: the lowest index of a pattern that matches at `first`
        // lines_content_frames: the frame's matching lines, all of them counted, and the records of those that were delivered (they own their bytes)
        struct Line { uint64_t start, length, number, match; std::vector<uint8_t> text; }; // zarc_gpu_line; text: the line's first min(length, max_line) bytes
        uint64_t lines = 0;
        uint64_t selected = 0;           // with a LineSelect: the lines it selects (lines: the hit lines); without one: lines
        std::vector<Line> line_records;  // a selected line without a match: match == ZARC_GPU_SEARCH_NONE
        // matches_content_frames: the matches in those of the frame's matching lines that took part, all of them counted, and the records of
        // those that were delivered (zarc_gpu_match; text: the match's first min(length, max_line) bytes; which: a set's pattern)
        struct Match { uint64_t start, length, number, line_start, which; std::vector<uint8_t> text; };
        uint64_t matches = 0;
        std::vector<Match> match_records;
        // range_content_frames: zarc_gpu_range_result's first five fields -- the truth whatever the caps; the delivered bytes are `data`
        struct Range { uint64_t units = 0, first = 0, taken = 0, start = 0, length = 0; };
        Range range;
        // count_content_frames: zarc_gpu_wc's six fields; all zero for a frame that did not decode
        struct Count { uint64_t lines = 0, words = 0, chars = 0, max_line = 0, max_line_start = 0, max_line_no = 0; };
        Count wc;
        // compare_content_frames: zarc_gpu_cmp's fields; all zero (relation ZARC_GPU_CMP_NONE) for a frame that did not decode
        struct Compare { uint32_t relation = 0, byte_a = 0, byte_b = 0; uint64_t prefix = 0, line = 0, differing = 0, suffix = 0; };
        Compare cmp;
    };
    // the other side of a pair of compare_content_frames: caller memory; data may be null where len is 0
    struct Other { const void *data = nullptr; size_t len = 0; };
    explicit FrameReader(int device = 0) : FrameReader(std::vector<int>{device}) {}
    explicit FrameReader(const std::vector<int> &devices)
    {
        if (devices.empty()) throw Error(ZARC_GPU_E_PARAM, "no device");
        for (int d : devices) engines_.emplace_back(new Engine(d));
        cap_copy_threads(engines_);
    }
    size_t devices() const { return engines_.size(); }

    // `archive` is the whole file; `wanted` are directory records (offset/length/uncompressed/digest).
    std::vector<Result> read_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted)
    {
        return run_frames(archive, archive_len, wanted, true);
    }
    // FrameIterator::verify() (frame_iterator.rs:83-88) for a batch WITHOUT the bytes: {digest, verify, status} of every frame exactly
    // as read_content_frames reports them, `data` left empty.  The same record checks, the same dealing over the handles; only the
    // compressed frames travel to the devices and nothing but statuses and digests comes back (zarc_gpu_verify_batch).
    std::vector<Result> check_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted)
    {
        return run_frames(archive, archive_len, wanted, false);
    }
    // check_content_frames plus a search of what was decoded, on the device (zarc_gpu_search_batch): {digest, verify, status, count, first}
    // per frame for ONE fixed byte string of 1 .. ZARC_GPU_SEARCH_MAX_PATTERN bytes; icase folds ASCII letters only.  The same dealing
    // over the handles, results in the caller's order and identical for every number of handles; no content comes back.
    std::vector<Result> search_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted, const std::string &pattern,
                                              bool icase = false)
    {
        if (pattern.empty() || pattern.size() > ZARC_GPU_SEARCH_MAX_PATTERN) throw Error(ZARC_GPU_E_PARAM, "the pattern has 1 to 256 bytes");
        const Search s{&pattern, icase ? (unsigned)ZARC_GPU_SEARCH_ICASE : 0u};
        return run_frames(archive, archive_len, wanted, false, &s);
    }

    // search_content_frames plus the matching lines, gathered on the device (zarc_gpu_search_lines_batch): `lines` of every frame and the
    // records the delivery rule gives it -- frames in the caller's order, per frame the first min(lines, max_lines or all, what rec_cap
    // leaves) matching lines.  Every handle runs its share with the caller's caps, the shares are merged in the caller's order and the rule
    // is applied once more on the merged list: the results are identical for every number of handles.  Only the delivered lines' bytes
    // come back.  The pattern must not contain 0x0A.  With an active `sel` the call is zarc_gpu_select_lines_batch: the records are the
    // selected lines, `lines` counts the hit lines and `selected` the selected ones, dealt and merged in the same way.
    std::vector<Result> lines_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted, const std::string &pattern,
                                             bool icase = false, uint64_t max_lines = 0, uint64_t max_line = 4096, size_t rec_cap = (size_t)1 << 20,
                                             const LineSelect &sel = LineSelect())
    {
        if (pattern.empty() || pattern.size() > ZARC_GPU_SEARCH_MAX_PATTERN) throw Error(ZARC_GPU_E_PARAM, "the pattern has 1 to 256 bytes");
        if (pattern.find('\n') != std::string::npos) throw Error(ZARC_GPU_E_PARAM, "the pattern must not contain a newline");
        if (max_line < 1 || max_line > ZARC_GPU_LINES_MAX_LINE) throw Error(ZARC_GPU_E_PARAM, "max_line is 1 to 65536");
        Search s{&pattern, icase ? (unsigned)ZARC_GPU_SEARCH_ICASE : 0u, true, max_lines, max_line, rec_cap};
        if (sel.active()) s.select = &sel;
        std::vector<Result> out = run_frames(archive, archive_len, wanted, false, &s);
        size_t left = rec_cap;
        for (Result &r : out) { // the delivery rule over the merged list (a handle saw fewer frames in front of this one: it delivered no less)
            if (r.line_records.size() > left) r.line_records.resize(left);
            left -= r.line_records.size();
        }
        return out;
    }

    // search_content_frames for a SET of 1 .. ZARC_GPU_SEARCH_MAX_SET fixed byte strings in one pass (zarc_gpu_search_set_batch): count is the
    // start positions at which at least one pattern matches, first the lowest of them, which the lowest index of a pattern matching there.
    // hits (may be null) receives, per pattern, the positions at which it matches, summed over the frames that were searched -- over all
    // handles: the sums and everything else are identical for every number of handles.
    std::vector<Result> search_set_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted,
                                                  const std::vector<std::string> &patterns, bool icase = false, std::vector<uint64_t> *hits = nullptr)
    {
        check_set(patterns, false);
        Search s{nullptr, icase ? (unsigned)ZARC_GPU_SEARCH_ICASE : 0u};
        s.set = &patterns; s.hits = hits;
        if (hits) hits->assign(patterns.size(), 0);
        return run_frames(archive, archive_len, wanted, false, &s);
    }
    // lines_content_frames for a set (zarc_gpu_search_set_lines_batch): a line matches when a match of any pattern starts in it, a
    // record's `match` is the lowest such position.  No pattern may contain 0x0A.
    std::vector<Result> lines_set_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted,
                                                 const std::vector<std::string> &patterns, bool icase = false, uint64_t max_lines = 0, uint64_t max_line = 4096,
                                                 size_t rec_cap = (size_t)1 << 20, std::vector<uint64_t> *hits = nullptr, const LineSelect &sel = LineSelect())
    {
        check_set(patterns, true);
        if (max_line < 1 || max_line > ZARC_GPU_LINES_MAX_LINE) throw Error(ZARC_GPU_E_PARAM, "max_line is 1 to 65536");
        Search s{nullptr, icase ? (unsigned)ZARC_GPU_SEARCH_ICASE : 0u, true, max_lines, max_line, rec_cap};
        s.set = &patterns; s.hits = hits;
        if (sel.active()) s.select = &sel;
        if (hits) hits->assign(patterns.size(), 0);
        std::vector<Result> out = run_frames(archive, archive_len, wanted, false, &s);
        size_t left = rec_cap;
        for (Result &r : out) { // the delivery rule over the merged list, as in lines_content_frames
            if (r.line_records.size() > left) r.line_records.resize(left);
            left -= r.line_records.size();
        }
        return out;
    }

    // search_content_frames with a regular expression in place of the fixed string (zarc_gpu_search_regex_batch; include/zarc_gpu.h has the
    // dialect): count is the positions at which a match starts inside its line, first the lowest of them.  A bad expression, or one whose
    // automaton needs more than ZARC_GPU_REGEX_MAX_STATES states, throws with the compiler's message before any handle is used.
    std::vector<Result> search_regex_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted, const std::string &regex,
                                                    bool icase = false)
    {
        check_regex(regex, icase);
        Search s{&regex, icase ? (unsigned)ZARC_GPU_SEARCH_ICASE : 0u};
        s.regex = true;
        return run_frames(archive, archive_len, wanted, false, &s);
    }
    // ... and lines_content_frames with one (zarc_gpu_search_regex_lines_batch)
    std::vector<Result> lines_regex_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted, const std::string &regex,
                                                   bool icase = false, uint64_t max_lines = 0, uint64_t max_line = 4096, size_t rec_cap = (size_t)1 << 20,
                                                   const LineSelect &sel = LineSelect())
    {
        check_regex(regex, icase);
        if (max_line < 1 || max_line > ZARC_GPU_LINES_MAX_LINE) throw Error(ZARC_GPU_E_PARAM, "max_line is 1 to 65536");
        Search s{&regex, icase ? (unsigned)ZARC_GPU_SEARCH_ICASE : 0u, true, max_lines, max_line, rec_cap};
        s.regex = true;
        if (sel.active()) s.select = &sel;
        std::vector<Result> out = run_frames(archive, archive_len, wanted, false, &s);
        size_t left = rec_cap;
        for (Result &r : out) { // the delivery rule over the merged list, as in lines_content_frames
            if (r.line_records.size() > left) r.line_records.resize(left);
            left -= r.line_records.size();
        }
        return out;
    }

    // Every match of the matching lines, cut out on the device (zarc_gpu_search_matches_batch; grep -o): per frame `lines`, `matches` and
    // the records the two delivery rules give it -- the frame's first min(lines, max_lines or all, what line_cap leaves) matching lines take
    // part, and of their matches the first that rec_cap leaves room for are delivered.  Every handle runs its share with the caller's caps.
    // Should line_cap run out over the merged list, the shares run once more, each with the lines the rule leaves its frames (they are the
    // caller's frames in the caller's order, so the sum of their allotments as a handle's line_cap gives every one of them exactly its
    // own); rec_cap is then applied on the merged list.  The results are identical for every number of handles.
    std::vector<Result> matches_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted, const MatchWhat &what,
                                               bool icase = false, uint64_t max_lines = 0, uint64_t max_line = 4096, size_t line_cap = (size_t)1 << 20,
                                               size_t rec_cap = (size_t)1 << 20, std::vector<uint64_t> *hits = nullptr)
    {
        if (what.kind == ZARC_GPU_MATCH_SET) check_set(what.set, true);
        else if (what.kind == ZARC_GPU_MATCH_REGEX) { check_regex(what.text, icase); check_regex_ends(what.text, icase); }
        else if (what.kind == ZARC_GPU_MATCH_FIXED) {
            if (what.text.empty() || what.text.size() > ZARC_GPU_SEARCH_MAX_PATTERN) throw Error(ZARC_GPU_E_PARAM, "the pattern has 1 to 256 bytes");
            if (what.text.find('\n') != std::string::npos) throw Error(ZARC_GPU_E_PARAM, "the pattern must not contain a newline");
        } else throw Error(ZARC_GPU_E_PARAM, "unknown matcher kind");
        if (max_line < 1 || max_line > ZARC_GPU_LINES_MAX_LINE) throw Error(ZARC_GPU_E_PARAM, "max_line is 1 to 65536");
        Search s{&what.text, icase ? (unsigned)ZARC_GPU_SEARCH_ICASE : 0u, true, max_lines, max_line, rec_cap};
        s.regex = what.kind == ZARC_GPU_MATCH_REGEX;
        if (what.kind == ZARC_GPU_MATCH_SET) { s.set = &what.set; s.hits = hits; }
        s.matches = true; s.line_cap = line_cap;
        if (s.hits) s.hits->assign(what.set.size(), 0);
        std::vector<Result> out = run_frames(archive, archive_len, wanted, false, &s);
        auto allot = [&](const Result &r) { return max_lines ? std::min<uint64_t>(r.lines, max_lines) : r.lines; };
        uint64_t asked = 0;
        for (const Result &r : out) asked += allot(r);
        if (engines_.size() > 1 && asked > line_cap) { // a handle saw fewer lines in front of a frame than the call has: once more, with every frame's own allotment
            std::vector<size_t> rl(wanted.size());
            for (size_t i = 0; i < wanted.size(); i++) rl[i] = wanted[i].uncompressed;
            const auto share = shard_assign(rl.data(), rl.size(), engines_.size());
            std::vector<uint64_t> mine(out.size());
            uint64_t left = line_cap;
            for (size_t i = 0; i < out.size(); i++) { mine[i] = std::min<uint64_t>(allot(out[i]), left); left -= mine[i]; }
            std::vector<size_t> caps(engines_.size(), 0);
            for (size_t d = 0; d < share.size(); d++) for (size_t i : share[d]) caps[d] += (size_t)mine[i];
            s.share_line_cap = &caps;
            if (s.hits) s.hits->assign(what.set.size(), 0);
            out = run_frames(archive, archive_len, wanted, false, &s);
        }
        size_t left = rec_cap;
        for (Result &r : out) { // the record rule over the merged list (a handle saw fewer frames in front of this one: it delivered no less)
            if (r.match_records.size() > left) r.match_records.resize(left);
            left -= r.match_records.size();
        }
        return out;
    }

    // check_content_frames plus one byte or line range of every frame, cut out on the device (zarc_gpu_read_ranges_batch): per frame
    // {digest, verify, status}, `range` and in `data` the bytes the delivery rule gives it -- frames in the caller's order, frame i the first
    // min(length, max_bytes or all, what text_cap leaves) bytes of its range.  ranges[i] belongs to wanted[i]; the same frame may stand in
    // the batch several times.  Every handle runs its share with the caller's caps, the shares are merged in the caller's order and the
    // rule is applied once more on the merged list (a handle saw fewer frames in front of a frame: it delivered no less): the results are
    // identical for every number of handles.  Only the delivered bytes come back.
    std::vector<Result> range_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted, const std::vector<zarc_gpu_range> &ranges,
                                             uint64_t max_bytes = 0, size_t text_cap = (size_t)256 << 20)
    {
        const size_t n = wanted.size();
        if (ranges.size() != n) throw Error(ZARC_GPU_E_PARAM, "one range per frame");
        for (const zarc_gpu_range &r : ranges) {
            if (r.unit != ZARC_GPU_RANGE_BYTES && r.unit != ZARC_GPU_RANGE_LINES) throw Error(ZARC_GPU_E_PARAM, "unknown range unit");
            if (r.flags & ~(uint32_t)ZARC_GPU_RANGE_FROM_END) throw Error(ZARC_GPU_E_PARAM, "unknown range flag");
        }
        std::vector<Result> out(n);
        check_frame_records(archive_len, wanted);
        if (n == 0) return out;
        std::vector<size_t> rl(n);
        for (size_t i = 0; i < n; i++) rl[i] = wanted[i].uncompressed;
        const size_t g = engines_.size();
        const auto share = shard_assign(rl.data(), n, g);
        std::vector<int> rc(g, ZARC_GPU_OK);
        auto range_share = [&](size_t d) {
            const std::vector<size_t> &idx = share[d];
            const size_t m = idx.size();
            if (m == 0) return;
            std::vector<const void *> fp(m);
            std::vector<size_t> fl(m), ul(m);
            std::vector<Digest> expect(m), got(m);
            std::vector<int> status(m);
            std::vector<zarc_gpu_range> rg(m);
            std::vector<zarc_gpu_range_result> res(m);
            uint64_t room = 0; // no frame delivers more than its content, or than max_bytes
            for (size_t j = 0; j < m; j++) {
                const Frame &f = wanted[idx[j]];
                fp[j] = archive + f.offset; fl[j] = f.length; ul[j] = f.uncompressed; expect[j] = f.digest; rg[j] = ranges[idx[j]];
                room += max_bytes ? std::min<uint64_t>(f.uncompressed, max_bytes) : f.uncompressed;
            }
            const size_t cap = (size_t)std::min<uint64_t>(text_cap, room);
            std::unique_ptr<uint8_t, void (*)(void *)> text((uint8_t *)std::malloc(std::max<size_t>(1, cap)), std::free);
            if (!text) { rc[d] = ZARC_GPU_E_NOMEM; return; }
            size_t text_used = 0;
            rc[d] = zarc_gpu_read_ranges_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(), rg.data(), max_bytes,
                                               (uint8_t(*)[32])got.data(), status.data(), res.data(), text.get(), cap, &text_used);
            if (rc[d] != ZARC_GPU_OK) return;
            for (size_t j = 0; j < m; j++) {
                Result &r = out[idx[j]];
                r.status = status[j];
                r.digest = got[j];
                if (status[j] == ZARC_GPU_FRAME_OK || status[j] == ZARC_GPU_FRAME_DIGEST) r.verify = got[j] == expect[j];
                r.range = Result::Range{res[j].units, res[j].first, res[j].taken, res[j].start, res[j].length};
                r.data.assign(text.get() + res[j].text_off, text.get() + res[j].text_off + res[j].text_len);
            }
        };
        if (g == 1) range_share(0);
        else {
            std::vector<std::thread> th;
            for (size_t d = 0; d < g; d++) th.emplace_back(range_share, d);
            for (auto &t : th) t.join();
        }
        for (size_t d = 0; d < g; d++) engines_[d]->check(rc[d]);
        uint64_t left = text_cap;
        for (Result &r : out) { // the delivery rule over the merged list
            if (r.data.size() > left) r.data.resize((size_t)left);
            left -= r.data.size();
        }
        return out;
    }

    // check_content_frames plus what `wc` says of every frame, counted on the device (zarc_gpu_count_batch): per frame {digest, verify,
    // status} and `wc`.  The same dealing over the handles, one thread per handle; every frame's answer is its own, so the results are in
    // the caller's order and identical for every number of handles.  Only 64 bytes a frame come back.
    std::vector<Result> count_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted)
    {
        const size_t n = wanted.size();
        std::vector<Result> out(n);
        check_frame_records(archive_len, wanted);
        if (n == 0) return out;
        std::vector<size_t> rl(n);
        for (size_t i = 0; i < n; i++) rl[i] = wanted[i].uncompressed;
        const size_t g = engines_.size();
        const auto share = shard_assign(rl.data(), n, g);
        std::vector<int> rc(g, ZARC_GPU_OK);
        auto count_share = [&](size_t d) {
            const std::vector<size_t> &idx = share[d];
            const size_t m = idx.size();
            if (m == 0) return;
            std::vector<const void *> fp(m);
            std::vector<size_t> fl(m), ul(m);
            std::vector<Digest> expect(m), got(m);
            std::vector<int> status(m);
            std::vector<zarc_gpu_wc> res(m);
            for (size_t j = 0; j < m; j++) {
                const Frame &f = wanted[idx[j]];
                fp[j] = archive + f.offset; fl[j] = f.length; ul[j] = f.uncompressed; expect[j] = f.digest;
            }
            rc[d] = zarc_gpu_count_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(), (uint8_t(*)[32])got.data(),
                                         status.data(), res.data());
            if (rc[d] != ZARC_GPU_OK) return;
            for (size_t j = 0; j < m; j++) {
                Result &r = out[idx[j]];
                r.status = status[j];
                r.digest = got[j];
                if (status[j] == ZARC_GPU_FRAME_OK || status[j] == ZARC_GPU_FRAME_DIGEST) r.verify = got[j] == expect[j];
                r.wc = Result::Count{res[j].lines, res[j].words, res[j].chars, res[j].max_line, res[j].max_line_start, res[j].max_line_no};
            }
        };
        if (g == 1) count_share(0);
        else {
            std::vector<std::thread> th;
            for (size_t d = 0; d < g; d++) th.emplace_back(count_share, d);
            for (auto &t : th) t.join();
        }
        for (size_t d = 0; d < g; d++) engines_[d]->check(rc[d]);
        return out;
    }

    // check_content_frames plus what `cmp` says of every frame's content against others[i], compared on the device
    // (zarc_gpu_compare_batch): per pair {digest, verify, status} and `cmp`.  wanted[i] and others[i] are one pair; a frame may stand in
    // several pairs.  The same dealing over the handles, one thread per handle; every pair's answer is its own, so the results are in the
    // caller's order and identical for every number of handles.  The frames and the other sides go up; 64 bytes a pair come back.
    std::vector<Result> compare_content_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted, const std::vector<Other> &others)
    {
        const size_t n = wanted.size();
        if (others.size() != n) throw Error(ZARC_GPU_E_PARAM, "compare: one other side per frame is needed");
        std::vector<Result> out(n);
        check_frame_records(archive_len, wanted);
        if (n == 0) return out;
        std::vector<size_t> rl(n);
        for (size_t i = 0; i < n; i++) rl[i] = std::max<size_t>(wanted[i].uncompressed, others[i].len);
        const size_t g = engines_.size();
        const auto share = shard_assign(rl.data(), n, g);
        std::vector<int> rc(g, ZARC_GPU_OK);
        auto compare_share = [&](size_t d) {
            const std::vector<size_t> &idx = share[d];
            const size_t m = idx.size();
            if (m == 0) return;
            std::vector<const void *> fp(m), op(m);
            std::vector<size_t> fl(m), ul(m), ol(m);
            std::vector<Digest> expect(m), got(m);
            std::vector<int> status(m);
            std::vector<zarc_gpu_cmp> res(m);
            for (size_t j = 0; j < m; j++) {
                const Frame &f = wanted[idx[j]];
                fp[j] = archive + f.offset; fl[j] = f.length; ul[j] = f.uncompressed; expect[j] = f.digest;
                op[j] = others[idx[j]].data; ol[j] = others[idx[j]].len;
            }
            rc[d] = zarc_gpu_compare_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(), op.data(), ol.data(),
                                           (uint8_t(*)[32])got.data(), status.data(), res.data());
            if (rc[d] != ZARC_GPU_OK) return;
            for (size_t j = 0; j < m; j++) {
                Result &r = out[idx[j]];
                r.status = status[j];
                r.digest = got[j];
                if (status[j] == ZARC_GPU_FRAME_OK || status[j] == ZARC_GPU_FRAME_DIGEST) r.verify = got[j] == expect[j];
                r.cmp = Result::Compare{res[j].relation, res[j].byte_a, res[j].byte_b, res[j].prefix, res[j].line, res[j].differing, res[j].suffix};
            }
        };
        if (g == 1) compare_share(0);
        else {
            std::vector<std::thread> th;
            for (size_t d = 0; d < g; d++) th.emplace_back(compare_share, d);
            for (auto &t : th) t.join();
        }
        for (size_t d = 0; d < g; d++) engines_[d]->check(rc[d]);
        return out;
    }

  private:
    struct Search {
        const std::string *pattern; unsigned flags; bool lines = false; uint64_t max_lines = 0, max_line = 0; size_t rec_cap = 0;
        bool regex = false;                            // `pattern` is a regular expression
        const std::vector<std::string> *set = nullptr; // a set of patterns in place of the one
        std::vector<uint64_t> *hits = nullptr;         // ... and its per-pattern sums over all handles
        const LineSelect *select = nullptr;            // lines: the selected lines in place of the matching ones
        bool matches = false;                          // lines: the matches of the matching lines in place of the lines (rec_cap is theirs)
        size_t line_cap = 0;                           // ... and the lines that may take part; per handle where share_line_cap says so
        const std::vector<size_t> *share_line_cap = nullptr;
    };
    static void check_regex_ends(const std::string &regex, bool icase)
    {
        char msg[256];
        const int rc = zarc_gpu_regex_compile_ends(regex.data(), regex.size(), icase ? (unsigned)ZARC_GPU_SEARCH_ICASE : 0u, nullptr, msg, sizeof msg);
        if (rc != ZARC_GPU_OK) throw Error(rc, msg);
    }
    static void check_regex(const std::string &regex, bool icase)
    {
        char msg[256];
        const int rc = zarc_gpu_regex_compile(regex.data(), regex.size(), icase ? (unsigned)ZARC_GPU_SEARCH_ICASE : 0u, nullptr, msg, sizeof msg);
        if (rc != ZARC_GPU_OK) throw Error(rc, msg);
    }
    static void check_set(const std::vector<std::string> &patterns, bool lines)
    {
        if (patterns.empty() || patterns.size() > ZARC_GPU_SEARCH_MAX_SET) throw Error(ZARC_GPU_E_PARAM, "a set has 1 to 1024 patterns");
        for (const std::string &p : patterns) {
            if (p.empty() || p.size() > ZARC_GPU_SEARCH_MAX_PATTERN) throw Error(ZARC_GPU_E_PARAM, "a pattern has 1 to 256 bytes");
            if (lines && p.find('\n') != std::string::npos) throw Error(ZARC_GPU_E_PARAM, "a pattern must not contain a newline");
        }
    }
    std::vector<Result> run_frames(const uint8_t *archive, size_t archive_len, const std::vector<Frame> &wanted, bool with_data, const Search *search = nullptr)
    {
        const size_t n = wanted.size();
        std::vector<Result> out(n);
        std::vector<size_t> rl(n);
        check_frame_records(archive_len, wanted);
        for (size_t i = 0; i < n; i++) {
            if (with_data) out[i].data.resize(wanted[i].uncompressed);
            rl[i] = wanted[i].uncompressed;
        }
        if (n == 0) return out;
        const size_t g = engines_.size();
        const auto share = shard_assign(rl.data(), n, g);
        std::vector<int> rc(g, ZARC_GPU_OK);
        // a set of patterns: one image for all handles, and every handle's own hits
        std::string set_bytes;
        std::vector<uint64_t> set_off, set_len;
        size_t shortest = search && search->pattern && !search->regex ? search->pattern->size() : 1;
        if (search && search->set) {
            shortest = SIZE_MAX;
            for (const std::string &p : *search->set) { set_off.push_back(set_bytes.size()); set_len.push_back(p.size()); set_bytes += p; shortest = std::min(shortest, p.size()); }
        }
        const zarc_gpu_pattern_set pset{set_bytes.data(), set_off.data(), set_len.data(), set_off.size()};
        std::vector<std::vector<uint64_t>> share_hits(g);
        auto unpack_share = [&](size_t d) {
            const std::vector<size_t> &idx = share[d];
            const size_t m = idx.size();
            if (m == 0) return;
            std::vector<const void *> fp(m);
            std::vector<void *> dp(m);
            std::vector<size_t> fl(m), ul(m);
            std::vector<Digest> expect(m), got(m);
            std::vector<int> status(m);
            std::vector<uint64_t> count(search ? m : 0), first(search ? m : 0), which(search && search->set ? m : 0);
            if (search && search->set) share_hits[d].assign(set_off.size(), 0);
            for (size_t j = 0; j < m; j++) {
                const Frame &f = wanted[idx[j]];
                fp[j] = archive + f.offset; fl[j] = f.length; ul[j] = f.uncompressed; dp[j] = out[idx[j]].data.data(); expect[j] = f.digest;
            }
            // lines: no frame holds more matching lines than it has room for matches, so a share's records never need more than this -- and
            // neither does its text buffer, which the call wants rec_cap * max_line bytes large (never touched beyond what is delivered)
            std::vector<uint64_t> nlines, nselected, nmatches;
            std::vector<zarc_gpu_line> rec;
            std::vector<zarc_gpu_match> mrec;
            std::unique_ptr<uint8_t, void (*)(void *)> text(nullptr, std::free);
            size_t rec_cap = 0, rec_used = 0, text_used = 0;
            if (search && search->lines) {
                uint64_t room = 0;
                for (size_t j = 0; j < m; j++) room += (search->select ? ul[j] : ul[j] / shortest) + 1; // (selected: no frame has more lines than bytes)
                rec_cap = (size_t)std::min<uint64_t>(search->rec_cap, room);
                nlines.resize(m); nselected.resize(m); nmatches.resize(m);
                if (search->matches) mrec.resize(rec_cap); else rec.resize(rec_cap); // (matches do not overlap: no frame has more than bytes / shortest)
                text.reset((uint8_t *)std::malloc(std::max<size_t>(1, rec_cap * (size_t)search->max_line)));
                if (!text) { rc[d] = ZARC_GPU_E_NOMEM; return; }
            }
            zarc_gpu_matcher mt{ZARC_GPU_MATCH_FIXED, search ? search->flags : 0u, nullptr, 0, nullptr};
            zarc_gpu_line_select ls{0, 0, 0, 0};
            if (search && (search->select || search->matches)) {
                if (search->set) { mt.kind = ZARC_GPU_MATCH_SET; mt.set = &pset; }
                else { mt.kind = search->regex ? ZARC_GPU_MATCH_REGEX : ZARC_GPU_MATCH_FIXED; mt.text = search->pattern->data(); mt.text_len = search->pattern->size(); }
            }
            if (search && search->select) {
                ls = zarc_gpu_line_select{search->select->invert ? (uint32_t)ZARC_GPU_SELECT_INVERT : 0u, search->select->before, search->select->after, 0};
            }
            rc[d] = search && search->matches
                        ? zarc_gpu_search_matches_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(), &mt,
                                                        search->max_lines, search->max_line, search->share_line_cap ? (*search->share_line_cap)[d] : search->line_cap,
                                                        (uint8_t(*)[32])got.data(), status.data(), count.data(), first.data(), search->set ? which.data() : nullptr,
                                                        search->set ? share_hits[d].data() : nullptr, nlines.data(), nmatches.data(), mrec.data(), rec_cap, &rec_used,
                                                        text.get(), rec_cap * (size_t)search->max_line, &text_used)
                    : search && search->lines && search->select
                        ? zarc_gpu_select_lines_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(), &mt, &ls,
                                                      search->max_lines, search->max_line, (uint8_t(*)[32])got.data(), status.data(), count.data(), first.data(),
                                                      search->set ? which.data() : nullptr, search->set ? share_hits[d].data() : nullptr, nlines.data(),
                                                      nselected.data(), rec.data(), rec_cap, &rec_used, text.get(), rec_cap * (size_t)search->max_line, &text_used)
                    : search && search->set && search->lines
                        ? zarc_gpu_search_set_lines_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(), &pset,
                                                          search->flags, search->max_lines, search->max_line, (uint8_t(*)[32])got.data(), status.data(), count.data(),
                                                          first.data(), which.data(), share_hits[d].data(), nlines.data(), rec.data(), rec_cap, &rec_used, text.get(),
                                                          rec_cap * (size_t)search->max_line, &text_used)
                    : search && search->set
                        ? zarc_gpu_search_set_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(), &pset, search->flags,
                                                    (uint8_t(*)[32])got.data(), status.data(), count.data(), first.data(), which.data(), share_hits[d].data())
                    : search && search->regex && search->lines
                        ? zarc_gpu_search_regex_lines_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(),
                                                            search->pattern->data(), search->pattern->size(), search->flags, search->max_lines, search->max_line,
                                                            (uint8_t(*)[32])got.data(), status.data(), count.data(), first.data(), nlines.data(), rec.data(), rec_cap,
                                                            &rec_used, text.get(), rec_cap * (size_t)search->max_line, &text_used)
                    : search && search->regex
                        ? zarc_gpu_search_regex_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(),
                                                      search->pattern->data(), search->pattern->size(), search->flags, (uint8_t(*)[32])got.data(),
                                                      status.data(), count.data(), first.data())
                    : search && search->lines
                        ? zarc_gpu_search_lines_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(),
                                                      search->pattern->data(), search->pattern->size(), search->flags, search->max_lines, search->max_line,
                                                      (uint8_t(*)[32])got.data(), status.data(), count.data(), first.data(), nlines.data(), rec.data(), rec_cap,
                                                      &rec_used, text.get(), rec_cap * (size_t)search->max_line, &text_used)
                    : search  ? zarc_gpu_search_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(),
                                                      search->pattern->data(), search->pattern->size(), search->flags, (uint8_t(*)[32])got.data(),
                                                      status.data(), count.data(), first.data())
                    : with_data ? zarc_gpu_unpack_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), dp.data(), (const uint8_t(*)[32])expect.data(),
                                                      (uint8_t(*)[32])got.data(), status.data())
                              : zarc_gpu_verify_batch(engines_[d]->get(), m, fp.data(), fl.data(), ul.data(), (const uint8_t(*)[32])expect.data(),
                                                      (uint8_t(*)[32])got.data(), status.data());
            if (rc[d] != ZARC_GPU_OK) return;
            for (size_t j = 0; j < m; j++) {
                Result &r = out[idx[j]];
                r.status = status[j];
                r.digest = got[j];
                const bool decoded = status[j] == ZARC_GPU_FRAME_OK || status[j] == ZARC_GPU_FRAME_DIGEST;
                if (decoded) r.verify = got[j] == expect[j]; // a mismatch is reported, not fatal (zarc-cli/src/unpack.rs:118-120)
                else r.data.clear();
                if (search) { r.count = count[j]; if (first[j] != ZARC_GPU_SEARCH_NONE) r.first = first[j]; }
                if (search && search->set && which[j] != ZARC_GPU_SEARCH_NONE) r.which = which[j];
                if (search && search->lines) { r.lines = nlines[j]; r.selected = search->select ? nselected[j] : nlines[j]; }
                if (search && search->matches) r.matches = nmatches[j];
            }
            for (size_t k = 0; search && search->matches && k < rec_used; k++) {
                const zarc_gpu_match &x = mrec[k];
                out[idx[x.frame]].match_records.push_back(Result::Match{x.start, x.length, x.number, x.line_start, x.which,
                                                                        std::vector<uint8_t>(text.get() + x.text_off, text.get() + x.text_off + x.text_len)});
            }
            for (size_t k = 0; !(search && search->matches) && k < rec_used; k++) {
                const zarc_gpu_line &l = rec[k];
                out[idx[l.frame]].line_records.push_back(Result::Line{l.start, l.length, l.number, l.match, std::vector<uint8_t>(text.get() + l.text_off, text.get() + l.text_off + l.text_len)});
            }
        };
        if (g == 1) unpack_share(0);
        else {
            std::vector<std::thread> th;
            for (size_t d = 0; d < g; d++) th.emplace_back(unpack_share, d);
            for (auto &t : th) t.join();
        }
        for (size_t d = 0; d < g; d++) engines_[d]->check(rc[d]);
        if (search && search->hits)
            for (const std::vector<uint64_t> &sh : share_hits)
                for (size_t k = 0; k < sh.size(); k++) (*search->hits)[k] += sh[k];
        return out;
    }

    std::vector<std::unique_ptr<Engine>> engines_; // one per device
};

} // namespace zarc
