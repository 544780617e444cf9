// tests/host/range_frames_test.cpp -- zarc::FrameReader::range_content_frames (zarc_amd/host/zarc_host.hpp) over 1, 2 and 4 handles: the same
// range descriptors and the same bytes for every number of handles, under three text_cap values, equal to a plain host walk of the entries
// and to check_content_frames in verdict.  Built by tests/test_range_host.py against the emulated library (or the product library on a GPU
// box).
#include "../../zarc_amd/host/zarc_host.hpp"
#include "../../zarc_amd/csrc/corpus.h"
#include <cstdio>
#include <cstdlib>
#include <sstream>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

struct Want { uint64_t units, first, taken, start, length; };
// the reference: the definition of include/zarc_gpu.h, unit by unit
static Want walk(const std::vector<uint8_t> &d, const zarc_gpu_range &r)
{
    std::vector<uint64_t> pos(1, 0); // pos[k] = the offset of unit k's first byte; pos[T] = the content's length
    if (r.unit == ZARC_GPU_RANGE_BYTES) for (size_t k = 1; k <= d.size(); k++) pos.push_back(k);
    else {
        for (size_t k = 0; k < d.size(); k++) if (d[k] == '\n') pos.push_back(k + 1);
        if (!d.empty() && d.back() != '\n') pos.push_back(d.size());
    }
    const uint64_t T = pos.size() - 1;
    uint64_t a, b;
    if (r.flags & ZARC_GPU_RANGE_FROM_END) { b = T - std::min<uint64_t>(r.skip, T); a = b - std::min<uint64_t>(r.take, b); }
    else { a = std::min<uint64_t>(r.skip, T); b = a + std::min<uint64_t>(r.take, T - a); }
    return Want{T, a, b - a, pos[a], pos[b] - pos[a]};
}

int main()
{
    const size_t sizes[] = {0, 1, 300, 70000, 200000, 65536, 5000, 131073, 65543, 9, 70000, 300};
    const size_t N = sizeof sizes / sizeof sizes[0];
    std::vector<std::vector<uint8_t>> ents;
    std::vector<const void *> ptr;
    std::vector<size_t> len;
    for (size_t i = 0; i < N; i++) {
        ents.emplace_back(sizes[i]);
        zarc_corpus_entry(ents.back().data(), sizes[i], 9800 + i, 0);
        std::vector<uint8_t> &e = ents.back();
        if (e.size() >= 65543) { e[65535] = '\n'; e[65536] = '\n'; }
    }
    for (auto &e : ents) { ptr.push_back(e.data()); len.push_back(e.size()); }
    std::ostringstream plain;
    std::vector<zarc::Frame> wanted;
    {
        zarc::Encoder enc(plain);
        enc.set_zstd_parameter(ZARC_GPU_P_CHECKSUM_FLAG, 1);
        enc.enable_compression(false); // the encoder is not the subject
        enc.add_data_frames(ptr.data(), len.data(), ptr.size());
        for (const zarc::Digest &d : enc.frame_order()) wanted.push_back(enc.frames().at(d));
    }
    CHECK(wanted.size() == N);
    std::string img = plain.str();
    wanted[7].uncompressed += 1; // a frame that does not decode: all zero, no bytes
    const uint64_t ALL = ZARC_GPU_RANGE_ALL;
    const zarc_gpu_range forms[] = {{ZARC_GPU_RANGE_LINES, 0, 0, 10}, {ZARC_GPU_RANGE_LINES, ZARC_GPU_RANGE_FROM_END, 0, 10}, {ZARC_GPU_RANGE_LINES, 0, 20, 200},
                                    {ZARC_GPU_RANGE_BYTES, 0, 100, 4096}, {ZARC_GPU_RANGE_BYTES, ZARC_GPU_RANGE_FROM_END, 3, ALL}, {ZARC_GPU_RANGE_LINES, 0, 2, ALL},
                                    {ZARC_GPU_RANGE_LINES, ZARC_GPU_RANGE_FROM_END, 5, ALL}};
    std::vector<zarc_gpu_range> ranges;
    for (size_t i = 0; i < N; i++) ranges.push_back(forms[i % (sizeof forms / sizeof forms[0])]);
    // the same frame twice with different ranges
    wanted.push_back(wanted[4]); ranges.push_back(forms[0]); ents.push_back(ents[4]);
    wanted.push_back(wanted[4]); ranges.push_back(forms[4]); ents.push_back(ents[4]);
    const size_t M = wanted.size();
    uint64_t total = 0;
    std::vector<Want> want;
    for (size_t i = 0; i < M; i++) { want.push_back(walk(ents[i], ranges[i])); if (i != 7) total += want[i].length; }
    CHECK(total > 300000 && want[12].taken == 10 && want[8].taken == 10 && want[5].length > 30000 && want[6].taken > 5);
    const int devices = zarc_gpu_device_count();
    struct Caps { uint64_t max_bytes; size_t text_cap; };
    const Caps caps[] = {{0, (size_t)1 << 24}, {0, (size_t)total - 70000}, {1000, 5500}, {0, 0}};
    for (const Caps &c : caps) {
        std::vector<zarc::FrameReader::Result> base;
        for (int g = 1; g <= 4; g *= 2) {
            if (g > devices) break;
            std::vector<int> dev;
            for (int d = 0; d < g; d++) dev.push_back(d);
            zarc::FrameReader rd(dev);
            const auto chk = rd.check_content_frames((const uint8_t *)img.data(), img.size(), wanted);
            const auto got = rd.range_content_frames((const uint8_t *)img.data(), img.size(), wanted, ranges, c.max_bytes, c.text_cap);
            CHECK(got.size() == M);
            uint64_t left = c.text_cap;
            for (size_t i = 0; i < M; i++) {
                CHECK(got[i].status == chk[i].status && got[i].digest == chk[i].digest && got[i].verify == chk[i].verify);
                const zarc::FrameReader::Result::Range &r = got[i].range;
                if (i == 7) { CHECK(got[i].status == ZARC_GPU_FRAME_SRCSIZE && r.units == 0 && r.first == 0 && r.taken == 0 && r.start == 0 && r.length == 0 && got[i].data.empty()); continue; }
                const Want &w = want[i];
                CHECK(r.units == w.units && r.first == w.first && r.taken == w.taken && r.start == w.start && r.length == w.length);
                const uint64_t e = std::min<uint64_t>(std::min<uint64_t>(w.length, c.max_bytes ? c.max_bytes : w.length), left);
                CHECK(got[i].data.size() == e && std::memcmp(got[i].data.data(), ents[i].data() + w.start, (size_t)e) == 0);
                left -= e;
            }
            if (g == 1) base = got;
            for (size_t i = 0; i < M; i++) CHECK(got[i].data == base[i].data && got[i].range.start == base[i].range.start && got[i].range.length == base[i].range.length);
        }
    }
    for (int g = 1; g <= 4 && g <= devices; g *= 2) std::printf("range_content_frames on %d device(s) OK\n", g);
    int threw = 0;
    zarc::FrameReader rd(0);
    std::vector<zarc_gpu_range> bad = ranges;
    bad[0].unit = 2;
    try { rd.range_content_frames((const uint8_t *)img.data(), img.size(), wanted, bad); } catch (const zarc::Error &) { threw++; }
    bad = ranges; bad[1].flags = 2;
    try { rd.range_content_frames((const uint8_t *)img.data(), img.size(), wanted, bad); } catch (const zarc::Error &) { threw++; }
    bad = ranges; bad.pop_back();
    try { rd.range_content_frames((const uint8_t *)img.data(), img.size(), wanted, bad); } catch (const zarc::Error &) { threw++; }
    CHECK(threw == 3);
    std::printf("range frames OK (%d device(s) visible)\n", devices);
    return 0;
}
