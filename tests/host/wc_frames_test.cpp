// tests/host/wc_frames_test.cpp -- zarc::FrameReader::count_content_frames (zarc_amd/host/zarc_host.hpp) over 1, 2 and 4 handles: the same
// counts for every number of handles, equal to a plain host walk of the entries and to check_content_frames in verdict.  Built by
// tests/test_wc_host.py against the emulated library (or the product library on a GPU box).
#include "../../zarc_amd/host/zarc_host.hpp"
#include "../../zarc_amd/csrc/corpus.h"
#include <cstdio>
#include <cstdlib>
#include <sstream>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

struct Want { uint64_t lines = 0, words = 0, chars = 0, max_line = 0, max_line_start = 0, max_line_no = 0; };
static bool sp(uint8_t c) { return c == 0x20 || (c >= 0x09 && c <= 0x0D); }
// the reference: the definition of include/zarc_gpu.h, byte by byte
static Want walk(const std::vector<uint8_t> &d)
{
    Want w;
    if (d.empty()) return w;
    uint64_t start = 0, no = 1;
    bool have = false;
    auto piece = [&](uint64_t end) { // [start, end) is a piece; only a longer one replaces the best
        if (!have || end - start > w.max_line) { w.max_line = end - start; w.max_line_start = start; w.max_line_no = no; have = true; }
    };
    for (size_t p = 0; p < d.size(); p++) {
        if (!sp(d[p]) && (p == 0 || sp(d[p - 1]))) w.words++;
        if ((d[p] & 0xC0) != 0x80) w.chars++;
        if (d[p] == '\n') { w.lines++; piece(p); start = p + 1; no++; }
    }
    piece(d.size());
    return w;
}

int main()
{
    const size_t sizes[] = {0, 1, 300, 70000, 200000, 65536, 5000, 131073, 65543, 9, 70000, 300, 33 * 65536 + 5};
    const int kinds[] = {0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 1, 3, 0};
    const size_t N = sizeof sizes / sizeof sizes[0];
    std::vector<std::vector<uint8_t>> ents;
    std::vector<const void *> ptr;
    std::vector<size_t> len;
    for (size_t i = 0; i < N; i++) {
        ents.emplace_back(sizes[i]);
        zarc_corpus_entry(ents.back().data(), sizes[i], 9900 + i, kinds[i]);
        std::vector<uint8_t> &e = ents.back();
        if (e.size() >= 65543) { e[65535] = '\n'; e[65536] = '\n'; }
        if (i == 4) for (size_t p = 65000; p < 66500; p++) if (e[p] == '\n') e[p] = 0xC3 + (p & 1) * (0xA9 - 0xC3); // a long line across the seam, of two-byte characters
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
    wanted[7].uncompressed += 1; // a frame that does not decode: all zero
    wanted.push_back(wanted[4]); ents.push_back(ents[4]); // the same frame twice
    const size_t M = wanted.size();
    std::vector<Want> want;
    for (size_t i = 0; i < M; i++) want.push_back(walk(ents[i]));
    CHECK(want[4].lines > 100 && want[4].max_line >= 1500 && want[4].max_line_start < 65536 && want[4].chars < 200000 && want[12].lines > 1000 && want[6].chars < 5000);
    CHECK(want[1].max_line_no == 1 && want[0].max_line_no == 0);
    const int devices = zarc_gpu_device_count();
    std::vector<zarc::FrameReader::Result> base;
    for (int g = 1; g <= 4; g *= 2) {
        if (g > devices) break;
        std::vector<int> dev;
        for (int d = 0; d < g; d++) dev.push_back(d);
        zarc::FrameReader rd(dev);
        const auto chk = rd.check_content_frames((const uint8_t *)img.data(), img.size(), wanted);
        const auto got = rd.count_content_frames((const uint8_t *)img.data(), img.size(), wanted);
        CHECK(got.size() == M);
        for (size_t i = 0; i < M; i++) {
            CHECK(got[i].status == chk[i].status && got[i].digest == chk[i].digest && got[i].verify == chk[i].verify && got[i].data.empty());
            const zarc::FrameReader::Result::Count &c = got[i].wc;
            if (i == 7) { CHECK(got[i].status == ZARC_GPU_FRAME_SRCSIZE && !c.lines && !c.words && !c.chars && !c.max_line && !c.max_line_start && !c.max_line_no); continue; }
            const Want &w = want[i];
            CHECK(got[i].status == ZARC_GPU_FRAME_OK && got[i].verify.value_or(false));
            CHECK(c.lines == w.lines && c.words == w.words && c.chars == w.chars);
            CHECK(c.max_line == w.max_line && c.max_line_start == w.max_line_start && c.max_line_no == w.max_line_no);
        }
        if (g == 1) base = got;
        for (size_t i = 0; i < M; i++)
            CHECK(got[i].wc.lines == base[i].wc.lines && got[i].wc.words == base[i].wc.words && got[i].wc.chars == base[i].wc.chars &&
                  got[i].wc.max_line == base[i].wc.max_line && got[i].wc.max_line_start == base[i].wc.max_line_start &&
                  got[i].wc.max_line_no == base[i].wc.max_line_no);
    }
    for (int g = 1; g <= 4 && g <= devices; g *= 2) std::printf("count_content_frames on %d device(s) OK\n", g);
    zarc::FrameReader rd(0);
    CHECK(rd.count_content_frames((const uint8_t *)img.data(), img.size(), std::vector<zarc::Frame>()).empty());
    std::printf("count frames OK (%d device(s) visible)\n", devices);
    return 0;
}
