// tests/host/lines_frames_test.cpp -- zarc::FrameReader::lines_content_frames (zarc_amd/host/zarc_host.hpp) over 1, 2 and 4 handles: the
// same lines and line records for every number of handles, under every cap, equal to a plain host scan of the entries line by line and to
// search_content_frames in verdict, count and first.  Built by tests/test_lines_host.py against the emulated library (or the product
// library on a GPU box).
#include "../../zarc_amd/host/zarc_host.hpp"
#include "../../zarc_amd/csrc/corpus.h"
#include <cstdio>
#include <cstdlib>
#include <sstream>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

typedef zarc::FrameReader::Result::Line Line;
static unsigned char fold(unsigned char c, bool icase) { return icase && c >= 'A' && c <= 'Z' ? (unsigned char)(c | 0x20) : c; }
// the reference: line by line, every start position byte by byte
static std::vector<Line> scan(const std::vector<uint8_t> &d, const std::string &p, bool icase, uint64_t max_line)
{
    std::vector<Line> out;
    uint64_t number = 1;
    for (size_t start = 0; start < d.size(); number++) {
        size_t end = start;
        while (end < d.size() && d[end] != '\n') end++;
        for (size_t at = start; at + p.size() <= end; at++) {
            size_t k = 0;
            while (k < p.size() && fold(d[at + k], icase) == fold((unsigned char)p[k], icase)) k++;
            if (k == p.size()) { out.push_back(Line{start, end - start, number, at, std::vector<uint8_t>(d.begin() + start, d.begin() + start + std::min<uint64_t>(end - start, max_line))}); break; }
        }
        start = end + 1;
    }
    return out;
}
static bool same(const std::vector<Line> &a, const std::vector<Line> &b, size_t nb)
{
    if (a.size() != nb) return false;
    for (size_t k = 0; k < nb; k++)
        if (a[k].start != b[k].start || a[k].length != b[k].length || a[k].number != b[k].number || a[k].match != b[k].match || a[k].text != b[k].text) return false;
    return true;
}

int main()
{
    const size_t sizes[] = {0, 1, 300, 70000, 200000, 65536, 5000, 131073, 65543, 9};
    const size_t N = sizeof sizes / sizeof sizes[0];
    const std::string needle = "\x01Zarc\xfeNeedle";
    std::vector<std::vector<uint8_t>> ents;
    std::vector<const void *> ptr;
    std::vector<size_t> len;
    for (size_t i = 0; i < N; i++) {
        ents.emplace_back(sizes[i]);
        zarc_corpus_entry(ents.back().data(), sizes[i], 9700 + i, 0);
        std::vector<uint8_t> &e = ents.back();
        for (size_t at = 15; at + needle.size() <= e.size(); at += 4001) memcpy(&e[at], needle.data(), needle.size()); // several per frame, some sharing a line
        if (e.size() >= 65543) { e[65536 - 6] = '\n'; memcpy(&e[65536 - 5], needle.data(), needle.size()); memcpy(&e[e.size() - needle.size()], needle.data(), needle.size()); }
        if (e.size() == 5000) for (size_t k = 0; k < needle.size(); k++) e[1000 + k] = (uint8_t)std::toupper((unsigned char)needle[k]);
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
    wanted[7].uncompressed += 1; // a frame that does not decode: no line, no record
    const int devices = zarc_gpu_device_count();
    struct Caps { uint64_t max_lines, max_line; size_t rec_cap; };
    for (const bool icase : {false, true}) {
        uint64_t total = 0;
        for (size_t i = 0; i < N; i++) if (i != 7) total += scan(ents[i], needle, icase, 4096).size();
        CHECK(total > 60);
        const Caps caps[] = {{0, 4096, (size_t)1 << 20}, {3, 16, (size_t)1 << 20}, {0, 4096, (size_t)total - 2}, {5, 65536, 17}, {0, 1, 1}, {0, 4096, 0}};
        for (const Caps &c : caps) {
            std::vector<zarc::FrameReader::Result> base;
            for (int g = 1; g <= 4; g *= 2) {
                if (g > devices) break;
                std::vector<int> dev;
                for (int d = 0; d < g; d++) dev.push_back(d);
                zarc::FrameReader rd(dev);
                const auto srch = rd.search_content_frames((const uint8_t *)img.data(), img.size(), wanted, needle, icase);
                const auto got = rd.lines_content_frames((const uint8_t *)img.data(), img.size(), wanted, needle, icase, c.max_lines, c.max_line, c.rec_cap);
                CHECK(got.size() == N);
                size_t left = c.rec_cap;
                for (size_t i = 0; i < N; i++) {
                    CHECK(got[i].status == srch[i].status && got[i].digest == srch[i].digest && got[i].verify == srch[i].verify && got[i].data.empty());
                    CHECK(got[i].count == srch[i].count && got[i].first == srch[i].first);
                    if (i == 7) { CHECK(got[i].status == ZARC_GPU_FRAME_SRCSIZE && got[i].lines == 0 && got[i].line_records.empty()); continue; }
                    const std::vector<Line> want = scan(ents[i], needle, icase, c.max_line);
                    CHECK(got[i].lines == want.size());
                    const size_t d = (size_t)std::min<uint64_t>(std::min<uint64_t>(want.size(), c.max_lines ? c.max_lines : want.size()), left);
                    CHECK(same(got[i].line_records, want, d));
                    left -= d;
                }
                if (g == 1) base = got;
                for (size_t i = 0; i < N; i++) CHECK(got[i].lines == base[i].lines && same(got[i].line_records, base[i].line_records, base[i].line_records.size()));
            }
        }
        for (int g = 1; g <= 4 && g <= devices; g *= 2) std::printf("lines_content_frames%s on %d device(s) OK\n", icase ? " (icase)" : "", g);
    }
    int threw = 0;
    zarc::FrameReader rd(0);
    try { rd.lines_content_frames((const uint8_t *)img.data(), img.size(), wanted, std::string("a\nb")); } catch (const zarc::Error &) { threw++; }
    try { rd.lines_content_frames((const uint8_t *)img.data(), img.size(), wanted, needle, false, 0, 65537); } catch (const zarc::Error &) { threw++; }
    try { rd.lines_content_frames((const uint8_t *)img.data(), img.size(), wanted, std::string()); } catch (const zarc::Error &) { threw++; }
    CHECK(threw == 3);
    std::printf("lines frames OK (%d device(s) visible)\n", devices);
    return 0;
}
