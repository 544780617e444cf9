// tests/host/select_frames_test.cpp -- the LineSelect argument of zarc::FrameReader's three lines calls (zarc_amd/host/zarc_host.hpp) over 1, 2 and
// 4 handles: the same hit lines, selected lines and line records for every number of handles, under every cap, equal to a plain host scan of
// the entries line by line, and to search_content_frames in verdict, count and first.  Built by tests/test_select_host.py against the emulated
// library (or the product library on a GPU box).
#include "../../zarc_amd/host/zarc_host.hpp"
#include "../../zarc_amd/csrc/corpus.h"
#include <cstdio>
#include <cstdlib>
#include <sstream>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

typedef zarc::FrameReader::Result::Line Line;
// the reference: every line with its lowest match (ZARC_GPU_SEARCH_NONE: none), then H and S by their definitions
static std::vector<Line> scan(const std::vector<uint8_t> &d, const std::string &p, const zarc::LineSelect &sel, uint64_t max_line, uint64_t *hits)
{
    std::vector<Line> all;
    uint64_t number = 1;
    for (size_t start = 0; start < d.size(); number++) {
        size_t end = start;
        while (end < d.size() && d[end] != '\n') end++;
        uint64_t match = ZARC_GPU_SEARCH_NONE;
        for (size_t at = start; at + p.size() <= end && match == ZARC_GPU_SEARCH_NONE; at++)
            if (!memcmp(&d[at], p.data(), p.size())) match = at;
        all.push_back(Line{start, end - start, number, match, std::vector<uint8_t>(d.begin() + start, d.begin() + start + std::min<uint64_t>(end - start, max_line))});
        start = end + 1;
    }
    std::vector<bool> hit(all.size());
    *hits = 0;
    for (size_t k = 0; k < all.size(); k++) { hit[k] = (all[k].match != ZARC_GPU_SEARCH_NONE) != sel.invert; *hits += hit[k]; }
    std::vector<Line> out;
    for (size_t k = 0; k < all.size(); k++) {
        bool in = false;
        for (size_t h = k - std::min<uint64_t>(k, sel.after); h <= k && !in; h++) in = hit[h];                                  // a hit within `after` in front
        for (size_t h = k; h < all.size() && h - k <= sel.before && !in; h++) in = hit[h];                                      // ... within `before` behind
        if (in) out.push_back(all[k]);
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
        zarc_corpus_entry(ents.back().data(), sizes[i], 9800 + i, 0);
        std::vector<uint8_t> &e = ents.back();
        for (size_t at = 15; at + needle.size() <= e.size(); at += 4001) memcpy(&e[at], needle.data(), needle.size()); // several per frame, some sharing a line
        if (e.size() >= 65543) { e[65536 - 6] = '\n'; memcpy(&e[65536 - 5], needle.data(), needle.size()); memcpy(&e[e.size() - needle.size()], needle.data(), needle.size()); }
        if (e.size() == 9) e[4] = '\n';
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
    const zarc::LineSelect sels[] = {{false, 2, 2}, {true, 0, 0}, {true, 1, 3}, {false, 0xFFFFFFFFu, 0}, {false, 0, 1}};
    const std::vector<std::string> set = {needle, "no such \x02 thing"};
    std::string rx;
    for (const char ch : needle) { char b[8]; std::snprintf(b, sizeof b, "\\x%02x", (unsigned)(unsigned char)ch); rx += b; } // the needle as an expression
    for (const zarc::LineSelect &sel : sels) {
        uint64_t total = 0, hits = 0, context = 0;
        for (size_t i = 0; i < N; i++) if (i != 7) { const auto w = scan(ents[i], needle, sel, 4096, &hits); total += w.size(); context += w.size() - hits; }
        CHECK(total > 60 && (context > 10 || !(sel.before || sel.after)));
        const Caps caps[] = {{0, 4096, (size_t)1 << 20}, {3, 16, (size_t)1 << 20}, {0, 4096, (size_t)total - 2}, {5, 65536, 17}, {0, 1, 1}, {0, 4096, 0}};
        for (const Caps &c : caps) {
            std::vector<zarc::FrameReader::Result> base;
            for (int g = 1; g <= 4; g *= 2) {
                if (g > devices) break;
                std::vector<int> dev;
                for (int d = 0; d < g; d++) dev.push_back(d);
                zarc::FrameReader rd(dev);
                const auto srch = rd.search_content_frames((const uint8_t *)img.data(), img.size(), wanted, needle, false);
                const auto got = rd.lines_content_frames((const uint8_t *)img.data(), img.size(), wanted, needle, false, c.max_lines, c.max_line, c.rec_cap, sel);
                CHECK(got.size() == N);
                size_t left = c.rec_cap;
                for (size_t i = 0; i < N; i++) {
                    CHECK(got[i].status == srch[i].status && got[i].digest == srch[i].digest && got[i].verify == srch[i].verify && got[i].data.empty());
                    CHECK(got[i].count == srch[i].count && got[i].first == srch[i].first); // the inversion does not touch them
                    if (i == 7) { CHECK(got[i].status == ZARC_GPU_FRAME_SRCSIZE && got[i].lines == 0 && got[i].selected == 0 && got[i].line_records.empty()); continue; }
                    const std::vector<Line> want = scan(ents[i], needle, sel, c.max_line, &hits);
                    CHECK(got[i].lines == hits && got[i].selected == want.size());
                    const size_t d = (size_t)std::min<uint64_t>(std::min<uint64_t>(want.size(), c.max_lines ? c.max_lines : want.size()), left);
                    CHECK(same(got[i].line_records, want, d));
                    left -= d;
                }
                if (g == 1) base = got;
                for (size_t i = 0; i < N; i++)
                    CHECK(got[i].lines == base[i].lines && got[i].selected == base[i].selected && same(got[i].line_records, base[i].line_records, base[i].line_records.size()));
                // the same literal as a set and as an expression: the same lines, selected and records
                std::vector<uint64_t> set_hits;
                const auto as_set = rd.lines_set_content_frames((const uint8_t *)img.data(), img.size(), wanted, set, false, c.max_lines, c.max_line, c.rec_cap, &set_hits, sel);
                const auto as_rx = rd.lines_regex_content_frames((const uint8_t *)img.data(), img.size(), wanted, rx, false, c.max_lines, c.max_line, c.rec_cap, sel);
                uint64_t count = 0;
                for (size_t i = 0; i < N; i++) {
                    count += got[i].count;
                    CHECK(as_set[i].lines == got[i].lines && as_set[i].selected == got[i].selected && same(as_set[i].line_records, got[i].line_records, got[i].line_records.size()));
                    CHECK(as_rx[i].lines == got[i].lines && as_rx[i].selected == got[i].selected && same(as_rx[i].line_records, got[i].line_records, got[i].line_records.size()));
                }
                CHECK(set_hits.size() == 2 && set_hits[0] == count && set_hits[1] == 0);
            }
        }
        for (int g = 1; g <= 4 && g <= devices; g *= 2)
            std::printf("select %s-B %u -A %u on %d device(s) OK\n", sel.invert ? "-v " : "", (unsigned)sel.before, (unsigned)sel.after, g);
    }
    // an inactive selection is the plain lines call
    zarc::FrameReader rd(0);
    const auto plain_lines = rd.lines_content_frames((const uint8_t *)img.data(), img.size(), wanted, needle);
    const auto off = rd.lines_content_frames((const uint8_t *)img.data(), img.size(), wanted, needle, false, 0, 4096, (size_t)1 << 20, zarc::LineSelect());
    for (size_t i = 0; i < N; i++) CHECK(off[i].lines == plain_lines[i].lines && off[i].selected == off[i].lines && same(off[i].line_records, plain_lines[i].line_records, plain_lines[i].line_records.size()));
    int threw = 0;
    const zarc::LineSelect v{true, 0, 0};
    try { rd.lines_content_frames((const uint8_t *)img.data(), img.size(), wanted, std::string("a\nb"), false, 0, 4096, 10, v); } catch (const zarc::Error &) { threw++; }
    try { rd.lines_content_frames((const uint8_t *)img.data(), img.size(), wanted, needle, false, 0, 65537, 10, v); } catch (const zarc::Error &) { threw++; }
    try { rd.lines_regex_content_frames((const uint8_t *)img.data(), img.size(), wanted, std::string("a("), false, 0, 4096, 10, v); } catch (const zarc::Error &) { threw++; }
    CHECK(threw == 3);
    std::printf("select frames OK (%d device(s) visible)\n", devices);
    return 0;
}
