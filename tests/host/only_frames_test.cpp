// tests/host/only_frames_test.cpp -- zarc::FrameReader::matches_content_frames (zarc_amd/host/zarc_host.hpp) over 1, 2 and 4 handles: the same
// lines, matches and match records for every number of handles, under every pair of caps -- line_cap running out over the merged list among
// them, which makes the shares run once more -- equal to a plain host scan of the entries (a fixed string: every occurrence from the end of
// the one before), to the same literal as a set of one and as an expression, and to lines_content_frames in verdict, count, first and lines.
// Built by tests/test_only_host.py against the emulated library (or the product library on a GPU box).
#include "../../zarc_amd/host/zarc_host.hpp"
#include "../../zarc_amd/csrc/corpus.h"
#include <cstdio>
#include <cstdlib>
#include <sstream>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

typedef zarc::FrameReader::Result::Match Match;
struct RefLine { uint64_t number; std::vector<Match> matches; };
// the reference: per matching line, every occurrence of p that starts at or behind the end of the one before
static std::vector<RefLine> scan(const std::vector<uint8_t> &d, const std::string &p, uint64_t max_line)
{
    std::vector<RefLine> out;
    uint64_t number = 1;
    for (size_t start = 0; start < d.size(); number++) {
        size_t end = start;
        while (end < d.size() && d[end] != '\n') end++;
        RefLine l{number, {}};
        for (size_t at = start; at + p.size() <= end;) {
            if (memcmp(&d[at], p.data(), p.size())) { at++; continue; }
            l.matches.push_back(Match{at, p.size(), number, start, ZARC_GPU_SEARCH_NONE, std::vector<uint8_t>(d.begin() + at, d.begin() + at + std::min<uint64_t>(p.size(), max_line))});
            at += p.size();
        }
        if (!l.matches.empty()) out.push_back(l);
        start = end + 1;
    }
    return out;
}
static bool same(const std::vector<Match> &a, const std::vector<Match> &b, size_t nb, bool which = true)
{
    if (a.size() != nb) return false;
    for (size_t k = 0; k < nb; k++)
        if (a[k].start != b[k].start || a[k].length != b[k].length || a[k].number != b[k].number || a[k].line_start != b[k].line_start || a[k].text != b[k].text ||
            (which && a[k].which != b[k].which)) return false;
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
        for (size_t at = 15; at + 2 * needle.size() <= e.size(); at += 4001) { // several per frame, some sharing a line, every third one doubled
            memcpy(&e[at], needle.data(), needle.size());
            if (at / 4001 % 3 == 0) memcpy(&e[at + needle.size()], needle.data(), needle.size());
        }
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
    wanted[7].uncompressed += 1; // a frame that does not decode: no line, no match, no record
    const int devices = zarc_gpu_device_count();
    uint64_t all_lines = 0, all_matches = 0;
    for (size_t i = 0; i < N; i++) if (i != 7) for (const RefLine &l : scan(ents[i], needle, 4096)) { all_lines++; all_matches += l.matches.size(); }
    CHECK(all_lines > 40 && all_matches > all_lines + 10);
    zarc::MatchWhat fixed, as_set, as_rx;
    fixed.text = needle;
    as_set.kind = ZARC_GPU_MATCH_SET; as_set.set = {needle, "no such \x02 thing"};
    as_rx.kind = ZARC_GPU_MATCH_REGEX;
    for (const char ch : needle) { char b[8]; std::snprintf(b, sizeof b, "\\x%02x", (unsigned)(unsigned char)ch); as_rx.text += b; } // the needle as an expression
    struct Caps { uint64_t max_lines, max_line; size_t line_cap, rec_cap; };
    const Caps caps[] = {{0, 4096, (size_t)1 << 20, (size_t)1 << 20}, {3, 5, (size_t)1 << 20, (size_t)1 << 20}, {0, 4096, (size_t)all_lines - 2, (size_t)1 << 20},
                         {0, 4096, (size_t)all_lines / 2, (size_t)all_matches / 3}, {2, 65536, 11, 17}, {0, 4096, (size_t)1 << 20, (size_t)all_matches - 1},
                         {0, 1, 1, 1}, {0, 4096, 0, 10}, {0, 4096, 10, 0}};
    size_t k = 0;
    for (const Caps &c : caps) {
        std::vector<zarc::FrameReader::Result> base;
        for (int g = 1; g <= 4; g *= 2) {
            if (g > devices) break;
            std::vector<int> dev;
            for (int d = 0; d < g; d++) dev.push_back(d);
            zarc::FrameReader rd(dev);
            const auto lines = rd.lines_content_frames((const uint8_t *)img.data(), img.size(), wanted, needle, false, c.max_lines, c.max_line, 0);
            const auto got = rd.matches_content_frames((const uint8_t *)img.data(), img.size(), wanted, fixed, false, c.max_lines, c.max_line, c.line_cap, c.rec_cap);
            CHECK(got.size() == N);
            uint64_t lines_left = c.line_cap;
            size_t left = c.rec_cap;
            for (size_t i = 0; i < N; i++) {
                CHECK(got[i].status == lines[i].status && got[i].digest == lines[i].digest && got[i].verify == lines[i].verify && got[i].data.empty());
                CHECK(got[i].count == lines[i].count && got[i].first == lines[i].first && got[i].lines == lines[i].lines && got[i].line_records.empty());
                if (i == 7) { CHECK(got[i].status == ZARC_GPU_FRAME_SRCSIZE && got[i].lines == 0 && got[i].matches == 0 && got[i].match_records.empty()); continue; }
                const std::vector<RefLine> want = scan(ents[i], needle, c.max_line);
                CHECK(got[i].lines == want.size());
                const uint64_t d = std::min<uint64_t>(std::min<uint64_t>(want.size(), c.max_lines ? c.max_lines : want.size()), lines_left);
                lines_left -= d;
                std::vector<Match> flat;
                for (uint64_t l = 0; l < d; l++) flat.insert(flat.end(), want[l].matches.begin(), want[l].matches.end());
                CHECK(got[i].matches == flat.size());
                const size_t e = std::min(flat.size(), left);
                CHECK(same(got[i].match_records, flat, e));
                left -= e;
            }
            if (g == 1) base = got;
            for (size_t i = 0; i < N; i++)
                CHECK(got[i].lines == base[i].lines && got[i].matches == base[i].matches && same(got[i].match_records, base[i].match_records, base[i].match_records.size()));
            // the same literal as a set and as an expression: the same lines, matches and records (a set's records name the pattern)
            std::vector<uint64_t> set_hits;
            const auto s = rd.matches_content_frames((const uint8_t *)img.data(), img.size(), wanted, as_set, false, c.max_lines, c.max_line, c.line_cap, c.rec_cap, &set_hits);
            const auto r = rd.matches_content_frames((const uint8_t *)img.data(), img.size(), wanted, as_rx, false, c.max_lines, c.max_line, c.line_cap, c.rec_cap);
            uint64_t count = 0;
            for (size_t i = 0; i < N; i++) {
                count += got[i].count;
                CHECK(s[i].lines == got[i].lines && s[i].matches == got[i].matches && same(s[i].match_records, got[i].match_records, got[i].match_records.size(), false));
                for (const Match &m : s[i].match_records) CHECK(m.which == 0);
                CHECK(r[i].lines == got[i].lines && r[i].matches == got[i].matches && same(r[i].match_records, got[i].match_records, got[i].match_records.size()));
            }
            CHECK(set_hits.size() == 2 && set_hits[0] == count && set_hits[1] == 0);
        }
        for (int g = 1; g <= 4 && g <= devices; g *= 2) std::printf("only caps %zu on %d device(s) OK\n", k, g);
        k++;
    }
    zarc::FrameReader rd(0);
    int threw = 0;
    zarc::MatchWhat bad = fixed;
    bad.text = "a\nb";
    try { rd.matches_content_frames((const uint8_t *)img.data(), img.size(), wanted, bad); } catch (const zarc::Error &) { threw++; }
    try { rd.matches_content_frames((const uint8_t *)img.data(), img.size(), wanted, fixed, false, 0, 65537); } catch (const zarc::Error &) { threw++; }
    bad = as_rx; bad.text = "a(";
    try { rd.matches_content_frames((const uint8_t *)img.data(), img.size(), wanted, bad); } catch (const zarc::Error &) { threw++; }
    bad.text = "(a|b)*a(a|b){6}"; // the lines call takes it, the forward table has no room
    CHECK(rd.lines_regex_content_frames((const uint8_t *)img.data(), img.size(), wanted, bad.text).size() == N);
    try { rd.matches_content_frames((const uint8_t *)img.data(), img.size(), wanted, bad); } catch (const zarc::Error &e) { threw += std::string(e.what()).find("needs 129 states") != std::string::npos; }
    bad.kind = 7;
    try { rd.matches_content_frames((const uint8_t *)img.data(), img.size(), wanted, bad); } catch (const zarc::Error &) { threw++; }
    CHECK(threw == 5);
    std::printf("only frames OK (%d device(s) visible)\n", devices);
    return 0;
}
