// tests/host/set_frames_test.cpp -- zarc::FrameReader::search_set_content_frames and lines_set_content_frames (zarc_amd/host/zarc_host.hpp)
// over 1, 2 and 4 handles.  The program judges nothing but that every number of handles gives the same answer: it reads the entries
// (files 0 .. N-1 of the directory argv[1]) and the patterns (the LF-terminated lines of argv[1]/patterns), packs the entries in store
// mode, gives frame 4 a wrong expected digest and frame 7 a wrong size, and prints what one handle answered.  tests/test_set_host.py
// compares that with Python's `re` over the same bytes.  Built there against the emulated library (or the product library on a GPU box).
#include "../../zarc_amd/host/zarc_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static std::string slurp(const std::string &path)
{
    std::ifstream in(path, std::ios::binary);
    return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

static bool same(const std::vector<zarc::FrameReader::Result> &a, const std::vector<zarc::FrameReader::Result> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i].status != b[i].status || !(a[i].digest == b[i].digest) || a[i].verify != b[i].verify || a[i].count != b[i].count || a[i].first != b[i].first ||
            a[i].which != b[i].which || a[i].lines != b[i].lines || a[i].line_records.size() != b[i].line_records.size())
            return false;
        for (size_t k = 0; k < a[i].line_records.size(); k++) {
            const auto &x = a[i].line_records[k], &y = b[i].line_records[k];
            if (x.start != y.start || x.length != y.length || x.number != y.number || x.match != y.match || x.text != y.text) return false;
        }
    }
    return true;
}

int main(int argc, char **argv)
{
    CHECK(argc == 3);
    const std::string dir = argv[1];
    const size_t N = (size_t)std::atoi(argv[2]);
    CHECK(N >= 8);
    std::vector<std::string> ents, pats;
    for (size_t i = 0; i < N; i++) ents.push_back(slurp(dir + "/" + std::to_string(i)));
    {
        std::istringstream in(slurp(dir + "/patterns"));
        for (std::string line; std::getline(in, line);) pats.push_back(line);
    }
    std::vector<const void *> ptr;
    std::vector<size_t> len;
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
    const std::string img = plain.str();
    wanted[4].digest.bytes[0] ^= 0x5A;  // the content differs from the digest asked for: searched all the same
    wanted[7].uncompressed += 1;        // and a frame that does not decode
    const int devices = zarc_gpu_device_count();
    for (const bool icase : {false, true}) {
        std::vector<zarc::FrameReader::Result> base, base_lines;
        std::vector<uint64_t> base_hits, base_lhits;
        for (int g = 1; g <= 4; g *= 2) {
            if (g > devices) break;
            std::vector<int> dev;
            for (int d = 0; d < g; d++) dev.push_back(d);
            zarc::FrameReader rd(dev);
            std::vector<uint64_t> hits, lhits;
            const auto chk = rd.check_content_frames((const uint8_t *)img.data(), img.size(), wanted);
            const auto got = rd.search_set_content_frames((const uint8_t *)img.data(), img.size(), wanted, pats, icase, &hits);
            const auto lin = rd.lines_set_content_frames((const uint8_t *)img.data(), img.size(), wanted, pats, icase, 3, 64, 7, &lhits);
            CHECK(got.size() == N && lin.size() == N && hits.size() == pats.size() && lhits == hits);
            for (size_t i = 0; i < N; i++) {
                CHECK(got[i].status == chk[i].status && got[i].digest == chk[i].digest && got[i].verify == chk[i].verify && got[i].data.empty());
                CHECK(lin[i].status == got[i].status && lin[i].count == got[i].count && lin[i].first == got[i].first && lin[i].which == got[i].which);
            }
            CHECK(got[4].status == ZARC_GPU_FRAME_DIGEST && got[7].status == ZARC_GPU_FRAME_SRCSIZE && got[7].count == 0 && !got[7].which.has_value());
            if (g == 1) {
                base = got; base_lines = lin; base_hits = hits; base_lhits = lhits;
                for (size_t i = 0; i < N; i++) {
                    std::printf("R %d %zu %d %llu %lld %lld %llu\n", (int)icase, i, got[i].status, (unsigned long long)got[i].count,
                                got[i].first ? (long long)*got[i].first : -1ll, got[i].which ? (long long)*got[i].which : -1ll, (unsigned long long)lin[i].lines);
                    for (const auto &l : lin[i].line_records)
                        std::printf("L %d %zu %llu %llu %llu %llu %zu\n", (int)icase, i, (unsigned long long)l.start, (unsigned long long)l.length,
                                    (unsigned long long)l.number, (unsigned long long)l.match, l.text.size());
                }
                std::printf("H %d", (int)icase);
                for (uint64_t v : hits) std::printf(" %llu", (unsigned long long)v);
                std::printf("\n");
            }
            CHECK(same(got, base) && same(lin, base_lines) && hits == base_hits && lhits == base_lhits);
            std::printf("search_set_content_frames%s on %d device(s) OK\n", icase ? " (icase)" : "", g);
        }
    }
    int threw = 0;
    zarc::FrameReader rd(0);
    try { rd.search_set_content_frames((const uint8_t *)img.data(), img.size(), wanted, {}); } catch (const zarc::Error &) { threw++; }
    try { rd.search_set_content_frames((const uint8_t *)img.data(), img.size(), wanted, {"a", ""}); } catch (const zarc::Error &) { threw++; }
    try { rd.lines_set_content_frames((const uint8_t *)img.data(), img.size(), wanted, {"a", "b\nc"}); } catch (const zarc::Error &) { threw++; }
    try { rd.search_set_content_frames((const uint8_t *)img.data(), img.size(), wanted, std::vector<std::string>(1025, "x")); } catch (const zarc::Error &) { threw++; }
    CHECK(threw == 4);
    std::printf("set frames OK (%d device(s) visible)\n", devices);
    return 0;
}
