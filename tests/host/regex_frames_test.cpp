// tests/host/regex_frames_test.cpp -- zarc::FrameReader::search_regex_content_frames and lines_regex_content_frames
// (zarc_amd/host/zarc_host.hpp) over 1, 2 and 4 handles.  The program judges nothing but that every number of handles gives the same
// answer: it reads the entries (files 0 .. N-1 of the directory argv[1]) and the expressions (the LF-terminated lines of
// argv[1]/expressions), packs the entries in store mode, gives frame 4 a wrong expected digest and frame 7 a wrong size, and prints what
// one handle answered.  tests/test_regex_host.py compares that with Python's `re` over the same bytes.  Built there against the emulated
// library (or the product library on a GPU box).
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
            a[i].lines != b[i].lines || a[i].line_records.size() != b[i].line_records.size())
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
    std::vector<std::string> ents, exprs;
    for (size_t i = 0; i < N; i++) ents.push_back(slurp(dir + "/" + std::to_string(i)));
    {
        std::istringstream in(slurp(dir + "/expressions"));
        for (std::string line; std::getline(in, line);) exprs.push_back(line);
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
    for (size_t x = 0; x < exprs.size(); x++)
        for (const bool icase : {false, true}) {
            std::vector<zarc::FrameReader::Result> base, base_lines;
            for (int g = 1; g <= 4; g *= 2) {
                if (g > devices) break;
                std::vector<int> dev;
                for (int d = 0; d < g; d++) dev.push_back(d);
                zarc::FrameReader rd(dev);
                const auto chk = rd.check_content_frames((const uint8_t *)img.data(), img.size(), wanted);
                const auto got = rd.search_regex_content_frames((const uint8_t *)img.data(), img.size(), wanted, exprs[x], icase);
                const auto lin = rd.lines_regex_content_frames((const uint8_t *)img.data(), img.size(), wanted, exprs[x], icase, 3, 64, 7);
                CHECK(got.size() == N && lin.size() == N);
                for (size_t i = 0; i < N; i++) {
                    CHECK(got[i].status == chk[i].status && got[i].digest == chk[i].digest && got[i].verify == chk[i].verify && got[i].data.empty());
                    CHECK(lin[i].status == got[i].status && lin[i].count == got[i].count && lin[i].first == got[i].first);
                }
                CHECK(got[4].status == ZARC_GPU_FRAME_DIGEST && got[7].status == ZARC_GPU_FRAME_SRCSIZE && got[7].count == 0 && !got[7].first.has_value());
                if (g == 1) {
                    base = got; base_lines = lin;
                    for (size_t i = 0; i < N; i++) {
                        std::printf("R %zu %d %zu %d %llu %lld %llu\n", x, (int)icase, i, got[i].status, (unsigned long long)got[i].count,
                                    got[i].first ? (long long)*got[i].first : -1ll, (unsigned long long)lin[i].lines);
                        for (const auto &l : lin[i].line_records)
                            std::printf("L %zu %d %zu %llu %llu %llu %llu %zu\n", x, (int)icase, i, (unsigned long long)l.start, (unsigned long long)l.length,
                                        (unsigned long long)l.number, (unsigned long long)l.match, l.text.size());
                    }
                }
                CHECK(same(got, base) && same(lin, base_lines));
                std::printf("search_regex_content_frames %zu%s on %d device(s) OK\n", x, icase ? " (icase)" : "", g);
            }
        }
    int param = 0, unsupported = 0;
    zarc::FrameReader rd(0);
    for (const char *bad : {"", "a(b", "x*", "a\nb", "a**", "\\b"})
        try { rd.search_regex_content_frames((const uint8_t *)img.data(), img.size(), wanted, bad); } catch (const zarc::Error &e) { param += std::string(e.what()).find("offset") != std::string::npos; }
    try { rd.lines_regex_content_frames((const uint8_t *)img.data(), img.size(), wanted, "[b-a]"); } catch (const zarc::Error &e) { param += std::string(e.what()).find("offset 1") != std::string::npos; }
    try { rd.lines_regex_content_frames((const uint8_t *)img.data(), img.size(), wanted, "ab", false, 0, 0); } catch (const zarc::Error &) { param++; }
    try { rd.search_regex_content_frames((const uint8_t *)img.data(), img.size(), wanted, ".{7}a"); } catch (const zarc::Error &e) { unsupported += std::string(e.what()).find("256 states") != std::string::npos; }
    CHECK(param == 8 && unsupported == 1);
    std::printf("regex frames OK (%d device(s) visible)\n", devices);
    return 0;
}
