// tests/host/search_frames_test.cpp -- zarc::FrameReader::search_content_frames (zarc_amd/host/zarc_host.hpp) over 1, 2 and 4 handles: the
// same {digest, verify, status, count, first} for every number of handles, equal to check_content_frames in the verdict and to a plain
// host scan of the entries in the counts.  Built by tests/test_search_host.py against the emulated library (or the product library on
// a GPU box).
#include "../../zarc_amd/host/zarc_host.hpp"
#include "../../zarc_amd/csrc/corpus.h"
#include <cstdio>
#include <cstdlib>
#include <sstream>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static unsigned char fold(unsigned char c, bool icase) { return icase && c >= 'A' && c <= 'Z' ? (unsigned char)(c | 0x20) : c; }
// the reference: every start position, byte by byte
static void scan(const std::vector<uint8_t> &d, const std::string &p, bool icase, uint64_t *count, std::optional<uint64_t> *first)
{
    *count = 0; first->reset();
    for (size_t at = 0; at + p.size() <= d.size(); at++) {
        size_t k = 0;
        while (k < p.size() && fold(d[at + k], icase) == fold((unsigned char)p[k], icase)) k++;
        if (k == p.size()) { if (!*count) *first = at; ++*count; }
    }
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
        zarc_corpus_entry(ents.back().data(), sizes[i], 9600 + i, (int)(i & 3));
        std::vector<uint8_t> &e = ents.back();
        if (e.size() >= 65543) { memcpy(&e[65536 - 5], needle.data(), needle.size()); memcpy(&e[e.size() - needle.size()], needle.data(), needle.size()); }
        if (e.size() == 5000) { memcpy(&e[15], needle.data(), needle.size()); for (size_t k = 0; k < needle.size(); k++) e[1000 + k] = (uint8_t)std::toupper((unsigned char)needle[k]); }
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
    img[(size_t)wanted[4].offset + (size_t)wanted[4].length / 2] ^= 0x5A; // store mode, no checksum: the content differs from its digest
    wanted[7].uncompressed += 1;                                            // and a frame that does not decode
    const int devices = zarc_gpu_device_count();
    for (const bool icase : {false, true}) {
        std::vector<zarc::FrameReader::Result> base;
        for (int g = 1; g <= 4; g *= 2) {
            if (g > devices) break;
            std::vector<int> dev;
            for (int d = 0; d < g; d++) dev.push_back(d);
            zarc::FrameReader rd(dev);
            const auto chk = rd.check_content_frames((const uint8_t *)img.data(), img.size(), wanted);
            const auto got = rd.search_content_frames((const uint8_t *)img.data(), img.size(), wanted, needle, icase);
            CHECK(got.size() == N && chk.size() == N);
            for (size_t i = 0; i < N; i++) {
                CHECK(got[i].status == chk[i].status && got[i].digest == chk[i].digest && got[i].verify == chk[i].verify && got[i].data.empty());
                const bool decoded = got[i].status == ZARC_GPU_FRAME_OK || got[i].status == ZARC_GPU_FRAME_DIGEST;
                if (!decoded) { CHECK(got[i].count == 0 && !got[i].first.has_value()); continue; }
                if (i == 4) continue; // damaged content: searched, but not what the entry holds
                uint64_t count; std::optional<uint64_t> first;
                scan(ents[i], needle, icase, &count, &first);
                CHECK(got[i].count == count && got[i].first == first);
            }
            CHECK(got[4].status == ZARC_GPU_FRAME_DIGEST && got[7].status == ZARC_GPU_FRAME_SRCSIZE);
            CHECK(got[6].count == (icase ? 2u : 1u) && got[6].first.value_or(99) == 15 && got[8].count == 1 && got[8].first.value_or(0) == 65536 - 5 && got[3].count == 2);
            if (g == 1) base = got;
            for (size_t i = 0; i < N; i++)
                CHECK(got[i].status == base[i].status && got[i].digest == base[i].digest && got[i].verify == base[i].verify && got[i].count == base[i].count && got[i].first == base[i].first);
            std::printf("search_content_frames%s on %d device(s) OK\n", icase ? " (icase)" : "", g);
        }
    }
    bool threw = false;
    try { zarc::FrameReader rd(0); rd.search_content_frames((const uint8_t *)img.data(), img.size(), wanted, std::string()); } catch (const zarc::Error &) { threw = true; }
    CHECK(threw);
    std::printf("search frames OK (%d device(s) visible)\n", devices);
    return 0;
}
