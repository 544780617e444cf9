// tests/host/compare_frames_test.cpp -- zarc::FrameReader::compare_content_frames (zarc_amd/host/zarc_host.hpp) over 1, 2 and 4 handles: the
// same results for every number of handles, equal to a plain host walk of both sides and to check_content_frames in verdict.  Built by
// tests/test_compare_host.py against the emulated library (or the product library on a GPU box).
#include "../../zarc_amd/host/zarc_host.hpp"
#include "../../zarc_amd/csrc/corpus.h"
#include <cstdio>
#include <cstdlib>
#include <sstream>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

struct Want { uint32_t relation = 0, byte_a = 0, byte_b = 0; uint64_t prefix = 0, line = 0, differing = 0, suffix = 0; };
// the reference: the table of include/zarc_gpu.h, byte by byte
static Want walk(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b)
{
    Want w;
    const uint64_t la = a.size(), lb = b.size(), common = la < lb ? la : lb;
    w.prefix = common;
    for (uint64_t p = common; p-- > 0;) if (a[p] != b[p]) { w.differing++; w.prefix = p; }
    w.relation = w.differing ? ZARC_GPU_CMP_DIFFER : la == lb ? ZARC_GPU_CMP_EQUAL : la < lb ? ZARC_GPU_CMP_FRAME_IS_PREFIX : ZARC_GPU_CMP_OTHER_IS_PREFIX;
    w.line = 1;
    for (uint64_t p = 0; p < w.prefix; p++) if (a[p] == '\n') w.line++;
    w.byte_a = w.prefix < la ? a[w.prefix] : ZARC_GPU_CMP_EOF;
    w.byte_b = w.prefix < lb ? b[w.prefix] : ZARC_GPU_CMP_EOF;
    while (w.suffix < common - w.prefix && a[la - 1 - w.suffix] == b[lb - 1 - w.suffix]) w.suffix++;
    return w;
}
static bool same(const zarc::FrameReader::Result::Compare &c, const Want &w)
{
    return c.relation == w.relation && c.byte_a == w.byte_a && c.byte_b == w.byte_b && c.prefix == w.prefix && c.line == w.line && c.differing == w.differing &&
           c.suffix == w.suffix;
}

int main()
{
    const size_t sizes[] = {0, 1, 300, 70000, 200000, 65536, 5000, 131073, 65543, 9, 70000, 300, 33 * 65536 + 5};
    const int kinds[] = {0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 1, 3, 0};
    const size_t N = sizeof sizes / sizeof sizes[0];
    std::vector<std::vector<uint8_t>> ents, oth;
    std::vector<const void *> ptr;
    std::vector<size_t> len;
    for (size_t i = 0; i < N; i++) {
        ents.emplace_back(sizes[i]);
        zarc_corpus_entry(ents.back().data(), sizes[i], 9950 + i, kinds[i]);
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
    wanted.push_back(wanted[4]); ents.push_back(ents[4]); // the same frame in two pairs, each with its own other side
    const size_t M = wanted.size();
    // the other sides: the same, one byte changed, a piece inserted, cut short, grown, empty
    for (size_t i = 0; i < M; i++) {
        std::vector<uint8_t> o = ents[i];
        switch (i % 6) {
        case 1: if (!o.empty()) o[o.size() / 2] ^= 0x11; break;
        case 2: o.insert(o.begin() + o.size() / 3, {0xF1, 0xF2, 0xF3, 0xF4, 0xF5}); break;
        case 3: o.resize(o.size() - o.size() / 4); break;
        case 4: o.insert(o.end(), {'m', 'o', 'r', 'e', '\n'}); break;
        case 5: o.clear(); break;
        default: break;
        }
        oth.push_back(o);
    }
    oth[M - 1] = ents[4]; oth[M - 1][65536] ^= 1; oth[M - 1][65535] ^= 1;
    std::vector<zarc::FrameReader::Other> others;
    for (auto &o : oth) others.push_back(zarc::FrameReader::Other{o.empty() ? nullptr : o.data(), o.size()});
    std::vector<Want> want;
    for (size_t i = 0; i < M; i++) want.push_back(walk(ents[i], oth[i]));
    CHECK(want[0].relation == ZARC_GPU_CMP_EQUAL && want[0].line == 1 && want[0].byte_a == ZARC_GPU_CMP_EOF);
    CHECK(want[12].relation == ZARC_GPU_CMP_EQUAL && want[12].line > 1000 && want[6].relation == ZARC_GPU_CMP_EQUAL);
    CHECK(want[1].relation == ZARC_GPU_CMP_DIFFER && want[1].differing == 1 && want[2].relation == ZARC_GPU_CMP_DIFFER && want[2].prefix == 100 && want[2].suffix == 200);
    CHECK(want[3].relation == ZARC_GPU_CMP_OTHER_IS_PREFIX && want[4].relation == ZARC_GPU_CMP_FRAME_IS_PREFIX && want[5].relation == ZARC_GPU_CMP_OTHER_IS_PREFIX);
    CHECK(want[8].prefix == 65543 / 3 && want[8].suffix == 65543 - 65543 / 3 && want[M - 1].differing == 2 && want[M - 1].prefix == 65535);
    const int devices = zarc_gpu_device_count();
    std::vector<zarc::FrameReader::Result> base;
    for (int g = 1; g <= 4; g *= 2) {
        if (g > devices) break;
        std::vector<int> dev;
        for (int d = 0; d < g; d++) dev.push_back(d);
        zarc::FrameReader rd(dev);
        const auto chk = rd.check_content_frames((const uint8_t *)img.data(), img.size(), wanted);
        const auto got = rd.compare_content_frames((const uint8_t *)img.data(), img.size(), wanted, others);
        CHECK(got.size() == M);
        for (size_t i = 0; i < M; i++) {
            CHECK(got[i].status == chk[i].status && got[i].digest == chk[i].digest && got[i].verify == chk[i].verify && got[i].data.empty());
            if (i == 7) { CHECK(got[i].status == ZARC_GPU_FRAME_SRCSIZE && same(got[i].cmp, Want())); continue; }
            CHECK(got[i].status == ZARC_GPU_FRAME_OK && got[i].verify.value_or(false));
            CHECK(same(got[i].cmp, want[i]));
        }
        if (g == 1) base = got;
        for (size_t i = 0; i < M; i++) {
            const zarc::FrameReader::Result::Compare &b = base[i].cmp;
            CHECK(same(got[i].cmp, Want{b.relation, b.byte_a, b.byte_b, b.prefix, b.line, b.differing, b.suffix}));
        }
    }
    for (int g = 1; g <= 4 && g <= devices; g *= 2) std::printf("compare_content_frames on %d device(s) OK\n", g);
    zarc::FrameReader rd(0);
    CHECK(rd.compare_content_frames((const uint8_t *)img.data(), img.size(), std::vector<zarc::Frame>(), std::vector<zarc::FrameReader::Other>()).empty());
    bool refused = false;
    try { rd.compare_content_frames((const uint8_t *)img.data(), img.size(), wanted, std::vector<zarc::FrameReader::Other>()); } catch (const zarc::Error &) { refused = true; }
    CHECK(refused);
    std::printf("compare frames OK (%d device(s) visible)\n", devices);
    return 0;
}
