// tests/host/check_frames_test.cpp -- zarc::FrameReader::check_content_frames against read_content_frames (zarc_amd/host/zarc_host.hpp):
// the same statuses, digests and verify() answers on one device and dealt over two, no data; Encoder::check_frames writes the archive
// body the plain encoder writes.  Built by tests/test_verify_host.py against the emulated library (or the product library on a GPU box).
#include "../../zarc_amd/host/zarc_host.hpp"
#include "../../zarc_amd/csrc/corpus.h"
#include <cstdio>
#include <cstdlib>
#include <sstream>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main()
{
    const size_t sizes[] = {0, 1, 300, 70000, 200000, 65536, 5000, 131073};
    std::vector<std::vector<uint8_t>> ents;
    std::vector<const void *> ptr;
    std::vector<size_t> len;
    for (size_t i = 0; i < 8; i++) { ents.emplace_back(sizes[i]); zarc_corpus_entry(ents.back().data(), sizes[i], 9500 + i, (int)(i & 3)); }
    for (auto &e : ents) { ptr.push_back(e.data()); len.push_back(e.size()); }
    std::ostringstream plain, checked;
    std::vector<zarc::Frame> wanted;
    {
        zarc::Encoder enc(plain);
        enc.set_zstd_parameter(ZARC_GPU_P_CHECKSUM_FLAG, 1);
        enc.add_data_frames(ptr.data(), len.data(), ptr.size());
        for (const zarc::Digest &d : enc.frame_order()) wanted.push_back(enc.frames().at(d));
        zarc::Encoder enc2(checked);
        enc2.set_zstd_parameter(ZARC_GPU_P_CHECKSUM_FLAG, 1);
        enc2.check_frames(true);
        enc2.add_data_frames(ptr.data(), len.data(), ptr.size());
        CHECK(!enc2.check_failed());
    }
    CHECK(plain.str() == checked.str() && wanted.size() == 8);
    std::string img = plain.str();
    // damage: a flipped byte in one frame, a wrong digest on another, a wrong size on a third
    img[(size_t)wanted[4].offset + (size_t)wanted[4].length / 2] ^= 0x5A;
    wanted[3].digest.bytes[0] ^= 1;
    wanted[6].uncompressed += 1;
    const int devices = zarc_gpu_device_count();
    for (int g = 1; g <= (devices >= 2 ? 2 : 1); g++) {
        std::vector<int> dev;
        for (int d = 0; d < g; d++) dev.push_back(d);
        zarc::FrameReader rd(dev);
        const auto full = rd.read_content_frames((const uint8_t *)img.data(), img.size(), wanted);
        const auto chk = rd.check_content_frames((const uint8_t *)img.data(), img.size(), wanted);
        CHECK(full.size() == 8 && chk.size() == 8);
        for (size_t i = 0; i < 8; i++) {
            CHECK(chk[i].status == full[i].status && chk[i].digest == full[i].digest && chk[i].verify == full[i].verify && chk[i].data.empty());
        }
        CHECK(chk[0].status == ZARC_GPU_FRAME_OK && chk[0].verify.value_or(false));
        CHECK(chk[3].status == ZARC_GPU_FRAME_DIGEST && chk[3].verify.has_value() && !*chk[3].verify);
        CHECK(chk[4].status != ZARC_GPU_FRAME_OK && chk[4].status != ZARC_GPU_FRAME_DIGEST && !chk[4].verify.has_value());
        CHECK(chk[6].status == ZARC_GPU_FRAME_SRCSIZE);
        std::printf("check_content_frames on %d device(s) OK\n", g);
    }
    std::printf("check frames OK (%d device(s) visible)\n", devices);
    return 0;
}
