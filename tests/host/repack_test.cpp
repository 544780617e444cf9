// tests/host/repack_test.cpp -- zarc::ArchiveWriter::repack_from / Encoder::repack_frames (zarc_amd/host): `repack_test INPUT OUTPUT`
// compares the parsed directories of an archive and of what `zarc repack` made of it, field by field -- every file entry equal, every
// frame record new in offset and length only -- and has every frame of OUTPUT judged on the device; it then repacks INPUT itself, on
// one device and dealt over two, and wants the same bytes from both.  Built by tests/test_repack_cli.py against the emulated library
// (or the product library on a GPU box).
#include "../../zarc_amd/host/zarc_container.hpp"
#include <cstdio>
#include <fstream>
#include <iterator>
#include <sstream>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static std::string slurp(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}
static bool same_owner(const std::optional<zarc::File::Owner> &a, const std::optional<zarc::File::Owner> &b)
{
    return a.has_value() == b.has_value() && (!a || (a->id == b->id && a->name == b->name));
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: repack_test INPUT OUTPUT\n"); return 2; }
    const std::string in = slurp(argv[1]), out = slurp(argv[2]);
    zarc::ArchiveReader a((const uint8_t *)in.data(), in.size()), b((const uint8_t *)out.data(), out.size());
    CHECK(a.files().size() == b.files().size() && !a.files().empty());
    for (size_t i = 0; i < a.files().size(); i++) {
        const zarc::File &x = a.files()[i], &y = b.files()[i];
        CHECK(x.edition == y.edition && x.name == y.name && x.digest == y.digest && x.mode == y.mode);
        CHECK(x.created == y.created && x.modified == y.modified && x.accessed == y.accessed);
        CHECK(x.special_kind == y.special_kind && x.link_target == y.link_target);
        CHECK(same_owner(x.user, y.user) && same_owner(x.group, y.group));
        CHECK(x.user_metadata == y.user_metadata && x.attributes == y.attributes && x.extended_attributes == y.extended_attributes);
    }
    CHECK(a.editions().size() == b.editions().size());
    // frame records: the same digests and uncompressed sizes; edition 1; in the input's order, back to back from the header on
    CHECK(a.frames().size() == b.frames().size());
    std::vector<zarc::Frame> fa, fb;
    for (const auto &kv : a.frames()) fa.push_back(kv.second);
    for (const auto &kv : b.frames()) fb.push_back(kv.second);
    auto by_offset = [](const zarc::Frame &p, const zarc::Frame &q) { return p.offset < q.offset; };
    std::sort(fa.begin(), fa.end(), by_offset);
    std::sort(fb.begin(), fb.end(), by_offset);
    uint64_t at = sizeof zarc::FILE_MAGIC;
    for (size_t i = 0; i < fa.size(); i++) {
        CHECK(fb[i].digest == fa[i].digest && fb[i].uncompressed == fa[i].uncompressed && fb[i].edition == 1);
        CHECK(fb[i].offset == at);
        at += fb[i].length;
    }
    const auto judged = b.check_frames();
    for (const auto &r : judged) CHECK(r.status == ZARC_GPU_FRAME_OK && r.verify.value_or(false));
    std::printf("repack directories equal: %zu files, %zu frames\n", a.files().size(), fa.size());

    // repack_from on one device and on two: the same archive body, the report of the run, nothing refused
    const int devices = zarc_gpu_device_count();
    std::string body[2];
    for (int g = 1; g <= (devices >= 2 ? 2 : 1); g++) {
        std::vector<int> dev;
        for (int d = 0; d < g; d++) dev.push_back(d);
        std::ostringstream os;
        zarc::ArchiveWriter w(os, dev);
        w.set_zstd_parameter(ZARC_GPU_P_CHECKSUM_FLAG, 1);
        w.set_zstd_parameter(ZARC_GPU_P_COMPRESSION_LEVEL, 1);
        const zarc::RepackReport rep = w.repack_from(a);
        CHECK(rep.bad.empty() && rep.frames == fa.size() && rep.kept == 0);
        uint64_t old_bytes = 0;
        for (const auto &f : fa) old_bytes += f.length;
        CHECK(rep.old_bytes == old_bytes && rep.new_bytes == w.offset() - sizeof zarc::FILE_MAGIC);
        w.finalise(a.editions().at(0).written_at);
        body[g - 1] = os.str();
        std::printf("repack_from on %d device(s) OK\n", g);
    }
    if (devices >= 2) CHECK(body[0] == body[1]);
    // a damaged frame is reported with its status and not written; its neighbours are
    {
        std::string bad = in;
        bad[(size_t)fa[0].offset + (size_t)fa[0].length / 2] ^= 0x5A;
        std::ostringstream os;
        zarc::Encoder enc(os);
        enc.set_zstd_parameter(ZARC_GPU_P_CHECKSUM_FLAG, 1);
        const auto res = enc.repack_frames((const uint8_t *)bad.data(), bad.size(), fa);
        CHECK(res[0].status != ZARC_GPU_FRAME_OK && res[0].new_length == 0 && !enc.frames().count(fa[0].digest));
        for (size_t i = 1; i < fa.size(); i++) CHECK(res[i].status == ZARC_GPU_FRAME_OK && enc.frames().count(fa[i].digest));
    }
    std::printf("repack OK (%d device(s) visible)\n", devices);
    return 0;
}
