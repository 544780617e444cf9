// zarc_amd/host/zarc_cli.cpp -- `zarc pack | unpack | verify | repack | list-files` over the engine (SURVEY.md section 8 rows f2 + f3).
//
// Same verbs, flags and outputs as the reference CLI (crates/zarc-cli/src/args.rs:17-84):
//   pack        --output PATH [--level N] [--zstd PARAM=VALUE]... [--store] [-L|--follow-symlinks] PATH...
//               crates/zarc-cli/src/pack.rs:9-84,219-272: ChecksumFlag(true) always, walk every PATH, file contents
//               -> add_data_frame, entry -> add_file_entry, finalise, prints "digest: <base64>"
//   unpack      INPUT [--filter REGEX]... [--verify DIGEST]        crates/zarc-cli/src/unpack.rs:18-138
//   list-files  INPUT [--only-files] [--decorate] [--filter REGEX]...   crates/zarc-cli/src/list_files.rs:8-63
//   repack      INPUT --output PATH [--level N] [--zstd PARAM=VALUE]... [--store] [--split-blocks] [--check] [--gpus N] [--verify DIGEST]
//               [--keep-smaller]     engine extension (the reference would unpack and pack again): the content frames of INPUT encoded
//               again with pack's flags, on the device; the directory is carried over
//   global      -v... (warn / info / debug / trace), --log-file [PATH] (JSON lines; a directory gets zarc.<UTC time>.log), $RUST_LOG
//               takes precedence -- crates/zarc-cli/src/args.rs:39-65, logs.rs:12-67
// What differs on purpose: file contents are gathered into batches of about 1 GiB before they go to the engine (frames
// and directory order do not change: frames in walk order, first occurrence of a content wins); the walk is sorted by
// name (WalkDir yields directory order).  Metadata carried (metadata/encode.rs:28-372): mode, owner / group (id + name through a
// uid / gid cache, owner_cache.rs:14-77), modified / accessed times, directories, symlinks with their target as a full path,
// chattr flags as `linux.*` attributes, extended attributes.
// I/O pipeline: pack reads the files of batch k+1 on a reader thread while the engine packs batch k (whose
// frames the engine's own staging moves over PCIe in chunks); unpack writes the files of batch k on a writer thread while
// batch k+1 is decoded.  The reference does all of it on one thread, file by file (pack.rs:244-265, unpack.rs:94-124).
#include "zarc_container.hpp"
#include <dirent.h>
#include <fcntl.h>
#include <fstream>
#include <grp.h>
#include <iostream>
#include <pwd.h>
#include <regex>
#include <condition_variable>
#include <deque>
#include <linux/fs.h>
#include <mutex>
#include <sys/ioctl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/xattr.h>
#include <thread>
#include <unistd.h>
#include <unordered_map>

namespace {

// ---------------------------------------------------------------- diagnostics (logs.rs:12-67) ----------------
// Levels as tracing's: 1 warn, 2 info, 3 debug, 4 trace.  Plain lines on stderr, or JSON lines in --log-file.
struct Log {
    int level = 0;
    FILE *file = nullptr;
    std::mutex mu;
    void init(int verbosity, const std::string &log_file, bool have_log_file)
    {
        if (const char *e = getenv("RUST_LOG")) { // "If $RUST_LOG is set, this flag is ignored" (args.rs:49)
            const std::string v = e;
            level = v.find("trace") != std::string::npos ? 4 : v.find("debug") != std::string::npos ? 3 : v.find("info") != std::string::npos ? 2 :
                    v.find("warn") != std::string::npos ? 1 : (v.find("error") != std::string::npos ? 1 : 2);
            return;
        }
        if (have_log_file && verbosity == 0) verbosity = 3; // "If a log level was not already specified, this will set it to -vvv"
        if (verbosity <= 0) return;
        level = verbosity > 4 ? 4 : verbosity;
        if (have_log_file) {
            std::string path = log_file.empty() ? "." : log_file;
            struct stat st;
            if (stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) {
                char name[64];
                const time_t now = time(nullptr);
                std::tm tm{};
                gmtime_r(&now, &tm);
                std::strftime(name, sizeof name, "zarc.%Y-%m-%dT%H-%M-%SZ.log", &tm);
                path += "/" + std::string(name);
            }
            file = std::fopen(path.c_str(), "w");
            if (!file) std::fprintf(stderr, "Failed to initialise logging, continuing with none\n%s: %s\n", path.c_str(), std::strerror(errno));
        }
        event(2, "logging initialised", "");
    }
    void event(int lvl, const char *msg, const std::string &fields) // fields: pre-formatted `key=value ...`
    {
        if (lvl > level || level == 0) return;
        static const char *names[] = {"", "WARN", "INFO", "DEBUG", "TRACE"};
        timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        std::tm tm{};
        gmtime_r(&ts.tv_sec, &tm);
        char t[40];
        std::strftime(t, sizeof t, "%Y-%m-%dT%H:%M:%S", &tm);
        std::lock_guard<std::mutex> g(mu);
        if (file) {
            std::string esc;
            for (char c : fields) { if (c == '"' || c == '\\') esc += '\\'; esc += c; }
            std::fprintf(file, "{\"timestamp\":\"%s.%06ldZ\",\"level\":\"%s\",\"fields\":{\"message\":\"%s\",\"detail\":\"%s\"},\"target\":\"zarc\"}\n", t, ts.tv_nsec / 1000,
                         names[lvl], msg, esc.c_str());
            std::fflush(file);
        } else std::fprintf(stderr, "%s.%06ldZ %5s zarc: %s %s\n", t, ts.tv_nsec / 1000, names[lvl], msg, fields.c_str());
    }
    ~Log() { if (file) std::fclose(file); }
};
Log g_log;
#define LOGF(lvl, msg, ...) do { if ((lvl) <= g_log.level) { char b_[600]; std::snprintf(b_, sizeof b_, __VA_ARGS__); g_log.event((lvl), (msg), b_); } } while (0)

// uid / gid <-> name lookups are slow (over 90 % of a pack before the reference cached them, owner_cache.rs:3-6): cache both ways
struct OwnerCache {
    std::unordered_map<uint32_t, std::optional<std::string>> users, groups;
    std::unordered_map<std::string, std::optional<uint32_t>> uid_by_name, gid_by_name;
    std::optional<std::string> user_from_uid(uint32_t uid)
    {
        auto it = users.find(uid);
        if (it != users.end()) return it->second;
        std::optional<std::string> n;
        if (const passwd *pw = getpwuid((uid_t)uid)) { n = pw->pw_name; uid_by_name[*n] = uid; }
        return users[uid] = n;
    }
    std::optional<std::string> group_from_gid(uint32_t gid)
    {
        auto it = groups.find(gid);
        if (it != groups.end()) return it->second;
        std::optional<std::string> n;
        if (const group *gr = getgrgid((gid_t)gid)) { n = gr->gr_name; gid_by_name[*n] = gid; }
        return groups[gid] = n;
    }
    std::optional<uint32_t> uid_from_name(const std::string &name)
    {
        auto it = uid_by_name.find(name);
        if (it != uid_by_name.end()) return it->second;
        std::optional<uint32_t> v;
        if (const passwd *pw = getpwnam(name.c_str())) v = (uint32_t)pw->pw_uid;
        return uid_by_name[name] = v;
    }
    std::optional<uint32_t> gid_from_name(const std::string &name)
    {
        auto it = gid_by_name.find(name);
        if (it != gid_by_name.end()) return it->second;
        std::optional<uint32_t> v;
        if (const group *gr = getgrnam(name.c_str())) v = (uint32_t)gr->gr_gid;
        return gid_by_name[name] = v;
    }
};
OwnerCache g_owners;

std::string base64(const uint8_t *p, size_t n) // base64ct::Base64: standard alphabet, padded
{
    static const char *T = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    std::string s;
    for (size_t i = 0; i < n; i += 3) {
        const uint32_t v = (uint32_t)p[i] << 16 | (i + 1 < n ? (uint32_t)p[i + 1] << 8 : 0) | (i + 2 < n ? p[i + 2] : 0);
        s += T[v >> 18]; s += T[(v >> 12) & 63];
        s += i + 1 < n ? T[(v >> 6) & 63] : '=';
        s += i + 2 < n ? T[v & 63] : '=';
    }
    return s;
}

std::vector<std::string> normal_components(const std::string &path) // Pathname::from_normal_components (strings.rs:18-31)
{
    std::vector<std::string> out;
    size_t i = 0;
    while (i < path.size()) {
        size_t j = path.find('/', i);
        if (j == std::string::npos) j = path.size();
        const std::string c = path.substr(i, j - i);
        if (!c.empty() && c != "." && c != "..") out.push_back(c);
        i = j + 1;
    }
    return out;
}
std::string to_path(const std::vector<std::string> &name) // Pathname::to_path (strings.rs:33-55)
{
    std::string p;
    for (const auto &c : name) { if (!p.empty()) p += '/'; p += c; }
    return p;
}

// A pathname from an archive is untrusted: a component that is empty, ".", "..", or contains '/' or NUL would let a crafted
// archive write outside the extraction directory (the reference joins components with PathBuf::push and has the same hole).
bool safe_name(const std::vector<std::string> &name)
{
    if (name.empty()) return false;
    for (const auto &c : name)
        if (c.empty() || c == "." || c == ".." || c.find('/') != std::string::npos || c.find('\0') != std::string::npos) return false;
    return true;
}

int usage()
{
    std::fprintf(stderr, "usage: zarc [-v...] [--log-file [PATH]] <pack|unpack|verify|repack|grep|cat|wc|compare|list-files> ...\n"
                         "       zarc pack --output PATH [--level N] [--zstd PARAM=VALUE]... [--store] [-L] [--gpus N] [--split-blocks] [--check] PATH...\n"
                         "         --split-blocks  cut 64 KiB blocks where their statistics change (smaller frames on binaries / JSON; off by default)\n"
                         "         --check         decode every frame again on the device and compare it with its file before it is written; a mismatch\n"
                         "                         ends the run with exit status 1 and no directory or trailer is written (off by default)\n"
                         "       zarc unpack INPUT [--filter REGEX]... [--verify DIGEST] [--gpus N]\n"
                         "       zarc verify INPUT [--filter REGEX]... [--verify DIGEST] [--gpus N]\n"
                         "         tests the content frames of the files (each distinct frame once) without writing anything; exit status 0 iff all are good\n"
                         "       zarc repack INPUT --output PATH [--level N] [--zstd PARAM=VALUE]... [--store] [--split-blocks] [--check] [--gpus N]\n"
                         "                   [--verify DIGEST] [--keep-smaller]\n"
                         "         encodes every content frame of INPUT again with these flags (pack's), on the device, and carries the directory over;\n"
                         "         --keep-smaller copies a frame unchanged when its new form is not smaller.  A frame that is not good ends the run with\n"
                         "         exit status 1 and nothing is left at PATH\n"
                         "       zarc grep [-i] [-l] [-b] [--hex] [--filter REGEX]... [--verify DIGEST] [--gpus N]\n"
                         "                 [--lines] [-n] [-c] [-a] [-m NUM] [--max-line BYTES] [--batch-lines N] [-v] [-A NUM] [-B NUM] [-C NUM] [--only-matching] PATTERN ARCHIVE\n"
                         "       zarc grep ... (-e PATTERN | -f FILE)... [--tally] ARCHIVE\n"
                         "       zarc grep -E ... (PATTERN | (-e PATTERN | -f FILE)...) ARCHIVE\n"
                         "         searches the content of the files for PATTERN on the device, each distinct frame once, and writes nothing.  PATTERN is a\n"
                         "         fixed string of 1 to 256 bytes (grep -F), never a regular expression; --hex reads it as hex digits.  One line per file with\n"
                         "         a match: PATH:COUNT (overlapping occurrences count); -b adds :OFFSET of the first one, -l prints PATH alone, -i folds ASCII\n"
                         "         letters.  Exit status as grep's: 0 a match, 1 none, 2 a frame that is not good or any other error.\n"
                         "         --lines, -n, -c, -a, -m, --max-line or --batch-lines select lines mode: the matching lines are gathered on the device and\n"
                         "         printed as PATH:LINE; -n adds NUMBER: and -b the line's byte OFFSET: in front of LINE, -c prints PATH:NLINES (matching lines)\n"
                         "         instead, -m NUM stops after NUM lines per file, -l prints PATH alone.  A file with a NUL byte in a line to print gives\n"
                         "         `Binary file PATH matches` unless -a is given.  A line prints its first --max-line bytes (default 4096, 1 to 65536).\n"
                         "         --batch-lines N (default 1048576) is the number of lines one device call can bring back; what did not fit is searched again.\n"
                         "         PATTERN must not contain a newline in lines mode\n"
                         "         -v selects the lines WITHOUT a match, -A NUM / -B NUM / -C NUM add NUM lines behind / in front of / around every selected\n"
                         "         line, chosen on the device; each selects lines mode (inside grep, -v is not the global verbosity flag).  Output is grep's:\n"
                         "         context lines carry `-` in place of every `:`, a line `--` stands between groups that are not adjacent; -c, -l and the exit\n"
                         "         status follow the selected (hit) lines; with -m NUM a file stops behind the trailing context of its NUM-th hit line.  They\n"
                         "         go with one PATTERN, -e / -f and -E, not with --tally\n"
                         "         -e PATTERN (any number of times) and -f FILE (one pattern per line; a CR stays part of it, an empty line is an error) give a\n"
                         "         SET of up to 1024 patterns that is searched in one pass; ARCHIVE is then the only other argument and --hex applies to every\n"
                         "         pattern.  Patterns that are equal (after -i) are searched once.  A position at which several patterns match counts once, a\n"
                         "         line with matches of several is one line; the output is the same as for one PATTERN.  --tally prints, instead of the lines per\n"
                         "         file, one line COUNT<TAB>PATTERN per pattern in the order given (as typed; zeros included): the positions at which it matches,\n"
                         "         over the distinct frames searched\n"
                         "         -E (--extended-regexp): PATTERN is a regular expression of up to 1024 bytes, matched on the device line by line -- POSIX ERE's\n"
                         "         operators ( ) | * + ? {n,m} [...] . ^ $ with the escapes \\t \\r \\f \\v \\0 \\xHH \\d \\D \\w \\W \\s \\S; no back-references or word\n"
                         "         boundaries.  COUNT is the number of positions at which a match starts; several -e and the lines of -f FILE are joined as\n"
                         "         (A)|(B)|...  An expression that is refused, or whose automaton needs more than 64 states, ends the run with exit status 2\n"
                         "         before ARCHIVE is opened.  --hex and --tally do not go with -E\n"
                         "         --only-matching (grep's -o; spelled out only) prints every match of a matching line instead of the line, cut out on the device, one per output line:\n"
                         "         PATH:[NUMBER:][OFFSET:]MATCH, the longest match at the leftmost position and on from its end, as grep -o.  -b gives the offset\n"
                         "         of the match itself, -m NUM counts lines, -c and -l ignore it, --max-line cuts a match and the binary-file rule looks at the\n"
                         "         matches.  --batch-lines N bounds the lines that take part in one device call and the matches it brings back.  With -E the\n"
                         "         expression needs a second table of at most 64 states: one that -E accepts can be refused with it, before ARCHIVE is opened.\n"
                         "         It does not go with -v, -A, -B, -C or --tally\n"
                         "       zarc cat [--filter REGEX]... [--verify DIGEST] [--gpus N] [--header] [--batch-bytes N]\n"
                         "                [--head [-]N | --tail [+]N | --lines A:[B] | --head-bytes [-]N | --tail-bytes [+]N | --bytes A:[B]] ARCHIVE\n"
                         "         writes the content of the regular files (grep's selection) to stdout, in directory order, as raw bytes.  At most one range\n"
                         "         option: --head N / --tail N the first / last N lines, --head -N all but the last N, --tail +K from line K on, --lines A:B\n"
                         "         lines A to B (1-based, inclusive; A: to the end), --bytes A:B bytes A to B (0-based, B excluded); the -bytes forms count\n"
                         "         bytes.  N is plain decimal.  With a range option the range is cut out on the device, each distinct frame once, and only its\n"
                         "         bytes come back; --batch-bytes N (default 268435456) is what one device call can bring back: what it cut off is fetched by a\n"
                         "         further call, which decodes the frame again.  --header prints `==> PATH <==` in front of each file, as head -v.  A frame\n"
                         "         that is not good prints nothing for its files and a message; a digest mismatch prints the content and a message.  Exit\n"
                         "         status 0 iff every selected file was printed clean\n"
                         "       zarc wc [-l] [-w] [-m] [-c] [--max-line-bytes] [--longest] [--filter REGEX]... [--verify DIGEST] [--gpus N] ARCHIVE\n"
                         "         counts the content of the regular files (grep's selection) on the device, each distinct frame once: one line per file, in\n"
                         "         directory order, with the selected counts in the fixed order lines (-l), words (-w), characters (-m), bytes (-c),\n"
                         "         max-line-bytes, each followed by one space, then the path.  There is no column padding.  Without a count option: lines,\n"
                         "         words and bytes, as wc.  A word is a run of bytes other than space, tab, LF, VT, FF and CR; a character is a byte that is no\n"
                         "         UTF-8 continuation byte; --max-line-bytes is the longest line in BYTES (not wc -L's display width).  --longest implies it\n"
                         "         and prints that column as LEN:LINE_NO:OFFSET of the first such line -- the line `zarc cat --lines LINE_NO:LINE_NO` cuts out.\n"
                         "         More than one file: a last line `... total` with the sums and the largest max-line-bytes.  A frame that is not good prints\n"
                         "         a message and no line.  Exit status 0 iff every selected file was counted clean\n"
                         "       zarc compare [-C DIR | --directory DIR] [--filter REGEX]... [--brief] [--report-identical] [--verify DIGEST] [--gpus N]\n"
                         "                    [--batch-bytes N] ARCHIVE\n"
                         "         compares the CONTENT of the regular files (grep's selection) with the files DIR/PATH on disk (DIR: the current directory),\n"
                         "         on the device, as tar --compare and cmp do; symbolic links, directories, modes, owners and times are not looked at.  The\n"
                         "         pairs go up in batches of --batch-bytes N (default 268435456) of disk content.  One line per file that is not identical,\n"
                         "         in directory order: `PATH: differ: byte N, line M, K bytes differ` (N counts from 1, as cmp; where the sizes differ as\n"
                         "         well: `, sizes A and B, common tail T`), `PATH: archive copy is a prefix: N of B bytes, line M`, `PATH: file is a prefix:\n"
                         "         N of A bytes, line M`, `PATH: missing`, `PATH: not a regular file`, `PATH: bad frame (STATUS)`, `PATH: unreadable (WHY)`.  --brief\n"
                         "         prints only PATH; --report-identical adds `PATH: identical`.  An entry whose name would leave DIR is not compared.  Exit\n"
                         "         status 0: all identical; 1: something differs or is missing; 2: a usage error, a bad frame, an unreadable file or archive\n"
                         "       zarc list-files INPUT [--only-files] [--decorate] [--filter REGEX]...\n");
    return 2;
}

// ---------------------------------------------------------------- pack --------------------------------------
struct ZstdParam { int id; int value; };
bool parse_zstd_param(const std::string &s, ZstdParam *out) // pack.rs:86-217: NAME=VALUE, names of zstd_safe::CParameter
{
    const size_t eq = s.find('=');
    if (eq == std::string::npos) return false;
    const std::string name = s.substr(0, eq), val = s.substr(eq + 1);
    static const struct { const char *n; int id; } ids[] = {
        {"CompressionLevel", 100}, {"WindowLog", 101}, {"HashLog", 102}, {"ChainLog", 103}, {"SearchLog", 104}, {"MinMatch", 105},
        {"TargetLength", 106}, {"Strategy", 107}, {"EnableLongDistanceMatching", 160}, {"LdmHashLog", 161}, {"LdmMinMatch", 162},
        {"LdmBucketSizeLog", 163}, {"LdmHashRateLog", 164}, {"ContentSizeFlag", 200}, {"ChecksumFlag", 201}, {"DictIdFlag", 202},
        {"NbWorkers", 400}, {"JobSize", 401}, {"OverlapSizeLog", 402}};
    static const char *strategies[] = {"", "fast", "dfast", "greedy", "lazy", "lazy2", "btlazy2", "btopt", "btultra", "btultra2"};
    for (const auto &e : ids)
        if (name == e.n) {
            out->id = e.id;
            if (val == "true") out->value = 1;
            else if (val == "false") out->value = 0;
            else if (e.id == 107 && !val.empty() && !std::isdigit((unsigned char)val[0])) {
                out->value = 0;
                for (int k = 1; k < 10; k++) if (val == strategies[k]) out->value = k;
                if (!out->value) return false;
            } else out->value = std::atoi(val.c_str());
            return true;
        }
    return false;
}

// The flags that say what frames an encoder writes: pack's, and repack's
struct EncoderFlags {
    std::vector<ZstdParam> params;
    bool store = false, have_level = false, split_blocks = false, check = false;
    int level = 0;
    // 1: a[i] (and its value, i advanced) was one of these flags; 0: it was not; -1: it was, with a bad value
    int parse(const std::vector<std::string> &a, size_t &i)
    {
        if (a[i] == "--level" && i + 1 < a.size()) { level = std::atoi(a[++i].c_str()); have_level = true; }
        else if (a[i].rfind("--level=", 0) == 0) { level = std::atoi(a[i].c_str() + 8); have_level = true; }
        else if (a[i] == "--zstd" && i + 1 < a.size()) { ZstdParam p; if (!parse_zstd_param(a[++i], &p)) { std::fprintf(stderr, "error: invalid --zstd value\n"); return -1; } params.push_back(p); }
        else if (a[i] == "--store") store = true;
        else if (a[i] == "--split-blocks") split_blocks = true;                          // engine extension: ZARC_GPU_PX_BLOCK_SPLIT
        else if (a[i] == "--check") check = true;                                        // engine extension: ZARC_GPU_PX_CHECK_FRAMES
        else return 0;
        return 1;
    }
    void apply(zarc::ArchiveWriter &enc) const
    {
        enc.set_zstd_parameter(ZARC_GPU_P_CHECKSUM_FLAG, 1); // pack.rs:227
        if (have_level) enc.set_zstd_parameter(ZARC_GPU_P_COMPRESSION_LEVEL, level);
        for (const auto &p : params) enc.set_zstd_parameter(p.id, p.value);
        // What the engine does differently from libzstd with these is said once, on stderr and in the log: a level runs its tier's finder, the
        // search-effort and long-distance-matching hints are accepted (the reference forwards them all, pack.rs:86-217) but change nothing.
        if (have_level && level != 0 && zarc_gpu_level_finder(level) != level) {
            std::fprintf(stderr, "warning: --level %d packs with the engine's level-%d finder (tiers: <= 1, 2..8, 9..14, 15..22)\n", level, zarc_gpu_level_finder(level));
            LOGF(1, "level mapped to a finder tier", "level=%d finder=%d", level, zarc_gpu_level_finder(level));
        }
        for (const auto &p : params)
            if (zarc_gpu_parameter_advisory(p.id)) {
                std::fprintf(stderr, "warning: --zstd parameter %d=%d is accepted but advisory on this engine: the frames are the level's frames\n", p.id, p.value);
                LOGF(1, "advisory zstd parameter", "id=%d value=%d", p.id, p.value);
            }
        if (store) enc.enable_compression(false);
        if (split_blocks) enc.split_blocks(true);
        if (check) enc.check_frames(true);
    }
};

struct Walked { std::string path; struct stat st; bool is_link; std::string target; };
void walk(const std::string &path, bool follow, std::vector<Walked> &out) // WalkDir::new(path).follow_links(follow), sorted
{
    Walked w;
    w.path = path;
    struct stat lst;
    if (lstat(path.c_str(), &lst) != 0) { std::fprintf(stderr, "read error: %s: %s\n", path.c_str(), std::strerror(errno)); return; }
    w.is_link = S_ISLNK(lst.st_mode);
    if (w.is_link) {
        char buf[4096];
        const ssize_t n = readlink(path.c_str(), buf, sizeof buf);
        if (n > 0) w.target.assign(buf, (size_t)n);
    }
    w.st = lst;
    if (w.is_link && follow && stat(path.c_str(), &w.st) != 0) w.st = lst; // dangling link: keep what lstat said
    out.push_back(w);
    if (!S_ISDIR(w.st.st_mode) || (w.is_link && !follow)) return;
    std::vector<std::string> names;
    if (DIR *d = opendir(path.c_str())) {
        while (dirent *e = readdir(d)) { const std::string n = e->d_name; if (n != "." && n != "..") names.push_back(n); }
        closedir(d);
    } else std::fprintf(stderr, "read error: %s: %s\n", path.c_str(), std::strerror(errno));
    std::sort(names.begin(), names.end());
    for (const auto &n : names) walk(path + (path.back() == '/' ? "" : "/") + n, follow, out);
}

// chattr flags as `linux.*` booleans plus the portable aliases (metadata/encode.rs:212-329)
std::optional<zarc::File::AttrMap> file_attributes(const Walked &w)
{
    if (!S_ISREG(w.st.st_mode) && !S_ISDIR(w.st.st_mode)) return std::nullopt; // FS_IOC_GETFLAGS needs an open regular file or directory
    const int fd = open(w.path.c_str(), O_RDONLY | O_NONBLOCK | O_NOFOLLOW | O_CLOEXEC);
    if (fd < 0) return std::nullopt;
    int flags = 0;
    const int rc = ioctl(fd, FS_IOC_GETFLAGS, &flags);
    close(fd);
    if (rc != 0) return std::nullopt; // file systems without flags (tmpfs, overlay ...)
    static const struct { const char *name; int bit; } names[] = {
        {"append-only", FS_APPEND_FL}, {"casefold", 0x40000000 /* FS_CASEFOLD_FL */}, {"compressed", FS_COMPR_FL}, {"delete-undo", FS_UNRM_FL},
        {"delete-zero", FS_SECRM_FL}, {"dir-sync", FS_DIRSYNC_FL}, {"encrypted", 0x00000800 /* FS_ENCRYPT_FL */}, {"file-sync", FS_SYNC_FL},
        {"immutable", FS_IMMUTABLE_FL}, {"no-atime", FS_NOATIME_FL}, {"no-backup", FS_NODUMP_FL}, {"no-cow", 0x00800000 /* FS_NOCOW_FL */},
        {"not-compressed", FS_NOCOMP_FL}};
    zarc::File::AttrMap m;
    zarc::File::Attr yes;
    yes.is_bool = true; yes.b = true;
    for (const auto &n : names) if (flags & n.bit) m[std::string("linux.") + n.name] = yes;
    if (m.empty()) return std::nullopt;
    if (m.count("linux.append-only")) m["append-only"] = yes;
    if (m.count("linux.immutable")) m["immutable"] = yes;
    if (m.count("linux.compressed")) m["compressed"] = yes;
    if (!(w.st.st_mode & 0222)) m["read-only"] = yes;
    return m;
}

// extended attributes, names that are valid UTF-8 only (metadata/encode.rs:343-372)
std::optional<zarc::File::AttrMap> file_extended_attributes(const Walked &w)
{
    std::vector<char> names(1024);
    ssize_t n;
    while ((n = llistxattr(w.path.c_str(), names.data(), names.size())) < 0 && errno == ERANGE) names.resize(names.size() * 4);
    if (n < 0) return std::nullopt; // unsupported here
    zarc::File::AttrMap m;
    for (ssize_t i = 0; i < n;) {
        const std::string name(names.data() + i);
        i += (ssize_t)name.size() + 1;
        if (!zarc::valid_utf8(name)) { LOGF(1, "not storing non-Unicode xattr", "path=%s", w.path.c_str()); continue; }
        std::vector<char> val(256);
        ssize_t v;
        while ((v = lgetxattr(w.path.c_str(), name.c_str(), val.data(), val.size())) < 0 && errno == ERANGE) val.resize(val.size() * 4);
        if (v < 0) continue;
        zarc::File::Attr a;
        a.s.assign(val.data(), (size_t)v);
        m[name] = a;
    }
    return m;
}

zarc::File build_file_with_metadata(const Walked &w) // metadata/encode.rs:28-85
{
    zarc::File f;
    f.name = normal_components(w.path);
    f.mode = (uint32_t)w.st.st_mode;
    zarc::File::Owner u, g;
    u.id = (uint64_t)w.st.st_uid;
    u.name = g_owners.user_from_uid((uint32_t)w.st.st_uid);
    g.id = (uint64_t)w.st.st_gid;
    g.name = g_owners.group_from_gid((uint32_t)w.st.st_gid);
    f.user = u; f.group = g;
    f.modified = zarc::Timestamp{(int64_t)w.st.st_mtim.tv_sec, (uint32_t)w.st.st_mtim.tv_nsec};
    f.accessed = zarc::Timestamp{(int64_t)w.st.st_atim.tv_sec, (uint32_t)w.st.st_atim.tv_nsec};
    if (S_ISDIR(w.st.st_mode)) f.special_kind = 1;
    else if (w.is_link && S_ISLNK(w.st.st_mode)) { f.special_kind = 10; f.link_target = w.target; }
    f.attributes = file_attributes(w);
    f.extended_attributes = file_extended_attributes(w);
    LOGF(4, "build_file_with_metadata", "path=%s mode=%o", w.path.c_str(), (unsigned)w.st.st_mode);
    return f;
}

int cmd_pack(const std::vector<std::string> &a)
{
    std::string output;
    std::vector<std::string> paths;
    EncoderFlags flags;
    bool follow = false;
    int gpus = 1;
    for (size_t i = 0; i < a.size(); i++) {
        if (const int r = flags.parse(a, i)) { if (r < 0) return 2; }
        else if (a[i] == "--output" && i + 1 < a.size()) output = a[++i];
        else if (a[i] == "-L" || a[i] == "--follow-symlinks") follow = true;
        else if (a[i] == "--gpus" && i + 1 < a.size()) gpus = std::atoi(a[++i].c_str()); // engine extension: deal every batch to N devices
        else if (!a[i].empty() && a[i][0] == '-') return usage();
        else paths.push_back(a[i]);
    }
    if (output.empty() || gpus < 1 || gpus > 64) return usage();
    if (gpus > zarc_gpu_device_count()) { std::fprintf(stderr, "Error: --gpus %d but %d device(s) are usable\n", gpus, zarc_gpu_device_count()); return 1; }
    std::ofstream file(output, std::ios::binary | std::ios::trunc);
    if (!file) { std::fprintf(stderr, "Error: %s: %s\n", output.c_str(), std::strerror(errno)); return 1; }
    std::vector<int> devices;
    for (int d = 0; d < gpus; d++) devices.push_back(d);
    zarc::ArchiveWriter enc(file, devices);
    flags.apply(enc);

    std::vector<Walked> entries;
    for (const auto &p : paths) walk(p, follow, entries);
    LOGF(2, "walked", "entries=%zu devices=%d split_blocks=%d", entries.size(), gpus, flags.split_blocks ? 1 : 0);
    // Contents go to the engine in batches of about 1 GiB.  A reader thread fills batch k+1 (file reads) while this thread has the
    // engine pack batch k and appends its frames to the archive; entries are added in walk order once their digest is known.
    struct Batch { size_t first = 0, last = 0; std::vector<std::vector<uint8_t>> contents; std::vector<size_t> owner; std::string error; };
    const size_t BATCH = (size_t)1 << 30;
    std::deque<Batch> ready;
    std::mutex mu;
    std::condition_variable cv;
    bool reader_done = false, abandon = false;
    std::thread reader([&] {
        size_t first = 0;
        while (first < entries.size()) {
            { std::lock_guard<std::mutex> lk(mu); if (abandon) break; }
            Batch b;
            b.first = first;
            size_t last = first, bytes = 0;
            while (last < entries.size() && (bytes < BATCH || last == first) && b.error.empty()) {
                const Walked &w = entries[last];
                if (S_ISREG(w.st.st_mode)) {
                    std::ifstream in(w.path, std::ios::binary);
                    if (!in) { b.error = w.path + ": " + std::strerror(errno); break; }
                    b.contents.emplace_back((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
                    b.owner.push_back(last);
                    bytes += b.contents.back().size();
                }
                last++;
            }
            b.last = last;
            const bool failed = !b.error.empty();
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return ready.size() < 2 || abandon; }); // at most two batches of file contents in memory
                if (abandon) break;
                ready.push_back(std::move(b));
            }
            cv.notify_all();
            if (failed) break;
            first = last;
        }
        { std::lock_guard<std::mutex> lk(mu); reader_done = true; }
        cv.notify_all();
    });
    // Whatever ends the loop below -- a read error, or an exception out of the engine / the archive writer (zarc::Error: engine
    // failure, an entry of 4 GiB or more, a failed write) -- the reader thread is told to stop and joined before this frame unwinds:
    // a joinable std::thread must never be destroyed (std::terminate), the error goes to main()'s handler ("Error: ...", exit 1).
    struct Joiner {
        std::thread &t; std::mutex &mu; std::condition_variable &cv; bool &stop;
        ~Joiner() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); if (t.joinable()) t.join(); }
    } joiner{reader, mu, cv, abandon};
    std::string failure;
    for (;;) {
        Batch b;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !ready.empty() || reader_done; });
            if (ready.empty()) break;
            b = std::move(ready.front());
            ready.pop_front();
        }
        cv.notify_all();
        if (!b.error.empty()) { failure = b.error; break; }
        std::vector<const void *> ptr;
        std::vector<size_t> len;
        for (auto &c : b.contents) { ptr.push_back(c.data()); len.push_back(c.size()); }
        LOGF(3, "add_data_frames", "entries=%zu files=%zu", b.last - b.first, ptr.size());
        std::vector<zarc::Digest> dig;
        try {
            dig = enc.add_data_frames(ptr.data(), len.data(), ptr.size());
        } catch (const zarc::Error &e) {
            // --check: a frame did not decode back to its file.  Nothing of the batch has been written and neither directory nor trailer
            // will be: what is left at --output is not a zarc archive
            if (e.code != ZARC_GPU_E_CHECK || !enc.check_failed()) throw;
            std::fprintf(stderr, "Error: %s: %s\n", entries[b.owner[*enc.check_failed()]].path.c_str(), e.what());
            return 1;
        }
        size_t k = 0;
        for (size_t i = b.first; i < b.last; i++) {
            zarc::File f = build_file_with_metadata(entries[i]);
            if (k < b.owner.size() && b.owner[k] == i) f.digest = dig[k++];
            enc.add_file_entry(f);
        }
    }
    if (!failure.empty()) { std::fprintf(stderr, "Error: %s\n", failure.c_str()); return 1; }
    timespec now;
    clock_gettime(CLOCK_REALTIME, &now);
    const zarc::Digest digest = enc.finalise(zarc::Timestamp{(int64_t)now.tv_sec, (uint32_t)now.tv_nsec});
    std::printf("digest: %s\n", base64(digest.bytes.data(), 32).c_str());
    return 0;
}

// ---------------------------------------------------------------- unpack / list-files -----------------------
struct Mapped {
    const uint8_t *p = nullptr; size_t n = 0; int fd = -1;
    explicit Mapped(const std::string &path)
    {
        fd = open(path.c_str(), O_RDONLY);
        struct stat st;
        if (fd < 0 || fstat(fd, &st) != 0) throw zarc::Error(ZARC_GPU_E_PARAM, path + ": " + std::strerror(errno));
        n = (size_t)st.st_size;
        if (n) { void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0); if (m == MAP_FAILED) throw zarc::Error(ZARC_GPU_E_PARAM, path + ": mmap failed"); p = (const uint8_t *)m; }
    }
    ~Mapped() { if (p) munmap((void *)p, n); if (fd >= 0) close(fd); }
};

bool passes(const std::vector<std::regex> &filters, const std::string &name)
{
    if (filters.empty()) return true;
    for (const auto &f : filters) if (std::regex_search(name, f)) return true;
    return false;
}

void mkdirs(const std::string &path, mode_t mode)
{
    for (size_t i = 1; i <= path.size(); i++)
        if (i == path.size() || path[i] == '/') { const std::string sub = path.substr(0, i); if (!sub.empty()) (void)mkdir(sub.c_str(), i == path.size() ? mode : 0777); }
}

void set_metadata(const zarc::File &f, int fd) // unpack.rs:126-138: ownership, permissions, timestamps
{
    uid_t uid = (uid_t)-1; gid_t gid = (gid_t)-1;
    // by name first, then by id (directory/posix_owner.rs:25-110), through the cache
    if (f.user) { std::optional<uint32_t> v; if (f.user->name) v = g_owners.uid_from_name(*f.user->name); if (!v && f.user->id) v = (uint32_t)*f.user->id; if (v) uid = (uid_t)*v; }
    if (f.group) { std::optional<uint32_t> v; if (f.group->name) v = g_owners.gid_from_name(*f.group->name); if (!v && f.group->id) v = (uint32_t)*f.group->id; if (v) gid = (gid_t)*v; }
    if ((uid != (uid_t)-1 || gid != (gid_t)-1) && fchown(fd, uid, gid) != 0) { /* needs privileges; an unprivileged unpack keeps the caller's ids */ }
    if (f.mode) (void)fchmod(fd, (mode_t)(*f.mode & 07777));
    if (f.modified || f.accessed) {
        timespec ts[2];
        ts[0].tv_sec = f.accessed ? (time_t)f.accessed->secs : 0; ts[0].tv_nsec = f.accessed ? (long)f.accessed->nanos : UTIME_OMIT;
        ts[1].tv_sec = f.modified ? (time_t)f.modified->secs : 0; ts[1].tv_nsec = f.modified ? (long)f.modified->nanos : UTIME_OMIT;
        (void)futimens(fd, ts);
    }
}

int cmd_unpack(const std::vector<std::string> &a)
{
    std::string input, verify;
    std::vector<std::regex> filters;
    int gpus = 1;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i] == "--filter" && i + 1 < a.size()) filters.emplace_back(a[++i]);
        else if (a[i] == "--verify" && i + 1 < a.size()) verify = a[++i];
        else if (a[i] == "--gpus" && i + 1 < a.size()) gpus = std::atoi(a[++i].c_str());
        else if (!a[i].empty() && a[i][0] == '-') return usage();
        else input = a[i];
    }
    if (input.empty() || gpus < 1 || gpus > 64) return usage();
    if (gpus > zarc_gpu_device_count()) { std::fprintf(stderr, "Error: --gpus %d but %d device(s) are usable\n", gpus, zarc_gpu_device_count()); return 1; }
    Mapped m(input);
    std::vector<int> devices;
    for (int d = 0; d < gpus; d++) devices.push_back(d);
    zarc::ArchiveReader rd(m.p, m.n, devices); // frames of a batch are dealt to the devices by uncompressed bytes (zarc_host.hpp)
    const std::string digest = base64(rd.trailer().digest.bytes.data(), 32);
    if (!verify.empty()) {
        if (verify != digest) { std::fprintf(stderr, "Error: integrity failure: zarc file digest is %s\n", digest.c_str()); return 1; }
    } else std::fprintf(stderr, "digest: %s\n", digest.c_str());
    unsigned long long unpacked = 0;
    const size_t BATCH = (size_t)1 << 30;
    std::vector<size_t> batch;
    size_t batch_bytes = 0;
    // A writer thread creates and fills the files of batch k while this thread has the engine decode batch k+1.
    struct Done { std::vector<size_t> idx; std::vector<zarc::FrameReader::Result> res; };
    std::deque<Done> todo;
    std::mutex mu;
    std::condition_variable cv;
    bool no_more = false;
    std::string failure;
    std::thread writer([&] {
        for (;;) {
            Done d;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !todo.empty() || no_more; });
                if (todo.empty()) return;
                d = std::move(todo.front());
                todo.pop_front();
            }
            cv.notify_all();
            for (size_t k = 0; k < d.idx.size(); k++) {
                const zarc::File &f = rd.files()[d.idx[k]];
                const std::string path = to_path(f.name);
                std::string err;
                if (d.res[k].status != ZARC_GPU_FRAME_OK && d.res[k].status != ZARC_GPU_FRAME_DIGEST) err = path + ": " + zarc_gpu_frame_status_name(d.res[k].status);
                int fd = -1;
                if (err.empty()) {
                    const size_t slash = path.rfind('/');
                    if (slash != std::string::npos) mkdirs(path.substr(0, slash), 0777); // parent, in case its entry was not in the zarc
                    fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_NOFOLLOW, 0666);
                    if (fd < 0) err = path + ": " + std::strerror(errno);
                }
                size_t off = 0;
                while (err.empty() && off < d.res[k].data.size()) {
                    const ssize_t w = write(fd, d.res[k].data.data() + off, d.res[k].data.size() - off);
                    if (w <= 0) err = path + ": write failed"; else off += (size_t)w;
                }
                if (!err.empty()) { if (fd >= 0) close(fd); std::lock_guard<std::mutex> lk(mu); if (failure.empty()) failure = err; continue; }
                if (!d.res[k].verify.value_or(false)) std::fprintf(stderr, "ERROR frame verification failed! path=%s\n", path.c_str()); // unpack.rs:118-120
                set_metadata(f, fd);
                close(fd);
                LOGF(3, "extract_file", "path=%s bytes=%zu", path.c_str(), d.res[k].data.size());
                std::lock_guard<std::mutex> lk(mu);
                unpacked++;
            }
        }
    });
    auto flush = [&]() {
        if (batch.empty()) return;
        Done d;
        d.idx = batch;
        d.res = rd.read_files(batch);
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return todo.size() < 2; }); // at most two decoded batches in memory
            todo.push_back(std::move(d));
        }
        cv.notify_all();
        batch.clear();
        batch_bytes = 0;
    };
    // As in cmd_pack: the writer thread is stopped and joined on every way out of this function, exceptions included (a corrupt
    // frame record makes read_files throw in the middle of the loop).
    struct Joiner {
        std::thread &t; std::mutex &mu; std::condition_variable &cv; bool &stop;
        ~Joiner() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); if (t.joinable()) t.join(); }
    } joiner{writer, mu, cv, no_more};
    // Directories are MADE when their entry comes up (the files below them follow in the archive), but their metadata is applied
    // last, deepest first, once the writer thread has put every file on disk: creating a file inside a directory moves the
    // directory's mtime, and a read-only mode would refuse the files.  (The reference applies it at once, unpack.rs:62-88, and so
    // restores directory mtimes only for empty directories.)
    std::vector<size_t> dirs;
    for (size_t i = 0; i < rd.files().size(); i++) {
        const zarc::File &f = rd.files()[i];
        const std::string name = to_path(f.name);
        if (!passes(filters, name)) continue;
        if (!safe_name(f.name)) { std::fprintf(stderr, "WARN unsafe pathname skipped: %s\n", name.c_str()); continue; }
        if (f.is_dir()) {
            mkdirs(name, 0777);
            dirs.push_back(i);
        } else if (f.is_normal()) {
            auto it = rd.frames().find(*f.digest);
            if (it == rd.frames().end()) { std::fprintf(stderr, "WARN frame not found\n"); continue; } // unpack.rs:107-110
            batch.push_back(i);
            batch_bytes += (size_t)it->second.uncompressed;
            if (batch_bytes >= BATCH) flush();
        }
    }
    flush();
    { std::lock_guard<std::mutex> lk(mu); no_more = true; }
    cv.notify_all();
    writer.join();
    if (!failure.empty()) throw zarc::Error(ZARC_GPU_E_PARAM, failure);
    std::stable_sort(dirs.begin(), dirs.end(), [&](size_t x, size_t y) { return rd.files()[x].name.size() > rd.files()[y].name.size(); }); // more components first
    for (size_t i : dirs) {
        const zarc::File &f = rd.files()[i];
        const int fd = open(to_path(f.name).c_str(), O_RDONLY | O_DIRECTORY);
        if (fd >= 0) { set_metadata(f, fd); close(fd); }
    }
    std::fprintf(stderr, "unpacked %llu files\n", unpacked);
    return 0;
}

// `zarc verify`: is this archive good?  Every distinct content frame behind the files that pass the filters is decoded and judged on the
// device exactly as unpack would judge it (zarc_gpu_verify_batch), and nothing is created, opened or changed in the file system.
int cmd_verify(const std::vector<std::string> &a)
{
    std::string input, verify;
    std::vector<std::regex> filters;
    int gpus = 1;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i] == "--filter" && i + 1 < a.size()) filters.emplace_back(a[++i]);
        else if (a[i] == "--verify" && i + 1 < a.size()) verify = a[++i];
        else if (a[i] == "--gpus" && i + 1 < a.size()) gpus = std::atoi(a[++i].c_str());
        else if (!a[i].empty() && a[i][0] == '-') return usage();
        else input = a[i];
    }
    if (input.empty() || gpus < 1 || gpus > 64) return usage();
    if (gpus > zarc_gpu_device_count()) { std::fprintf(stderr, "Error: --gpus %d but %d device(s) are usable\n", gpus, zarc_gpu_device_count()); return 1; }
    Mapped m(input);
    std::vector<int> devices;
    for (int d = 0; d < gpus; d++) devices.push_back(d);
    zarc::ArchiveReader rd(m.p, m.n, devices);
    const std::string digest = base64(rd.trailer().digest.bytes.data(), 32);
    if (!verify.empty()) {
        if (verify != digest) { std::fprintf(stderr, "Error: integrity failure: zarc file digest is %s\n", digest.c_str()); return 1; }
    } else std::fprintf(stderr, "digest: %s\n", digest.c_str());
    // the files of every distinct frame: a frame is checked ONCE however many files share it
    std::map<zarc::Digest, std::vector<size_t>> files_of;
    std::vector<zarc::Digest> order;
    unsigned long long n_files = 0, failed = 0, bytes = 0;
    for (size_t i = 0; i < rd.files().size(); i++) {
        const zarc::File &f = rd.files()[i];
        if (!f.is_normal() || !passes(filters, to_path(f.name))) continue;
        n_files++;
        if (!rd.frames().count(*f.digest)) { // an archive test that shrugs at a missing frame is no test
            std::fprintf(stderr, "WARN frame not found path=%s\n", to_path(f.name).c_str());
            failed++;
            continue;
        }
        auto &v = files_of[*f.digest];
        if (v.empty()) order.push_back(*f.digest);
        v.push_back(i);
    }
    const size_t BATCH = (size_t)1 << 30;
    std::vector<zarc::Digest> batch;
    size_t batch_bytes = 0;
    auto flush = [&]() {
        if (batch.empty()) return;
        const std::vector<zarc::FrameReader::Result> res = rd.check_frames(batch);
        for (size_t k = 0; k < batch.size(); k++) {
            const bool decoded = res[k].status == ZARC_GPU_FRAME_OK || res[k].status == ZARC_GPU_FRAME_DIGEST;
            if (decoded && res[k].verify.value_or(false)) continue;
            for (size_t i : files_of[batch[k]]) {
                const std::string path = to_path(rd.files()[i].name);
                if (decoded) std::fprintf(stderr, "ERROR frame verification failed! path=%s\n", path.c_str()); // the text unpack prints (unpack.rs:118-120)
                else std::fprintf(stderr, "ERROR %s path=%s\n", zarc_gpu_frame_status_name(res[k].status), path.c_str());
                failed++;
            }
        }
        LOGF(3, "check_frames", "frames=%zu bytes=%zu", batch.size(), batch_bytes);
        batch.clear();
        batch_bytes = 0;
    };
    for (const zarc::Digest &d : order) {
        const uint64_t u = rd.frames().at(d).uncompressed;
        batch.push_back(d);
        batch_bytes += (size_t)u;
        bytes += u;
        if (batch_bytes >= BATCH) flush();
    }
    flush();
    std::fprintf(stderr, "verified %llu files (%zu frames, %llu bytes), %llu failed\n", n_files, order.size(), bytes, failed);
    return failed ? 1 : 0;
}

// `zarc cat`: the content of the files that pass the filters, or one byte or line range of each, on stdout.  With a range option every
// distinct content frame is decoded and judged on the device and only the range's bytes come back (zarc_gpu_read_ranges_batch); a frame
// that many files share is read once and printed once per file.  Nothing is created, opened or changed in the file system.
bool cat_number(const std::string &s, uint64_t *out) // plain decimal, no sign, no suffix
{
    if (s.empty() || s.size() > 20) return false;
    unsigned __int128 v = 0;
    for (char c : s) { if (c < '0' || c > '9') return false; v = v * 10 + (unsigned)(c - '0'); }
    if (v > (unsigned __int128)UINT64_MAX) return false;
    *out = (uint64_t)v;
    return true;
}
// A:[B] -> a and, where given, b
bool cat_pair(const std::string &s, uint64_t *a, uint64_t *b, bool *have_b)
{
    const size_t colon = s.find(':');
    if (colon == std::string::npos || !cat_number(s.substr(0, colon), a)) return false;
    *have_b = colon + 1 < s.size();
    return !*have_b || cat_number(s.substr(colon + 1), b);
}
int cmd_cat(const std::vector<std::string> &a)
{
    std::string input, verify;
    std::vector<std::regex> filters;
    int gpus = 1, range_options = 0;
    bool header = false;
    uint64_t batch_bytes = (uint64_t)256 << 20;
    zarc_gpu_range range{ZARC_GPU_RANGE_BYTES, 0, 0, ZARC_GPU_RANGE_ALL};
    for (size_t i = 0; i < a.size(); i++) {
        const bool value = i + 1 < a.size();
        if (a[i] == "--filter" && value) filters.emplace_back(a[++i]);
        else if (a[i] == "--verify" && value) verify = a[++i];
        else if (a[i] == "--gpus" && value) gpus = std::atoi(a[++i].c_str());
        else if (a[i] == "--header") header = true;
        else if (a[i] == "--batch-bytes" && value) { if (!cat_number(a[++i], &batch_bytes) || batch_bytes < 1) return usage(); }
        else if ((a[i] == "--head" || a[i] == "--head-bytes") && value) { // N: the first N; -N: all but the last N
            const uint32_t unit = a[i] == "--head" ? ZARC_GPU_RANGE_LINES : ZARC_GPU_RANGE_BYTES;
            const std::string v = a[++i];
            uint64_t n;
            const bool minus = !v.empty() && v[0] == '-';
            if (!cat_number(minus ? v.substr(1) : v, &n)) return usage();
            range = minus ? zarc_gpu_range{unit, ZARC_GPU_RANGE_FROM_END, n, ZARC_GPU_RANGE_ALL} : zarc_gpu_range{unit, 0, 0, n};
            range_options++;
        } else if ((a[i] == "--tail" || a[i] == "--tail-bytes") && value) { // N: the last N; +K: from the K-th on (+0 is +1, as tail has it)
            const uint32_t unit = a[i] == "--tail" ? ZARC_GPU_RANGE_LINES : ZARC_GPU_RANGE_BYTES;
            const std::string v = a[++i];
            uint64_t n;
            const bool plus = !v.empty() && v[0] == '+';
            if (!cat_number(plus ? v.substr(1) : v, &n)) return usage();
            range = plus ? zarc_gpu_range{unit, 0, n ? n - 1 : 0, ZARC_GPU_RANGE_ALL} : zarc_gpu_range{unit, ZARC_GPU_RANGE_FROM_END, 0, n};
            range_options++;
        } else if (a[i] == "--lines" && value) { // A:[B], 1-based, inclusive
            uint64_t from, to = 0;
            bool have_to;
            if (!cat_pair(a[++i], &from, &to, &have_to) || from < 1 || (have_to && to < from)) return usage();
            range = zarc_gpu_range{ZARC_GPU_RANGE_LINES, 0, from - 1, have_to ? to - from + 1 : ZARC_GPU_RANGE_ALL};
            range_options++;
        } else if (a[i] == "--bytes" && value) { // A:[B], 0-based, half-open
            uint64_t from, to = 0;
            bool have_to;
            if (!cat_pair(a[++i], &from, &to, &have_to) || (have_to && to < from)) return usage();
            range = zarc_gpu_range{ZARC_GPU_RANGE_BYTES, 0, from, have_to ? to - from : ZARC_GPU_RANGE_ALL};
            range_options++;
        } else if (!a[i].empty() && a[i][0] == '-') return usage();
        else if (!input.empty()) return usage();
        else input = a[i];
    }
    if (input.empty() || gpus < 1 || gpus > 64 || range_options > 1) return usage();
    if (gpus > zarc_gpu_device_count()) { std::fprintf(stderr, "Error: --gpus %d but %d device(s) are usable\n", gpus, zarc_gpu_device_count()); return 1; }
    Mapped m(input);
    std::vector<int> devices;
    for (int d = 0; d < gpus; d++) devices.push_back(d);
    zarc::ArchiveReader rd(m.p, m.n, devices);
    const std::string digest = base64(rd.trailer().digest.bytes.data(), 32);
    if (!verify.empty()) {
        if (verify != digest) { std::fprintf(stderr, "Error: integrity failure: zarc file digest is %s\n", digest.c_str()); return 1; }
    } else std::fprintf(stderr, "digest: %s\n", digest.c_str());
    unsigned long long n_files = 0, failed = 0, bytes = 0;
    bool first_header = true;
    // one file's turn: its header and bytes, or the message of a frame that is not good
    auto print = [&](size_t file, const zarc::FrameReader::Result &r) {
        const std::string path = to_path(rd.files()[file].name);
        if (r.status != ZARC_GPU_FRAME_OK && r.status != ZARC_GPU_FRAME_DIGEST) {
            std::fprintf(stderr, "ERROR %s path=%s\n", zarc_gpu_frame_status_name(r.status), path.c_str());
            failed++;
            return;
        }
        if (header) { std::fprintf(stdout, "%s==> %s <==\n", first_header ? "" : "\n", path.c_str()); first_header = false; } // head -v, byte for byte
        if (!r.data.empty() && std::fwrite(r.data.data(), 1, r.data.size(), stdout) != r.data.size()) throw zarc::Error(ZARC_GPU_E_PARAM, "stdout: write failed");
        bytes += r.data.size();
        if (!r.verify.value_or(false)) { std::fprintf(stderr, "ERROR frame verification failed! path=%s\n", path.c_str()); failed++; } // delivered all the same (unpack.rs:118-120)
    };
    // the selection is grep's: regular files that pass the filters, in directory order
    std::vector<size_t> selected;
    std::map<zarc::Digest, size_t> uses; // files of every distinct frame that are still to print
    for (size_t i = 0; i < rd.files().size(); i++) {
        const zarc::File &f = rd.files()[i];
        if (!f.is_normal() || !passes(filters, to_path(f.name))) continue;
        n_files++;
        if (!rd.frames().count(*f.digest)) { std::fprintf(stderr, "WARN frame not found path=%s\n", to_path(f.name).c_str()); failed++; continue; }
        selected.push_back(i);
        uses[*f.digest]++;
    }
    const size_t n_frames = uses.size();
    const size_t BATCH = (size_t)1 << 30;
    if (!range_options) { // whole files: unpack's path
        std::vector<size_t> batch;
        size_t weight = 0;
        auto flush = [&]() {
            if (batch.empty()) return;
            const std::vector<zarc::FrameReader::Result> res = rd.read_files(batch);
            for (size_t k = 0; k < batch.size(); k++) print(batch[k], res[k]);
            batch.clear();
            weight = 0;
        };
        for (size_t i : selected) {
            batch.push_back(i);
            weight += (size_t)rd.frames().at(*rd.files()[i].digest).uncompressed;
            if (weight >= BATCH) flush();
        }
        flush();
    } else {
        // batches of distinct frames in the order their first file comes up; a batch's files are printed in directory order behind it, and
        // a frame's result stays until its last file is out
        std::map<zarc::Digest, zarc::FrameReader::Result> have;
        std::vector<zarc::Digest> batch;
        std::vector<size_t> waiting; // files of this batch's turn
        size_t weight = 0;
        auto flush = [&]() {
            if (!batch.empty()) {
                std::vector<zarc::FrameReader::Result> res = rd.read_ranges(batch, std::vector<zarc_gpu_range>(batch.size(), range), 0, (size_t)batch_bytes);
                for (;;) { // what --batch-bytes cut off: the rest by BYTES ranges (the frames are decoded again), until nothing is cut
                    std::vector<size_t> cut;
                    std::vector<zarc::Digest> again;
                    std::vector<zarc_gpu_range> rest;
                    for (size_t k = 0; k < batch.size(); k++)
                        if (res[k].data.size() < res[k].range.length) {
                            cut.push_back(k); again.push_back(batch[k]);
                            rest.push_back(zarc_gpu_range{ZARC_GPU_RANGE_BYTES, 0, res[k].range.start + res[k].data.size(), res[k].range.length - res[k].data.size()});
                        }
                    if (cut.empty()) break;
                    const std::vector<zarc::FrameReader::Result> more = rd.read_ranges(again, rest, 0, (size_t)batch_bytes);
                    for (size_t j = 0; j < cut.size(); j++) res[cut[j]].data.insert(res[cut[j]].data.end(), more[j].data.begin(), more[j].data.end());
                    LOGF(3, "read_ranges", "continued frames=%zu", cut.size());
                }
                for (size_t k = 0; k < batch.size(); k++) have.emplace(batch[k], std::move(res[k]));
                LOGF(3, "read_ranges", "frames=%zu bytes=%zu", batch.size(), weight);
            }
            for (size_t i : waiting) {
                const zarc::Digest &d = *rd.files()[i].digest;
                print(i, have.at(d));
                if (--uses[d] == 0) have.erase(d);
            }
            batch.clear();
            waiting.clear();
            weight = 0;
        };
        std::map<zarc::Digest, bool> asked;
        for (size_t i : selected) {
            const zarc::Digest &d = *rd.files()[i].digest;
            waiting.push_back(i);
            if (!asked[d]) {
                asked[d] = true;
                batch.push_back(d);
                weight += (size_t)rd.frames().at(d).uncompressed;
                if (weight >= BATCH) flush();
            }
        }
        flush();
    }
    std::fflush(stdout);
    std::fprintf(stderr, "printed %llu files (%zu frames, %llu bytes), %llu failed\n", n_files, n_frames, bytes, failed);
    return failed ? 1 : 0;
}

// `zarc wc`: lines, words, characters, bytes and the longest line of the files that pass the filters.  Every distinct content frame is
// decoded, judged and counted on the device (zarc_gpu_count_batch) and 64 bytes a frame come back; a frame that many files share is counted
// once and reported for each of them.  Nothing is created, opened or changed in the file system.
int cmd_wc(const std::vector<std::string> &a)
{
    std::string input, verify;
    std::vector<std::regex> filters;
    int gpus = 1;
    bool want_l = false, want_w = false, want_m = false, want_c = false, want_max = false, longest = false;
    for (size_t i = 0; i < a.size(); i++) {
        const bool value = i + 1 < a.size();
        if (a[i] == "--filter" && value) filters.emplace_back(a[++i]);
        else if (a[i] == "--verify" && value) verify = a[++i];
        else if (a[i] == "--gpus" && value) gpus = std::atoi(a[++i].c_str());
        else if (a[i] == "-l") want_l = true;
        else if (a[i] == "-w") want_w = true;
        else if (a[i] == "-m") want_m = true;
        else if (a[i] == "-c") want_c = true;
        else if (a[i] == "--max-line-bytes") want_max = true;
        else if (a[i] == "--longest") longest = want_max = true;
        else if (!a[i].empty() && a[i][0] == '-') return usage();
        else if (!input.empty()) return usage();
        else input = a[i];
    }
    if (input.empty() || gpus < 1 || gpus > 64) return usage();
    if (!(want_l || want_w || want_m || want_c || want_max)) want_l = want_w = want_c = true; // as wc
    if (gpus > zarc_gpu_device_count()) { std::fprintf(stderr, "Error: --gpus %d but %d device(s) are usable\n", gpus, zarc_gpu_device_count()); return 1; }
    Mapped m(input);
    std::vector<int> devices;
    for (int d = 0; d < gpus; d++) devices.push_back(d);
    zarc::ArchiveReader rd(m.p, m.n, devices);
    const std::string digest = base64(rd.trailer().digest.bytes.data(), 32);
    if (!verify.empty()) {
        if (verify != digest) { std::fprintf(stderr, "Error: integrity failure: zarc file digest is %s\n", digest.c_str()); return 1; }
    } else std::fprintf(stderr, "digest: %s\n", digest.c_str());
    unsigned long long n_files = 0, failed = 0, printed = 0;
    zarc::FrameReader::Result::Count total;
    uint64_t total_bytes = 0;
    auto row = [&](const zarc::FrameReader::Result::Count &c, uint64_t bytes, bool is_total, const std::string &name) {
        std::string s;
        if (want_l) s += std::to_string(c.lines) + " ";
        if (want_w) s += std::to_string(c.words) + " ";
        if (want_m) s += std::to_string(c.chars) + " ";
        if (want_c) s += std::to_string(bytes) + " ";
        if (want_max) {
            s += std::to_string(c.max_line);
            if (longest && !is_total) s += ":" + std::to_string(c.max_line_no) + ":" + std::to_string(c.max_line_start);
            s += " ";
        }
        std::fprintf(stdout, "%s%s\n", s.c_str(), name.c_str());
    };
    // one file's turn: its line, or the message of a frame that is not good
    auto print = [&](size_t file, const zarc::FrameReader::Result &r) {
        const std::string path = to_path(rd.files()[file].name);
        const bool decoded = r.status == ZARC_GPU_FRAME_OK || r.status == ZARC_GPU_FRAME_DIGEST;
        if (!decoded || !r.verify.value_or(false)) { // verify's messages
            if (decoded) std::fprintf(stderr, "ERROR frame verification failed! path=%s\n", path.c_str());
            else std::fprintf(stderr, "ERROR %s path=%s\n", zarc_gpu_frame_status_name(r.status), path.c_str());
            failed++;
            return;
        }
        const uint64_t bytes = rd.frames().at(*rd.files()[file].digest).uncompressed;
        row(r.wc, bytes, false, path);
        printed++;
        total.lines += r.wc.lines; total.words += r.wc.words; total.chars += r.wc.chars; total_bytes += bytes;
        total.max_line = std::max(total.max_line, r.wc.max_line);
    };
    // the selection is grep's: regular files that pass the filters, in directory order.  Batches of distinct frames in the order their first
    // file comes up; a batch's files are printed in directory order behind it, and a frame's result stays until its last file is out
    std::vector<size_t> selected;
    std::map<zarc::Digest, size_t> uses;
    for (size_t i = 0; i < rd.files().size(); i++) {
        const zarc::File &f = rd.files()[i];
        if (!f.is_normal() || !passes(filters, to_path(f.name))) continue;
        n_files++;
        if (!rd.frames().count(*f.digest)) { std::fprintf(stderr, "WARN frame not found path=%s\n", to_path(f.name).c_str()); failed++; continue; }
        selected.push_back(i);
        uses[*f.digest]++;
    }
    const size_t n_frames = uses.size();
    const size_t BATCH = (size_t)1 << 30;
    std::map<zarc::Digest, zarc::FrameReader::Result> have;
    std::vector<zarc::Digest> batch;
    std::vector<size_t> waiting; // files of this batch's turn
    size_t weight = 0;
    auto flush = [&]() {
        if (!batch.empty()) {
            std::vector<zarc::FrameReader::Result> res = rd.count_frames(batch);
            for (size_t k = 0; k < batch.size(); k++) have.emplace(batch[k], std::move(res[k]));
            LOGF(3, "count_frames", "frames=%zu bytes=%zu", batch.size(), weight);
        }
        for (size_t i : waiting) {
            const zarc::Digest &d = *rd.files()[i].digest;
            print(i, have.at(d));
            if (--uses[d] == 0) have.erase(d);
        }
        batch.clear();
        waiting.clear();
        weight = 0;
    };
    std::map<zarc::Digest, bool> asked;
    for (size_t i : selected) {
        const zarc::Digest &d = *rd.files()[i].digest;
        waiting.push_back(i);
        if (!asked[d]) {
            asked[d] = true;
            batch.push_back(d);
            weight += (size_t)rd.frames().at(d).uncompressed;
            if (weight >= BATCH) flush();
        }
    }
    flush();
    if (printed > 1) row(total, total_bytes, true, "total");
    std::fflush(stdout);
    std::fprintf(stderr, "counted %llu files (%zu frames), %llu failed\n", n_files, n_frames, failed);
    return failed ? 1 : 0;
}

// the work of `zarc compare` behind its options; a zarc::Error leaves through cmd_compare
int compare_run(const std::string &input, const std::string &verify, const std::string &dir, const std::vector<std::regex> &filters, int gpus, bool brief,
                bool identical, uint64_t batch_bytes)
{
    Mapped m(input);
    std::vector<int> devices;
    for (int d = 0; d < gpus; d++) devices.push_back(d);
    zarc::ArchiveReader rd(m.p, m.n, devices);
    const std::string digest = base64(rd.trailer().digest.bytes.data(), 32);
    if (!verify.empty()) {
        if (verify != digest) { std::fprintf(stderr, "Error: integrity failure: zarc file digest is %s\n", digest.c_str()); return 2; }
    } else std::fprintf(stderr, "digest: %s\n", digest.c_str());
    unsigned long long n_files = 0, n_same = 0, n_differ = 0, n_missing = 0, n_bad = 0;
    // a file's turn: a line that is known without the device, or the pair it waits for
    struct Turn { std::string path, line; size_t pair; };
    std::vector<Turn> turns;
    std::vector<zarc::Digest> batch;
    std::vector<std::vector<uint8_t>> disk;
    uint64_t weight = 0;
    auto say = [&](const std::string &path, const std::string &what) { std::fprintf(stdout, brief ? "%s\n" : "%s: %s\n", path.c_str(), what.c_str()); };
    auto flush = [&]() {
        std::vector<zarc::FrameReader::Result> res;
        if (!batch.empty()) {
            std::vector<zarc::FrameReader::Other> others;
            for (const auto &d : disk) others.push_back(zarc::FrameReader::Other{d.empty() ? nullptr : d.data(), d.size()});
            res = rd.compare_frames(batch, others);
            LOGF(3, "compare_frames", "pairs=%zu bytes=%llu", batch.size(), (unsigned long long)weight);
        }
        for (const Turn &t : turns) {
            if (!t.line.empty()) { say(t.path, t.line); continue; }
            const zarc::FrameReader::Result &r = res[t.pair];
            const bool decoded = r.status == ZARC_GPU_FRAME_OK || r.status == ZARC_GPU_FRAME_DIGEST;
            if (!decoded || !r.verify.value_or(false)) { // verify's words
                say(t.path, std::string("bad frame (") + (decoded ? "frame verification failed!" : zarc_gpu_frame_status_name(r.status)) + ")");
                n_bad++;
                continue;
            }
            const zarc::FrameReader::Result::Compare &c = r.cmp;
            const unsigned long long la = rd.frames().at(batch[t.pair]).uncompressed, lb = disk[t.pair].size();
            const std::string line = ", line " + std::to_string(c.line);
            switch (c.relation) {
            case ZARC_GPU_CMP_EQUAL:
                n_same++;
                if (identical) say(t.path, "identical");
                break;
            case ZARC_GPU_CMP_DIFFER: {
                std::string s = "differ: byte " + std::to_string(c.prefix + 1) + line + ", " + std::to_string(c.differing) + " bytes differ";
                if (la != lb) s += ", sizes " + std::to_string(la) + " and " + std::to_string(lb) + ", common tail " + std::to_string(c.suffix);
                say(t.path, s);
                n_differ++;
                break;
            }
            case ZARC_GPU_CMP_FRAME_IS_PREFIX:
                say(t.path, "archive copy is a prefix: " + std::to_string(la) + " of " + std::to_string(lb) + " bytes" + line);
                n_differ++;
                break;
            case ZARC_GPU_CMP_OTHER_IS_PREFIX:
                say(t.path, "file is a prefix: " + std::to_string(lb) + " of " + std::to_string(la) + " bytes" + line);
                n_differ++;
                break;
            default:
                say(t.path, "bad frame (no result)");
                n_bad++;
            }
        }
        turns.clear();
        batch.clear();
        disk.clear();
        weight = 0;
    };
    // the selection is grep's: regular files that pass the filters, in directory order
    for (size_t i = 0; i < rd.files().size(); i++) {
        const zarc::File &f = rd.files()[i];
        const std::string path = to_path(f.name);
        if (!f.is_normal() || !passes(filters, path)) continue;
        n_files++;
        if (!rd.frames().count(*f.digest)) { turns.push_back(Turn{path, "bad frame (frame not found)", 0}); n_bad++; continue; }
        // (an entry name is untrusted, as in unpack: nothing outside DIR is looked at)
        if (!safe_name(f.name)) { turns.push_back(Turn{path, "unsafe pathname, not compared", 0}); n_bad++; continue; }
        const std::string on_disk = dir + "/" + path;
        struct stat st;
        if (lstat(on_disk.c_str(), &st) != 0) {
            if (errno == ENOENT || errno == ENOTDIR) { turns.push_back(Turn{path, "missing", 0}); n_missing++; }
            else { turns.push_back(Turn{path, std::string("unreadable (") + std::strerror(errno) + ")", 0}); n_bad++; }
            continue;
        }
        if (!S_ISREG(st.st_mode)) { turns.push_back(Turn{path, "not a regular file", 0}); n_differ++; continue; }
        if ((uint64_t)st.st_size >= 0xFFFFFFF0ull) { turns.push_back(Turn{path, "unreadable (files of 4 GiB or more are not supported)", 0}); n_bad++; continue; }
        std::vector<uint8_t> bytes((size_t)st.st_size);
        const int fd = open(on_disk.c_str(), O_RDONLY);
        size_t got = 0;
        int read_errno = fd >= 0 ? 0 : errno;
        while (!read_errno && got < bytes.size()) {
            const ssize_t k = read(fd, bytes.data() + got, bytes.size() - got);
            if (k < 0 && errno == EINTR) continue;
            if (k < 0) { read_errno = errno; break; }
            if (k == 0) break; // (a file that shrank meanwhile is what was read of it)
            got += (size_t)k;
        }
        if (fd >= 0) close(fd);
        if (read_errno) { turns.push_back(Turn{path, std::string("unreadable (") + std::strerror(read_errno) + ")", 0}); n_bad++; continue; }
        bytes.resize(got);
        turns.push_back(Turn{path, "", batch.size()});
        batch.push_back(*f.digest);
        weight += bytes.size();
        disk.push_back(std::move(bytes));
        if (weight >= batch_bytes) flush();
    }
    flush();
    std::fflush(stdout);
    std::fprintf(stderr, "compared %llu files: %llu identical, %llu differ, %llu missing, %llu failed\n", n_files, n_same, n_differ, n_missing, n_bad);
    return n_bad ? 2 : (n_differ || n_missing) ? 1 : 0;
}

// `zarc compare`: is the tree on disk still what was packed, and where does it differ?  The content of every regular file that passes the
// filters is decoded and judged on the device and compared there with the bytes of DIR/PATH (zarc_gpu_compare_batch): the frames and the
// disk content go up, 64 bytes a pair come back.  A frame that several files share is one pair per file.  Content only: no symbolic
// links, directories, modes, owners or times.  Nothing is created or changed in the file system.
int cmd_compare(const std::vector<std::string> &a)
{
    std::string input, verify, dir = ".";
    std::vector<std::regex> filters;
    int gpus = 1;
    bool brief = false, identical = false;
    uint64_t batch_bytes = (uint64_t)256 << 20;
    for (size_t i = 0; i < a.size(); i++) {
        const bool value = i + 1 < a.size();
        if (a[i] == "--filter" && value) filters.emplace_back(a[++i]);
        else if (a[i] == "--verify" && value) verify = a[++i];
        else if (a[i] == "--gpus" && value) gpus = std::atoi(a[++i].c_str());
        else if ((a[i] == "-C" || a[i] == "--directory") && value) dir = a[++i];
        else if (a[i] == "--brief") brief = true;
        else if (a[i] == "--report-identical") identical = true;
        else if (a[i] == "--batch-bytes" && value) { if (!cat_number(a[++i], &batch_bytes) || batch_bytes < 1) return usage(); }
        else if (!a[i].empty() && a[i][0] == '-') return usage();
        else if (!input.empty()) return usage();
        else input = a[i];
    }
    if (input.empty() || dir.empty() || gpus < 1 || gpus > 64) return usage();
    if (gpus > zarc_gpu_device_count()) { std::fprintf(stderr, "Error: --gpus %d but %d device(s) are usable\n", gpus, zarc_gpu_device_count()); return 2; }
    // exit status 1 means "something differs": an archive that cannot be read or an engine error is trouble, 2, with what was found so far
    try {
        return compare_run(input, verify, dir, filters, gpus, brief, identical, batch_bytes);
    } catch (const zarc::Error &e) {
        std::fflush(stdout);
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 2;
    }
}

// `zarc grep`: which files contain this byte string?  Every distinct content frame behind the files that pass the filters is decoded,
// judged and searched on the device (zarc_gpu_search_batch; with -e / -f / --tally a set of strings in one pass, zarc_gpu_search_set_batch;
// with -E a regular expression, zarc_gpu_search_regex_batch):
// the compressed bytes go up, a few words per frame come back, and a frame that many files share is searched once.  Nothing is created, opened or changed in the file system.  Exit status: grep's.
int cmd_grep(const std::vector<std::string> &a)
{
    std::string pattern, input, verify;
    std::vector<std::regex> filters;
    bool icase = false, names_only = false, with_offset = false, hex = false, have_pattern = false, options = true;
    bool lines_mode = false, numbers = false, count_lines = false, as_text = false; // lines mode (any of its flags selects it)
    long long max_per_file = 0, max_line = 4096, batch_lines = 1048576;
    int gpus = 1;
    std::vector<std::string> typed; // -e / -f: the patterns of a set, as given
    bool use_set = false, tally = false;
    bool ere = false; // -E: PATTERN is a regular expression (zarc_gpu_search_regex_batch*)
    bool only = false; // --only-matching (grep's -o; the short form stays the usage error it was): every match of the matching lines in place of the lines (zarc_gpu_search_matches_batch); selects lines mode
    zarc::LineSelect sel; // -v, -A, -B, -C: the selected lines (zarc_gpu_select_lines_batch); any of them selects lines mode
    auto context = [&](char which, const std::string &num) { // -A NUM, -B NUM, -C NUM; false: not a number
        if (num.empty() || num.find_first_not_of("0123456789") != std::string::npos) return false;
        const unsigned long long v = std::strtoull(num.c_str(), nullptr, 10);
        const uint32_t n = v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
        if (which != 'B') sel.after = n;
        if (which != 'A') sel.before = n;
        lines_mode = true;
        return true;
    };
    for (size_t i = 0; i < a.size(); i++) {
        if (options && a[i] == "--filter" && i + 1 < a.size()) filters.emplace_back(a[++i]);
        else if (options && a[i] == "-e" && i + 1 < a.size()) { typed.push_back(a[++i]); use_set = true; }
        else if (options && a[i] == "-f" && i + 1 < a.size()) {
            use_set = true;
            std::ifstream in(a[++i], std::ios::binary);
            if (!in) { std::fprintf(stderr, "Error: cannot read the pattern file %s\n", a[i].c_str()); return 2; }
            const std::string all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            for (size_t at = 0; at < all.size();) { // LF-terminated lines; a final LF opens no further line
                const size_t nl = all.find('\n', at);
                const std::string line = all.substr(at, nl == std::string::npos ? std::string::npos : nl - at);
                if (line.empty()) { std::fprintf(stderr, "Error: an empty line in the pattern file %s\n", a[i].c_str()); return 2; }
                typed.push_back(line);
                at = nl == std::string::npos ? all.size() : nl + 1;
            }
        }
        else if (options && a[i] == "--tally") tally = true;
        else if (options && a[i] == "--lines") lines_mode = true;
        else if (options && a[i] == "-m" && i + 1 < a.size()) { max_per_file = std::atoll(a[++i].c_str()); lines_mode = true; if (max_per_file < 1) return usage(); }
        else if (options && a[i] == "--max-line" && i + 1 < a.size()) { max_line = std::atoll(a[++i].c_str()); lines_mode = true; if (max_line < 1 || max_line > ZARC_GPU_LINES_MAX_LINE) return usage(); }
        else if (options && a[i] == "--batch-lines" && i + 1 < a.size()) { batch_lines = std::atoll(a[++i].c_str()); lines_mode = true; if (batch_lines < 1) return usage(); }
        else if (options && a[i] == "--verify" && i + 1 < a.size()) verify = a[++i];
        else if (options && a[i] == "--gpus" && i + 1 < a.size()) gpus = std::atoi(a[++i].c_str());
        else if (options && a[i] == "--hex") hex = true;
        else if (options && a[i] == "--extended-regexp") ere = true;
        else if (options && a[i] == "--only-matching") only = lines_mode = true;
        else if (options && a[i] == "--") options = false;
        else if (options && a[i].size() >= 2 && a[i][0] == '-' && a[i][1] != '-') { // -i -l -b -F, alone or bundled
            for (size_t k = 1; k < a[i].size(); k++) {
                if (a[i][k] == 'i') icase = true;
                else if (a[i][k] == 'l') names_only = true;
                else if (a[i][k] == 'b') with_offset = true;
                else if (a[i][k] == 'F') {} // fixed strings are the default
                else if (a[i][k] == 'E') ere = true;
                else if (a[i][k] == 'n') numbers = lines_mode = true;
                else if (a[i][k] == 'c') count_lines = lines_mode = true;
                else if (a[i][k] == 'a') as_text = lines_mode = true;
                else if (a[i][k] == 'v') sel.invert = lines_mode = true;
                else if (a[i][k] == 'A' || a[i][k] == 'B' || a[i][k] == 'C') { // the number follows in this argument or is the next one
                    const std::string num = k + 1 < a[i].size() ? a[i].substr(k + 1) : (i + 1 < a.size() ? a[i + 1] : std::string());
                    if (!context(a[i][k], num)) return usage();
                    if (k + 1 >= a[i].size()) i++;
                    break;
                }
                else return usage();
            }
        } else if (options && a[i].size() >= 2 && a[i][0] == '-') return usage();
        else if (!have_pattern) { pattern = a[i]; have_pattern = true; }
        else if (input.empty()) input = a[i];
        else return usage();
    }
    if (use_set || tally) { // the set's patterns came with -e / -f (--tally alone: the one PATTERN is a set of one): ARCHIVE is the only other argument
        if (use_set) { if (!have_pattern || !input.empty()) return usage(); input = pattern; }
        else { if (!have_pattern) return usage(); typed.push_back(pattern); use_set = true; }
        have_pattern = true;
        if (typed.empty()) { std::fprintf(stderr, "Error: no pattern\n"); return 2; }
    } else typed.push_back(pattern);
    if (!have_pattern || input.empty() || gpus < 1 || gpus > 64) return usage();
    if (sel.active() && tally) return usage(); // the tally counts positions: there is no line to select
    if (only && (sel.active() || tally)) return usage(); // a line without a match, a context line and the tally have no match to print
    if (count_lines || names_only) only = false; // as in GNU grep with -o: -c and -l count and name what they would without it
    if (ere) { // several expressions are one alternation, as in grep; a bad one is refused here, before the archive is opened
        if (hex || tally) return usage();
        std::string joined;
        for (size_t k = 0; k < typed.size(); k++) joined += use_set ? (k ? "|(" : "(") + typed[k] + ")" : typed[k];
        char why[256];
        if (zarc_gpu_regex_compile(joined.data(), joined.size(), icase ? (unsigned)ZARC_GPU_SEARCH_ICASE : 0u, nullptr, why, sizeof why) != ZARC_GPU_OK) {
            std::fprintf(stderr, "Error: %s\n", why);
            return 2;
        }
        if (only && zarc_gpu_regex_compile_ends(joined.data(), joined.size(), icase ? (unsigned)ZARC_GPU_SEARCH_ICASE : 0u, nullptr, why, sizeof why) != ZARC_GPU_OK) {
            std::fprintf(stderr, "Error: --only-matching: %s\n", why); // (the table that finds a match's end is a second one: it can be too large where the first is not)
            return 2;
        }
        typed.assign(1, joined);
        use_set = false;
    }
    std::vector<std::string> given = typed; // the patterns' bytes
    if (hex)
        for (std::string &g : given) {
            std::string raw;
            if (g.size() % 2) { std::fprintf(stderr, "Error: --hex wants an even number of hex digits\n"); return 2; }
            for (size_t k = 0; k < g.size(); k += 2) {
                if (!std::isxdigit((unsigned char)g[k]) || !std::isxdigit((unsigned char)g[k + 1])) { std::fprintf(stderr, "Error: --hex wants hex digits\n"); return 2; }
                raw.push_back((char)std::stoi(g.substr(k, 2), nullptr, 16));
            }
            g = raw;
        }
    for (const std::string &g : given) {
        if (ere) break; // (the compiler has judged it)
        if (g.empty() || g.size() > ZARC_GPU_SEARCH_MAX_PATTERN) { std::fprintf(stderr, "Error: the pattern has 1 to %d bytes\n", ZARC_GPU_SEARCH_MAX_PATTERN); return 2; }
        if (lines_mode && !tally && g.find('\n') != std::string::npos) { std::fprintf(stderr, "Error: the pattern must not contain a newline when lines are asked for\n"); return 2; }
    }
    pattern = given[0];
    // a set: patterns that are equal after folding are searched once; slot_of[k] = where the k-th given pattern lies in the set
    std::vector<std::string> set;
    std::vector<size_t> slot_of;
    if (use_set) {
        std::map<std::string, size_t> seen;
        for (const std::string &g : given) {
            std::string key = g;
            if (icase) for (char &ch : key) if (ch >= 'A' && ch <= 'Z') ch = (char)(ch | 0x20);
            auto it = seen.find(key);
            if (it == seen.end()) { it = seen.emplace(key, set.size()).first; set.push_back(g); }
            slot_of.push_back(it->second);
        }
        if (set.size() > ZARC_GPU_SEARCH_MAX_SET) { std::fprintf(stderr, "Error: a set has at most %d different patterns\n", ZARC_GPU_SEARCH_MAX_SET); return 2; }
        if (tally) lines_mode = false; // the tally replaces the per-file output: the counting pass gives it
    }
    try {
        if (gpus > zarc_gpu_device_count()) { std::fprintf(stderr, "Error: --gpus %d but %d device(s) are usable\n", gpus, zarc_gpu_device_count()); return 2; }
        Mapped m(input);
        std::vector<int> devices;
        for (int d = 0; d < gpus; d++) devices.push_back(d);
        zarc::ArchiveReader rd(m.p, m.n, devices);
        const std::string digest = base64(rd.trailer().digest.bytes.data(), 32);
        if (!verify.empty()) {
            if (verify != digest) { std::fprintf(stderr, "Error: integrity failure: zarc file digest is %s\n", digest.c_str()); return 2; }
        } else std::fprintf(stderr, "digest: %s\n", digest.c_str());
        // the files of every distinct frame: a frame is searched ONCE however many files share it
        std::map<zarc::Digest, std::vector<size_t>> files_of;
        std::vector<zarc::Digest> order;
        unsigned long long n_files = 0, failed = 0, bytes = 0, matched = 0;
        for (size_t i = 0; i < rd.files().size(); i++) {
            const zarc::File &f = rd.files()[i];
            if (!f.is_normal() || !passes(filters, to_path(f.name))) continue;
            n_files++;
            if (!rd.frames().count(*f.digest)) {
                std::fprintf(stderr, "WARN frame not found path=%s\n", to_path(f.name).c_str());
                failed++;
                continue;
            }
            auto &v = files_of[*f.digest];
            if (v.empty()) order.push_back(*f.digest);
            v.push_back(i);
        }
        if (lines_mode && only) {
            // ---- --only-matching: every match of the matching lines (zarc_gpu_search_matches_batch), printed per file in directory order as
            // PATH:[NUMBER:][OFFSET:]MATCH.  -m NUM counts lines, as in GNU grep.  One call lets at most --batch-lines lines take part and
            // brings back at most --batch-lines matches; frames behind the one at which either ran out are searched again in a following
            // call, and a frame that is first in its call and still has more than fit prints what it got and says so.
            zarc::MatchWhat what;
            what.kind = use_set ? ZARC_GPU_MATCH_SET : ere ? ZARC_GPU_MATCH_REGEX : ZARC_GPU_MATCH_FIXED;
            what.text = pattern; what.set = set;
            const uint64_t per_frame = (uint64_t)max_per_file;
            std::map<zarc::Digest, zarc::FrameReader::Result> done;
            std::map<zarc::Digest, uint64_t> lines_in; // the lines of the frame that took part
            const size_t BATCH = (size_t)1 << 30;
            size_t at = 0;
            for (const zarc::Digest &d : order) bytes += rd.frames().at(d).uncompressed;
            while (at < order.size()) {
                std::vector<zarc::Digest> batch;
                for (size_t batch_bytes = 0; at + batch.size() < order.size() && batch_bytes < BATCH; batch_bytes += (size_t)rd.frames().at(batch.back()).uncompressed)
                    batch.push_back(order[at + batch.size()]);
                std::vector<zarc::FrameReader::Result> res = rd.search_matches(batch, what, icase, per_frame, (uint64_t)max_line, (size_t)batch_lines, (size_t)batch_lines);
                LOGF(3, "search_matches", "frames=%zu", batch.size());
                size_t taken = batch.size();
                uint64_t lines_left = (uint64_t)batch_lines;
                for (size_t k = 0; k < batch.size(); k++) {
                    const uint64_t want = per_frame ? std::min<uint64_t>(res[k].lines, per_frame) : res[k].lines;
                    const uint64_t got = std::min<uint64_t>(want, lines_left);
                    if (k > 0 && (got < want || res[k].match_records.size() < res[k].matches)) { taken = k; break; } // a cap ran out here: this frame and the rest again
                    lines_left -= got;
                    lines_in[batch[k]] = got;
                    done[batch[k]] = std::move(res[k]);
                }
                at += taken;
            }
            for (size_t i = 0; i < rd.files().size(); i++) {
                const zarc::File &f = rd.files()[i];
                if (!f.is_normal() || !passes(filters, to_path(f.name)) || !done.count(*f.digest)) continue;
                const zarc::FrameReader::Result &r = done.at(*f.digest);
                const std::string path = to_path(f.name);
                const bool decoded = r.status == ZARC_GPU_FRAME_OK || r.status == ZARC_GPU_FRAME_DIGEST;
                if (!(decoded && r.verify.value_or(false))) {
                    if (decoded) std::fprintf(stderr, "ERROR frame verification failed! path=%s\n", path.c_str());
                    else std::fprintf(stderr, "ERROR %s path=%s\n", zarc_gpu_frame_status_name(r.status), path.c_str());
                    failed++;
                    continue;
                }
                if (!r.lines) continue;
                matched++;
                bool binary = false;
                if (!as_text) for (const auto &x : r.match_records) binary = binary || std::memchr(x.text.data(), 0, x.text.size()) != nullptr;
                if (binary) { std::printf("Binary file %s matches\n", path.c_str()); continue; }
                for (const auto &x : r.match_records) {
                    std::printf("%s:", path.c_str());
                    if (numbers) std::printf("%llu:", (unsigned long long)x.number);
                    if (with_offset) std::printf("%llu:", (unsigned long long)x.start);
                    std::fwrite(x.text.data(), 1, x.text.size(), stdout);
                    std::fputc('\n', stdout);
                    if (x.length > x.text.size())
                        std::fprintf(stderr, "WARN match cut path=%s line=%llu offset=%llu length=%llu\n", path.c_str(), (unsigned long long)x.number,
                                     (unsigned long long)x.start, (unsigned long long)x.length);
                }
                const uint64_t shown = per_frame ? std::min<uint64_t>(r.lines, per_frame) : r.lines;
                if (lines_in[*f.digest] < shown)
                    std::fprintf(stderr, "WARN path=%s: the matches of %llu more matching lines not shown\n", path.c_str(), (unsigned long long)(shown - lines_in[*f.digest]));
                if (r.match_records.size() < r.matches)
                    std::fprintf(stderr, "WARN path=%s: %llu more matches not shown\n", path.c_str(), (unsigned long long)(r.matches - r.match_records.size()));
            }
            std::fprintf(stderr, "searched %llu files (%zu frames, %llu bytes), %llu match, %llu failed\n", n_files, order.size(), bytes, matched, failed);
            return failed ? 2 : (matched ? 0 : 1);
        }
        if (lines_mode) {
            // ---- lines mode: the matching lines of every distinct frame (zarc_gpu_search_lines_batch), printed per file in directory order.
            // -c and -l need no line: a counting call.  Otherwise one call brings back at most --batch-lines lines; frames behind the one
            // at which they ran out are searched again in a following call, and a frame that is first in its call and still has more
            // than fit prints what it got and says so.
            // With -v / -A / -B / -C the lines are the selected ones (zarc_gpu_select_lines_batch).  -m NUM then follows GNU grep: a file stops
            // after its NUM-th hit line, that line's trailing context is still printed, as context even where it matches -- so the device is
            // asked for NUM * (before + after + 1) lines, which hold all of that, and the rest is trimmed here by line number.
            const bool need_lines = !count_lines && !names_only;
            uint64_t per_frame = (uint64_t)max_per_file;
            if (sel.active() && max_per_file) {
                const uint64_t group = (uint64_t)sel.before + sel.after + 1;
                per_frame = (uint64_t)max_per_file > UINT64_MAX / group ? 0 : (uint64_t)max_per_file * group; // (saturates to "no limit")
            }
            std::map<zarc::Digest, zarc::FrameReader::Result> done;
            const size_t BATCH = (size_t)1 << 30;
            size_t at = 0;
            std::vector<zarc::Digest> todo = order;
            for (const zarc::Digest &d : order) bytes += rd.frames().at(d).uncompressed;
            while (at < todo.size()) {
                std::vector<zarc::Digest> batch;
                for (size_t batch_bytes = 0; at + batch.size() < todo.size() && batch_bytes < BATCH; batch_bytes += (size_t)rd.frames().at(batch.back()).uncompressed)
                    batch.push_back(todo[at + batch.size()]);
                std::vector<zarc::FrameReader::Result> res =
                    use_set ? rd.search_set_lines(batch, set, icase, per_frame, (uint64_t)max_line, need_lines ? (size_t)batch_lines : 0, nullptr, sel)
                    : ere   ? rd.search_regex_lines(batch, pattern, icase, per_frame, (uint64_t)max_line, need_lines ? (size_t)batch_lines : 0, sel)
                            : rd.search_lines(batch, pattern, icase, per_frame, (uint64_t)max_line, need_lines ? (size_t)batch_lines : 0, sel);
                LOGF(3, "search_lines", "frames=%zu", batch.size());
                size_t taken = batch.size();
                for (size_t k = 0; k < batch.size(); k++) {
                    const uint64_t want = need_lines ? (per_frame ? std::min<uint64_t>(res[k].selected, per_frame) : res[k].selected) : 0;
                    if (k > 0 && res[k].line_records.size() < want) { taken = k; break; } // the call's records ran out here: this frame and the rest again
                    done[batch[k]] = std::move(res[k]);
                }
                at += taken;
            }
            const bool groups = sel.before || sel.after; // grep prints `--` between groups of lines that are not adjacent
            bool printed = false;
            for (size_t i = 0; i < rd.files().size(); i++) {
                const zarc::File &f = rd.files()[i];
                if (!f.is_normal() || !passes(filters, to_path(f.name)) || !done.count(*f.digest)) continue;
                const zarc::FrameReader::Result &r = done.at(*f.digest);
                const std::string path = to_path(f.name);
                const bool decoded = r.status == ZARC_GPU_FRAME_OK || r.status == ZARC_GPU_FRAME_DIGEST;
                if (!(decoded && r.verify.value_or(false))) {
                    if (decoded) std::fprintf(stderr, "ERROR frame verification failed! path=%s\n", path.c_str());
                    else std::fprintf(stderr, "ERROR %s path=%s\n", zarc_gpu_frame_status_name(r.status), path.c_str());
                    failed++;
                    continue;
                }
                if (!r.lines) continue;
                matched++;
                const uint64_t shown = max_per_file ? std::min<uint64_t>(r.lines, (uint64_t)max_per_file) : r.lines;
                if (names_only) { std::printf("%s\n", path.c_str()); continue; }
                if (count_lines) { std::printf("%s:%llu\n", path.c_str(), (unsigned long long)shown); continue; }
                bool binary = false;
                if (!as_text) for (const auto &l : r.line_records) binary = binary || std::memchr(l.text.data(), 0, l.text.size()) != nullptr;
                if (binary) { std::printf("Binary file %s matches\n", path.c_str()); continue; }
                uint64_t hits_seen = 0, stop_behind = UINT64_MAX, last_number = UINT64_MAX - 1; // (a file's first line opens a new group)
                for (const auto &l : r.line_records) {
                    if (l.number > stop_behind) break; // -m with context: behind the last hit line's trailing context
                    const bool stopped = stop_behind != UINT64_MAX;
                    const bool hit = !stopped && (l.match != ZARC_GPU_SEARCH_NONE) != sel.invert;
                    if (groups && printed && l.number != last_number + 1) std::printf("--\n");
                    const char sep = hit ? ':' : '-';
                    std::printf("%s%c", path.c_str(), sep);
                    if (numbers) std::printf("%llu%c", (unsigned long long)l.number, sep);
                    if (with_offset) std::printf("%llu%c", (unsigned long long)l.start, sep);
                    std::fwrite(l.text.data(), 1, l.text.size(), stdout);
                    std::fputc('\n', stdout);
                    printed = true; last_number = l.number;
                    if (l.length > l.text.size())
                        std::fprintf(stderr, "WARN line cut path=%s line=%llu length=%llu\n", path.c_str(), (unsigned long long)l.number, (unsigned long long)l.length);
                    if (hit && sel.active() && max_per_file && ++hits_seen == (uint64_t)max_per_file) stop_behind = l.number + sel.after;
                }
                const uint64_t expected = sel.active() ? (per_frame ? std::min<uint64_t>(r.selected, per_frame) : r.selected) : shown;
                if (r.line_records.size() < expected)
                    std::fprintf(stderr, "WARN path=%s: %llu more matching lines not shown\n", path.c_str(), (unsigned long long)(expected - r.line_records.size()));
            }
            std::fprintf(stderr, "searched %llu files (%zu frames, %llu bytes), %llu match, %llu failed\n", n_files, order.size(), bytes, matched, failed);
            return failed ? 2 : (matched ? 0 : 1);
        }
        // results by file index, printed in directory order once every batch is through
        struct Hit { uint64_t count; uint64_t first; };
        std::map<size_t, Hit> hits;
        const size_t BATCH = (size_t)1 << 30;
        std::vector<zarc::Digest> batch;
        size_t batch_bytes = 0;
        std::vector<uint64_t> set_hits(set.size(), 0); // --tally: per pattern of the set, over every batch
        auto flush = [&]() {
            if (batch.empty()) return;
            std::vector<uint64_t> batch_hits;
            const std::vector<zarc::FrameReader::Result> res = use_set ? rd.search_set(batch, set, icase, tally ? &batch_hits : nullptr)
                                                                : ere ? rd.search_regex(batch, pattern, icase) : rd.search_frames(batch, pattern, icase);
            for (size_t k = 0; k < batch_hits.size(); k++) set_hits[k] += batch_hits[k];
            for (size_t k = 0; k < batch.size(); k++) {
                const bool decoded = res[k].status == ZARC_GPU_FRAME_OK || res[k].status == ZARC_GPU_FRAME_DIGEST;
                for (size_t i : files_of[batch[k]]) {
                    const std::string path = to_path(rd.files()[i].name);
                    if (decoded && res[k].verify.value_or(false)) { if (res[k].count) hits[i] = Hit{res[k].count, res[k].first.value_or(0)}; continue; }
                    if (decoded) std::fprintf(stderr, "ERROR frame verification failed! path=%s\n", path.c_str()); // verify's wording
                    else std::fprintf(stderr, "ERROR %s path=%s\n", zarc_gpu_frame_status_name(res[k].status), path.c_str());
                    failed++;
                }
            }
            LOGF(3, "search_frames", "frames=%zu bytes=%zu", batch.size(), batch_bytes);
            batch.clear();
            batch_bytes = 0;
        };
        for (const zarc::Digest &d : order) {
            const uint64_t u = rd.frames().at(d).uncompressed;
            batch.push_back(d);
            batch_bytes += (size_t)u;
            bytes += u;
            if (batch_bytes >= BATCH) flush();
        }
        flush();
        if (tally) {
            for (size_t k = 0; k < typed.size(); k++) std::printf("%llu\t%s\n", (unsigned long long)set_hits[slot_of[k]], typed[k].c_str());
            matched = hits.size();
            hits.clear();
        }
        for (const auto &kv : hits) {
            const std::string path = to_path(rd.files()[kv.first].name);
            if (names_only) std::printf("%s\n", path.c_str());
            else if (with_offset) std::printf("%s:%llu:%llu\n", path.c_str(), (unsigned long long)kv.second.count, (unsigned long long)kv.second.first);
            else std::printf("%s:%llu\n", path.c_str(), (unsigned long long)kv.second.count);
            matched++;
        }
        std::fprintf(stderr, "searched %llu files (%zu frames, %llu bytes), %llu match, %llu failed\n", n_files, order.size(), bytes, matched, failed);
        return failed ? 2 : (matched ? 0 : 1);
    } catch (const zarc::Error &e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 2;
    }
}

// `zarc repack`: one archive into another.  The content frames are decoded, judged and encoded again on the device
// (zarc_gpu_repack_batch through ArchiveWriter::repack_from): no file is created but the output, no content crosses PCIe raw, and the
// directory -- owners, times, links, attributes, whatever this file system could not hold -- is carried over as it is.
int cmd_repack(const std::vector<std::string> &a)
{
    std::string input, output, verify;
    EncoderFlags flags;
    bool keep_smaller = false;
    int gpus = 1;
    for (size_t i = 0; i < a.size(); i++) {
        if (const int r = flags.parse(a, i)) { if (r < 0) return 2; }
        else if (a[i] == "--output" && i + 1 < a.size()) output = a[++i];
        else if (a[i] == "--verify" && i + 1 < a.size()) verify = a[++i];
        else if (a[i] == "--gpus" && i + 1 < a.size()) gpus = std::atoi(a[++i].c_str());
        else if (a[i] == "--keep-smaller") keep_smaller = true;
        else if (!a[i].empty() && a[i][0] == '-') return usage();
        else input = a[i];
    }
    if (input.empty() || output.empty() || gpus < 1 || gpus > 64) return usage();
    if (gpus > zarc_gpu_device_count()) { std::fprintf(stderr, "Error: --gpus %d but %d device(s) are usable\n", gpus, zarc_gpu_device_count()); return 1; }
    Mapped m(input);
    std::vector<int> devices;
    for (int d = 0; d < gpus; d++) devices.push_back(d);
    zarc::ArchiveReader rd(m.p, m.n, devices);
    const std::string in_digest = base64(rd.trailer().digest.bytes.data(), 32);
    if (!verify.empty() && verify != in_digest) { std::fprintf(stderr, "Error: integrity failure: zarc file digest is %s\n", in_digest.c_str()); return 1; }
    // written beside --output under a temporary name and renamed at the end: a run that fails leaves no file there
    const std::string tmp = output + ".tmp." + std::to_string((long)getpid());
    struct Temp { std::string path; bool keep = false; ~Temp() { if (!keep) (void)unlink(path.c_str()); } } temp{tmp};
    zarc::RepackReport rep;
    zarc::Digest digest;
    {
        std::ofstream file(tmp, std::ios::binary | std::ios::trunc);
        if (!file) { std::fprintf(stderr, "Error: %s: %s\n", tmp.c_str(), std::strerror(errno)); temp.keep = true; return 1; }
        zarc::ArchiveWriter enc(file, devices);
        flags.apply(enc);
        rep = enc.repack_from(rd, keep_smaller);
        LOGF(2, "repacked", "frames=%zu kept=%zu devices=%d", rep.frames, rep.kept, gpus);
        if (rep.bad.empty()) {
            // the edition is carried over like the rest of the directory (editions are not repack's to make): the same input and flags
            // give the same file, whenever and on however many devices
            timespec now;
            clock_gettime(CLOCK_REALTIME, &now);
            digest = enc.finalise(rd.editions().empty() ? zarc::Timestamp{(int64_t)now.tv_sec, (uint32_t)now.tv_nsec} : rd.editions()[0].written_at);
        }
    }
    if (!rep.bad.empty()) { // every bad frame with its digest and the files that use it; the output is given up
        for (const auto &b : rep.bad) {
            const std::string d64 = base64(b.digest.bytes.data(), 32);
            const char *why = b.status == ZARC_GPU_FRAME_DIGEST ? "frame verification failed!" : zarc_gpu_frame_status_name(b.status);
            size_t users = 0;
            for (const zarc::File &f : rd.files())
                if (f.digest && *f.digest == b.digest) { std::fprintf(stderr, "ERROR %s digest=%s path=%s\n", why, d64.c_str(), to_path(f.name).c_str()); users++; }
            if (!users) std::fprintf(stderr, "ERROR %s digest=%s (no file uses this frame)\n", why, d64.c_str());
        }
        std::fprintf(stderr, "Error: %zu of %zu frames are not good: nothing was written to %s\n", rep.bad.size(), rep.frames, output.c_str());
        return 1;
    }
    if (rename(tmp.c_str(), output.c_str()) != 0) { std::fprintf(stderr, "Error: %s: %s\n", output.c_str(), std::strerror(errno)); return 1; }
    temp.keep = true;
    std::printf("digest: %s\n", base64(digest.bytes.data(), 32).c_str());
    std::fprintf(stderr, "repacked %zu frames (%llu -> %llu bytes), %zu kept\n", rep.frames, (unsigned long long)rep.old_bytes, (unsigned long long)rep.new_bytes, rep.kept);
    return 0;
}

int cmd_list_files(const std::vector<std::string> &a)
{
    std::string input;
    std::vector<std::regex> filters;
    bool only_files = false;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i] == "--filter" && i + 1 < a.size()) filters.emplace_back(a[++i]);
        else if (a[i] == "--only-files") only_files = true;
        else if (a[i] == "--decorate") {} // accepted; the reference decorates whether or not it is given (list_files.rs:50-56)
        else if (!a[i].empty() && a[i][0] == '-') return usage();
        else input = a[i];
    }
    if (input.empty()) return usage();
    Mapped m(input);
    zarc::ArchiveReader rd(m.p, m.n);
    for (const zarc::File &f : rd.files()) {
        if (only_files && f.special_kind) continue;
        const std::string name = to_path(f.name);
        if (!passes(filters, name)) continue;
        std::printf("%s%s\n", name.c_str(), f.is_dir() ? "/" : (f.is_symlink() ? "@" : (f.is_hardlink() ? "#" : "")));
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    // global flags come before the subcommand (args.rs:39-65): -v / -vv / --verbose (counted), --log-file [PATH]
    int verbosity = 0, i = 1;
    bool have_log_file = false;
    std::string log_file;
    for (; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--verbose") verbosity++;
        else if (a.size() >= 2 && a[0] == '-' && a[1] == 'v' && a.find_first_not_of('v', 1) == std::string::npos) verbosity += (int)a.size() - 1;
        else if (a.rfind("--log-file=", 0) == 0) { have_log_file = true; log_file = a.substr(11); }
        else if (a == "--log-file") {
            have_log_file = true;
            // num_args = 0..=1: a following word that is not a subcommand is the path
            if (i + 1 < argc) { const std::string n = argv[i + 1]; const bool verb = !n.empty() && (std::string("pack").rfind(n, 0) == 0 || std::string("unpack").rfind(n, 0) == 0 || std::string("list-files").rfind(n, 0) == 0 || std::string("verify").rfind(n, 0) == 0 || std::string("repack").rfind(n, 0) == 0 || std::string("grep").rfind(n, 0) == 0 || std::string("cat").rfind(n, 0) == 0 || std::string("wc").rfind(n, 0) == 0 || std::string("compare").rfind(n, 0) == 0); if (!verb && n[0] != '-') log_file = argv[++i]; }
        } else break;
    }
    if (i >= argc) return usage();
    g_log.init(verbosity, log_file, have_log_file);
    const std::string verb = argv[i];
    std::vector<std::string> rest(argv + i + 1, argv + argc);
    try {
        // `infer_subcommands = true` (args.rs:23): unambiguous prefixes select the subcommand
        if (!verb.empty() && std::string("pack").rfind(verb, 0) == 0) return cmd_pack(rest);
        if (!verb.empty() && std::string("unpack").rfind(verb, 0) == 0) return cmd_unpack(rest);
        if (!verb.empty() && std::string("list-files").rfind(verb, 0) == 0) return cmd_list_files(rest);
        if (!verb.empty() && std::string("verify").rfind(verb, 0) == 0) return cmd_verify(rest);
        if (!verb.empty() && std::string("repack").rfind(verb, 0) == 0) return cmd_repack(rest);
        if (!verb.empty() && std::string("grep").rfind(verb, 0) == 0) return cmd_grep(rest);
        if (!verb.empty() && std::string("cat").rfind(verb, 0) == 0) return cmd_cat(rest);
        if (!verb.empty() && std::string("wc").rfind(verb, 0) == 0) return cmd_wc(rest);
        if (!verb.empty() && std::string("compare").rfind(verb, 0) == 0) return cmd_compare(rest);
        return usage();
    } catch (const zarc::Error &e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    } catch (const std::regex_error &e) {
        std::fprintf(stderr, "error: invalid regex: %s\n", e.what());
        return 2;
    }
}
