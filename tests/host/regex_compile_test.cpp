// tests/host/regex_compile_test.cpp -- the regular-expression compiler (zarc_amd/csrc/zre_compile.h) on its own: no library, no GPU, no
// Python.  Usage: regex_compile_test FILE [-i]
// FILE holds one expression per line (raw bytes, the line feed is not part of it).  Per expression one line goes to stdout:
//     ok <states> <start> <accepting states>        or        E_PARAM <message>        or        E_UNSUPPORTED <message>
// A compiled table is checked for what the kernels rely on (every entry below `states`, the 0x0A column, no accept bit on `start`); a
// violation is reported as BROKEN and the exit status is 1.
#include <cstdio>
#include <string>
#include <vector>

#include "zre_compile.h"

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s FILE [-i]\n", argv[0]); return 2; }
    const unsigned flags = argc > 2 && std::string(argv[2]) == "-i" ? ZARC_GPU_SEARCH_ICASE : 0;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<std::string> lines(1);
    for (int c; (c = fgetc(f)) != EOF;) { if (c == '\n') lines.emplace_back(); else lines.back().push_back((char)c); }
    fclose(f);
    if (lines.back().empty()) lines.pop_back();
    int broken = 0;
    for (const std::string &re : lines) {
        zarc_gpu_regex_dfa dfa;
        std::string err;
        const int rc = zre::compile(re.data(), re.size(), flags, &dfa, err);
        if (rc == ZARC_GPU_E_PARAM) { printf("E_PARAM %s\n", err.c_str()); continue; }
        if (rc == ZARC_GPU_E_UNSUPPORTED) { printf("E_UNSUPPORTED %s\n", err.c_str()); continue; }
        std::string err2;
        bool good = rc == 0 && dfa.states >= 1 && dfa.states <= ZARC_GPU_REGEX_MAX_STATES && dfa.start < dfa.states && dfa.accept[dfa.start] == 0 &&
                    zre::compile(re.data(), re.size(), flags, nullptr, err2) == 0; // (without a table as well)
        uint32_t accepting = 0;
        for (uint32_t q = 0; good && q < dfa.states; q++) {
            accepting += dfa.accept[q] != 0;
            good = dfa.accept[q] <= 3 && dfa.delta[q * 256 + 0x0A] == dfa.start;
            for (uint32_t b = 0; good && b < 256; b++) good = dfa.delta[q * 256 + b] < dfa.states;
        }
        if (!good) { printf("BROKEN rc %d\n", rc); broken = 1; continue; }
        printf("ok %u %u %u\n", dfa.states, dfa.start, accepting);
    }
    return broken;
}
