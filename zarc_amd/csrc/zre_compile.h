// zarc_amd/csrc/zre_compile.h -- the regular-expression compiler of zarc_gpu_search_regex_* (zarc_gpu_regex_compile).  Host code only: no
// HIP, no library; engine.hip includes it and so can a stand-alone program (tests/host/regex_compile_test.cpp).
//
//   regex text -> syntax tree -> position automaton of SIGMA* . reverse(R) -> subset construction -> minimisation -> byte table
//
// The table is a complete DFA that reads a LINE FROM ITS LAST BYTE TO ITS FIRST, because the question the kernels ask of every byte
// position p is "does a match START here": after the bytes of the line from its end down to p have been read, the state says whether some
// suffix-of-what-was-read, taken from p on, is in L(R).  SIGMA* in front (the line's tail that the match does not reach) makes every
// position a candidate at once; that is also why the state count is exponential in the worst case (.{k}a needs 2^(k+1) states).
//
// Anchors are LINE BOUNDARY symbols that no class matches: a line is read as  E  bytes, last to first  B, where only `$` reads E (the
// line's end) and only `^` reads B (its beginning).  Reversed, `$` sits in front and `^` behind.  The device never sees them:
//   start        the state after the E at a line's end (E applied until nothing changes, so that `x$$` is `x$`)
//   accept bit 0 a match starts at the byte just read
//   accept bit 1 a match starts at the byte just read IF it is the line's first byte (B, once or more, would lead to acceptance)
//   delta[q][0x0A] = start for every q: reading backward across a line feed resets the automaton by itself.  No class matches 0x0A and R
//   consumes at least one byte, so `start` has no accept bit and a 0x0A position is never marked.
// ZARC_GPU_SEARCH_ICASE is folded into the classes here (ASCII letters only); the content is never touched.
//
// compile(..., ends = true) makes the second table of the matches calls (zarc_gpu_regex_compile_ends) from the same position automaton: R
// alone, read FORWARDS from a match's first byte, stepped along the successors (pred transposed) from R's first positions, with one dead
// state.  It answers where the match that starts here ENDS; its layout is in include/zarc_gpu.h.
//
// Dialect, refusals and the offsets in the messages: include/zarc_gpu.h, the section of zarc_gpu_regex_compile.
#ifndef ZRE_COMPILE_H
#define ZRE_COMPILE_H
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "zarc_gpu.h"

namespace zre {

constexpr uint32_t MAX_POSITIONS = 2048; // symbol positions after counted repetitions are expanded
constexpr uint32_t MAX_SUBSET = 4096;    // states of the subset construction, before minimisation
constexpr uint32_t INF = 0xFFFFFFFFu;

struct ByteSet {
    uint64_t w[4] = {0, 0, 0, 0};
    void add(unsigned b) { w[b >> 6] |= 1ull << (b & 63); }
    void del(unsigned b) { w[b >> 6] &= ~(1ull << (b & 63)); }
    bool has(unsigned b) const { return (w[b >> 6] >> (b & 63) & 1) != 0; }
    void range(unsigned lo, unsigned hi) { for (unsigned b = lo; b <= hi; b++) add(b); }
    void join(const ByteSet &o) { for (int k = 0; k < 4; k++) w[k] |= o.w[k]; }
    void flip() { for (int k = 0; k < 4; k++) w[k] = ~w[k]; }
    void fold() // closed under ASCII case
    {
        for (unsigned c = 'a'; c <= 'z'; c++) {
            if (has(c)) add(c - 32);
            if (has(c - 32)) add(c);
        }
    }
};

enum Kind : uint8_t { EPS, SET, BOL, EOL, CAT, ALT, STAR, PLUS, OPT, REP };
struct Node {
    Kind kind = EPS;
    ByteSet set;          // SET
    int a = -1, b = -1;   // children
    uint32_t lo = 0, hi = 0; // REP: {lo,hi}, hi == INF: {lo,}
};

inline ByteSet class_of(unsigned c) // \d \w \s and, upper case, their complements
{
    ByteSet s;
    switch (c | 0x20) {
    case 'd': s.range('0', '9'); break;
    case 'w': s.range('0', '9'); s.range('A', 'Z'); s.range('a', 'z'); s.add('_'); break;
    default: s.add(' '); s.range(0x09, 0x0D); break; // 's'
    }
    if (!(c & 0x20)) s.flip();
    return s;
}

struct Parser {
    const uint8_t *s;
    size_t n, i = 0;
    bool icase;
    std::vector<Node> nodes;
    bool failed = false;
    size_t err_at = 0;
    std::string err;

    int fail(size_t at, const char *why)
    {
        if (!failed) { failed = true; err_at = at; err = why; }
        return -1;
    }
    int add(const Node &nd) { nodes.push_back(nd); return (int)nodes.size() - 1; }
    int leaf(ByteSet set)
    {
        set.del(0x0A);
        Node nd;
        nd.kind = SET; nd.set = set;
        return add(nd);
    }
    int unary(Kind k, int a, uint32_t lo = 0, uint32_t hi = 0)
    {
        Node nd;
        nd.kind = k; nd.a = a; nd.lo = lo; nd.hi = hi;
        return add(nd);
    }
    int binary(Kind k, int a, int b)
    {
        Node nd;
        nd.kind = k; nd.a = a; nd.b = b;
        return add(nd);
    }
    static int hex(unsigned c) { return c >= '0' && c <= '9' ? (int)c - '0' : (c | 0x20) >= 'a' && (c | 0x20) <= 'f' ? (int)(c | 0x20) - 'a' + 10 : -1; }

    // behind a backslash at `at`: -> one byte (single) or a class; false: refused
    bool escape(size_t at, ByteSet &out, bool &single, unsigned &byte)
    {
        if (i >= n) { fail(at, "a backslash at the end"); return false; }
        const unsigned c = s[i++];
        single = true;
        switch (c) {
        case 't': byte = 0x09; break;
        case 'r': byte = 0x0D; break;
        case 'f': byte = 0x0C; break;
        case 'v': byte = 0x0B; break;
        case '0':
            if (i < n && s[i] >= '0' && s[i] <= '9') { fail(at, "octal escapes are not supported"); return false; }
            byte = 0;
            break;
        case 'x': {
            const int h = i + 1 < n ? hex(s[i]) : -1, l = i + 1 < n ? hex(s[i + 1]) : -1;
            if (h < 0 || l < 0) { fail(at, "\\x needs two hexadecimal digits"); return false; }
            byte = (unsigned)(h * 16 + l);
            i += 2;
            break;
        }
        case 'd': case 'D': case 'w': case 'W': case 's': case 'S':
            single = false;
            out = class_of(c);
            return true;
        case 'n': fail(at, "a line feed never matches: matching is per line"); return false;
        default:
            if ((c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z')) {
                fail(at, "unsupported escape (no back-references, word boundaries or look-around)");
                return false;
            }
            byte = c; // punctuation and everything else: that byte
        }
        if (byte == 0x0A) { fail(at, "a line feed never matches: matching is per line"); return false; }
        out = ByteSet();
        out.add(byte);
        return true;
    }

    int bracket()
    {
        const size_t at = i++; // '['
        bool neg = false;
        if (i < n && s[i] == '^') { neg = true; i++; }
        ByteSet set;
        for (bool first = true;; first = false) {
            if (i >= n) return fail(at, "unbalanced [");
            if (s[i] == ']' && !first) { i++; break; }
            const size_t item_at = i;
            ByteSet one;
            bool single = true;
            unsigned lo = s[i];
            if (lo == '\\') { i++; if (!escape(item_at, one, single, lo)) return -1; }
            else if (lo == 0x0A) return fail(item_at, "a line feed never matches: matching is per line");
            else { i++; one.add(lo); }
            if (i + 1 < n && s[i] == '-' && s[i + 1] != ']') { // a range
                if (!single) return fail(item_at, "a class cannot start a range");
                i++;
                const size_t hi_at = i;
                ByteSet other;
                bool hi_single = true;
                unsigned hi = s[i];
                if (hi == '\\') { i++; if (!escape(hi_at, other, hi_single, hi)) return -1; }
                else if (hi == 0x0A) return fail(hi_at, "a line feed never matches: matching is per line");
                else i++;
                if (!hi_single) return fail(hi_at, "a class cannot end a range");
                if (hi < lo) return fail(item_at, "a range that runs backward");
                set.range(lo, hi);
            } else set.join(one);
        }
        if (icase) set.fold();
        if (neg) set.flip();
        return leaf(set);
    }

    // the bound behind a '{' at i; -> false: not a valid bound
    bool bound(uint32_t &lo, uint32_t &hi, const char *&why)
    {
        size_t j = i + 1;
        auto number = [&](uint32_t &v) {
            if (j >= n || s[j] < '0' || s[j] > '9') return false;
            uint64_t x = 0;
            while (j < n && s[j] >= '0' && s[j] <= '9') { x = x * 10 + (s[j] - '0'); if (x > 100000) x = 100000; j++; }
            v = (uint32_t)x;
            return true;
        };
        why = "{ that is not a valid bound";
        if (!number(lo)) return false; // ({,m} as well)
        hi = lo;
        if (j < n && s[j] == ',') {
            j++;
            if (j < n && s[j] == '}') hi = INF;
            else if (!number(hi)) return false;
        }
        if (j >= n || s[j] != '}') return false;
        if (hi != INF && hi < lo) { why = "a bound {n,m} with n above m"; return false; }
        if (lo > 255 || (hi != INF && hi > 255)) { why = "a bound above 255"; return false; }
        i = j + 1;
        return true;
    }

    int piece(int depth)
    {
        const size_t at = i;
        const unsigned c = s[i];
        int atom;
        bool anchor = false; // a bare ^ or $: nothing to repeat ((^)* is allowed, as in Python)
        switch (c) {
        case '(': {
            i++;
            atom = alt(depth + 1);
            if (failed) return -1;
            if (i >= n || s[i] != ')') return fail(at, "unbalanced (");
            i++;
            break;
        }
        case '*': case '+': case '?': return fail(at, "a quantifier with nothing to repeat");
        case '{': return fail(at, "{ with nothing to repeat (\\{ is the byte)");
        case '[': atom = bracket(); break;
        case '.': { i++; ByteSet all; all.flip(); atom = leaf(all); break; }
        case '^': i++; atom = unary(BOL, -1); anchor = true; break;
        case '$': i++; atom = unary(EOL, -1); anchor = true; break;
        case 0x0A: return fail(at, "a line feed never matches: matching is per line");
        case '\\': {
            i++;
            ByteSet set;
            bool single;
            unsigned byte = 0;
            if (!escape(at, set, single, byte)) return -1;
            if (icase && single) set.fold();
            atom = leaf(set);
            break;
        }
        default: {
            i++;
            ByteSet set;
            set.add(c);
            if (icase) set.fold();
            atom = leaf(set);
        }
        }
        if (failed) return -1;
        if (i < n && (s[i] == '*' || s[i] == '+' || s[i] == '?' || s[i] == '{')) {
            const size_t qat = i;
            if (anchor) return fail(qat, "a quantifier with nothing to repeat (an anchor)");
            if (s[i] == '{') {
                uint32_t lo, hi;
                const char *why;
                if (!bound(lo, hi, why)) return fail(qat, why);
                atom = unary(REP, atom, lo, hi);
            } else {
                atom = unary(s[i] == '*' ? STAR : s[i] == '+' ? PLUS : OPT, atom);
                i++;
            }
            if (i < n) {
                if (s[i] == '?') return fail(i, "lazy quantifiers are not supported");
                if (s[i] == '+') return fail(i, "possessive quantifiers are not supported");
                if (s[i] == '*' || s[i] == '{') return fail(i, "a quantifier on a quantifier");
            }
        }
        return atom;
    }
    int cat(int depth)
    {
        int left = -1;
        while (!failed && i < n && s[i] != '|' && s[i] != ')') {
            const int p = piece(depth);
            if (failed) return -1;
            left = left < 0 ? p : binary(CAT, left, p);
        }
        return left < 0 ? add(Node()) : left;
    }
    int alt(int depth)
    {
        if (depth > 256) return fail(i, "groups nested deeper than 256");
        int left = cat(depth);
        while (!failed && i < n && s[i] == '|') {
            i++;
            const int right = cat(depth);
            if (failed) return -1;
            left = binary(ALT, left, right);
        }
        return failed ? -1 : left;
    }
};

// can the tree match without a content byte (anchors count as empty)
inline bool nullable(const std::vector<Node> &t, int v)
{
    const Node &x = t[v];
    switch (x.kind) {
    case EPS: case BOL: case EOL: case STAR: case OPT: return true;
    case SET: return false;
    case CAT: return nullable(t, x.a) && nullable(t, x.b);
    case ALT: return nullable(t, x.a) || nullable(t, x.b);
    case PLUS: return nullable(t, x.a);
    default: return x.lo == 0 || nullable(t, x.a); // REP
    }
}
inline uint64_t positions_of(const std::vector<Node> &t, int v) // after expansion, saturating
{
    const Node &x = t[v];
    uint64_t r;
    switch (x.kind) {
    case EPS: return 0;
    case SET: case BOL: case EOL: return 1;
    case CAT: case ALT: r = positions_of(t, x.a) + positions_of(t, x.b); break;
    case REP: r = positions_of(t, x.a) * (x.hi == INF ? std::max(x.lo, 1u) : x.hi); break;
    default: r = positions_of(t, x.a);
    }
    return std::min<uint64_t>(r, 1u << 30);
}

// the position automaton (Glushkov) of the expanded tree: position 0 is the SIGMA* loop, 1 .. P the leaves
struct Glushkov {
    const std::vector<Node> &t;
    uint32_t P = 0, W = 0;
    std::vector<ByteSet> set;     // per position: the bytes it reads (anchors: none)
    std::vector<uint8_t> anchor;  // per position: 0, or the boundary symbol it reads (1: the line's beginning, 2: its end)
    std::vector<uint64_t> pred;   // per position: the positions that may come right in front of it (bitset rows of W words)
    struct Frag { bool nullable; std::vector<uint32_t> first, last; };

    explicit Glushkov(const std::vector<Node> &tree, uint32_t positions) : t(tree)
    {
        W = (positions + 1 + 63) / 64;
        set.resize(positions + 1);
        anchor.assign(positions + 1, 0);
        pred.assign((size_t)(positions + 1) * W, 0);
    }
    void link(const std::vector<uint32_t> &from, const std::vector<uint32_t> &to)
    {
        for (uint32_t q : to) for (uint32_t p : from) pred[(size_t)q * W + p / 64] |= 1ull << (p & 63);
    }
    static void join(std::vector<uint32_t> &a, const std::vector<uint32_t> &b) { a.insert(a.end(), b.begin(), b.end()); }
    Frag seq(Frag a, const Frag &b)
    {
        link(a.last, b.first);
        Frag r;
        r.nullable = a.nullable && b.nullable;
        r.first = a.first;
        if (a.nullable) join(r.first, b.first);
        r.last = b.last;
        if (b.nullable) join(r.last, a.last);
        return r;
    }
    Frag star(Frag a) { link(a.last, a.first); a.nullable = true; return a; }
    Frag build(int v)
    {
        const Node &x = t[v];
        Frag r;
        switch (x.kind) {
        case EPS: r.nullable = true; return r;
        case SET: case BOL: case EOL:
            P++;
            set[P] = x.set; anchor[P] = x.kind == BOL ? 1 : x.kind == EOL ? 2 : 0;
            r.nullable = false; r.first = {P}; r.last = {P};
            return r;
        case CAT: { Frag a = build(x.a); return seq(std::move(a), build(x.b)); }
        case ALT: {
            r = build(x.a);
            const Frag b = build(x.b);
            r.nullable = r.nullable || b.nullable;
            join(r.first, b.first); join(r.last, b.last);
            return r;
        }
        case STAR: return star(build(x.a));
        case PLUS: { r = build(x.a); link(r.last, r.first); return r; }
        case OPT: r = build(x.a); r.nullable = true; return r;
        default: { // REP: lo copies, then hi - lo optional ones nested (x(x(x)?)?)?; {n,}: the last of the copies loops
            r.nullable = true;
            if (x.hi == INF) {
                if (x.lo == 0) return star(build(x.a));
                for (uint32_t k = 0; k + 1 < x.lo; k++) r = seq(std::move(r), build(x.a));
                Frag loop = build(x.a);
                link(loop.last, loop.first);
                return seq(std::move(r), loop);
            }
            for (uint32_t k = 0; k < x.lo; k++) r = seq(std::move(r), build(x.a));
            if (x.hi > x.lo) {
                Frag tail;
                tail.nullable = true;
                std::vector<Frag> opt;
                for (uint32_t k = x.lo; k < x.hi; k++) opt.push_back(build(x.a));
                for (size_t k = opt.size(); k-- > 0;) { tail = seq(opt[k], tail); tail.nullable = true; }
                r = seq(std::move(r), tail);
            }
            return r;
        }
        }
    }
};

inline int refuse(int code, size_t at, const std::string &why, std::string &err)
{
    char head[64];
    snprintf(head, sizeof head, "regex: offset %zu: ", at);
    err = head + why;
    return code;
}

// -> 0, ZARC_GPU_E_PARAM or ZARC_GPU_E_UNSUPPORTED; out may be null.  ends: the FORWARD table of R alone (zarc_gpu_regex_compile_ends, see
// compile_ends below) in place of the backward table of SIGMA* . reverse(R); parsing, refusals and byte classes are the same.
inline int compile(const void *regex, size_t len, unsigned flags, zarc_gpu_regex_dfa *out, std::string &err, bool ends = false)
{
    err.clear();
    if (!regex || len == 0) return refuse(ZARC_GPU_E_PARAM, 0, "an empty expression", err);
    if (len > ZARC_GPU_REGEX_MAX_PATTERN) return refuse(ZARC_GPU_E_PARAM, ZARC_GPU_REGEX_MAX_PATTERN, "an expression has at most 1024 bytes", err);
    if (flags & ~(unsigned)ZARC_GPU_SEARCH_ICASE) return refuse(ZARC_GPU_E_PARAM, 0, "unknown flag", err);
    Parser ps;
    ps.s = (const uint8_t *)regex; ps.n = len; ps.icase = (flags & ZARC_GPU_SEARCH_ICASE) != 0;
    ps.nodes.reserve(2 * len + 2);
    const int root = ps.alt(0);
    if (!ps.failed && ps.i < len) ps.fail(ps.i, "unbalanced )");
    if (ps.failed) return refuse(ZARC_GPU_E_PARAM, ps.err_at, ps.err, err);
    if (nullable(ps.nodes, root)) return refuse(ZARC_GPU_E_PARAM, 0, "the expression can match without consuming a byte (it would match every line)", err);
    const uint64_t want = positions_of(ps.nodes, root);
    if (want > MAX_POSITIONS) {
        char msg[128];
        snprintf(msg, sizeof msg, "needs more than %u states (%llu symbol positions after the bounds are expanded); the limit is %d", MAX_POSITIONS,
                 (unsigned long long)want, ZARC_GPU_REGEX_MAX_STATES);
        return refuse(ZARC_GPU_E_UNSUPPORTED, 0, msg, err);
    }
    Glushkov g(ps.nodes, (uint32_t)want);
    const Glushkov::Frag whole = g.build(root);
    const uint32_t P = g.P, W = g.W;
    typedef std::vector<uint64_t> Bits;
    Bits first_r(W, 0), last_r(W, 0); // of R: where a match may begin / end
    for (uint32_t p : whole.first) first_r[p / 64] |= 1ull << (p & 63);
    for (uint32_t p : whole.last) last_r[p / 64] |= 1ull << (p & 63);

    // byte classes: bytes that every position treats alike
    uint8_t cls[256] = {0};
    uint32_t ncls = 1;
    for (uint32_t p = 1; p <= P; p++) {
        if (g.anchor[p]) continue;
        std::map<uint32_t, uint32_t> split;
        uint32_t next = 0;
        for (unsigned b = 0; b < 256; b++) {
            const uint32_t key = cls[b] * 2u + (g.set[p].has(b) ? 1u : 0u);
            auto it = split.find(key);
            if (it == split.end()) it = split.emplace(key, next++).first;
            cls[b] = (uint8_t)it->second; // (at most 256 classes)
        }
        ncls = next;
    }
    std::vector<Bits> reads(ncls + 2, Bits(W, 0)); // per class, and behind them the two boundary symbols: the positions that read it
    const uint32_t BEGIN = ncls, END = ncls + 1;
    for (unsigned b = 0; b < 256; b++) {
        bool seen = false;
        for (unsigned a = 0; a < b && !seen; a++) seen = cls[a] == cls[b];
        if (seen) continue;
        for (uint32_t p = 1; p <= P; p++) if (!g.anchor[p] && g.set[p].has(b)) reads[cls[b]][p / 64] |= 1ull << (p & 63);
    }
    for (uint32_t p = 1; p <= P; p++) if (g.anchor[p]) reads[g.anchor[p] == 1 ? BEGIN : END][p / 64] |= 1ull << (p & 63);

    // one step of SIGMA* . reverse(R): what was read last is p; next comes a position that R allows in front of p -- or, from the loop, one of
    // R's last positions -- provided it reads the symbol
    auto step = [&](const Bits &from, const Bits &sym) {
        Bits u = last_r;
        for (uint32_t k = 0; k < W; k++) {
            uint64_t bits = from[k];
            while (bits) {
                const uint32_t p = k * 64 + (uint32_t)__builtin_ctzll(bits);
                bits &= bits - 1;
                if (p == 0) continue;
                const uint64_t *row = &g.pred[(size_t)p * W];
                for (uint32_t j = 0; j < W; j++) u[j] |= row[j];
            }
        }
        for (uint32_t j = 0; j < W; j++) u[j] &= sym[j];
        u[0] |= 1; // the loop
        return u;
    };
    auto meets = [&](const Bits &a, const Bits &b) { for (uint32_t j = 0; j < W; j++) if (a[j] & b[j]) return true; return false; };
    Bits init(W, 0);
    init[0] = 1;
    Bits start = step(init, reads[END]);
    for (uint32_t k = 0; k <= P; k++) { // the line's end, once or more: the sets only grow
        Bits more = step(start, reads[END]);
        if (more == start) break;
        start = more;
    }
    auto accept_of = [&](const Bits &q) {
        uint8_t a = meets(q, first_r) ? 1 : 0;
        Bits b = step(q, reads[BEGIN]);
        for (uint32_t k = 0; k <= P; k++) {
            if (meets(b, first_r)) { a |= 2; break; }
            Bits more = step(b, reads[BEGIN]);
            if (more == b) break;
            b = more;
        }
        return a;
    };

    // The forward automaton of R alone: position 0 stands for "nothing read yet", a step goes along the successors (pred transposed) and
    // there is no loop, so the empty set is the dead state.  The boundary symbols are read where a line allows them: BEGIN, once or more,
    // in front of the line's first byte only (start_ls); END, once or more, behind its last only (accept bit 1).
    std::vector<uint64_t> succ;
    if (ends) {
        succ.assign((size_t)(P + 1) * W, 0);
        for (uint32_t q = 1; q <= P; q++)
            for (uint32_t p = 1; p <= P; p++)
                if (g.pred[(size_t)q * W + p / 64] >> (p & 63) & 1) succ[(size_t)p * W + q / 64] |= 1ull << (q & 63);
    }
    auto fstep = [&](const Bits &from, const Bits &sym) {
        Bits u(W, 0);
        for (uint32_t k = 0; k < W; k++) {
            uint64_t bits = from[k];
            while (bits) {
                const uint32_t p = k * 64 + (uint32_t)__builtin_ctzll(bits);
                bits &= bits - 1;
                const uint64_t *row = p ? &succ[(size_t)p * W] : first_r.data();
                for (uint32_t j = 0; j < W; j++) u[j] |= row[j];
            }
        }
        for (uint32_t j = 0; j < W; j++) u[j] &= sym[j];
        return u;
    };
    auto faccept_of = [&](const Bits &q) {
        uint8_t a = meets(q, last_r) ? 1 : 0;
        Bits b = fstep(q, reads[END]);
        for (uint32_t k = 0; k <= P; k++) { // (no loop: the sets need not grow, but a chain of anchors is at most P long)
            if (meets(b, last_r)) { a |= 2; break; }
            b = fstep(b, reads[END]);
        }
        return a;
    };
    Bits start_ls = init; // ends: the state in front of a line's first byte
    if (ends) {
        start = init;
        Bits b = init;
        for (uint32_t k = 0; k <= P; k++) {
            b = fstep(b, reads[BEGIN]);
            for (uint32_t j = 0; j < W; j++) start_ls[j] |= b[j];
        }
    }

    // subset construction from `start` over the byte classes
    std::map<Bits, uint32_t> ids;
    std::vector<Bits> states;
    std::vector<uint32_t> trans; // states x ncls
    std::vector<uint8_t> acc;
    ids.emplace(start, 0);
    states.push_back(start);
    uint32_t ls_id = 0, dead_id = 0;
    if (ends) { // the line-start state and the dead state are states whether or not a byte leads to them
        for (const Bits *b : {(const Bits *)&start_ls, (const Bits *)nullptr}) {
            const Bits s = b ? *b : Bits(W, 0);
            auto it = ids.find(s);
            if (it == ids.end()) { it = ids.emplace(s, (uint32_t)states.size()).first; states.push_back(s); }
            (b ? ls_id : dead_id) = it->second;
        }
    }
    for (uint32_t q = 0; q < states.size(); q++) {
        acc.push_back(ends ? faccept_of(states[q]) : accept_of(states[q]));
        for (uint32_t c = 0; c < ncls; c++) {
            Bits to = ends ? fstep(states[q], reads[c]) : step(states[q], reads[c]);
            auto it = ids.find(to);
            if (it == ids.end()) {
                if (states.size() >= MAX_SUBSET) {
                    char msg[128];
                    snprintf(msg, sizeof msg, "needs more than %u states before minimisation; the limit is %d", MAX_SUBSET, ZARC_GPU_REGEX_MAX_STATES);
                    return refuse(ZARC_GPU_E_UNSUPPORTED, 0, msg, err);
                }
                it = ids.emplace(to, (uint32_t)states.size()).first;
                states.push_back(std::move(to));
            }
            trans.push_back(it->second);
        }
    }
    const uint32_t N = (uint32_t)states.size();
    acc[0] &= 0; // (R consumes a byte: nothing starts behind a line's end)

    // minimisation (Moore): refine by accept bits, then by the blocks the classes lead to.  The 0x0A column is the same for every state.
    std::vector<uint32_t> block(N);
    for (uint32_t q = 0; q < N; q++) block[q] = acc[q];
    uint32_t nblocks = 0;
    for (;;) {
        std::map<std::vector<uint32_t>, uint32_t> sig_ids;
        std::vector<uint32_t> next(N), sig(ncls + 1);
        for (uint32_t q = 0; q < N; q++) { // (states are visited from `start` on: block 0 is its block)
            sig[0] = block[q];
            for (uint32_t c = 0; c < ncls; c++) sig[c + 1] = block[trans[(size_t)q * ncls + c]];
            next[q] = sig_ids.emplace(sig, (uint32_t)sig_ids.size()).first->second;
        }
        const uint32_t count = (uint32_t)sig_ids.size();
        block.swap(next);
        if (count == nblocks) break;
        nblocks = count;
    }
    if (nblocks > ZARC_GPU_REGEX_MAX_STATES) {
        char msg[128];
        snprintf(msg, sizeof msg, "needs %u states; the limit is %d", nblocks, ZARC_GPU_REGEX_MAX_STATES);
        return refuse(ZARC_GPU_E_UNSUPPORTED, 0, msg, err);
    }
    if (ends && out) { // the dead state is the last one; the 0x0A column, which no walk reads, holds the line-start state at `start`
        const uint32_t dead = block[dead_id], last = nblocks - 1;
        auto name = [&](uint32_t b) { return b == dead ? last : b == last ? dead : b; };
        memset(out, 0, sizeof *out);
        out->states = nblocks;
        out->start = name(block[0]);
        for (uint32_t q = 0; q < N; q++) {
            const uint32_t b = name(block[q]);
            out->accept[b] = acc[q];
            for (unsigned c = 0; c < 256; c++) out->delta[b * 256 + c] = (uint8_t)name(block[trans[(size_t)q * ncls + cls[c]]]);
        }
        for (uint32_t b = 0; b < nblocks; b++) out->delta[b * 256 + 0x0A] = (uint8_t)last;
        out->delta[out->start * 256 + 0x0A] = (uint8_t)name(block[ls_id]);
        return 0;
    }
    if (out) {
        memset(out, 0, sizeof *out);
        out->states = nblocks;
        out->start = block[0];
        for (uint32_t q = 0; q < N; q++) {
            const uint32_t b = block[q];
            out->accept[b] = acc[q];
            for (unsigned c = 0; c < 256; c++) out->delta[b * 256 + c] = (uint8_t)block[trans[(size_t)q * ncls + cls[c]]];
            out->delta[b * 256 + 0x0A] = (uint8_t)block[0];
        }
    }
    return 0;
}

} // namespace zre
#endif
