// zarc_amd/csrc/zdec_matches.hip -- every MATCH of the matching lines (zarc_gpu_search_matches_batch*): grep's -o; included by zstd_decode.hip
// behind zdec_select.hip.
//
// The lines kernels say which lines hold a match and where the lowest one starts.  These say where every match of such a line starts and
// ENDS, as `grep -o` cuts them out: from c = the line's start, the lowest matching start position p >= c, its end E(p) -- the pattern's
// length, the longest pattern of a set that matches at p, the longest run from p inside the line that is in L(R) -- then c = E(p).  They run
// behind zarc_lines_emit* of a part, over that part's line records where they lie on the device (ZarcLineRec; they never leave it):
//
//   zarc_matches_count*  a LANE per line record walks its line and leaves the line's number of matches.  The regex twin first reads the line
//                        from its last byte to its first with the backward table (zre_compile.h) and stores the line's start bits -- bit j
//                        of the record's region: a match starts at the line's byte j -- then goes from start to start by ctz over those
//                        words and walks the FORWARD table (zarc_gpu_regex_compile_ends) from each to the dead state or the line's end,
//                        remembering the last accept.  Starts are never looked for with the forward table: behind the last match of a line
//                        every position would walk to the line's end.  Per line: length + the walks of its matches, dependent lookups.
//   zarc_matches_scan    exclusive sums over the part's records, one workgroup looping as zarc_lines_scan does: the bit regions' first
//                        words ((length + 31) / 32 words each), the matches in front of every line (and the total), text_off of the match
//                        records.
//   -- the host reads the sums and applies the record rule: the part's first `limit` matches get a record --
//   zarc_matches_emit*   the same walk (a regex: the forward half, reading the stored bits): one ZarcMatchRec per match below `limit`.
//   zarc_matches_gather  zarc_lines_gather over match records.
//
// A lane owns its record, its count and its bit region: no atomic anywhere, vector stores only.  Content is read in 16-byte steps from
// aligned addresses by the regex walks and as unaligned words by the fixed-string tests, never further than 15 bytes behind the line's end
// (inside the frame's content or the padding behind it that the other search kernels read) and never in front of the 16-byte step that
// holds the line's first byte (a frame starts aligned).
// LDS per workgroup: fixed 256 B; a set its image (at most 40 KiB, usually a few hundred bytes); regex count 2 x 16 KiB tables + 128 B of
// accept bytes (four workgroups a CU), regex emit 16 KiB + 64 B.
// Cost: one lane walks one line, so a frame that is one long line is walked serially; ordinary text is 256 lines a workgroup side by side.

constexpr uint64_t ZM_NONE = 0xFFFFFFFFFFFFFFFFull;

// a line record as its lane sees it
struct ZmLine {
    const uint8_t *f;  // the frame's first byte (16-byte aligned)
    uint32_t ls, le;   // the line [ls, le)
    uint32_t from;     // its lowest matching start position
};
__device__ __forceinline__ ZmLine zm_line(const ZarcLineRec &r, const uint8_t *__restrict__ dec_base, const uint64_t *__restrict__ dec_off)
{
    ZmLine L;
    L.f = dec_base + dec_off[r.frame];
    L.ls = (uint32_t)r.start; L.le = (uint32_t)(r.start + r.length); L.from = (uint32_t)r.match;
    return L;
}

// what a walk does with the matches it meets: count them, or write the records below `limit`
struct ZmCount {
    uint32_t n = 0;
    __device__ __forceinline__ void match(uint32_t, uint32_t, uint64_t) { n++; }
    __device__ __forceinline__ bool full() const { return false; }
};
struct ZmEmit {
    ZarcMatchRec *rec;
    uint64_t g, limit;        // the next match's index among the part's; the first one without a record
    uint64_t frame, number, line_start;
    uint32_t max_line;
    __device__ __forceinline__ void match(uint32_t p, uint32_t e, uint64_t which)
    {
        ZarcMatchRec r;
        r.frame = frame; r.start = p; r.length = e - p; r.number = number; r.line_start = line_start; r.which = which; r.text_off = 0;
        r.text_len = e - p < max_line ? e - p : max_line;
        rec[g++] = r;
    }
    __device__ __forceinline__ bool full() const { return g >= limit; }
};

// ---- a fixed string ----
// pat: the (folded) pattern in LDS, words; m its length.  Positions are tested as zarc_search_scan tests them: the first four bytes, then
// the rest a word a step.
template <class Sink> __device__ __forceinline__ void zm_walk_fixed(const ZmLine &L, const uint32_t *pat, uint32_t m, bool fold, Sink &out)
{
    if (L.le - L.ls < m) return;
    const uint32_t p4 = pat[0], mask4 = m >= 4 ? 0xFFFFFFFFu : (1u << (8 * m)) - 1u;
    const uint32_t tail = m & 3u, words = m / 4, tail_mask = (1u << (8 * tail)) - 1u;
    const uint32_t last = L.le - m; // the line's last start position
    for (uint32_t p = L.from; p <= last && !out.full();) {
        const uint8_t *t = L.f + p;
        uint32_t w = zd::load_u32(t);
        if (fold) w = search_fold4(w);
        bool same = ((w ^ p4) & mask4) == 0;
        for (uint32_t k = 1; k < words && same; k++) {
            w = zd::load_u32(t + 4 * k);
            if (fold) w = search_fold4(w);
            same = w == pat[k];
        }
        if (same && m > 4 && tail) {
            w = zd::load_u32(t + 4 * words);
            if (fold) w = search_fold4(w);
            same = ((w ^ pat[words]) & tail_mask) == 0;
        }
        if (same) { out.match(p, p + m, ZM_NONE); p += m; } else p++;
    }
}

__device__ __forceinline__ void zm_load_pattern(const uint8_t *__restrict__ pattern, uint32_t m, uint32_t *pat)
{
    const uint32_t tid = threadIdx.x;
    if (tid < ZARC_SEARCH_MAX_PATTERN / 4) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; k++) if (tid * 4 + k < m) w |= (uint32_t)pattern[tid * 4 + k] << (8 * k);
        pat[tid] = w;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) zarc_matches_count(uint64_t nrec, const ZarcLineRec *__restrict__ lrec, const uint8_t *__restrict__ dec_base,
                                                          const uint64_t *__restrict__ dec_off, const uint8_t *__restrict__ pattern, uint32_t m, uint32_t icase,
                                                          uint32_t *__restrict__ counts)
{
    __shared__ uint32_t pat[ZARC_SEARCH_MAX_PATTERN / 4];
    zm_load_pattern(pattern, m, pat);
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nrec || m == 0 || m > ZARC_SEARCH_MAX_PATTERN) return;
    ZmCount c;
    zm_walk_fixed(zm_line(lrec[k], dec_base, dec_off), pat, m, icase != 0, c);
    counts[k] = c.n;
}

__global__ void __launch_bounds__(256) zarc_matches_emit(uint64_t nrec, const ZarcLineRec *__restrict__ lrec, const uint8_t *__restrict__ dec_base,
                                                         const uint64_t *__restrict__ dec_off, const uint8_t *__restrict__ pattern, uint32_t m, uint32_t icase,
                                                         const uint64_t *__restrict__ prefix, uint64_t limit, uint32_t max_line, ZarcMatchRec *__restrict__ mrec)
{
    __shared__ uint32_t pat[ZARC_SEARCH_MAX_PATTERN / 4];
    zm_load_pattern(pattern, m, pat);
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nrec || m == 0 || m > ZARC_SEARCH_MAX_PATTERN || prefix[k] >= limit) return;
    const ZarcLineRec r = lrec[k];
    ZmEmit e;
    e.rec = mrec; e.g = prefix[k]; e.limit = limit; e.frame = r.frame; e.number = r.number; e.line_start = r.start; e.max_line = max_line;
    zm_walk_fixed(zm_line(r, dec_base, dec_off), pat, m, icase != 0, e);
}

// ---- a set ----
// The longest pattern that matches at p and ends inside the line, and the lowest index among the patterns of that length.  The length
// classes are walked downwards: every pattern of class 3 (4 bytes and more) is longer than any of the classes below.  -> its length, 0: none
__device__ __forceinline__ uint32_t zm_set_at(const ZarcSetDesc &sd, const uint32_t *img, const uint32_t *__restrict__ set, const uint8_t *t, uint32_t room, bool fold,
                                              uint32_t &which)
{
    uint32_t w0 = zd::load_u32(t);
    if (fold) w0 = search_fold4(w0);
    for (uint32_t c = 4; c-- > 0;) {
        if (!(sd.classes >> c & 1u) || room < c + 1) continue;
        const uint32_t key = c == 3 ? w0 : w0 & ((1u << (8 * (c + 1))) - 1u);
        const uint32_t h = key * ZARC_SET_HASH;
        const uint32_t bit = c == 0 ? key : h >> (32 - sd.flog[c]);
        if (!(img[sd.foff[c] + (bit >> 5)] >> (bit & 31u) & 1u)) continue;
        const uint32_t *tab = img + sd.toff[c];
        const uint32_t tmask = (1u << sd.tlog[c]) - 1u;
        uint32_t slot = h >> (32 - sd.tlog[c]), list = 0;
        for (;;) { // (the table is at most half full: an empty slot ends every probe)
            const uint32_t ref = tab[2 * slot + 1];
            if (ref == 0) break;
            if (tab[2 * slot] == key) { list = ref; break; }
            slot = (slot + 1) & tmask;
        }
        if (!list) continue;
        const uint32_t nl = set[list];
        uint32_t best = 0;
        for (uint32_t e = 0; e < nl; e++) { // (ascending indices: a longer pattern replaces, an equal one does not)
            const uint32_t id = set[list + 1 + e];
            const uint32_t at = set[sd.pat_off + 2 * id], len = set[sd.pat_off + 2 * id + 1];
            if (len > room || len <= best) continue;
            const uint32_t words = len / 4, tail = len & 3u;
            bool same = true;
            for (uint32_t k = 1; k < words && same; k++) {
                uint32_t w = zd::load_u32(t + 4 * k);
                if (fold) w = search_fold4(w);
                same = w == set[at + k];
            }
            if (same && len > 4 && tail) {
                uint32_t w = zd::load_u32(t + 4 * words);
                if (fold) w = search_fold4(w);
                same = ((w ^ set[at + words]) & ((1u << (8 * tail)) - 1u)) == 0;
            }
            if (same) { best = len; which = id; }
        }
        if (best) return best;
    }
    return 0;
}

template <class Sink> __device__ __forceinline__ void zm_walk_set(const ZmLine &L, const ZarcSetDesc &sd, const uint32_t *img, const uint32_t *__restrict__ set, bool fold,
                                                                  Sink &out)
{
    for (uint32_t p = L.from; p < L.le && !out.full();) {
        uint32_t which = 0;
        const uint32_t len = zm_set_at(sd, img, set, L.f + p, L.le - p, fold, which);
        if (len) { out.match(p, p + len, which); p += len; } else p++;
    }
}

__global__ void __launch_bounds__(256) zarc_matches_count_set(uint64_t nrec, const ZarcLineRec *__restrict__ lrec, const uint8_t *__restrict__ dec_base,
                                                              const uint64_t *__restrict__ dec_off, ZarcSetDesc sd, const uint32_t *__restrict__ set, uint32_t icase,
                                                              uint32_t *__restrict__ counts)
{
    HIP_DYNAMIC_SHARED(uint32_t, img)
    zset_load(sd, set, img);
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nrec || sd.count == 0 || sd.min_len == 0) return;
    ZmCount c;
    zm_walk_set(zm_line(lrec[k], dec_base, dec_off), sd, img, set, icase != 0, c);
    counts[k] = c.n;
}

__global__ void __launch_bounds__(256) zarc_matches_emit_set(uint64_t nrec, const ZarcLineRec *__restrict__ lrec, const uint8_t *__restrict__ dec_base,
                                                             const uint64_t *__restrict__ dec_off, ZarcSetDesc sd, const uint32_t *__restrict__ set, uint32_t icase,
                                                             const uint64_t *__restrict__ prefix, uint64_t limit, uint32_t max_line, ZarcMatchRec *__restrict__ mrec)
{
    HIP_DYNAMIC_SHARED(uint32_t, img)
    zset_load(sd, set, img);
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nrec || sd.count == 0 || sd.min_len == 0 || prefix[k] >= limit) return;
    const ZarcLineRec r = lrec[k];
    ZmEmit e;
    e.rec = mrec; e.g = prefix[k]; e.limit = limit; e.frame = r.frame; e.number = r.number; e.line_start = r.start; e.max_line = max_line;
    zm_walk_set(zm_line(r, dec_base, dec_off), sd, img, set, icase != 0, e);
}

// ---- a regular expression ----
// byte j (0 .. 15) of a 16-byte step
__device__ __forceinline__ uint32_t zm_byte(const uint4 &x, int j)
{
    const uint32_t w = j < 4 ? x.x : j < 8 ? x.y : j < 12 ? x.z : x.w;
    return (w >> (8 * (j & 3))) & 0xFFu;
}

// The line from its last byte to its first with the backward table: bit j of bits[] = a match starts at the line's byte j.  Words
// [0, (length + 31) / 32) are written, each once.
__device__ __forceinline__ void zm_regex_starts(const ZmLine &L, const uint8_t *delta, const uint8_t *accept, uint32_t start, uint32_t *__restrict__ bits)
{
    uint32_t q = start, cur = 0;
    const uint32_t k0 = L.ls / 16;
    for (uint32_t k = (L.le + 15) / 16; k-- > k0;) {
        const uint4 x = ((const uint4 *)L.f)[k];
#pragma unroll
        for (int j = 15; j >= 0; j--) {
            const uint32_t pos = 16 * k + (uint32_t)j;
            if (pos >= L.le || pos < L.ls) continue;
            q = delta[q * 256 + zm_byte(x, j)];
            const uint32_t ac = accept[q], rel = pos - L.ls;
            if ((ac & 1u) || ((ac & 2u) && rel == 0)) cur |= 1u << (rel & 31u);
            if ((rel & 31u) == 0) { bits[rel >> 5] = cur; cur = 0; }
        }
    }
}

// The forward table from p: -> the end of the longest match that starts at p, 0: none.  dead: the state at which a walk stops; the 0x0A
// column of `start` holds the state for a line's first byte.
__device__ __forceinline__ uint32_t zm_regex_end(const ZmLine &L, const uint8_t *fdelta, const uint8_t *faccept, uint32_t fstart, uint32_t dead, uint32_t p)
{
    uint32_t q = p == L.ls ? fdelta[fstart * 256 + 0x0A] : fstart, end = 0;
    for (uint32_t k = p / 16; 16 * k < L.le; k++) {
        const uint4 x = ((const uint4 *)L.f)[k];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t pos = 16 * k + (uint32_t)j;
            if (pos < p) continue;
            if (pos >= L.le) return end;
            q = fdelta[q * 256 + zm_byte(x, j)];
            if (q == dead) return end;
            const uint32_t ac = faccept[q];
            if ((ac & 1u) || ((ac & 2u) && pos + 1 == L.le)) end = pos + 1;
        }
    }
    return end;
}

template <class Sink> __device__ __forceinline__ void zm_walk_regex(const ZmLine &L, const uint8_t *fdelta, const uint8_t *faccept, uint32_t fstart, uint32_t dead,
                                                                    const uint32_t *bits, Sink &out)
{
    const uint32_t len = L.le - L.ls, nw = (len + 31) / 32;
    for (uint32_t c = L.from - L.ls; c < len && !out.full();) {
        uint32_t w = c >> 5, m = bits[w] & ~((1u << (c & 31u)) - 1u);
        while (!m && ++w < nw) m = bits[w];
        if (!m) return;
        const uint32_t p = L.ls + w * 32 + (uint32_t)zd::ctz32(m);
        const uint32_t e = zm_regex_end(L, fdelta, faccept, fstart, dead, p);
        if (e > p) { out.match(p, e, ZM_NONE); c = e - L.ls; } else c = p + 1 - L.ls; // (the two tables agree on where a match starts: e > p)
    }
}

// rows [0, states) of a table into LDS; the caller's barrier makes them visible
__device__ __forceinline__ void zm_load_dfa(const ZarcRegexDfa *__restrict__ dfa, uint64_t *delta, uint8_t *accept, uint32_t &states, uint32_t &start)
{
    states = zd::uniform(dfa->states);
    start = zd::uniform(dfa->start);
    if (states > ZARC_REGEX_MAX_STATES) states = ZARC_REGEX_MAX_STATES;
    if (states == 0) states = 1;
    if (start >= states) start = 0;
    const uint64_t *src = (const uint64_t *)dfa->delta;
    for (uint32_t k = threadIdx.x; k < states * 32; k += 256) delta[k] = src[k];
    if (threadIdx.x < ZARC_REGEX_MAX_STATES) accept[threadIdx.x] = dfa->accept[threadIdx.x];
}

// bit_off[k]: the first word of record k's start bits
__global__ void __launch_bounds__(256) zarc_matches_count_regex(uint64_t nrec, const ZarcLineRec *__restrict__ lrec, const uint8_t *__restrict__ dec_base,
                                                                const uint64_t *__restrict__ dec_off, const ZarcRegexDfa *__restrict__ dfa,
                                                                const ZarcRegexDfa *__restrict__ fdfa, const uint64_t *__restrict__ bit_off, uint32_t *bits,
                                                                uint32_t *__restrict__ counts)
{
    __shared__ uint64_t delta[ZARC_REGEX_MAX_STATES * 256 / 8], fdelta[ZARC_REGEX_MAX_STATES * 256 / 8];
    __shared__ uint8_t accept[ZARC_REGEX_MAX_STATES], faccept[ZARC_REGEX_MAX_STATES];
    uint32_t states, start, fstates, fstart;
    zm_load_dfa(dfa, delta, accept, states, start);
    zm_load_dfa(fdfa, fdelta, faccept, fstates, fstart);
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nrec) return;
    const ZmLine L = zm_line(lrec[k], dec_base, dec_off);
    uint32_t *mine = bits + bit_off[k];
    zm_regex_starts(L, (const uint8_t *)delta, accept, start, mine);
    ZmCount c;
    zm_walk_regex(L, (const uint8_t *)fdelta, faccept, fstart, fstates - 1, mine, c);
    counts[k] = c.n;
}

__global__ void __launch_bounds__(256) zarc_matches_emit_regex(uint64_t nrec, const ZarcLineRec *__restrict__ lrec, const uint8_t *__restrict__ dec_base,
                                                               const uint64_t *__restrict__ dec_off, const ZarcRegexDfa *__restrict__ fdfa,
                                                               const uint64_t *__restrict__ bit_off, const uint32_t *__restrict__ bits,
                                                               const uint64_t *__restrict__ prefix, uint64_t limit, uint32_t max_line, ZarcMatchRec *__restrict__ mrec)
{
    __shared__ uint64_t fdelta[ZARC_REGEX_MAX_STATES * 256 / 8];
    __shared__ uint8_t faccept[ZARC_REGEX_MAX_STATES];
    uint32_t fstates, fstart;
    zm_load_dfa(fdfa, fdelta, faccept, fstates, fstart);
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nrec || prefix[k] >= limit) return;
    const ZarcLineRec r = lrec[k];
    ZmEmit e;
    e.rec = mrec; e.g = prefix[k]; e.limit = limit; e.frame = r.frame; e.number = r.number; e.line_start = r.start; e.max_line = max_line;
    zm_walk_regex(zm_line(r, dec_base, dec_off), (const uint8_t *)fdelta, faccept, fstart, fstates - 1, bits + bit_off[k], e);
}

// ---- the sums ----
// One workgroup, looping.  what 0: out[k] = the words of the start bits in front of record k's, out[nrec] = all of them (lrec);
// 1: out[k] = the matches in front of line k, out[nrec] = all of them (counts); 2: mrec[k].text_off = the running sum of text_len,
// out[0] = the sum.
__global__ void __launch_bounds__(256) zarc_matches_scan(uint32_t what, uint64_t nrec, const ZarcLineRec *__restrict__ lrec, const uint32_t *__restrict__ counts,
                                                         ZarcMatchRec *__restrict__ mrec, uint64_t *__restrict__ out)
{
    __shared__ uint32_t red[4];
    uint64_t run = 0;
    for (uint64_t base = 0; base < nrec; base += 256) {
        const uint64_t k = base + threadIdx.x;
        uint32_t v = 0; // (any 32-bit value: a round's 256 of them are summed in halves of 16 bits)
        if (k < nrec) v = what == 0 ? (uint32_t)((lrec[k].length + 31) / 32) : what == 1 ? counts[k] : (uint32_t)mrec[k].text_len;
        uint32_t all_lo, all_hi;
        const uint32_t ex_lo = lines_block_excl(v & 0xFFFFu, red, all_lo), ex_hi = lines_block_excl(v >> 16, red, all_hi);
        const uint64_t ex = ex_lo + ((uint64_t)ex_hi << 16);
        if (k < nrec) { if (what == 2) mrec[k].text_off = run + ex; else out[k] = run + ex; }
        run += all_lo + ((uint64_t)all_hi << 16);
    }
    if (threadIdx.x == 0) out[what == 2 ? 0 : nrec] = run;
}

// one wave per record: text_len bytes from the match's start to text + text_off, 16 bytes a lane where the destination is aligned
__global__ void __launch_bounds__(256) zarc_matches_gather(uint64_t nrec, const ZarcMatchRec *__restrict__ rec, const uint8_t *__restrict__ dec_base,
                                                           const uint64_t *__restrict__ dec_off, uint8_t *__restrict__ text)
{
    const uint64_t k = (uint64_t)blockIdx.x * 4 + (uint32_t)zd::wave_id();
    if (k >= nrec) return;
    const uint32_t lane = (uint32_t)zd::lane_id();
    const uint8_t *s = dec_base + dec_off[rec[k].frame] + rec[k].start;
    uint8_t *d = text + rec[k].text_off;
    const uint32_t L = (uint32_t)rec[k].text_len;
    uint32_t head = (uint32_t)((16 - ((uintptr_t)d & 15)) & 15);
    if (head > L) head = L;
    if (lane < head) d[lane] = s[lane];
    const uint32_t body = (L - head) / 16;
    for (uint32_t v = lane; v < body; v += 64) {
        const uint8_t *p = s + head + 16 * v;
        const uint64_t lo = zd::load_u64(p), hi = zd::load_u64(p + 8);
        *(uint4 *)(d + head + 16 * v) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    }
    const uint32_t done = head + 16 * body;
    if (lane < L - done) d[done + lane] = s[done + lane];
}
