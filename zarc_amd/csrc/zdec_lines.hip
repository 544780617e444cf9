// zarc_amd/csrc/zdec_lines.hip -- the matching LINES of a search (zarc_gpu_search_lines_batch*); included by zstd_decode.hip.
//
// zarc_search_scan says how often a byte string occurs in a frame.  These kernels say in which lines: a line is a maximal run of bytes
// without 0x0A, its number is 1 + the 0x0A bytes in front of it, it matches when a matching start position lies in it (the pattern holds
// no 0x0A, so a match never spans two lines).  They run behind the search kernel of a part, over the same decoded bytes in scratch:
//
//   zarc_lines_mark    workgroup per (frame, 64 KiB slice), the grid of zarc_search_scan.  The filter and verification of that kernel,
//                      restated (its code path stays as it is), give two bitmaps of the slice in LDS -- match starts, 0x0A positions,
//                      2 x 8 KiB -- and from them one ZarcLineSlice summary.
//   zarc_lines_carry   wave per frame, 64 slices a step: what a slice must know of the slices in front of it (is the line open at its
//                      start a matching line already, where did that line start, how many 0x0A and matching lines came before) and
//                      behind it (where the line open at its end ends), and lines[i].  A frame of one slice is finished by mark.
//   -- the host reads lines[] with the statuses and decides what every frame delivers (record base, number of records) --
//   zarc_lines_emit    the grid again, but only slices that deliver something rebuild their bitmaps (cheaper than 16 KiB of HBM traffic
//                      per 64 KiB slice for bitmaps nearly nobody reads): one ZarcLineRec per delivered line.
//   zarc_lines_scan    exclusive sum of text_len over the part's records (one workgroup, looping).
//   zarc_lines_gather  wave per record: the line's first text_len bytes into the compact text buffer.
//
// Inside a slice a thread owns 256 consecutive positions (8 words of either bitmap) and walks them segment by segment; what a thread
// must know of the threads in front of it comes from ballots and wave scans, never from one lane walking the slice.
// Frames are under 4 GiB: positions, line numbers and counts are 32-bit words.  Reads stay inside the frame's content plus the padding
// behind it (19 bytes at most, as in zarc_search_scan); the gather reads content only.

constexpr uint32_t ZL_NONE = 0xFFFFFFFFu;
constexpr uint32_t ZL_HEAD = 1u, ZL_TAIL = 2u, ZL_IN = 4u; // ZarcLineSlice::flags

// bit j = byte j of w is 0x0A (exact per byte: no borrow crosses a byte)
__device__ __forceinline__ uint32_t lines_nl4(uint32_t w)
{
    const uint32_t x = w ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); // bit 7 of every zero byte
    return (((z >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// the frame and slice of this workgroup (wave-uniform); false: not a workgroup of the grid
__device__ __forceinline__ bool lines_locate(uint32_t n, const uint64_t *__restrict__ slice_prefix, uint32_t &i, uint64_t &slice0)
{
    const uint64_t wg = blockIdx.x;
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (slice_prefix[mid] <= wg) lo = mid; else hi = mid;
    }
    i = lo;
    if (i >= n || wg >= slice_prefix[i + 1]) return false;
    slice0 = slice_prefix[i];
    return true;
}

// The two bitmaps of the slice at `a` (16-byte aligned): nbytes content bytes, of which the first cnt may start a match.  Words
// [0, 128 * steps) of both are written, steps = the 4 KiB rounds the slice needs (returned); every thread of the workgroup comes here.
__device__ __forceinline__ uint32_t lines_bitmaps(const uint8_t *__restrict__ a, uint32_t nbytes, uint32_t cnt, const uint8_t *__restrict__ pattern, uint32_t m,
                                                  bool fold, uint32_t *pat, uint32_t *bm_match, uint32_t *bm_nl)
{
    const uint32_t tid = threadIdx.x;
    if (tid < ZARC_SEARCH_MAX_PATTERN / 4) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; k++) if (tid * 4 + k < m) w |= (uint32_t)pattern[tid * 4 + k] << (8 * k);
        pat[tid] = w;
    }
    __syncthreads();
    const uint32_t p4 = zd::uniform(pat[0]);
    const uint32_t mask4 = m >= 4 ? 0xFFFFFFFFu : (1u << (8 * m)) - 1u;
    const uint32_t tail = m & 3u, words = m / 4;
    const uint32_t tail_mask = (1u << (8 * tail)) - 1u;
    const uint4 *a16 = (const uint4 *)a;
    const uint32_t n16 = (nbytes + 15) / 16, steps = (n16 + 255) / 256;
    for (uint32_t s = 0; s < steps; s++) { // (a uniform trip count: the pair exchange below needs the whole wave)
        const uint32_t v = tid + 256 * s, rel = v * 16;
        uint32_t hm = 0, nm = 0;
        if (v < n16) {
            const uint4 x = a16[v];
            uint32_t w0 = x.x, w1 = x.y, w2 = x.z, w3 = x.w;
            nm = lines_nl4(w0) | lines_nl4(w1) << 4 | lines_nl4(w2) << 8 | lines_nl4(w3) << 12;
            if (nbytes - rel < 16) nm &= (1u << (nbytes - rel)) - 1u; // the frame ends inside this step
            if (rel < cnt) {
                uint32_t w4 = ((const uint32_t *)(a16 + v + 1))[0];
                if (fold) { w0 = search_fold4(w0); w1 = search_fold4(w1); w2 = search_fold4(w2); w3 = search_fold4(w3); w4 = search_fold4(w4); }
                const uint64_t q0 = w0 | (uint64_t)w1 << 32, q1 = w1 | (uint64_t)w2 << 32, q2 = w2 | (uint64_t)w3 << 32, q3 = w3 | (uint64_t)w4 << 32;
                uint32_t hits = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    hits |= ((((uint32_t)(q0 >> (8 * j)) ^ p4) & mask4) == 0 ? 1u : 0u) << j;
                    hits |= ((((uint32_t)(q1 >> (8 * j)) ^ p4) & mask4) == 0 ? 1u : 0u) << (4 + j);
                    hits |= ((((uint32_t)(q2 >> (8 * j)) ^ p4) & mask4) == 0 ? 1u : 0u) << (8 + j);
                    hits |= ((((uint32_t)(q3 >> (8 * j)) ^ p4) & mask4) == 0 ? 1u : 0u) << (12 + j);
                }
                if (cnt - rel < 16) hits &= (1u << (cnt - rel)) - 1u;
                while (hits) { // the rest of the pattern, as zarc_search_scan looks at it
                    const uint32_t j = (uint32_t)zd::ctz32(hits);
                    hits &= hits - 1;
                    const uint8_t *t = a + rel + j;
                    bool same = true;
                    for (uint32_t k = 1; k < words && same; k++) {
                        uint32_t w = zd::load_u32(t + 4 * k);
                        if (fold) w = search_fold4(w);
                        same = w == pat[k];
                    }
                    if (same && m > 4 && tail) {
                        uint32_t w = zd::load_u32(t + 4 * words);
                        if (fold) w = search_fold4(w);
                        same = ((w ^ pat[words]) & tail_mask) == 0;
                    }
                    if (same) hm |= 1u << j;
                }
            }
        }
        // two neighbouring lanes hold the halves of one bitmap word: the even lane stores it (no LDS atomic anywhere)
        const uint32_t om = zd::shfl_xor(hm, 1), on = zd::shfl_xor(nm, 1);
        if (!(tid & 1u)) { bm_match[v >> 1] = hm | om << 16; bm_nl[v >> 1] = nm | on << 16; }
    }
    __syncthreads();
    return steps;
}

// A thread's 8 words of both bitmaps, segment by segment: f.low(p) at the lowest match of a segment, f.nl(p, has) at every 0x0A (has:
// the segment it ends held a match), f.end(has) behind the last word.  p counts from the chunk's first position.
template <class F> __device__ __forceinline__ void lines_walk(const uint32_t *mw, const uint32_t *nw, F &f)
{
    bool has = false;
    for (uint32_t k = 0; k < 8; k++) {
        uint32_t mm = mw[k], nn = nw[k];
        for (;;) {
            const uint32_t nb = nn ? (uint32_t)zd::ctz32(nn) : 32u;
            const uint32_t seg = nb < 32 ? mm & ((1u << nb) - 1u) : mm;
            if (seg && !has) { has = true; f.low(k * 32 + (uint32_t)zd::ctz32(seg)); }
            if (nb == 32) break;
            f.nl(k * 32 + nb, has);
            has = false;
            const uint32_t keep = nb == 31 ? 0u : ~((2u << nb) - 1u);
            mm &= keep; nn &= keep;
        }
    }
    f.end(has);
}

// what a thread's chunk looks like from outside
struct ZlChunk {
    uint32_t nls = 0, first = ZL_NONE, last = ZL_NONE; // its 0x0A bytes
    uint32_t inner = 0;                                 // segments that begin behind a 0x0A of the chunk and hold a match
    bool head = false, tail = false;                    // a match in front of its first / behind its last 0x0A (no 0x0A: anywhere)
    bool seen = false;
    __device__ __forceinline__ void low(uint32_t) {}
    __device__ __forceinline__ void nl(uint32_t p, bool has)
    {
        if (!seen) { head = has; first = p; seen = true; } else inner += has ? 1u : 0u;
        last = p; nls++;
    }
    __device__ __forceinline__ void end(bool has)
    {
        if (!seen) head = tail = has; else { tail = has; inner += has ? 1u : 0u; }
    }
};

__device__ __forceinline__ void lines_chunk(const uint32_t *mw, const uint32_t *nw, ZlChunk &c)
{
    uint32_t anym = 0;
    for (uint32_t k = 0; k < 8; k++) anym |= mw[k];
    if (anym) { lines_walk(mw, nw, c); return; }
    for (uint32_t k = 0; k < 8; k++) { // no match in the chunk (nearly every chunk): its 0x0A bytes by words
        if (!nw[k]) continue;
        if (!c.seen) { c.first = k * 32 + (uint32_t)zd::ctz32(nw[k]); c.seen = true; }
        c.last = k * 32 + (uint32_t)zd::hb32(nw[k]);
        c.nls += (uint32_t)__popc(nw[k]);
    }
}

// the words of thread tid's chunk; chunks behind the rounds that were written are empty
__device__ __forceinline__ void lines_load_chunk(const uint32_t *bm_match, const uint32_t *bm_nl, uint32_t steps, uint32_t *mw, uint32_t *nw)
{
    const uint32_t tid = threadIdx.x;
    const bool live = tid * 8 < steps * 128;
    for (uint32_t k = 0; k < 8; k++) { mw[k] = live ? bm_match[tid * 8 + k] : 0u; nw[k] = live ? bm_nl[tid * 8 + k] : 0u; }
}

// Every thread's chunk either ends a line (reset: it holds a 0x0A; val: a match behind its last one) or lengthens the open one (val: a
// match anywhere).  -> in: the line open at the thread's first position holds a match already, in front of the chunk (seed: in front of
// the slice); nl_before: a 0x0A of the slice lies in front of the chunk; out: `in` of a thread behind the last.  lds: 4 words.
struct ZlState { bool in, nl_before, out; };
__device__ __forceinline__ uint64_t lines_from_top(uint64_t bits) { return ~((1ull << (63 - __clzll((long long)bits))) - 1ull); } // the highest set bit and all above; bits != 0
__device__ __forceinline__ ZlState lines_state(bool reset, bool val, bool seed, uint32_t *lds)
{
    const uint32_t lane = (uint32_t)zd::lane_id(), wave = (uint32_t)zd::wave_id();
    const uint64_t R = zd::ballot(reset), V = zd::ballot(val);
    const uint64_t below = (1ull << lane) - 1ull, rb = R & below;
    const bool local_in = (V & (rb ? below & lines_from_top(rb) : below)) != 0;
    const bool wave_val = (V & (R ? lines_from_top(R) : ~0ull)) != 0;
    if (lane == 0) lds[wave] = (R ? 1u : 0u) | (wave_val ? 2u : 0u);
    __syncthreads();
    bool st = seed, nlb = false, out = seed;
    for (uint32_t w = 0; w < 4; w++) {
        if (w == wave) { st = out; }
        const uint32_t f = lds[w];
        if (f & 1u) { out = (f & 2u) != 0; if (w < wave) nlb = true; } else out = out || (f & 2u) != 0;
    }
    __syncthreads();
    ZlState r;
    r.in = rb ? local_in : (st || local_in);
    r.nl_before = nlb || rb != 0;
    r.out = out;
    return r;
}

// exclusive sum over the workgroup's 256 threads, and the total.  lds: 4 words.
__device__ __forceinline__ uint32_t lines_block_excl(uint32_t v, uint32_t *lds, uint32_t &total)
{
    const uint32_t incl = zd::wave_scan_incl(v);
    if (zd::lane_id() == 63) lds[zd::wave_id()] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (uint32_t w = 0; w < 4; w++) { if (w < (uint32_t)zd::wave_id()) base += lds[w]; all += lds[w]; }
    __syncthreads();
    total = all;
    return base + incl - v;
}
// exclusive maximum over the threads in front (0 in front of thread 0) ...
__device__ __forceinline__ uint32_t lines_block_max_before(uint32_t v, uint32_t *lds)
{
    const uint32_t lane = (uint32_t)zd::lane_id();
    uint32_t x = v;
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t t = zd::shfl_up(x, d); if (lane >= d && t > x) x = t; }
    if (lane == 63) lds[zd::wave_id()] = x;
    uint32_t e = zd::shfl_up(x, 1u);
    if (lane == 0) e = 0;
    __syncthreads();
    for (uint32_t w = 0; w < (uint32_t)zd::wave_id(); w++) e = lds[w] > e ? lds[w] : e;
    __syncthreads();
    return e;
}
// ... and exclusive minimum over the threads behind (ZL_NONE behind thread 255)
__device__ __forceinline__ uint32_t lines_block_min_after(uint32_t v, uint32_t *lds)
{
    const uint32_t lane = (uint32_t)zd::lane_id();
    uint32_t x = v;
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t t = zd::shfl_down(x, d); if (lane + d < 64 && t < x) x = t; }
    if (lane == 0) lds[zd::wave_id()] = x;
    uint32_t e = zd::shfl_down(x, 1u);
    if (lane == 63) e = ZL_NONE;
    __syncthreads();
    for (uint32_t w = (uint32_t)zd::wave_id() + 1; w < 4; w++) e = lds[w] < e ? lds[w] : e;
    __syncthreads();
    return e;
}

__global__ void __launch_bounds__(256) zarc_lines_mark(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                       const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                       const int32_t *__restrict__ status, const uint8_t *__restrict__ pattern, uint32_t m, uint32_t icase,
                                                       ZarcLineSlice *__restrict__ slices, uint32_t *__restrict__ lines)
{
    __shared__ uint32_t pat[ZARC_SEARCH_MAX_PATTERN / 4];
    __shared__ uint32_t bm_match[ZARC_CHECK_SLICE / 32], bm_nl[ZARC_CHECK_SLICE / 32];
    __shared__ uint32_t red[4];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const uint32_t tid = threadIdx.x;
    const bool single = slice_prefix[i + 1] - slice0 == 1;
    const int32_t st = status[i];
    const uint64_t len = raw_len[i];
    const uint64_t at = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    ZarcLineSlice S;
    S.nl_count = 0; S.first_nl = ZL_NONE; S.last_nl = ZL_NONE; S.nlow = 0; S.flags = 0; S.open_start = 0; S.nl_base = 0; S.excl = 0;
    S.next_end = (uint32_t)len; S.pad = 0;
    if ((st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) || m == 0 || m > ZARC_SEARCH_MAX_PATTERN || at >= len) { // nothing decoded, or an empty frame: no line
        if (tid == 0) { slices[blockIdx.x] = S; if (single) lines[i] = 0; }
        return;
    }
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    const uint64_t starts = len >= m && at <= len - m ? len - m + 1 - at : 0;
    const uint32_t cnt = (uint32_t)(starts > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : starts);
    const uint32_t steps = lines_bitmaps(dec_base + dec_off[i] + at, nbytes, cnt, pattern, m, icase != 0, pat, bm_match, bm_nl);
    uint32_t mw[8], nw[8];
    lines_load_chunk(bm_match, bm_nl, steps, mw, nw);
    ZlChunk c;
    lines_chunk(mw, nw, c);
    const ZlState s = lines_state(c.seen, c.seen ? c.tail : c.head, false, red);
    // a chunk's head segment is a line of its own when a 0x0A of the slice lies in front of it; otherwise it is part of the slice's head
    uint32_t total_low, total_nl;
    (void)lines_block_excl(c.inner + (c.head && !s.in && s.nl_before ? 1u : 0u), red, total_low);
    (void)lines_block_excl(c.nls, red, total_nl);
    const uint32_t first = lines_block_min_after(c.seen ? tid * 256 + c.first : ZL_NONE, red); // (thread 0 sees every other thread's ...
    const uint32_t last = lines_block_max_before(c.seen ? tid * 256 + c.last + 1 : 0u, red);   //  ... and thread 255 every other's)
    uint32_t heads;
    (void)lines_block_excl(c.head && !s.nl_before ? 1u : 0u, red, heads);
    const bool head_any = heads != 0;
    if (tid == 0) red[0] = c.seen ? c.first : first;
    if (tid == 255) red[1] = c.seen ? tid * 256 + c.last + 1 : last;
    __syncthreads();
    if (tid == 0) {
        S.nl_count = total_nl;
        S.first_nl = red[0];
        S.last_nl = red[1] ? red[1] - 1 : ZL_NONE;
        S.nlow = total_low;
        S.flags = (head_any ? ZL_HEAD : 0u) | (s.out ? ZL_TAIL : 0u);
        slices[blockIdx.x] = S;
        if (single) lines[i] = total_low + (head_any ? 1u : 0u);
    }
}

// one wave per frame (four frames a workgroup); frames of one slice were finished by zarc_lines_mark
__global__ void __launch_bounds__(256) zarc_lines_carry(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint64_t *__restrict__ raw_len,
                                                        ZarcLineSlice *__restrict__ slices, uint32_t *__restrict__ lines)
{
    const uint32_t i = blockIdx.x * 4 + (uint32_t)zd::wave_id(), lane = (uint32_t)zd::lane_id();
    if (i >= n) return;
    const uint64_t s0 = slice_prefix[i];
    const uint32_t ns = (uint32_t)(slice_prefix[i + 1] - s0);
    if (ns <= 1) return;
    ZarcLineSlice *S = slices + s0;
    const uint64_t below = (1ull << lane) - 1ull;
    bool c_in = false;
    uint32_t c_open = 0, c_nl = 0, c_lines = 0;
    for (uint32_t base = 0; base < ns; base += 64) { // forwards: what lies in front of a slice
        const uint32_t j = base + lane;
        const bool valid = j < ns;
        const uint32_t nlc = valid ? S[j].nl_count : 0u, fl = valid ? S[j].flags : 0u, nlow = valid ? S[j].nlow : 0u;
        const uint32_t end_of_last = valid && nlc ? j * ZARC_CHECK_SLICE + S[j].last_nl + 1 : 0u; // where the line open at the slice's end starts
        const bool reset = nlc != 0, val = reset ? (fl & ZL_TAIL) != 0 : (fl & ZL_HEAD) != 0;
        const uint64_t R = zd::ballot(reset), V = zd::ballot(val), rb = R & below;
        const bool in = rb ? (V & below & lines_from_top(rb)) != 0 : (c_in || (V & below) != 0);
        const uint32_t from = zd::shfl(end_of_last, rb ? 63 - __clzll((long long)rb) : 0);
        const uint32_t open = rb ? from : c_open;
        const uint32_t mine = nlow + ((fl & ZL_HEAD) && !in ? 1u : 0u);
        const uint32_t nl_incl = zd::wave_scan_incl(nlc), ln_incl = zd::wave_scan_incl(mine);
        if (valid) {
            S[j].flags = fl | (in ? ZL_IN : 0u);
            S[j].open_start = open;
            S[j].nl_base = c_nl + nl_incl - nlc;
            S[j].excl = c_lines + ln_incl - mine;
        }
        const uint32_t top = zd::shfl(end_of_last, R ? 63 - __clzll((long long)R) : 0);
        c_in = R ? (V & lines_from_top(R)) != 0 : (c_in || V != 0);
        c_open = R ? top : c_open;
        c_nl += zd::shfl(nl_incl, 63);
        c_lines += zd::shfl(ln_incl, 63);
    }
    uint32_t c_next = (uint32_t)raw_len[i];
    for (uint32_t base = (ns - 1) / 64 * 64;; base -= 64) { // backwards: where the line open at a slice's end ends
        const uint32_t j = base + lane;
        const bool valid = j < ns;
        const bool has = valid && S[j].nl_count != 0;
        const uint32_t first = has ? j * ZARC_CHECK_SLICE + S[j].first_nl : 0u;
        const uint64_t F = zd::ballot(has), above = lane == 63 ? 0ull : F & ~((2ull << lane) - 1ull);
        const uint32_t from = zd::shfl(first, above ? zd::ctz64(above) : 0);
        if (valid) S[j].next_end = above ? from : c_next;
        const uint32_t low = zd::shfl(first, F ? zd::ctz64(F) : 0);
        c_next = F ? low : c_next;
        if (base == 0) break;
    }
    if (lane == 0) lines[i] = c_lines;
}

// the records of a thread's chunk, as the walk meets them
struct ZlEmit {
    ZarcLineRec *rec;          // the frame's records
    uint32_t deliver, rank;    // how many of them there are; the rank of the chunk's next matching line
    uint32_t frame, at;        // the frame (decoder's order); the slice's first position
    uint32_t chunk0;           // the chunk's first position in the slice
    uint32_t open_start;       // where the line open at the chunk's first position starts
    uint32_t number;           // ... and its number
    uint32_t next_end;         // where the line open behind the chunk ends
    uint32_t max_line;
    bool in;                   // that first line holds a match in front of the chunk: no record for it here
    bool seen = false, pending = false;
    uint32_t p_start = 0, p_match = 0, p_number = 0, start = 0;
    __device__ __forceinline__ void put(uint32_t end)
    {
        if (rank < deliver) {
            ZarcLineRec r;
            r.frame = frame; r.start = p_start; r.length = end - p_start; r.number = p_number; r.match = p_match; r.text_off = 0;
            r.text_len = r.length < max_line ? r.length : max_line;
            rec[rank] = r;
        }
        rank++;
        pending = false;
    }
    __device__ __forceinline__ void low(uint32_t p)
    {
        if (!seen && in) return;
        pending = true;
        p_start = seen ? start : open_start; p_match = at + chunk0 + p; p_number = number;
    }
    __device__ __forceinline__ void nl(uint32_t p, bool)
    {
        if (pending) put(at + chunk0 + p);
        seen = true; start = at + chunk0 + p + 1; number++;
    }
    __device__ __forceinline__ void end(bool) { if (pending) put(next_end); }
};

__global__ void __launch_bounds__(256) zarc_lines_emit(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                       const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                       const uint8_t *__restrict__ pattern, uint32_t m, uint32_t icase,
                                                       const ZarcLineSlice *__restrict__ slices, const uint64_t *__restrict__ rec_base,
                                                       const uint32_t *__restrict__ deliver, uint32_t max_line, ZarcLineRec *__restrict__ rec)
{
    __shared__ uint32_t pat[ZARC_SEARCH_MAX_PATTERN / 4];
    __shared__ uint32_t bm_match[ZARC_CHECK_SLICE / 32], bm_nl[ZARC_CHECK_SLICE / 32];
    __shared__ uint32_t red[4];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const uint32_t want = deliver[i];
    const ZarcLineSlice S = slices[blockIdx.x];
    const bool seed = (S.flags & ZL_IN) != 0;
    if (S.excl >= want || S.nlow + ((S.flags & ZL_HEAD) && !seed ? 1u : 0u) == 0) return; // nothing of this slice is delivered (nearly every slice)
    const uint32_t tid = threadIdx.x;
    const uint64_t len = raw_len[i];
    const uint64_t at = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    const uint64_t starts = len >= m && at <= len - m ? len - m + 1 - at : 0;
    const uint32_t cnt = (uint32_t)(starts > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : starts);
    const uint32_t steps = lines_bitmaps(dec_base + dec_off[i] + at, nbytes, cnt, pattern, m, icase != 0, pat, bm_match, bm_nl);
    uint32_t mw[8], nw[8];
    lines_load_chunk(bm_match, bm_nl, steps, mw, nw);
    ZlChunk c;
    lines_chunk(mw, nw, c);
    const ZlState s = lines_state(c.seen, c.seen ? c.tail : c.head, seed, red);
    uint32_t total;
    const uint32_t rank = lines_block_excl(c.inner + (c.head && !s.in ? 1u : 0u), red, total);
    const uint32_t nl_before = lines_block_excl(c.nls, red, total);
    const uint32_t prev_end = lines_block_max_before(c.seen ? tid * 256 + c.last + 1 : 0u, red); // behind the last 0x0A in front of the chunk
    const uint32_t next_nl = lines_block_min_after(c.seen ? tid * 256 + c.first : ZL_NONE, red); // the first 0x0A behind the chunk
    if (c.inner + (c.head && !s.in ? 1u : 0u) == 0 || S.excl + rank >= want) return;
    ZlEmit e;
    e.rec = rec + rec_base[i]; e.deliver = want; e.rank = S.excl + rank; e.frame = i; e.at = (uint32_t)at; e.chunk0 = tid * 256;
    e.open_start = prev_end ? (uint32_t)at + prev_end : S.open_start;
    e.number = S.nl_base + nl_before + 1;
    e.next_end = next_nl != ZL_NONE ? (uint32_t)at + next_nl : S.next_end;
    e.max_line = max_line; e.in = s.in;
    lines_walk(mw, nw, e);
}

// text_off of the part's records: the running sum of text_len in record order; *total = the sum.  One workgroup.
__global__ void __launch_bounds__(256) zarc_lines_scan(uint64_t nrec, ZarcLineRec *__restrict__ rec, uint64_t *__restrict__ total)
{
    __shared__ uint32_t red[4];
    uint64_t run = 0;
    for (uint64_t base = 0; base < nrec; base += 256) {
        const uint64_t k = base + threadIdx.x;
        const uint32_t v = k < nrec ? (uint32_t)rec[k].text_len : 0u; // (at most 65536 each: a round's sum fits 32 bits)
        uint32_t all;
        const uint32_t ex = lines_block_excl(v, red, all);
        if (k < nrec) rec[k].text_off = run + ex;
        run += all;
    }
    if (threadIdx.x == 0) *total = run;
}

// one wave per record: text_len bytes from the line's start to text + text_off, 16 bytes a lane where the destination is aligned
__global__ void __launch_bounds__(256) zarc_lines_gather(uint64_t nrec, const ZarcLineRec *__restrict__ rec, const uint8_t *__restrict__ dec_base,
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
