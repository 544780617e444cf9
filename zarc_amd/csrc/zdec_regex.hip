// zarc_amd/csrc/zdec_regex.hip -- a REGULAR EXPRESSION matched over the decoded bytes (zarc_gpu_search_regex_*); included by zstd_decode.hip.
//
// The host compiles the expression (zre_compile.h) into a table that reads a line from its LAST byte to its first: the state behind byte
// p says whether a match starts at p (accept bit 0), or starts there if p is its line's first byte (bit 1).  delta[q][0x0A] is `start`
// for every q, so reading backward across a line feed restarts the automaton by itself.  These kernels fill the match-start bitmap of a
// slice from that table; everything behind the bitmap is zdec_lines.hip's, as it is.
//
// The grid, the 64 KiB slice, the 256 threads and a thread owning 256 consecutive positions (8 words of either bitmap) are those of the
// other search kernels.  What is new is that a thread does not know the state at its chunk's last byte before the bytes behind it have
// been read.  A chunk's TRANSITION FUNCTION maps the state in front of its last byte to the state behind its first:
//   - a chunk that holds a 0x0A has a CONSTANT function: one walk from its lowest 0x0A down, at most 256 steps (nearly every chunk of text);
//   - a chunk without one needs the table: `states` chains over its 256 bytes, four at a time, kept in LDS (256 threads x 64 bytes);
//   - a chunk behind the frame's end is the identity.
// A thread's entry state is then found by walking up to the nearest constant chunk (or the slice's entry state) and applying the tables
// in between: at most 255 LDS lookups, nearly always none.  Slices work the same way one level up:
//
//   zarc_regex_summary  the slice grid: one ZarcRegexSlice per slice of a frame of several slices -- constant and its value, or the
//                       slice's table, one lane per state chaining through the chunk tables.
//   zarc_regex_carry    a wave per frame, 64 slices a step from the frame's last slice (`start`) down: every slice's entry state.
//   zarc_regex_scan     regex_bitmaps, then the popcount and lowest bit into count[] and first[], as zarc_search_scan leaves them.
//   zarc_lines_mark_regex / zarc_lines_emit_regex   zarc_lines_mark / zarc_lines_emit with regex_bitmaps filling the bitmaps.
//
// LDS per workgroup: delta 16 KiB, chunk tables 16 KiB, the two bitmaps 16 KiB, under 1 KiB of small arrays: three workgroups per CU.
// Bitmap words are assembled in registers and stored by their owner: no LDS atomic anywhere.  A lane reads its 256 contiguous bytes with
// sixteen 16-byte loads, twice (once for the 0x0A bitmap and the chunk function, once with the entry state known; the second pass hits
// the cache).  The dependent delta lookup per byte is the critical path; the accept lookup hangs off it.
// Reads stay inside the frame's content plus the 15 bytes behind it that a 16-byte step of the other search kernels reads as well.

constexpr uint32_t ZRE_CONST = 0, ZRE_TABLE = 1, ZRE_IDENT = 2; // what a chunk's transition function is

struct ZreLds {
    const uint8_t *delta;       // [states][256]
    const uint8_t *accept;      // [64]
    uint8_t *tab;               // [256 threads][64]: the tables of the chunks without a 0x0A
    uint8_t *kind, *cval;       // [256]: ZRE_*; the value of a constant chunk
    uint32_t *bm_match, *bm_nl; // the slice's bitmaps
};
#define ZRE_LDS(L)                                                                                          \
    __shared__ uint64_t zre_delta[ZARC_REGEX_MAX_STATES * 256 / 8];                                         \
    __shared__ uint8_t zre_accept[ZARC_REGEX_MAX_STATES], zre_tab[256 * ZARC_REGEX_MAX_STATES];             \
    __shared__ uint8_t zre_kind[256], zre_cval[256];                                                        \
    __shared__ uint32_t bm_match[ZARC_CHECK_SLICE / 32], bm_nl[ZARC_CHECK_SLICE / 32];                      \
    const ZreLds L = {(const uint8_t *)zre_delta, zre_accept, zre_tab, zre_kind, zre_cval, bm_match, bm_nl}

// the table into LDS (rows [0, states) of delta); the barrier is regex_chunks's.  Every thread of the workgroup comes here.
__device__ __forceinline__ void regex_load(const ZarcRegexDfa *__restrict__ dfa, uint64_t *delta, uint8_t *accept, uint32_t &states, uint32_t &start)
{
    states = zd::uniform(dfa->states);
    start = zd::uniform(dfa->start);
    if (states > ZARC_REGEX_MAX_STATES) states = ZARC_REGEX_MAX_STATES; // (the engine's own compiler never makes more)
    const uint64_t *src = (const uint64_t *)dfa->delta;                // (8-byte aligned: 72 bytes into the structure)
    for (uint32_t k = threadIdx.x; k < states * 32; k += 256) delta[k] = src[k];
    if (threadIdx.x < ZARC_REGEX_MAX_STATES) accept[threadIdx.x] = dfa->accept[threadIdx.x];
}

// the bytes [0, len) at c (16-byte aligned) from the last to the first: f(byte)
template <class F> __device__ __forceinline__ void regex_walk_down(const uint8_t *__restrict__ c, uint32_t len, F &&f)
{
    for (uint32_t k = (len + 15) / 16; k-- > 0;) {
        const uint4 x = ((const uint4 *)c)[k];
        const uint32_t nb = len - 16 * k; // (16 and more: the whole step)
#pragma unroll
        for (int j = 15; j >= 0; j--) {
            const uint32_t w = j < 4 ? x.x : j < 8 ? x.y : j < 12 ? x.z : x.w;
            if ((uint32_t)j < nb) f((w >> (8 * (j & 3))) & 0xFFu);
        }
    }
}

// First half of a slice's work: the 0x0A bitmap (all 2048 words of both bitmaps are written; bm_match is zeroed) and every chunk's
// transition function.  nbytes content bytes at `a` (16-byte aligned).  -> the length of this thread's chunk.  Every thread comes here.
__device__ __forceinline__ uint32_t regex_chunks(const ZreLds &L, const uint8_t *__restrict__ a, uint32_t nbytes, uint32_t states, uint32_t start)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t clen = nbytes > tid * 256 ? (nbytes - tid * 256 < 256 ? nbytes - tid * 256 : 256u) : 0u;
    const uint8_t *c = a + tid * 256;
    uint32_t low = ZL_NONE;
    for (uint32_t w = 0; w < 8; w++) {
        uint32_t m = 0;
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t k = 2 * w + h;
            if (16 * k >= clen) continue;
            const uint4 x = ((const uint4 *)c)[k];
            uint32_t nm = lines_nl4(x.x) | lines_nl4(x.y) << 4 | lines_nl4(x.z) << 8 | lines_nl4(x.w) << 12;
            if (clen - 16 * k < 16) nm &= (1u << (clen - 16 * k)) - 1u; // the frame ends inside this step
            m |= nm << (16 * h);
        }
        L.bm_nl[tid * 8 + w] = m;
        L.bm_match[tid * 8 + w] = 0;
        if (m && low == ZL_NONE) low = w * 32 + (uint32_t)zd::ctz32(m);
    }
    __syncthreads(); // delta and accept are in LDS (regex_load)
    uint32_t kind = ZRE_IDENT, val = 0;
    if (low != ZL_NONE) { // whatever comes in, the 0x0A restarts: the bytes in front of the lowest one decide
        uint32_t q = start;
        regex_walk_down(c, low, [&](uint32_t b) { q = L.delta[q * 256 + b]; });
        kind = ZRE_CONST; val = q;
    } else if (clen) { // (content without line feeds)
        kind = ZRE_TABLE;
        const uint32_t top = states - 1;
        uint8_t *t = L.tab + tid * ZARC_REGEX_MAX_STATES;
        for (uint32_t s0 = 0; s0 < states; s0 += 4) { // four independent chains a pass
            uint32_t q0 = s0, q1 = s0 + 1 < top ? s0 + 1 : top, q2 = s0 + 2 < top ? s0 + 2 : top, q3 = s0 + 3 < top ? s0 + 3 : top;
            regex_walk_down(c, clen, [&](uint32_t b) {
                q0 = L.delta[q0 * 256 + b]; q1 = L.delta[q1 * 256 + b]; q2 = L.delta[q2 * 256 + b]; q3 = L.delta[q3 * 256 + b];
            });
            t[s0] = (uint8_t)q0;
            if (s0 + 1 < states) t[s0 + 1] = (uint8_t)q1;
            if (s0 + 2 < states) t[s0 + 2] = (uint8_t)q2;
            if (s0 + 3 < states) t[s0 + 3] = (uint8_t)q3;
        }
    }
    L.kind[tid] = (uint8_t)kind;
    L.cval[tid] = (uint8_t)val;
    __syncthreads();
    return clen;
}

// Second half: every thread finds the state in front of its chunk's last byte, walks its bytes from the last to the first and stores its
// words of bm_match.  e_in: the state in front of the slice's last byte; line0: the slice's first byte is a line's first byte.
__device__ __forceinline__ void regex_marks(const ZreLds &L, const uint8_t *__restrict__ a, uint32_t clen, uint32_t e_in, bool line0)
{
    const uint32_t tid = threadIdx.x;
    if (clen) {
        uint32_t u = tid + 1;
        while (u < 256 && L.kind[u] != ZRE_CONST) u++;
        uint32_t q = u < 256 ? L.cval[u] : e_in;
        for (uint32_t v = u - 1; v > tid; v--) if (L.kind[v] == ZRE_TABLE) q = L.tab[v * ZARC_REGEX_MAX_STATES + q];
        const uint8_t *c = a + tid * 256;
        const uint32_t before = tid ? L.bm_nl[tid * 8 - 1] >> 31 : (line0 ? 1u : 0u); // a 0x0A (or nothing) in front of the chunk
        uint32_t hi0 = 0, hi1 = 0;
        for (uint32_t k = (clen + 15) / 16; k-- > 0;) {
            const uint4 x = ((const uint4 *)c)[k];
            const uint32_t nb = clen - 16 * k;
            uint32_t b0 = 0, b1 = 0;
#pragma unroll
            for (int j = 15; j >= 0; j--) {
                const uint32_t w = j < 4 ? x.x : j < 8 ? x.y : j < 12 ? x.z : x.w;
                if ((uint32_t)j < nb) {
                    q = L.delta[q * 256 + ((w >> (8 * (j & 3))) & 0xFFu)];
                    const uint32_t ac = L.accept[q];
                    b0 |= (ac & 1u) << j;
                    b1 |= (ac >> 1 & 1u) << j;
                }
            }
            if (k & 1u) { hi0 = b0; hi1 = b1; continue; }
            const uint32_t w = k >> 1;
            const uint32_t starts = L.bm_nl[tid * 8 + w] << 1 | (w ? L.bm_nl[tid * 8 + w - 1] >> 31 : before); // positions that start a line
            L.bm_match[tid * 8 + w] = (b0 | hi0 << 16) | ((b1 | hi1 << 16) & starts);
            hi0 = hi1 = 0;
        }
    }
    __syncthreads();
}

// lines_bitmaps of zdec_lines.hip with the automaton filling the match bitmap -> the 4 KiB rounds written (all 16).  i: the frame;
// multi: it has several slices (its slices have an entry state).  Every thread of the workgroup comes here.
__device__ __forceinline__ uint32_t regex_bitmaps(const ZreLds &L, uint64_t *delta, uint8_t *accept, const ZarcRegexDfa *__restrict__ dfa,
                                                  const uint8_t *__restrict__ a, uint32_t nbytes, bool frame_start, bool multi,
                                                  const uint8_t *__restrict__ entry)
{
    uint32_t states, start;
    regex_load(dfa, delta, accept, states, start);
    const uint32_t clen = regex_chunks(L, a, nbytes, states, start);
    const uint32_t e_in = multi ? (uint32_t)entry[blockIdx.x] : start;
    regex_marks(L, a, clen, e_in, frame_start || a[-1] == 0x0A);
    return ZARC_CHECK_SLICE / 4096;
}

__global__ void __launch_bounds__(256) zarc_regex_summary(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                          const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                          const int32_t *__restrict__ status, const ZarcRegexDfa *__restrict__ dfa,
                                                          ZarcRegexSlice *__restrict__ summary)
{
    ZRE_LDS(L);
    __shared__ uint32_t red[4];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    if (slice_prefix[i + 1] - slice0 == 1) return; // a frame of one slice: its entry state is `start`
    const int32_t st = status[i];
    if (st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) return;
    const uint64_t len = raw_len[i];
    const uint64_t at = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    if (at >= len) return;
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    const uint32_t tid = threadIdx.x;
    uint32_t states, start;
    regex_load(dfa, zre_delta, zre_accept, states, start);
    (void)regex_chunks(L, dec_base + dec_off[i] + at, nbytes, states, start);
    // the lowest constant chunk: whatever enters the slice, the state is its value there
    const uint64_t C = zd::ballot(L.kind[tid] == ZRE_CONST);
    if (zd::lane_id() == 0) red[zd::wave_id()] = C ? (uint32_t)zd::wave_id() * 64 + (uint32_t)zd::ctz64(C) : ZL_NONE;
    __syncthreads();
    uint32_t lowest = ZL_NONE;
    for (uint32_t w = 0; w < 4; w++) lowest = red[w] < lowest ? red[w] : lowest;
    ZarcRegexSlice *R = summary + blockIdx.x;
    if (lowest != ZL_NONE) {
        if (tid == 0) {
            uint32_t q = L.cval[lowest];
            for (uint32_t v = lowest; v-- > 0;) if (L.kind[v] == ZRE_TABLE) q = L.tab[v * ZARC_REGEX_MAX_STATES + q];
            R->constant = 1; R->value = (uint8_t)q;
        }
    } else if (tid < ZARC_REGEX_MAX_STATES) { // a slice without a 0x0A: one lane per state through the chunk tables, from the last chunk down
        uint32_t q = tid < states ? tid : 0u;
        for (uint32_t v = 256; v-- > 0;) if (L.kind[v] == ZRE_TABLE) q = L.tab[v * ZARC_REGEX_MAX_STATES + q];
        R->table[tid] = (uint8_t)q;
        if (tid == 0) { R->constant = 0; R->value = 0; }
    }
}

// one wave per frame (four frames a workgroup): entry[] of every slice of a frame of several slices
__global__ void __launch_bounds__(256) zarc_regex_carry(uint32_t n, const uint64_t *__restrict__ slice_prefix, const int32_t *__restrict__ status,
                                                        const ZarcRegexDfa *__restrict__ dfa, const ZarcRegexSlice *__restrict__ summary,
                                                        uint8_t *__restrict__ entry)
{
    const uint32_t i = blockIdx.x * 4 + (uint32_t)zd::wave_id(), lane = (uint32_t)zd::lane_id();
    if (i >= n) return;
    const int32_t st = status[i];
    if (st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) return;
    const uint64_t s0 = slice_prefix[i];
    const uint32_t ns = (uint32_t)(slice_prefix[i + 1] - s0);
    if (ns <= 1) return;
    const ZarcRegexSlice *S = summary + s0;
    uint8_t *E = entry + s0;
    uint32_t carry = dfa->start; // the state in front of the last byte of the step's highest slice
    for (uint32_t base = (ns - 1) / 64 * 64;; base -= 64) {
        const uint32_t j = base + lane;
        const bool valid = j < ns;
        const bool isc = valid && S[j].constant != 0;
        const uint32_t val = isc ? S[j].value : 0u;
        const uint64_t C = zd::ballot(isc), above = lane == 63 ? 0ull : C & ~((2ull << lane) - 1ull);
        const uint32_t u = above ? (uint32_t)zd::ctz64(above) : 64u; // the nearest constant slice behind this one
        const uint32_t from = zd::shfl(val, above ? (int)u : 0);
        uint32_t q = above ? from : carry;
        for (uint32_t v = u - 1; v > lane; v--) if (base + v < ns) q = S[base + v].table[q]; // (slices without a 0x0A in between: rare)
        if (valid) E[j] = (uint8_t)q;
        const uint32_t out = isc ? val : (valid ? (uint32_t)S[j].table[q] : q); // behind this slice's first byte
        carry = zd::shfl(out, 0);
        if (base == 0) break;
    }
}

__global__ void __launch_bounds__(256) zarc_regex_scan(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                       const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                       const int32_t *__restrict__ status, const ZarcRegexDfa *__restrict__ dfa,
                                                       const uint8_t *__restrict__ entry, uint32_t *__restrict__ count, uint32_t *__restrict__ first)
{
    ZRE_LDS(L);
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const int32_t st = status[i];
    if (st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) return; // nothing decoded (a digest mismatch still delivers its bytes)
    const uint64_t len = raw_len[i];
    const uint64_t at = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    if (at >= len) return;
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    (void)regex_bitmaps(L, zre_delta, zre_accept, dfa, dec_base + dec_off[i] + at, nbytes, at == 0, slice_prefix[i + 1] - slice0 > 1, entry);
    const uint32_t tid = threadIdx.x;
    uint32_t found = 0, lowest = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t m = bm_match[tid * 8 + k];
        if (!m) continue;
        if (lowest == 0xFFFFFFFFu) lowest = (uint32_t)at + tid * 256 + k * 32 + (uint32_t)zd::ctz32(m);
        found += (uint32_t)__popc(m);
    }
    if (zd::ballot(found != 0) == 0) return; // the common case: nothing leaves the wave
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = zd::shfl_xor(lowest, d); lowest = o < lowest ? o : lowest; }
    found = zd::wave_sum(found);
    if (zd::lane_id() == 0) { atomicAdd(&count[i], found); atomicMin(&first[i], lowest); }
}

// zarc_lines_mark with the automaton in place of the pattern
__global__ void __launch_bounds__(256) zarc_lines_mark_regex(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                             const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                             const int32_t *__restrict__ status, const ZarcRegexDfa *__restrict__ dfa,
                                                             const uint8_t *__restrict__ entry, ZarcLineSlice *__restrict__ slices, uint32_t *__restrict__ lines)
{
    ZRE_LDS(L);
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
    if ((st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) || at >= len) { // nothing decoded, or an empty frame: no line
        if (tid == 0) { slices[blockIdx.x] = S; if (single) lines[i] = 0; }
        return;
    }
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    const uint32_t steps = regex_bitmaps(L, zre_delta, zre_accept, dfa, dec_base + dec_off[i] + at, nbytes, at == 0, !single, entry);
    uint32_t mw[8], nw[8];
    lines_load_chunk(bm_match, bm_nl, steps, mw, nw);
    ZlChunk c;
    lines_chunk(mw, nw, c);
    const ZlState s = lines_state(c.seen, c.seen ? c.tail : c.head, false, red);
    // a chunk's head segment is a line of its own when a 0x0A of the slice lies in front of it; otherwise it is part of the slice's head
    uint32_t total_low, total_nl;
    (void)lines_block_excl(c.inner + (c.head && !s.in && s.nl_before ? 1u : 0u), red, total_low);
    (void)lines_block_excl(c.nls, red, total_nl);
    const uint32_t first = lines_block_min_after(c.seen ? tid * 256 + c.first : ZL_NONE, red);
    const uint32_t last = lines_block_max_before(c.seen ? tid * 256 + c.last + 1 : 0u, red);
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

// zarc_lines_emit with the automaton in place of the pattern
__global__ void __launch_bounds__(256) zarc_lines_emit_regex(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                             const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                             const ZarcRegexDfa *__restrict__ dfa, const uint8_t *__restrict__ entry,
                                                             const ZarcLineSlice *__restrict__ slices, const uint64_t *__restrict__ rec_base,
                                                             const uint32_t *__restrict__ deliver, uint32_t max_line, ZarcLineRec *__restrict__ rec)
{
    ZRE_LDS(L);
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
    const uint32_t steps = regex_bitmaps(L, zre_delta, zre_accept, dfa, dec_base + dec_off[i] + at, nbytes, at == 0, slice_prefix[i + 1] - slice0 > 1, entry);
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
