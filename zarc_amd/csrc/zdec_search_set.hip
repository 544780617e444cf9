// zarc_amd/csrc/zdec_search_set.hip -- a SET of fixed strings searched in one pass (zarc_gpu_search_set_*); included by zstd_decode.hip.
//
// zarc_search_scan looks for one byte string.  These kernels look for 1 .. ZARC_SEARCH_MAX_SET of them in the same read-once pass over the
// decoded bytes of a verify pass: per frame the number of start positions at which AT LEAST ONE pattern matches (a position counts once),
// the lowest of them, the lowest pattern index that matches there, and per pattern the number of positions at which it matches.
//
// The host compiles the set (folded when icase) into one blob of words (engine.hip, search_upload_set; ZarcSetDesc says where things are):
//
//   words [0, lds_words)  the image every workgroup copies into LDS: per length CLASS that the set holds -- 1, 2, 3 bytes, and 4 bytes
//                         and more keyed by their first four -- a bit filter and behind it an exact open-addressed table
//                         {key, list} of the class's distinct keys.  Both are powers of two sized from the number of distinct keys,
//                         so a workgroup's set-up load is proportional to the set: a set of one pattern loads 6 words, the fullest
//                         set of 1024 about 9 K words.  (Chosen over a persistent grid that loads a fixed-size image once: the
//                         image of the sets people really pass is a few hundred bytes, and the grid of zarc_search_scan keeps a
//                         million tiny frames and a few huge ones equally busy.)
//                         The one-byte class's filter is the 256-bit mask itself; the others are hashed.
//   lists                 per distinct key: n, then the n pattern indices that share it, ascending
//   patterns              per pattern: {where its bytes lie (a word index), its length}
//   bytes                 every pattern padded with zeros to whole words
//
// zarc_set_scan has the grid, the frame / slice location and the 16 + 4 byte step of zarc_search_scan.  A lane tests its 16 start
// positions against the filter of every class the set holds (class flags are wave-uniform: a set without short patterns pays nothing for
// them).  A filter hit is looked up in the exact table, in LDS: a false positive never reaches global memory.  A true key hit walks the
// key's list: for every pattern of it the frame's end is checked first (p + len <= the frame's length: the rule is per pattern), then the
// rest of the pattern is compared 4 bytes a step, text from memory, pattern from the blob (L2-resident).  ALL candidates of a position
// are looked at: every matching pattern gets its hit (a 32-bit atomicAdd; matches are rare), the position counts once.
// The worst case is zarc_search_scan's, times the candidates per position; it is accepted as it is there.
// Reads stay inside the frame's content plus the 19 bytes behind it that zarc_search_scan relies on.
//
// zarc_set_which runs behind the scan, one lane per frame: for a frame with a match, the lowest pattern index matching at first[i].
// The lines kernels differ from zdec_lines.hip only in who fills the match bitmap: lines_bitmaps_set and the two kernels that call it.

struct ZsetCtx {
    const uint32_t *img;   // LDS: the filters and tables
    const uint32_t *set;   // global: the whole blob
    const uint8_t *a;      // the slice's first byte
    uint32_t room;         // content bytes of the frame from the slice's first byte on
    bool fold;
    uint32_t *hits;        // per pattern, or null (the lines kernels: zarc_set_scan has counted already)
};

// start positions of this slice at which a pattern of `len` bytes still ends inside the frame
__device__ __forceinline__ uint32_t zset_starts(uint32_t room, uint32_t len)
{
    const uint32_t s = room >= len ? room - len + 1 : 0u;
    return s > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : s;
}

// the patterns that share `key` (class c) against the text at position rel: -> does at least one match
__device__ __forceinline__ bool zset_verify(const ZarcSetDesc &sd, const ZsetCtx &x, uint32_t c, uint32_t key, uint32_t h, uint32_t rel)
{
    const uint32_t *tab = x.img + sd.toff[c];
    const uint32_t tmask = (1u << sd.tlog[c]) - 1u;
    uint32_t slot = h >> (32 - sd.tlog[c]), list = 0;
    for (;;) { // (the table is at most half full: an empty slot ends every probe)
        const uint32_t ref = tab[2 * slot + 1];
        if (ref == 0) return false;
        if (tab[2 * slot] == key) { list = ref; break; }
        slot = (slot + 1) & tmask;
    }
    const uint32_t nl = x.set[list];
    const uint8_t *t = x.a + rel;
    bool any = false;
    for (uint32_t e = 0; e < nl; e++) {
        const uint32_t id = x.set[list + 1 + e];
        const uint32_t at = x.set[sd.pat_off + 2 * id], len = x.set[sd.pat_off + 2 * id + 1];
        if (rel + len > x.room) continue; // the frame ends inside this pattern: nothing behind the filter word is read for it
        const uint32_t words = len / 4, tail = len & 3u;
        bool same = true;
        for (uint32_t k = 1; k < words && same; k++) {
            uint32_t w = zd::load_u32(t + 4 * k);
            if (x.fold) w = search_fold4(w);
            same = w == x.set[at + k];
        }
        if (same && len > 4 && tail) { // (reads up to 3 bytes past the match: inside the next entry or the padding, masked away)
            uint32_t w = zd::load_u32(t + 4 * words);
            if (x.fold) w = search_fold4(w);
            same = ((w ^ x.set[at + words]) & ((1u << (8 * tail)) - 1u)) == 0;
        }
        if (same) { any = true; if (x.hits) atomicAdd(&x.hits[id], 1u); }
    }
    return any;
}

// One step of a lane: the 16 start positions rel .. rel + 15 of the slice, w0 .. w4 = the (folded) 20 bytes from rel on.
// -> bit j: at least one pattern matches at rel + j
__device__ __forceinline__ uint32_t zset_step(const ZarcSetDesc &sd, const ZsetCtx &x, uint32_t rel, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4)
{
    const uint64_t q0 = w0 | (uint64_t)w1 << 32, q1 = w1 | (uint64_t)w2 << 32, q2 = w2 | (uint64_t)w3 << 32, q3 = w3 | (uint64_t)w4 << 32;
    uint32_t matched = 0;
    for (uint32_t c = 0; c < 4; c++) { // wave-uniform: the classes of the set
        if (!(sd.classes >> c & 1u)) continue;
        const uint32_t kmask = c == 3 ? 0xFFFFFFFFu : (1u << (8 * (c + 1))) - 1u;
        const uint32_t cnt = zset_starts(x.room, c + 1); // (class 3: 4 bytes and more -- the first four must fit)
        if (rel >= cnt) continue;
        const uint32_t *filt = x.img + sd.foff[c];
        const uint32_t fshift = 32 - sd.flog[c];
        uint32_t cand = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t q = j < 4 ? q0 : j < 8 ? q1 : j < 12 ? q2 : q3;
            const uint32_t key = (uint32_t)(q >> (8 * (j & 3))) & kmask;
            const uint32_t bit = c == 0 ? key : (key * ZARC_SET_HASH) >> fshift;
            cand |= (filt[bit >> 5] >> (bit & 31u) & 1u) << j;
        }
        if (cnt - rel < 16) cand &= (1u << (cnt - rel)) - 1u; // the slice's (or the frame's) last start position of this class lies inside this step
        while (cand) { // rare on real content
            const uint32_t j = (uint32_t)zd::ctz32(cand);
            cand &= cand - 1;
            const uint64_t q = j < 4 ? q0 : j < 8 ? q1 : j < 12 ? q2 : q3;
            const uint32_t key = (uint32_t)(q >> (8 * (j & 3))) & kmask;
            if (zset_verify(sd, x, c, key, key * ZARC_SET_HASH, rel + j)) matched |= 1u << j;
        }
    }
    return matched;
}

// the set's image into LDS; every thread of the workgroup comes here
__device__ __forceinline__ void zset_load(const ZarcSetDesc &sd, const uint32_t *__restrict__ set, uint32_t *img)
{
    for (uint32_t w = threadIdx.x; w < sd.lds_words; w += 256) img[w] = set[w];
    __syncthreads();
}

__global__ void __launch_bounds__(256) zarc_set_scan(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                     const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                     const int32_t *__restrict__ status, ZarcSetDesc sd, const uint32_t *__restrict__ set, uint32_t icase,
                                                     uint32_t *__restrict__ count, uint32_t *__restrict__ first, uint32_t *__restrict__ hits)
{
    HIP_DYNAMIC_SHARED(uint32_t, img)
    // the frame of this workgroup: the last i with slice_prefix[i] <= blockIdx.x (wave-uniform: scalar loads)
    const uint64_t wg = blockIdx.x;
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (slice_prefix[mid] <= wg) lo = mid; else hi = mid;
    }
    const uint32_t i = lo;
    if (i >= n || wg >= slice_prefix[i + 1]) return;
    const int32_t st = status[i];
    if (st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) return; // nothing decoded (a digest mismatch still delivers its bytes)
    const uint64_t len = raw_len[i];
    const uint64_t at = (wg - slice_prefix[i]) * (uint64_t)ZARC_CHECK_SLICE;
    if (sd.count == 0 || sd.min_len == 0 || at >= len) return;
    ZsetCtx x;
    x.img = img; x.set = set; x.a = dec_base + dec_off[i] + at; x.fold = icase != 0; x.hits = hits;
    x.room = (uint32_t)(len - at); // (frames are under 4 GiB)
    const uint32_t cnt = zset_starts(x.room, sd.min_len); // start positions that leave room for the shortest pattern
    if (cnt == 0) return;
    zset_load(sd, set, img);
    const uint32_t tid = threadIdx.x;
    const uint4 *a16 = (const uint4 *)x.a;
    const uint32_t n16 = (cnt + 15) / 16;
    uint32_t found = 0, lowest = 0xFFFFFFFFu;
    for (uint32_t v = tid; v < n16; v += 256) {
        const uint4 q = a16[v];
        uint32_t w0 = q.x, w1 = q.y, w2 = q.z, w3 = q.w, w4 = ((const uint32_t *)(a16 + v + 1))[0];
        if (x.fold) { w0 = search_fold4(w0); w1 = search_fold4(w1); w2 = search_fold4(w2); w3 = search_fold4(w3); w4 = search_fold4(w4); }
        const uint32_t m = zset_step(sd, x, v * 16, w0, w1, w2, w3, w4);
        if (m) {
            if (lowest == 0xFFFFFFFFu) lowest = (uint32_t)at + v * 16 + (uint32_t)zd::ctz32(m); // (v grows: a lane's first match is its lowest)
            found += (uint32_t)__popc(m);
        }
    }
    if (zd::ballot(found != 0) == 0) return; // the common case: nothing leaves the wave
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = zd::shfl_xor(lowest, d); lowest = o < lowest ? o : lowest; }
    found = zd::wave_sum(found);
    if (zd::lane_id() == 0) { atomicAdd(&count[i], found); atomicMin(&first[i], lowest); }
}

// one lane per frame: which[i] = the lowest pattern index that matches at first[i] (0xFFFFFFFF: the frame has no match)
__global__ void __launch_bounds__(256) zarc_set_which(uint32_t n, const uint8_t *__restrict__ dec_base, const uint64_t *__restrict__ dec_off,
                                                      const uint64_t *__restrict__ raw_len, ZarcSetDesc sd, const uint32_t *__restrict__ set, uint32_t icase,
                                                      const uint32_t *__restrict__ count, const uint32_t *__restrict__ first, uint32_t *__restrict__ which)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t best = 0xFFFFFFFFu;
    if (count[i] != 0) {
        const uint32_t p = first[i], len_i = (uint32_t)raw_len[i];
        const uint8_t *t = dec_base + dec_off[i] + p;
        const bool fold = icase != 0;
        for (uint32_t id = 0; id < sd.count && best == 0xFFFFFFFFu; id++) {
            const uint32_t at = set[sd.pat_off + 2 * id], len = set[sd.pat_off + 2 * id + 1];
            if (len > len_i - p) continue;
            const uint32_t words = len / 4, tail = len & 3u;
            bool same = true;
            for (uint32_t k = 0; k < words && same; k++) {
                uint32_t w = zd::load_u32(t + 4 * k);
                if (fold) w = search_fold4(w);
                same = w == set[at + k];
            }
            if (same && tail) { // (up to 3 bytes past the pattern: the next entry or the padding, masked away)
                uint32_t w = zd::load_u32(t + 4 * words);
                if (fold) w = search_fold4(w);
                same = ((w ^ set[at + words]) & ((1u << (8 * tail)) - 1u)) == 0;
            }
            if (same) best = id;
        }
    }
    which[i] = best;
}

// lines_bitmaps of zdec_lines.hip with the set matcher filling the match bitmap: nbytes content bytes at x.a (x.room >= nbytes: the frame
// goes on behind the slice).  Words [0, 128 * steps) of both bitmaps are written; every thread of the workgroup comes here.
__device__ __forceinline__ uint32_t lines_bitmaps_set(const ZarcSetDesc &sd, const ZsetCtx &x, uint32_t nbytes, uint32_t *img, uint32_t *bm_match, uint32_t *bm_nl)
{
    zset_load(sd, x.set, img);
    const uint32_t tid = threadIdx.x;
    const uint32_t cnt = zset_starts(x.room, sd.min_len);
    const uint4 *a16 = (const uint4 *)x.a;
    const uint32_t n16 = (nbytes + 15) / 16, steps = (n16 + 255) / 256;
    for (uint32_t s = 0; s < steps; s++) { // (a uniform trip count: the pair exchange below needs the whole wave)
        const uint32_t v = tid + 256 * s, rel = v * 16;
        uint32_t hm = 0, nm = 0;
        if (v < n16) {
            const uint4 q = a16[v];
            uint32_t w0 = q.x, w1 = q.y, w2 = q.z, w3 = q.w;
            nm = lines_nl4(w0) | lines_nl4(w1) << 4 | lines_nl4(w2) << 8 | lines_nl4(w3) << 12;
            if (nbytes - rel < 16) nm &= (1u << (nbytes - rel)) - 1u; // the frame ends inside this step
            if (rel < cnt) {
                uint32_t w4 = ((const uint32_t *)(a16 + v + 1))[0];
                if (x.fold) { w0 = search_fold4(w0); w1 = search_fold4(w1); w2 = search_fold4(w2); w3 = search_fold4(w3); w4 = search_fold4(w4); }
                hm = zset_step(sd, x, rel, w0, w1, w2, w3, w4);
            }
        }
        // two neighbouring lanes hold the halves of one bitmap word: the even lane stores it (no LDS atomic anywhere)
        const uint32_t om = zd::shfl_xor(hm, 1), on = zd::shfl_xor(nm, 1);
        if (!(tid & 1u)) { bm_match[v >> 1] = hm | om << 16; bm_nl[v >> 1] = nm | on << 16; }
    }
    __syncthreads();
    return steps;
}

// zarc_lines_mark with the set in place of the pattern
__global__ void __launch_bounds__(256) zarc_lines_mark_set(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                           const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                           const int32_t *__restrict__ status, ZarcSetDesc sd, const uint32_t *__restrict__ set, uint32_t icase,
                                                           ZarcLineSlice *__restrict__ slices, uint32_t *__restrict__ lines)
{
    HIP_DYNAMIC_SHARED(uint32_t, img)
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
    if ((st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) || sd.count == 0 || sd.min_len == 0 || at >= len) { // nothing decoded, or an empty frame: no line
        if (tid == 0) { slices[blockIdx.x] = S; if (single) lines[i] = 0; }
        return;
    }
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    ZsetCtx x;
    x.img = img; x.set = set; x.a = dec_base + dec_off[i] + at; x.room = (uint32_t)(len - at); x.fold = icase != 0; x.hits = nullptr;
    const uint32_t steps = lines_bitmaps_set(sd, x, nbytes, img, bm_match, bm_nl);
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

// zarc_lines_emit with the set in place of the pattern
__global__ void __launch_bounds__(256) zarc_lines_emit_set(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                           const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len, ZarcSetDesc sd,
                                                           const uint32_t *__restrict__ set, uint32_t icase, const ZarcLineSlice *__restrict__ slices,
                                                           const uint64_t *__restrict__ rec_base, const uint32_t *__restrict__ deliver, uint32_t max_line,
                                                           ZarcLineRec *__restrict__ rec)
{
    HIP_DYNAMIC_SHARED(uint32_t, img)
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
    ZsetCtx x;
    x.img = img; x.set = set; x.a = dec_base + dec_off[i] + at; x.room = (uint32_t)(len - at); x.fold = icase != 0; x.hits = nullptr;
    const uint32_t steps = lines_bitmaps_set(sd, x, nbytes, img, bm_match, bm_nl);
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
