// zarc_amd/csrc/zdec_wc.hip -- line, word, character and longest-line COUNTS of decoded frames (zarc_gpu_count_batch*); included by
// zstd_decode.hip.
//
// What `wc` answers, for every frame of a batch, behind the verdict of a verify pass and over the decoded bytes in scratch:
//
//   zarc_wc_count   workgroup per (frame, 64 KiB slice), the grid of zarc_search_scan; only slices of decoded frames work.  Pass 1 reads the
//                   slice once in aligned 16-byte steps and makes three 16-bit masks a step -- 0x0A, white space, UTF-8 continuation bytes.
//                   Words and characters are popcounts (a word start needs the white-space bit of the byte in front: the neighbouring
//                   lane's mask, or one byte loaded from the frame for the first lane of a wave, so a slice's count needs nothing of the
//                   slice in front).  The 0x0A mask goes into a bitmap of the slice in LDS.  Pass 2: thread t owns 256 bits of it and finds
//                   its line feeds, the first and the last, and the longest line between two of them; the block adds the lines that cross
//                   chunks and takes the maximum over the key (length << 32) | ~start -- the longest wins, the lowest among equals.  One
//                   ZarcWcSlice per slice, written by one thread.  No atomics: nothing depends on scheduling.
//   zarc_wc_carry   lane per frame: the slices' records are folded in slice order (wc_join); a frame above ZW_LANE_SLICES slices is taken
//                   by the whole wave, one such frame after the other: every lane folds a 64th of the slices, the 64 partial results are
//                   folded in lane order.  Head and tail of the frame join the candidates, and the lane writes the frame's zarc_gpu_wc.
//                   It reads no content.
//
// Frames are under 4 GiB: positions and per-slice counts are 32-bit words; a frame's words and characters are summed in 64 bits.  The
// count kernel reads whole 16-byte steps: at most 15 bytes behind a frame's content, inside the padding every decoded frame has behind it.

constexpr uint32_t ZW_LANE_SLICES = 32; // zarc_wc_carry: a frame of up to this many slices is its lane's alone
constexpr uint32_t ZW_NONE = ZARC_WC_NONE; // no line feed (first, last); no line between two line feeds (best_len): below every real length

// bit 7 of every byte of w that is c4's (exact per byte: no borrow crosses a byte)
__device__ __forceinline__ uint32_t wc_eq_bits(uint32_t w, uint32_t c4)
{
    const uint32_t x = w ^ c4;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
// ... that is white space: 0x20, or 0x09 .. 0x0D (low seven bits at least 9 and below 14, bit 7 clear; the sums stay inside their bytes)
__device__ __forceinline__ uint32_t wc_sp_bits(uint32_t w)
{
    const uint32_t low = w & 0x7F7F7F7Fu;
    return (((low + 0x77777777u) & ~(low + 0x72727272u) & ~w) | wc_eq_bits(w, 0x20202020u)) & 0x80808080u;
}
// ... that is a UTF-8 continuation byte: bit 7 set, bit 6 clear
__device__ __forceinline__ uint32_t wc_cont_bits(uint32_t w) { return w & ~(w << 1) & 0x80808080u; }
// the four bit-7 flags of z as bits 0 .. 3
__device__ __forceinline__ uint32_t wc_pack4(uint32_t z) { return (((z >> 7) * 0x00204081u) >> 21) & 0xFu; }

__device__ __forceinline__ uint64_t wc_shfl64(uint64_t v, int src) { return zd::shfl((uint32_t)v, src) | (uint64_t)zd::shfl((uint32_t)(v >> 32), src) << 32; }
__device__ __forceinline__ uint64_t wc_wave_max64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t t = zd::shfl_xor((uint32_t)v, d) | (uint64_t)zd::shfl_xor((uint32_t)(v >> 32), d) << 32;
        v = t > v ? t : v;
    }
    return v;
}

__global__ void __launch_bounds__(256) zarc_wc_count(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                     const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                     const int32_t *__restrict__ status, ZarcWcSlice *__restrict__ rec)
{
    __shared__ uint32_t bm[ZARC_CHECK_SLICE / 32]; // bit p = byte p of the slice is 0x0A
    __shared__ uint32_t red[4], sums[8], pick[2];
    __shared__ uint64_t keys[4];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const int32_t st = status[i];
    if (st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) return; // nobody reads this slice's record
    const uint32_t tid = threadIdx.x, lane = (uint32_t)zd::lane_id(), wave = (uint32_t)zd::wave_id();
    const uint64_t len = raw_len[i];
    const uint64_t at64 = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    uint4 *const out = (uint4 *)(rec + blockIdx.x);
    if (at64 >= len) { // an empty frame's one slice
        if (tid == 0) { out[0] = make_uint4(0u, 0u, 0u, ZW_NONE); out[1] = make_uint4(ZW_NONE, ZW_NONE, 0u, 0u); }
        return;
    }
    const uint32_t at = (uint32_t)at64;
    const uint32_t nbytes = (uint32_t)(len - at64 > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at64);
    const uint8_t *const a = dec_base + dec_off[i] + at64;
    const uint4 *const a16 = (const uint4 *)a;
    const uint32_t n16 = (nbytes + 15) / 16, steps = (n16 + 255) / 256;
    uint32_t words = 0, chars = 0;
    for (uint32_t s = 0; s < steps; s++) { // (a uniform trip count: the lane exchanges below need the whole wave)
        const uint32_t v = tid + 256 * s, rel = v * 16;
        uint32_t nm = 0, sm = 0, cm = 0, valid = 0;
        if (v < n16) {
            const uint4 x = a16[v];
            nm = wc_pack4(wc_eq_bits(x.x, 0x0A0A0A0Au)) | wc_pack4(wc_eq_bits(x.y, 0x0A0A0A0Au)) << 4 | wc_pack4(wc_eq_bits(x.z, 0x0A0A0A0Au)) << 8 |
                 wc_pack4(wc_eq_bits(x.w, 0x0A0A0A0Au)) << 12;
            sm = wc_pack4(wc_sp_bits(x.x)) | wc_pack4(wc_sp_bits(x.y)) << 4 | wc_pack4(wc_sp_bits(x.z)) << 8 | wc_pack4(wc_sp_bits(x.w)) << 12;
            cm = wc_pack4(wc_cont_bits(x.x)) | wc_pack4(wc_cont_bits(x.y)) << 4 | wc_pack4(wc_cont_bits(x.z)) << 8 | wc_pack4(wc_cont_bits(x.w)) << 12;
            valid = nbytes - rel < 16 ? (1u << (nbytes - rel)) - 1u : 0xFFFFu; // the frame ends inside this step
            nm &= valid;
        }
        // the white-space bit of the byte in front of the step: the lane below holds it (step v - 1 is a whole step of the same round);
        // the first lane of a wave loads the byte, and the frame's first byte has white space in front of it by definition
        uint32_t prev = zd::shfl_up1(sm) >> 15;
        if (lane == 0 && v < n16) {
            if (at == 0 && rel == 0) prev = 1u;
            else { const uint32_t c = a[(int64_t)rel - 1]; prev = c == 0x20u || c - 9u < 5u ? 1u : 0u; }
        }
        words += (uint32_t)__popc(~sm & (sm << 1 | prev) & valid);
        chars += (uint32_t)__popc(~cm & valid);
        // two neighbouring lanes hold the halves of one bitmap word: the even lane stores it (no LDS atomic anywhere)
        const uint32_t on = zd::shfl_xor(nm, 1);
        if (!(tid & 1u)) bm[v >> 1] = nm | on << 16;
    }
    words = zd::wave_sum(words);
    chars = zd::wave_sum(chars);
    if (lane == 0) { sums[wave] = words; sums[4 + wave] = chars; }
    __syncthreads();

    // pass 2: the thread's 256 positions.  nls, first, last (chunk-relative) and the longest line between two line feeds of the chunk
    const bool live = tid * 8 < steps * 128; // (chunks behind the rounds that were written are empty)
    uint32_t nls = 0, first = ZW_NONE, last = ZW_NONE, ord = 0;
    uint64_t key = 0; // (length << 32) | ~start of the best line so far; 0: none (a real start is below 2^32 - 1)
    const uint32_t chunk = at + tid * 256;
    for (uint32_t k = 0; k < 8; k++) {
        uint32_t m = live ? bm[tid * 8 + k] : 0u;
        while (m) {
            const uint32_t p = k * 32 + (uint32_t)zd::ctz32(m);
            m &= m - 1;
            if (last == ZW_NONE) first = p;
            else {
                const uint64_t c = (uint64_t)(p - last - 1) << 32 | (uint32_t)~(chunk + last + 1);
                if (c > key) { key = c; ord = nls; }
            }
            last = p;
            nls++;
        }
    }
    uint32_t total_nl;
    const uint32_t before = lines_block_excl(nls, red, total_nl);
    const uint32_t next = lines_block_min_after(nls ? tid * 256 + first : ZW_NONE, red); // the first 0x0A behind the chunk (slice-relative)
    ord += before;
    if (nls && next != ZW_NONE) { // the line that begins behind the chunk's last 0x0A and ends in a later chunk
        const uint64_t c = (uint64_t)(next - (tid * 256 + last) - 1) << 32 | (uint32_t)~(chunk + last + 1);
        if (c > key) { key = c; ord = before + nls; }
    }
    const uint64_t wmax = wc_wave_max64(key);
    if (lane == 0) keys[wave] = wmax;
    if (tid == 0) { pick[0] = 0; pick[1] = nls ? at + first : (next != ZW_NONE ? at + next : ZW_NONE); } // the slice's first 0x0A
    __syncthreads();
    uint64_t best = keys[0];
    for (uint32_t w = 1; w < 4; w++) best = keys[w] > best ? keys[w] : best;
    if (key && key == best) pick[0] = ord; // (keys differ in their starts: one thread)
    const uint32_t prev_last = lines_block_max_before(nls ? tid * 256 + last + 1 : 0u, red); // (a barrier: pick[] is visible behind it)
    if (tid == 255) {
        const uint32_t l1 = nls ? tid * 256 + last + 1 : prev_last; // behind the slice's last 0x0A; 0: none
        out[0] = make_uint4(total_nl, sums[0] + sums[1] + sums[2] + sums[3], sums[4] + sums[5] + sums[6] + sums[7], pick[1]);
        out[1] = make_uint4(l1 ? at + l1 - 1 : ZW_NONE, best ? (uint32_t)(best >> 32) : ZW_NONE, best ? ~(uint32_t)best : 0u, best ? pick[0] : 0u);
    }
}

// what a run of slices looks like from outside: ZarcWcSlice with the counts of a frame
struct WcSeg {
    uint64_t words, chars;
    uint32_t nls, first, last, best_len, best_start, best_ord;
};
__device__ __forceinline__ WcSeg wc_empty_seg()
{
    WcSeg s;
    s.words = s.chars = 0; s.nls = 0; s.first = s.last = s.best_len = ZW_NONE; s.best_start = s.best_ord = 0;
    return s;
}
// a line of `len` bytes is longer than the best of s (none: any line is)
__device__ __forceinline__ bool wc_longer(uint32_t len, const WcSeg &s) { return s.best_len == ZW_NONE || len > s.best_len; }
// A then B: the line that crosses the seam lies in front of every line of B and behind every line of A, and only a longer line replaces
__device__ __forceinline__ void wc_join(WcSeg &A, const WcSeg &B)
{
    if (A.last != ZW_NONE && B.first != ZW_NONE && wc_longer(B.first - A.last - 1, A)) {
        A.best_len = B.first - A.last - 1; A.best_start = A.last + 1; A.best_ord = A.nls;
    }
    if (B.best_len != ZW_NONE && wc_longer(B.best_len, A)) { A.best_len = B.best_len; A.best_start = B.best_start; A.best_ord = B.best_ord + A.nls; }
    A.nls += B.nls; A.words += B.words; A.chars += B.chars;
    if (A.first == ZW_NONE) A.first = B.first;
    if (B.last != ZW_NONE) A.last = B.last;
}
__device__ __forceinline__ WcSeg wc_load_seg(const ZarcWcSlice *__restrict__ r)
{
    const uint4 lo = ((const uint4 *)r)[0], hi = ((const uint4 *)r)[1];
    WcSeg s;
    s.nls = lo.x; s.words = lo.y; s.chars = lo.z; s.first = lo.w; s.last = hi.x; s.best_len = hi.y; s.best_start = hi.z; s.best_ord = hi.w;
    return s;
}
__device__ __forceinline__ WcSeg wc_shfl_seg(const WcSeg &s, int src)
{
    WcSeg r;
    r.words = wc_shfl64(s.words, src); r.chars = wc_shfl64(s.chars, src);
    r.nls = zd::shfl(s.nls, src); r.first = zd::shfl(s.first, src); r.last = zd::shfl(s.last, src);
    r.best_len = zd::shfl(s.best_len, src); r.best_start = zd::shfl(s.best_start, src); r.best_ord = zd::shfl(s.best_ord, src);
    return r;
}

__global__ void __launch_bounds__(256) zarc_wc_carry(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint64_t *__restrict__ raw_len,
                                                     const int32_t *__restrict__ status, const ZarcWcSlice *__restrict__ rec, ZarcWcFrame *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = (uint32_t)zd::lane_id();
    const bool valid = i < n; // (no lane leaves early: the wave works together below)
    uint64_t s0 = 0;
    uint32_t ns = 0, len = 0;
    bool work = false;
    if (valid) {
        const int32_t st = status[i];
        len = (uint32_t)raw_len[i];
        s0 = slice_prefix[i];
        ns = (uint32_t)(slice_prefix[i + 1] - s0);
        work = (st == ZARC_FRAME_OK || st == ZARC_FRAME_DIGEST) && len > 0;
    }
    WcSeg F = wc_empty_seg();
    const bool small = work && ns <= ZW_LANE_SLICES;
    if (small)
        for (uint32_t j = 0; j < ns; j++) wc_join(F, wc_load_seg(rec + s0 + j));
    uint64_t big = zd::ballot(work && !small);
    while (big) { // wave-uniform: the frame of lane `src`, by all 64 lanes
        const int src = zd::ctz64(big);
        big &= big - 1;
        const uint64_t b_s0 = wc_shfl64(s0, src);
        const uint32_t b_ns = zd::shfl(ns, src);
        const uint32_t per = (b_ns + 63) / 64, j0 = lane * per < b_ns ? lane * per : b_ns, j1 = j0 + per < b_ns ? j0 + per : b_ns;
        WcSeg mine = wc_empty_seg();
        for (uint32_t j = j0; j < j1; j++) wc_join(mine, wc_load_seg(rec + b_s0 + j));
        WcSeg all = wc_empty_seg();
        for (int l = 0; l < 64; l++) wc_join(all, wc_shfl_seg(mine, l)); // (every lane folds the same 64: no lane waits for another)
        if ((int)lane == src) F = all;
    }
    if (!valid) return;
    uint4 *const o = (uint4 *)(out + i);
    uint32_t best_len = 0, best_start = 0, best_ord = 0;
    if (work) {
        if (F.nls == 0) { best_len = len; best_ord = 1; }
        else {
            best_len = F.first; // the head
            if (F.best_len != ZW_NONE && F.best_len > best_len) { best_len = F.best_len; best_start = F.best_start; best_ord = F.best_ord; }
            if (len - F.last - 1 > best_len) { best_len = len - F.last - 1; best_start = F.last + 1; best_ord = F.nls; }
            best_ord += 1;
        }
    }
    o[0] = make_uint4(F.nls, 0u, (uint32_t)F.words, (uint32_t)(F.words >> 32));
    o[1] = make_uint4((uint32_t)F.chars, (uint32_t)(F.chars >> 32), best_len, 0u);
    o[2] = make_uint4(best_start, 0u, best_ord, 0u);
    o[3] = make_uint4(0u, 0u, 0u, 0u);
}
