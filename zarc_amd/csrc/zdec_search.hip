// zarc_amd/csrc/zdec_search.hip -- fixed-string search over decoded frames (zarc_gpu_search_batch*); included by zstd_decode.hip.
//
// A verify pass leaves every frame's decoded bytes in scratch of the handle (16-byte aligned entries in the decoder's order).  This kernel
// looks for ONE byte string of 1 .. ZARC_SEARCH_MAX_PATTERN bytes in them while they are there: per frame the number of matching start
// positions (overlapping occurrences count) and the lowest one.  It is a read-once bandwidth pass.
//
// One 256-thread workgroup per (frame, slice of ZARC_CHECK_SLICE bytes), the grid of zarc_check_compare: slice_prefix[] (decoder order)
// says which frame a workgroup serves, so a few huge frames and a million tiny ones both fill the chip.  A slice owns the START positions
// [at, at + 65536) and reads up to m - 1 bytes past them.  Every lane loads 16 aligned bytes per step plus the 4 bytes behind them (a
// second load: the line its neighbour lane brings in anyway), tests its 16 start positions against the first four pattern bytes
// (all of them when m < 4) with 64-bit shifts and compares, and looks at the rest of the pattern -- 4 bytes a step, text from memory,
// pattern from LDS -- only where that filter hits.  The worst case is every position a candidate (a run of one byte searched for that
// byte repeated): O(n * m).  It is accepted, not engineered around: a longer filter would cost every other input.
//
// Frame end: position p counts only when p + m <= len of its own frame.  The bytes behind a frame's end belong to the next frame or to
// padding; the loads may touch them (ZARC_GPU_PAD and more is readable behind the last entry), they never complete a match.
// Case folding (icase): 'A'..'Z' become 'a'..'z' in registers, nothing else changes; the host folded the pattern the same way.
// A wave that found nothing sends nothing; one that did sends one atomicAdd and one atomicMin.  Frames are under 4 GiB: 32-bit words.

// 'A'..'Z' -> 'a'..'z' in each byte of w, every other byte as it is (no carry crosses a byte: the operands have bit 7 clear)
__device__ __forceinline__ uint32_t search_fold4(uint32_t w)
{
    const uint32_t t = w & 0x7F7F7F7Fu;
    const uint32_t upper = (t + 0x3F3F3F3Fu) & ~(t + 0x25252525u) & ~w & 0x80808080u; // bit 7 of a byte: 0x41 <= byte <= 0x5A
    return w | (upper >> 2);
}

__global__ void __launch_bounds__(256) zarc_search_scan(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                        const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                        const int32_t *__restrict__ status, const uint8_t *__restrict__ pattern, uint32_t m,
                                                        uint32_t icase, uint32_t *__restrict__ count, uint32_t *__restrict__ first)
{
    __shared__ uint32_t pat[ZARC_SEARCH_MAX_PATTERN / 4];
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
    if (m == 0 || m > ZARC_SEARCH_MAX_PATTERN || len < m || at > len - m) return;
    const uint64_t starts = len - m + 1 - at; // start positions from `at` on that leave room for the pattern inside the frame
    const uint32_t cnt = (uint32_t)(starts > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : starts);
    const uint8_t *a = dec_base + dec_off[i] + at;
    const uint32_t tid = threadIdx.x;
    // the pattern: words in LDS for the verification, the first four bytes (the filter) in a uniform register
    if (tid < ZARC_SEARCH_MAX_PATTERN / 4) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; k++) if (tid * 4 + k < m) w |= (uint32_t)pattern[tid * 4 + k] << (8 * k);
        pat[tid] = w;
    }
    __syncthreads();
    const uint32_t p4 = zd::uniform(pat[0]);
    const uint32_t mask4 = m >= 4 ? 0xFFFFFFFFu : (1u << (8 * m)) - 1u;
    const uint32_t tail = m & 3u, words = m / 4; // whole pattern words, and the bytes of the last partial one
    const uint32_t tail_mask = (1u << (8 * tail)) - 1u;
    const bool fold = icase != 0;

    const uint4 *a16 = (const uint4 *)a;
    const uint32_t n16 = (cnt + 15) / 16;
    uint32_t found = 0, lowest = 0xFFFFFFFFu;
#pragma unroll 2
    for (uint32_t v = tid; v < n16; v += 256) {
        const uint4 x = a16[v];
        uint32_t w0 = x.x, w1 = x.y, w2 = x.z, w3 = x.w, w4 = ((const uint32_t *)(a16 + v + 1))[0];
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
        const uint32_t rel = v * 16;
        if (cnt - rel < 16) hits &= (1u << (cnt - rel)) - 1u; // the slice's (or the frame's) last start position lies inside this step
        while (hits) { // rare on real content: the rest of the pattern, 4 bytes a step
            const uint32_t j = (uint32_t)zd::ctz32(hits);
            hits &= hits - 1;
            const uint8_t *t = a + rel + j;
            bool same = true;
            for (uint32_t k = 1; k < words && same; k++) {
                uint32_t w = zd::load_u32(t + 4 * k);
                if (fold) w = search_fold4(w);
                same = w == pat[k];
            }
            if (same && m > 4 && tail) { // (reads up to 3 bytes past the match: inside the next entry or the padding, masked away)
                uint32_t w = zd::load_u32(t + 4 * words);
                if (fold) w = search_fold4(w);
                same = ((w ^ pat[words]) & tail_mask) == 0;
            }
            if (same) { found++; if (lowest == 0xFFFFFFFFu) lowest = (uint32_t)at + rel + j; } // (v and j grow: a lane's first match is its lowest)
        }
    }
    if (zd::ballot(found != 0) == 0) return; // the common case: nothing leaves the wave
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = zd::shfl_xor(lowest, d); lowest = o < lowest ? o : lowest; }
    found = zd::wave_sum(found);
    if (zd::lane_id() == 0) { atomicAdd(&count[i], found); atomicMin(&first[i], lowest); }
}
