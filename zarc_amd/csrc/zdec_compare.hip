// zarc_amd/csrc/zdec_compare.hip -- decoded frames COMPARED with other bytes (zarc_gpu_compare_batch*); included by zstd_decode.hip.
//
// What `cmp` answers, for every pair of a batch, behind the verdict of a verify pass: A is the decoded content in scratch, B the other
// side's bytes (16-byte aligned, padding behind them), common = min(|A|, |B|).
//
//   zarc_cmp_scan   workgroup per (frame, 64 KiB slice of A), the grid of zarc_search_scan; only slices of decoded frames work.  The forward
//                   pass reads A and B at the same offsets in aligned 16-byte steps, and makes two 16-bit masks a step -- the bytes that
//                   differ, and the 0x0A bytes of A -- both cut at `common`: what lies behind either content is somebody else's data.  The
//                   slice's differing bytes are a popcount, its lowest and highest a ctz and a clz; the 0x0A mask goes into a bitmap of
//                   the slice in LDS, and the line feeds in front of the lowest differing byte are a popcount of it: no second read.
//                   The backward pass runs only where |A| != |B|: A[p] belongs to B[p + |B| - |A|], which lies at any byte shift against
//                   A, so A's loads stay aligned and B comes through two unaligned 8-byte loads a step; a position whose B index is
//                   negative is a mismatch, and the slice keeps the highest mismatching position.  (With equal lengths the forward pass's
//                   highest differing byte is that answer, and B is read once.)  One ZarcCmpSlice per slice, written by one thread.  No
//                   atomics: nothing depends on scheduling.
//   zarc_cmp_carry  lane per frame: the slices' records are folded in slice order (cmp_join); a frame above ZC_LANE_SLICES slices is taken
//                   by the whole wave, as zarc_wc_carry takes it.  The lane applies the rules of include/zarc_gpu.h -- the common tail never
//                   overlaps the common head -- loads the two bytes at `prefix` and writes the frame's zarc_gpu_cmp.
//
// Frames and other sides are under 4 GiB: positions are 32-bit words; a frame's differing bytes are summed in 64 bits.  The scan reads
// whole 16-byte steps: at most 15 bytes behind either content, inside the padding both have behind them.

constexpr uint32_t ZC_LANE_SLICES = 32; // zarc_cmp_carry: a frame of up to this many slices is its lane's alone
constexpr uint32_t ZC_NONE = ZARC_CMP_NONE;

// bit 7 of every byte of x that is not zero (exact per byte: no carry crosses a byte)
__device__ __forceinline__ uint32_t cmp_nz_bits(uint32_t x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }
// bit k: byte k of the two steps differs
__device__ __forceinline__ uint32_t cmp_ne16(const uint4 x, const uint4 y)
{
    return wc_pack4(cmp_nz_bits(x.x ^ y.x)) | wc_pack4(cmp_nz_bits(x.y ^ y.y)) << 4 | wc_pack4(cmp_nz_bits(x.z ^ y.z)) << 8 | wc_pack4(cmp_nz_bits(x.w ^ y.w)) << 12;
}
__device__ __forceinline__ uint32_t cmp_wave_min(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const uint32_t t = zd::shfl_xor(v, d); v = t < v ? t : v; }
    return v;
}

__global__ void __launch_bounds__(256) zarc_cmp_scan(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                     const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                     const int32_t *__restrict__ status, const uint8_t *__restrict__ oth_base,
                                                     const uint64_t *__restrict__ oth_off, const uint64_t *__restrict__ oth_len, ZarcCmpSlice *__restrict__ rec)
{
    __shared__ uint32_t bm[ZARC_CHECK_SLICE / 32]; // bit p = byte p of the slice is 0x0A, and below common
    __shared__ uint32_t red[4 * 5], sums[4];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const int32_t st = status[i];
    if (st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) return; // nobody reads this slice's record
    const uint32_t tid = threadIdx.x, lane = (uint32_t)zd::lane_id(), wave = (uint32_t)zd::wave_id();
    const uint64_t la = raw_len[i], lb = oth_len[i], common = la < lb ? la : lb;
    const uint64_t at64 = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    uint4 *const out = (uint4 *)(rec + blockIdx.x);
    if (at64 >= la) { // an empty frame's one slice
        if (tid == 0) { out[0] = make_uint4(0u, ZC_NONE, ZC_NONE, 0u); out[1] = make_uint4(0u, ZC_NONE, 0u, 0u); }
        return;
    }
    const uint32_t at = (uint32_t)at64;
    const uint32_t nbytes = (uint32_t)(la - at64 > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : la - at64);
    const uint32_t cb = common > at64 ? (uint32_t)(common - at64 > nbytes ? nbytes : common - at64) : 0u; // the slice's bytes below common
    const uint8_t *const a = dec_base + dec_off[i] + at64, *const b = oth_base + oth_off[i];
    const uint4 *const a16 = (const uint4 *)a, *const b16 = (const uint4 *)(b + at64); // (read only below common: at64 < |B| there)

    // forward: A[p] against B[p], p below common
    const uint32_t n16 = (cb + 15) / 16, steps = (n16 + 255) / 256;
    uint32_t cnt = 0, nls = 0, lo = ZC_NONE, hi1 = 0; // lo: slice-relative; hi1: the highest differing position + 1, 0: none
    for (uint32_t s = 0; s < steps; s++) { // (a uniform trip count: the lane exchange below needs the whole wave)
        const uint32_t v = tid + 256 * s, rel = v * 16;
        uint32_t dm = 0, nm = 0;
        if (v < n16) {
            const uint4 x = a16[v], y = b16[v];
            const uint32_t valid = cb - rel < 16 ? (1u << (cb - rel)) - 1u : 0xFFFFu; // common ends inside this step
            dm = cmp_ne16(x, y) & valid;
            nm = (wc_pack4(wc_eq_bits(x.x, 0x0A0A0A0Au)) | wc_pack4(wc_eq_bits(x.y, 0x0A0A0A0Au)) << 4 | wc_pack4(wc_eq_bits(x.z, 0x0A0A0A0Au)) << 8 |
                  wc_pack4(wc_eq_bits(x.w, 0x0A0A0A0Au)) << 12) & valid;
        }
        cnt += (uint32_t)__popc(dm);
        nls += (uint32_t)__popc(nm);
        if (dm) { // (the steps of a thread ascend: its first hit is its lowest, its last its highest)
            if (lo == ZC_NONE) lo = rel + (uint32_t)zd::ctz32(dm);
            hi1 = rel + (uint32_t)zd::hb32(dm) + 1;
        }
        // two neighbouring lanes hold the halves of one bitmap word: the even lane stores it (no LDS atomic anywhere)
        const uint32_t on = zd::shfl_xor(nm, 1);
        if (!(tid & 1u)) bm[v >> 1] = nm | on << 16;
    }

    // backward: A[p] against B[p + |B| - |A|], every p of the slice; back1: the highest mismatching position + 1, 0: none
    uint32_t back1 = 0;
    if (la != lb) {
        const int64_t delta = (int64_t)lb - (int64_t)la;
        const uint32_t m16 = (nbytes + 15) / 16;
        for (uint32_t v = tid; v < m16; v += 256) {
            const uint32_t rel = v * 16;
            const uint32_t valid = nbytes - rel < 16 ? (1u << (nbytes - rel)) - 1u : 0xFFFFu; // the frame ends inside this step
            const int64_t bi = (int64_t)at64 + rel + delta; // B's index of the step's first byte; below |B| as rel is below nbytes
            uint32_t mm = 0xFFFFu; // B's index is negative in the whole step: nothing of B belongs to these bytes
            if (bi >= 0) {
                const uint4 x = a16[v];
                const uint64_t l8 = zd::load_u64(b + bi), h8 = zd::load_u64(b + bi + 8);
                mm = cmp_ne16(x, make_uint4((uint32_t)l8, (uint32_t)(l8 >> 32), (uint32_t)h8, (uint32_t)(h8 >> 32)));
            } else if (bi > -16) { // B begins inside this step (one step of the frame): byte by byte
                const uint32_t neg = (uint32_t)(-bi);
                mm = (1u << neg) - 1u;
                for (uint32_t k = neg; k < 16; k++)
                    if ((valid >> k & 1u) && a[rel + k] != b[k - neg]) mm |= 1u << k;
            }
            mm &= valid;
            if (mm) back1 = rel + (uint32_t)zd::hb32(mm) + 1;
        }
    }

    cnt = zd::wave_sum(cnt);
    nls = zd::wave_sum(nls);
    lo = cmp_wave_min(lo);
    hi1 = zd::wave_max(hi1);
    back1 = zd::wave_max(back1);
    if (lane == 0) { red[wave] = cnt; red[4 + wave] = nls; red[8 + wave] = lo; red[12 + wave] = hi1; red[16 + wave] = back1; }
    __syncthreads();
    cnt = red[0] + red[1] + red[2] + red[3];
    nls = red[4] + red[5] + red[6] + red[7];
    lo = red[8];
    hi1 = red[12];
    back1 = red[16];
    for (uint32_t w = 1; w < 4; w++) {
        lo = red[8 + w] < lo ? red[8 + w] : lo;
        hi1 = red[12 + w] > hi1 ? red[12 + w] : hi1;
        back1 = red[16 + w] > back1 ? red[16 + w] : back1;
    }
    // the 0x0A bytes in front of the lowest differing byte: the thread's 256 bits of the bitmap, below `lo`
    uint32_t before = 0;
    if (lo != ZC_NONE && tid * 8 < steps * 128) // (words behind the rounds that were written hold nothing)
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t base = (tid * 8 + k) * 32;
            if (base < lo) before += (uint32_t)__popc(lo - base < 32 ? bm[tid * 8 + k] & ((1u << (lo - base)) - 1u) : bm[tid * 8 + k]);
        }
    before = zd::wave_sum(before);
    if (lane == 0) sums[wave] = before;
    __syncthreads();
    if (tid == 0) {
        out[0] = make_uint4(cnt, lo != ZC_NONE ? at + lo : ZC_NONE, hi1 ? at + hi1 - 1 : ZC_NONE, nls);
        out[1] = make_uint4(sums[0] + sums[1] + sums[2] + sums[3], back1 ? at + back1 - 1 : ZC_NONE, 0u, 0u);
    }
}

// what a run of slices looks like from outside: the differing bytes, the lowest and the highest of them, the 0x0A bytes in front of the
// lowest (of the whole run where nothing differs), and the highest mismatch of the backward pass
struct CmpSeg {
    uint64_t differing;
    uint32_t lines, lo, hi, back;
};
__device__ __forceinline__ CmpSeg cmp_empty_seg()
{
    CmpSeg s;
    s.differing = 0; s.lines = 0; s.lo = s.hi = s.back = ZC_NONE;
    return s;
}
// A then B
__device__ __forceinline__ void cmp_join(CmpSeg &A, const CmpSeg &B)
{
    if (A.lo == ZC_NONE) { A.lines += B.lines; A.lo = B.lo; }
    if (B.hi != ZC_NONE) A.hi = B.hi;
    if (B.back != ZC_NONE) A.back = B.back;
    A.differing += B.differing;
}
__device__ __forceinline__ CmpSeg cmp_load_seg(const ZarcCmpSlice *__restrict__ r)
{
    const uint4 lo = ((const uint4 *)r)[0], hi = ((const uint4 *)r)[1];
    CmpSeg s;
    s.differing = lo.x; s.lo = lo.y; s.hi = lo.z; s.lines = lo.x ? hi.x : lo.w; s.back = hi.y;
    return s;
}
__device__ __forceinline__ CmpSeg cmp_shfl_seg(const CmpSeg &s, int src)
{
    CmpSeg r;
    r.differing = wc_shfl64(s.differing, src);
    r.lines = zd::shfl(s.lines, src); r.lo = zd::shfl(s.lo, src); r.hi = zd::shfl(s.hi, src); r.back = zd::shfl(s.back, src);
    return r;
}

__global__ void __launch_bounds__(256) zarc_cmp_carry(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                      const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                      const int32_t *__restrict__ status, const uint8_t *__restrict__ oth_base,
                                                      const uint64_t *__restrict__ oth_off, const uint64_t *__restrict__ oth_len,
                                                      const ZarcCmpSlice *__restrict__ rec, ZarcCmpFrame *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = (uint32_t)zd::lane_id();
    const bool valid = i < n; // (no lane leaves early: the wave works together below)
    uint64_t s0 = 0;
    uint32_t ns = 0, la = 0, lb = 0;
    bool work = false;
    if (valid) {
        const int32_t st = status[i];
        la = (uint32_t)raw_len[i];
        lb = (uint32_t)oth_len[i];
        s0 = slice_prefix[i];
        ns = (uint32_t)(slice_prefix[i + 1] - s0);
        work = st == ZARC_FRAME_OK || st == ZARC_FRAME_DIGEST;
    }
    CmpSeg F = cmp_empty_seg();
    const bool small = work && ns <= ZC_LANE_SLICES;
    if (small)
        for (uint32_t j = 0; j < ns; j++) cmp_join(F, cmp_load_seg(rec + s0 + j));
    uint64_t big = zd::ballot(work && !small);
    while (big) { // wave-uniform: the frame of lane `src`, by all 64 lanes
        const int src = zd::ctz64(big);
        big &= big - 1;
        const uint64_t b_s0 = wc_shfl64(s0, src);
        const uint32_t b_ns = zd::shfl(ns, src);
        const uint32_t per = (b_ns + 63) / 64, j0 = lane * per < b_ns ? lane * per : b_ns, j1 = j0 + per < b_ns ? j0 + per : b_ns;
        CmpSeg mine = cmp_empty_seg();
        for (uint32_t j = j0; j < j1; j++) cmp_join(mine, cmp_load_seg(rec + b_s0 + j));
        CmpSeg all = cmp_empty_seg();
        for (int l = 0; l < 64; l++) cmp_join(all, cmp_shfl_seg(mine, l)); // (every lane folds the same 64: no lane waits for another)
        if ((int)lane == src) F = all;
    }
    if (!valid) return;
    uint4 *const o = (uint4 *)(out + i);
    uint32_t relation = ZARC_CMP_R_NONE, byte_a = 0, byte_b = 0, prefix = 0, suffix = 0;
    uint64_t line = 0;
    if (work) {
        const uint32_t common = la < lb ? la : lb;
        prefix = F.lo != ZC_NONE ? F.lo : common;
        line = 1 + (uint64_t)F.lines;
        const uint32_t last = la == lb ? F.hi : F.back; // the highest position that does not belong to the common tail
        suffix = last == ZC_NONE ? la : la - 1 - last;
        if (suffix > common - prefix) suffix = common - prefix; // the tail never overlaps the head
        relation = F.differing ? ZARC_CMP_R_DIFFER : la == lb ? ZARC_CMP_R_EQUAL : la < lb ? ZARC_CMP_R_FRAME_IS_PREFIX : ZARC_CMP_R_OTHER_IS_PREFIX;
        byte_a = prefix < la ? dec_base[dec_off[i] + prefix] : ZARC_CMP_EOF;
        byte_b = prefix < lb ? oth_base[oth_off[i] + prefix] : ZARC_CMP_EOF;
    }
    o[0] = make_uint4(relation, byte_a, byte_b, 0u);
    o[1] = make_uint4(prefix, 0u, (uint32_t)line, (uint32_t)(line >> 32));
    o[2] = make_uint4((uint32_t)F.differing, (uint32_t)(F.differing >> 32), suffix, 0u);
    o[3] = make_uint4(0u, 0u, 0u, 0u);
}
