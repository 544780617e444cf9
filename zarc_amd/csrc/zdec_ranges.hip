// zarc_amd/csrc/zdec_ranges.hip -- byte and line RANGES of decoded frames (zarc_gpu_read_ranges_batch*); included by zstd_decode.hip.
//
// A range names units of a frame's content: bytes, or lines with their 0x0A (a last line without one is a unit as well).  The units tile
// the content, so a range [a, b) of units is one run of bytes [pos(a), pos(b)), pos(0) = 0, pos(T) = the frame's length and pos(k) = the
// offset behind the k-th 0x0A otherwise.  These kernels run behind the verdict of a verify pass, over the decoded bytes in scratch:
//
//   zarc_range_count   workgroup per (frame, 64 KiB slice), the grid of zarc_search_scan; only slices of decoded frames with a LINES range
//                      work: the 0x0A bytes of the slice, one plain store per slice.  No atomics: the result does not depend on scheduling.
//   zarc_range_carry   lane per frame.  BYTES ranges are arithmetic.  A LINES frame of up to ZR_LANE_SLICES slices is summed and walked by its
//                      lane; a larger one is taken by the whole wave, one such frame after the other: every lane sums a 64th of the slices,
//                      a wave scan finds the 64th that holds a boundary and wave scans over that 64th find the slice.  A million one-slice
//                      frames are 4096 workgroups, one frame of 16 384 slices is 256 loads a lane and four scans a boundary.  T, a, b and
//                      every boundary that needs no content (unit 0, unit T) are final here; the others go to the open list.
//   zarc_range_locate  workgroup per open boundary (a fixed grid walks the list): thread t counts the 0x0A bytes of its 256 bytes of the
//                      slice, a block scan finds the thread that holds the ord-th, that thread finds the byte in its masks.
//   -- the host reads the descriptors, applies the delivery rule in the caller's order and uploads the copy plan --
//   zarc_range_gather  workgroup per 64 KiB of output, addressed through a prefix array: destination-aligned 16-byte stores, the source
//                      through aligned 16-byte loads where it happens to be aligned as well and through unaligned 8-byte loads otherwise,
//                      head and tail bytewise.  It writes [dst, dst + len) and reads [start, start + len) of the frame and nothing else.
//
// Frames are under 4 GiB: offsets and unit numbers are 32-bit words.  The count and locate kernels read whole 16-byte steps: at most 15
// bytes behind a frame's content, inside the padding every decoded frame has behind it.

constexpr uint32_t ZR_LANE_SLICES = 32; // zarc_range_carry: a LINES frame of up to this many slices is its lane's alone

// bit 7 of every byte of w that is 0x0A (exact per byte: no borrow crosses a byte)
__device__ __forceinline__ uint32_t range_nl_bits(uint32_t w)
{
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
// ... of the first `valid` (0 .. 4, may be given beyond) bytes only
__device__ __forceinline__ uint32_t range_keep_bytes(uint32_t z, uint32_t valid) { return valid >= 4 ? z : z & ((1u << (8 * valid)) - 1u); }

__global__ void __launch_bounds__(256) zarc_range_count(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                        const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                        const int32_t *__restrict__ status, const ZarcRangeReq *__restrict__ req, uint32_t *__restrict__ cnt)
{
    __shared__ uint32_t red[4];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const int32_t st = status[i];
    if ((st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) || req[i].unit != ZARC_RANGE_LINES) return; // nobody reads this slice's count
    const uint32_t tid = threadIdx.x;
    const uint64_t len = raw_len[i];
    const uint64_t at = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    if (at >= len) { if (tid == 0) cnt[blockIdx.x] = 0; return; } // an empty frame's one slice
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    const uint4 *a16 = (const uint4 *)(dec_base + dec_off[i] + at);
    const uint32_t n16 = (nbytes + 15) / 16;
    uint32_t c = 0;
    for (uint32_t v = tid; v < n16; v += 256) {
        const uint4 x = a16[v];
        uint32_t z0 = range_nl_bits(x.x), z1 = range_nl_bits(x.y), z2 = range_nl_bits(x.z), z3 = range_nl_bits(x.w);
        const uint32_t left = nbytes - v * 16;
        if (left < 16) { // the frame ends inside this step
            z0 = range_keep_bytes(z0, left); z1 = range_keep_bytes(z1, left > 4 ? left - 4 : 0u);
            z2 = range_keep_bytes(z2, left > 8 ? left - 8 : 0u); z3 = range_keep_bytes(z3, left > 12 ? left - 12 : 0u);
        }
        c += (uint32_t)(__popc(z0) + __popc(z1) + __popc(z2) + __popc(z3));
    }
    c = zd::wave_sum(c);
    if (zd::lane_id() == 0) red[zd::wave_id()] = c;
    __syncthreads();
    if (tid == 0) cnt[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// T units -> the range [a, b) of them; every sum saturates by construction
__device__ __forceinline__ void range_units(const ZarcRangeReq &q, uint32_t T, uint32_t &a, uint32_t &b)
{
    if (q.flags & ZARC_RANGE_FROM_END) {
        b = T - (uint32_t)(q.skip < T ? q.skip : T);
        a = b - (uint32_t)(q.take < b ? q.take : b);
    } else {
        a = (uint32_t)(q.skip < T ? q.skip : T);
        b = a + (uint32_t)(q.take < T - a ? q.take : T - a);
    }
}
__device__ __forceinline__ uint64_t range_shfl64(uint64_t v, int src) { return zd::shfl((uint32_t)v, src) | (uint64_t)zd::shfl((uint32_t)(v >> 32), src) << 32; }

__global__ void __launch_bounds__(256) zarc_range_carry(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                        const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                        const int32_t *__restrict__ status, const ZarcRangeReq *__restrict__ req,
                                                        const uint32_t *__restrict__ cnt, ZarcRangeFrame *__restrict__ out, uint32_t *__restrict__ open,
                                                        uint32_t *__restrict__ open_count)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = (uint32_t)zd::lane_id();
    const bool valid = i < n; // (no lane leaves early: the wave works together below)
    ZarcRangeFrame F;
    F.units = F.first = F.taken = 0; F.pos[0] = F.pos[1] = 0; F.slice[0] = F.slice[1] = ZARC_RANGE_NONE; F.ord[0] = F.ord[1] = 0; F.decoded = 0;
    ZarcRangeReq q;
    q.unit = q.flags = 0; q.skip = q.take = 0;
    uint64_t s0 = 0;
    uint32_t ns = 0, len = 0, open_tail = 0;
    bool lines = false;
    if (valid) {
        const int32_t st = status[i];
        F.decoded = st == ZARC_FRAME_OK || st == ZARC_FRAME_DIGEST ? 1u : 0u;
        q = req[i];
        len = (uint32_t)raw_len[i];
        s0 = slice_prefix[i];
        ns = (uint32_t)(slice_prefix[i + 1] - s0);
        lines = F.decoded && q.unit == ZARC_RANGE_LINES && len > 0;
        if (F.decoded && !lines) { // bytes are their own offsets; an empty frame has no unit
            F.units = q.unit == ZARC_RANGE_LINES ? 0u : len;
            uint32_t a, b;
            range_units(q, F.units, a, b);
            F.first = a; F.taken = b - a; F.pos[0] = a; F.pos[1] = b;
        }
        if (lines) open_tail = dec_base[dec_off[i] + len - 1] != 0x0A ? 1u : 0u;
    }
    const bool small = lines && ns <= ZR_LANE_SLICES;
    if (small) {
        uint32_t N = 0;
        for (uint32_t j = 0; j < ns; j++) N += cnt[s0 + j];
        const uint32_t T = N + open_tail;
        uint32_t a, b;
        range_units(q, T, a, b);
        F.units = T; F.first = a; F.taken = b - a;
        for (uint32_t w = 0; w < 2; w++) {
            const uint32_t k = w ? b : a;
            if (k == 0) continue;
            if (k == T) { F.pos[w] = len; continue; }
            uint32_t run = 0;
            for (uint32_t j = 0; j < ns; j++) { // (k <= N here: the k-th 0x0A exists)
                const uint32_t c = cnt[s0 + j];
                if (k <= run + c) { F.slice[w] = (uint32_t)(s0 + j); F.ord[w] = k - run; break; }
                run += c;
            }
        }
    }
    uint64_t big = zd::ballot(lines && !small);
    while (big) { // wave-uniform: the frame of lane `src`, by all 64 lanes
        const int src = zd::ctz64(big);
        big &= big - 1;
        const uint64_t b_s0 = range_shfl64(s0, src);
        const uint32_t b_ns = zd::shfl(ns, src), b_len = zd::shfl(len, src), b_tail = zd::shfl(open_tail, src);
        ZarcRangeReq bq;
        bq.unit = ZARC_RANGE_LINES; bq.flags = zd::shfl(q.flags, src); bq.skip = range_shfl64(q.skip, src); bq.take = range_shfl64(q.take, src);
        const uint32_t *c = cnt + b_s0;
        const uint32_t per = (b_ns + 63) / 64, j0 = lane * per, j1 = j0 + per < b_ns ? j0 + per : b_ns;
        uint32_t mine = 0;
        for (uint32_t j = j0; j < j1; j++) mine += c[j];
        const uint32_t incl = zd::wave_scan_incl(mine);
        const uint32_t T = zd::shfl(incl, 63) + b_tail;
        uint32_t a, b;
        range_units(bq, T, a, b);
        uint32_t pos[2] = {0, 0}, slice[2] = {ZARC_RANGE_NONE, ZARC_RANGE_NONE}, ord[2] = {0, 0};
        for (uint32_t w = 0; w < 2; w++) {
            const uint32_t k = w ? b : a;
            if (k == 0) continue;
            if (k == T) { pos[w] = b_len; continue; }
            const int owner = zd::ctz64(zd::ballot(incl - mine < k && k <= incl)); // the 64th of the frame that holds the k-th 0x0A
            uint32_t run = zd::shfl(incl - mine, owner);
            const uint32_t o0 = (uint32_t)owner * per, o1 = o0 + per < b_ns ? o0 + per : b_ns;
            for (uint32_t base = o0; base < o1; base += 64) {
                const uint32_t j = base + lane;
                const uint32_t v = j < o1 ? c[j] : 0u;
                const uint32_t sc = zd::wave_scan_incl(v);
                const uint64_t hit = zd::ballot(run + sc - v < k && k <= run + sc);
                if (hit) {
                    const int l = zd::ctz64(hit);
                    slice[w] = (uint32_t)b_s0 + base + (uint32_t)l;
                    ord[w] = k - (run + zd::shfl(sc - v, l));
                    break;
                }
                run += zd::shfl(sc, 63);
            }
        }
        if ((int)lane == src) {
            F.units = T; F.first = a; F.taken = b - a;
            F.pos[0] = pos[0]; F.pos[1] = pos[1]; F.slice[0] = slice[0]; F.slice[1] = slice[1]; F.ord[0] = ord[0]; F.ord[1] = ord[1];
        }
    }
    // the open boundaries of the wave: one addition to the list's length per wave; their order in the list decides nothing
    const uint32_t want = (F.slice[0] != ZARC_RANGE_NONE ? 1u : 0u) + (F.slice[1] != ZARC_RANGE_NONE ? 1u : 0u);
    const uint32_t incl = zd::wave_scan_incl(want), total = zd::shfl(incl, 63);
    uint32_t base = 0;
    if (total && lane == 0) base = atomicAdd(open_count, total);
    base = zd::shfl(base, 0);
    if (want) {
        uint32_t at = base + incl - want;
        if (F.slice[0] != ZARC_RANGE_NONE) open[at++] = i * 2;
        if (F.slice[1] != ZARC_RANGE_NONE) open[at] = i * 2 + 1;
    }
    if (valid) out[i] = F;
}

__global__ void __launch_bounds__(256) zarc_range_locate(const uint32_t *__restrict__ open, const uint32_t *__restrict__ open_count,
                                                         const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                         const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len, ZarcRangeFrame *out)
{
    __shared__ uint32_t red[4];
    const uint32_t tid = threadIdx.x, total = *open_count;
    for (uint32_t e = blockIdx.x; e < total; e += gridDim.x) { // (uniform over the workgroup)
        const uint32_t i = open[e] >> 1, w = open[e] & 1u;
        const uint32_t ord = out[i].ord[w];
        const uint64_t at = (out[i].slice[w] - slice_prefix[i]) * (uint64_t)ZARC_CHECK_SLICE;
        const uint64_t len = raw_len[i];
        const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
        const uint4 *a16 = (const uint4 *)(dec_base + dec_off[i] + at);
        uint32_t nw[8], mine = 0; // bit p of the eight words = byte p of the thread's 256 is 0x0A
        for (uint32_t k = 0; k < 8; k++) {
            uint32_t m = 0;
            for (uint32_t hh = 0; hh < 2; hh++) {
                const uint32_t v = tid * 16 + k * 2 + hh, rel = v * 16;
                if (rel >= nbytes) continue;
                const uint4 x = a16[v];
                uint32_t nm = lines_nl4(x.x) | lines_nl4(x.y) << 4 | lines_nl4(x.z) << 8 | lines_nl4(x.w) << 12;
                if (nbytes - rel < 16) nm &= (1u << (nbytes - rel)) - 1u;
                m |= nm << (16 * hh);
            }
            nw[k] = m;
            mine += (uint32_t)__popc(m);
        }
        uint32_t all;
        const uint32_t before = lines_block_excl(mine, red, all);
        if (before < ord && ord <= before + mine) { // this thread holds it
            uint32_t left = ord - before;
            for (uint32_t k = 0; k < 8; k++) {
                const uint32_t pc = (uint32_t)__popc(nw[k]);
                if (left > pc) { left -= pc; continue; }
                uint32_t m = nw[k];
                while (--left) m &= m - 1;
                out[i].pos[w] = (uint32_t)at + tid * 256 + k * 32 + (uint32_t)zd::ctz32(m) + 1; // behind the line feed
                break;
            }
        }
    }
}

__global__ void __launch_bounds__(256) zarc_range_gather(uint32_t m, const uint64_t *__restrict__ block_prefix, const ZarcRangeCopy *__restrict__ plan,
                                                         const uint8_t *__restrict__ dec_base, const uint64_t *__restrict__ dec_off, uint8_t *__restrict__ text)
{
    uint32_t k;
    uint64_t block0;
    if (!lines_locate(m, block_prefix, k, block0)) return;
    const ZarcRangeCopy c = plan[k];
    const uint64_t lo = (blockIdx.x - block0) * (uint64_t)ZARC_CHECK_SLICE;
    if (lo >= c.len) return;
    const uint32_t L = (uint32_t)(c.len - lo > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : c.len - lo), tid = threadIdx.x;
    const uint8_t *s = dec_base + dec_off[c.frame] + c.start + lo;
    uint8_t *d = text + c.dst + lo;
    uint32_t head = (uint32_t)((16 - ((uintptr_t)d & 15)) & 15);
    if (head > L) head = L;
    if (tid < head) d[tid] = s[tid];
    const uint32_t body = (L - head) / 16;
    if ((((uintptr_t)(s + head)) & 15) == 0) {
        for (uint32_t v = tid; v < body; v += 256) *(uint4 *)(d + head + 16 * v) = *(const uint4 *)(s + head + 16 * v);
    } else {
        for (uint32_t v = tid; v < body; v += 256) {
            const uint8_t *p = s + head + 16 * v;
            const uint64_t l8 = zd::load_u64(p), h8 = zd::load_u64(p + 8);
            *(uint4 *)(d + head + 16 * v) = make_uint4((uint32_t)l8, (uint32_t)(l8 >> 32), (uint32_t)h8, (uint32_t)(h8 >> 32));
        }
    }
    const uint32_t done = head + 16 * body;
    if (tid < L - done) d[done + tid] = s[done + tid];
}
