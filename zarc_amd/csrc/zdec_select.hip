// zarc_amd/csrc/zdec_select.hip -- the SELECTED lines of a search (zarc_gpu_select_lines_batch*): grep's -v and -A / -B / -C; included by
// zstd_decode.hip behind zdec_regex.hip.
//
// The kernels of zdec_lines.hip deliver the lines that hold a match.  These deliver S = the lines within `before` in front of and `after`
// behind a HIT line, a hit being a matching line, or with `invert` a line without a match.  Both are decisions behind the two bitmaps of a
// slice (match starts, 0x0A positions), so one tail serves the three matchers; the bitmap builders and the lines_* helpers are those of
// zdec_lines.hip, zdec_search_set.hip and zdec_regex.hip (but lines_walk: see sel_walk).
//
// A line belongs to the slice in which it ENDS -- at its 0x0A, or at the frame's end for an unterminated last line -- and to the thread
// whose 256 positions hold that end.  Whether it is a hit is then known from the slice's own bitmaps and one word carried forwards (the
// lowest match of the line open at the slice's start, which is rec.match as well); its number is nl_base + its rank among the slice's ends.
//
//   zarc_lines_select_mark{,_set,_regex}   the grid of zarc_search_scan.  The bitmaps as zarc_lines_mark* build them, then sel_mark_tail: one
//                      ZarcSelSlice.  The first line that ends in a slice may have begun in an earlier one, so the summary keeps it apart:
//                      hits, first, last and the selected count of all the other ends, and whether that first line matches in this slice.
//   zarc_lines_select_carry   wave per frame, 64 slices a step, three passes over the summaries.  Forwards: the open line's lowest match and
//                      start, nl_base, the first line's verdict, the number of the last hit line in front of a slice.  Backwards: next_end,
//                      the number of the first hit line behind, and from both the slice's selected count in closed form.  Forwards again:
//                      its exclusive prefix; lines[i] = |H|, selected[i] = |S|.  The content is not read to count.
//   -- the host decides what every frame delivers, as for zarc_lines_emit --
//   zarc_lines_select_emit{,_set,_regex}   only slices that deliver rebuild their bitmaps; sel_emit_tail decides every line of a thread's
//                      chunk again, now with the carries as seeds, ranks them by an exclusive scan and writes one ZarcLineRec each.
//   zarc_lines_scan and zarc_lines_gather follow unchanged.
//
// No lane walks more than its own 256 positions, however long a line or a run of context is: what lies in front of and behind a chunk
// comes from ballots, shuffles and workgroup scans.  LDS per workgroup: the bitmaps (2 x 8 KiB) and 32 bytes of scan words, beside what the
// matcher's builder keeps (fixed string: 256 bytes; set: its image; regex: its tables).  No LDS atomic, no scalar memory write.

constexpr uint32_t ZS_VIRT = 8u; // ZarcSelSlice::flags, beside ZL_HEAD / ZL_TAIL / ZL_IN: the frame's unterminated last line ends in this slice

// lines_walk with the word loop unrolled by force and a bit per 0x0A passed in and out: a walker that keeps or reads a bit per line never
// indexes a register array by a position (the compiler answers that with scratch memory; tools/spills.sh shows none for these kernels).
// f.nl(p, has, in) gets bit p of `in` and returns bit p of `out`.
template <class F> __device__ __forceinline__ void sel_walk(const uint32_t *mw, const uint32_t *nw, const uint32_t *in, uint32_t *out, F &f)
{
    bool has = false;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        uint32_t mm = mw[k], nn = nw[k], o = 0;
        const uint32_t iw = in[k];
        for (;;) {
            const uint32_t nb = nn ? (uint32_t)zd::ctz32(nn) : 32u;
            const uint32_t seg = nb < 32 ? mm & ((1u << nb) - 1u) : mm;
            if (seg && !has) { has = true; f.low(k * 32 + (uint32_t)zd::ctz32(seg)); }
            if (nb == 32) break;
            if (f.nl(k * 32 + nb, has, (iw >> nb & 1u) != 0)) o |= 1u << nb;
            has = false;
            const uint32_t keep = nb == 31 ? 0u : ~((2u << nb) - 1u);
            mm &= keep; nn &= keep;
        }
        out[k] = o;
    }
    f.end(has);
}
__device__ __forceinline__ void sel_set_bit(uint32_t *w, uint32_t p, bool on)
{
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) { // (a mask per word, no word picked by the position: the array stays in registers)
        const uint32_t m = j == (p >> 5) ? 1u << (p & 31) : 0u;
        w[j] = on ? w[j] | m : w[j] & ~m;
    }
}

// Every lane either ends a line (reset; val: the lowest match behind its last 0x0A) or lengthens the open one (val: its lowest match), val
// ZL_NONE without one.  -> the lowest match of the line open at the lane's start in front of the lane, `carry` standing in front of lane 0;
// carry becomes what stands in front of the lane behind lane 63.  Positions rise with the lanes: the lowest is the first.
__device__ __forceinline__ uint32_t sel_wave_open(bool reset, uint32_t val, uint32_t &carry)
{
    const uint32_t lane = (uint32_t)zd::lane_id();
    const uint64_t R = zd::ballot(reset), V = zd::ballot(val != ZL_NONE);
    const uint64_t below = (1ull << lane) - 1ull, rb = R & below;
    const uint64_t c = V & (rb ? below & lines_from_top(rb) : below);
    const uint32_t got = zd::shfl(val, c ? zd::ctz64(c) : 0);
    const uint32_t mine = rb ? (c ? got : ZL_NONE) : (carry != ZL_NONE ? carry : (c ? got : ZL_NONE));
    const uint64_t co = V & (R ? lines_from_top(R) : ~0ull);
    const uint32_t top = zd::shfl(val, co ? zd::ctz64(co) : 0);
    carry = R ? (co ? top : ZL_NONE) : (carry != ZL_NONE ? carry : (co ? top : ZL_NONE));
    return mine;
}
// ... over the workgroup's 256 threads, seed standing in front of thread 0.  out: what stands behind thread 255; nl_before: a 0x0A of the
// slice lies in front of the thread.  lds: 8 words.
struct ZsOpen { uint32_t low, out; bool nl_before; };
__device__ __forceinline__ ZsOpen sel_block_open(bool reset, uint32_t val, uint32_t seed, uint32_t *lds)
{
    const uint32_t lane = (uint32_t)zd::lane_id(), wave = (uint32_t)zd::wave_id();
    const uint64_t R = zd::ballot(reset), rb = R & ((1ull << lane) - 1ull);
    uint32_t wc = ZL_NONE;
    const uint32_t local = sel_wave_open(reset, val, wc);
    if (lane == 0) { lds[wave] = R ? 1u : 0u; lds[4 + wave] = wc; }
    __syncthreads();
    uint32_t carry = seed, st = seed;
    bool nlb = false;
    for (uint32_t w = 0; w < 4; w++) {
        if (w == wave) st = carry;
        const uint32_t f = lds[w], v = lds[4 + w];
        if (f) { carry = v; if (w < wave) nlb = true; } else if (carry == ZL_NONE) carry = v;
    }
    __syncthreads();
    ZsOpen r;
    r.low = rb ? local : (st != ZL_NONE ? st : local);
    r.out = carry;
    r.nl_before = nlb || rb != 0;
    return r;
}

// a thread's chunk: its 0x0A bytes, the lowest match in front of the first and behind the last one (no 0x0A: anywhere), and which 0x0A
// end a segment OF THE CHUNK that holds a match.  Positions count from the chunk's first.
struct ZsChunk {
    uint32_t nls = 0, first = ZL_NONE, last = ZL_NONE;
    uint32_t head_low = ZL_NONE, tail_low = ZL_NONE, cur = ZL_NONE;
    uint32_t ml[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    __device__ __forceinline__ void low(uint32_t p) { cur = p; }
    __device__ __forceinline__ bool nl(uint32_t p, bool, bool)
    {
        const bool matched = cur != ZL_NONE;
        if (!nls) { first = p; head_low = cur; }
        last = p; nls++; cur = ZL_NONE;
        return matched; // -> ml
    }
    __device__ __forceinline__ void end(bool) { tail_low = cur; if (!nls) head_low = cur; }
};

// What a thread decides about the lines that end in its chunk.  Numbers are line numbers, or with base 0 ranks in the slice from 1.
struct ZsPick {
    ZsChunk c;
    ZsOpen o;
    uint32_t sw[8];                // the 0x0A that end a selected line
    bool v_own, v_hit, v_sel;      // the frame's unterminated last line ends in this chunk; it is a hit; it is selected
    uint32_t nl_before, total_nl;  // 0x0A of the slice in front of the chunk, in the slice
    uint32_t num0;                 // the number of the first line that ends in the chunk
    uint32_t nhits, nsel, first_hit, last_hit; // of the chunk: counts, and the numbers of its first (ZL_NONE) and last (0) hit line
};

// at: the slice's first position in the frame; last_slice: the frame ends in the slice; seed_low / prev_seed / next_seed: the carries of
// the slices around (mark: ZL_NONE, 0, ZL_NONE); skip_first: the first line that ends in the slice is no hit (mark: the carry judges it).
// Every thread of the workgroup comes here.  lds: 8 words.
__device__ __forceinline__ void sel_pick(const uint32_t *mw, const uint32_t *nw, uint32_t at, uint32_t nbytes, bool last_slice, const ZarcSelect &q,
                                         uint32_t seed_low, uint32_t base, uint32_t prev_seed, uint32_t next_seed, bool skip_first, uint32_t *lds, ZsPick &k)
{
    const uint32_t tid = threadIdx.x;
    ZsChunk &c = k.c;
    uint32_t anym = 0;
    for (uint32_t j = 0; j < 8; j++) anym |= mw[j];
    if (anym) sel_walk(mw, nw, nw, c.ml, c);
    else
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) { // no match in the chunk (nearly every chunk): its 0x0A bytes by words
        if (!nw[j]) continue;
        if (!c.nls) c.first = j * 32 + (uint32_t)zd::ctz32(nw[j]);
        c.last = j * 32 + (uint32_t)zd::hb32(nw[j]);
        c.nls += (uint32_t)__popc(nw[j]);
    }
    k.v_own = last_slice && tid == (nbytes - 1) >> 8 && c.last != ((nbytes - 1) & 255u);
    k.o = sel_block_open(c.nls != 0, c.tail_low != ZL_NONE ? at + tid * 256 + c.tail_low : ZL_NONE, seed_low, lds);
    k.nl_before = lines_block_excl(c.nls, lds, k.total_nl);
    k.num0 = base + k.nl_before + 1;
    // the hit lines: the first line of the chunk may hold its match in front of the chunk
    const bool slice_first = skip_first && !k.o.nl_before;
    uint32_t hw[8];
    if (c.nls && k.o.low != ZL_NONE) sel_set_bit(c.ml, c.first, true);
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) hw[j] = q.invert ? nw[j] & ~c.ml[j] : c.ml[j];
    if (c.nls && slice_first) sel_set_bit(hw, c.first, false);
    const bool v_match = c.nls ? c.tail_low != ZL_NONE : (c.head_low != ZL_NONE || k.o.low != ZL_NONE);
    k.v_hit = k.v_own && v_match != (q.invert != 0) && !(slice_first && !c.nls);
    k.nhits = k.v_hit ? 1u : 0u;
    uint32_t lo_idx = ZL_NONE, hi_idx = 0, seen = 0; // ranks in the chunk of its first and last hit line (hi_idx: + 1)
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        if (hw[j]) {
            k.nhits += (uint32_t)__popc(hw[j]);
            if (lo_idx == ZL_NONE) lo_idx = seen + (uint32_t)__popc(nw[j] & ((1u << zd::ctz32(hw[j])) - 1u));
            const uint32_t hb = (uint32_t)zd::hb32(hw[j]);
            hi_idx = seen + (uint32_t)__popc(nw[j] & ((2u << hb) - 1u)); // (hb == 31: the shift wraps to 0, the mask to all ones)
        }
        seen += (uint32_t)__popc(nw[j]);
    }
    if (k.v_hit) { if (lo_idx == ZL_NONE) lo_idx = c.nls; hi_idx = c.nls + 1; }
    k.first_hit = lo_idx != ZL_NONE ? k.num0 + lo_idx : ZL_NONE;
    k.last_hit = hi_idx ? k.num0 + hi_idx - 1 : 0u;
    uint32_t prev = lines_block_max_before(k.last_hit, lds), next = lines_block_min_after(k.first_hit, lds);
    prev = prev > prev_seed ? prev : prev_seed;
    next = next < next_seed ? next : next_seed;
    // the selected lines: within `after` behind the last hit at or in front of them, or within `before` in front of the next
    k.v_sel = k.v_hit;
    if (q.before == 0 && q.after == 0) {
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) k.sw[j] = hw[j];
    } else {
        uint32_t no = k.num0, last = prev;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            uint32_t nn = nw[j], out = 0;
            while (nn) {
                const uint32_t bit = nn & (0u - nn);
                nn ^= bit;
                if (hw[j] & bit) last = no;
                if (last && no - last <= q.after) out |= bit;
                no++;
            }
            k.sw[j] = out;
        }
        if (k.v_own) { if (k.v_hit) last = no; k.v_sel = last && no - last <= q.after; no++; }
        uint32_t nxt = next;
        if (k.v_own) { no--; if (k.v_hit) nxt = no; if (nxt != ZL_NONE && nxt - no <= q.before) k.v_sel = true; }
#pragma unroll
        for (uint32_t jj = 0; jj < 8; jj++) {
            const uint32_t j = 7 - jj;
            uint32_t nn = nw[j], out = 0;
            while (nn) {
                const uint32_t bit = 1u << zd::hb32(nn);
                nn ^= bit;
                no--;
                if (hw[j] & bit) nxt = no;
                if (nxt != ZL_NONE && nxt - no <= q.before) out |= bit;
            }
            k.sw[j] |= out;
        }
    }
    k.nsel = k.v_sel ? 1u : 0u;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) k.nsel += (uint32_t)__popc(k.sw[j]);
}

// the summary of a slice nothing of which is looked at: an undecoded or empty frame, a matcher that cannot match
__device__ __forceinline__ ZarcSelSlice sel_blank(uint32_t len)
{
    ZarcSelSlice S;
    S.nl_count = 0; S.first_nl = ZL_NONE; S.last_nl = ZL_NONE; S.flags = 0; S.hits = 0; S.first_hit = 0; S.last_hit = 0; S.sel = 0;
    S.tail_low = ZL_NONE; S.open_start = 0; S.open_low = ZL_NONE; S.nl_base = 0; S.prev_hit = 0; S.next_hit = ZL_NONE; S.next_end = len; S.sel_excl = 0;
    return S;
}

// the shared tail of the three mark kernels: bm_match and bm_nl hold the slice's bitmaps (steps rounds of them)
__device__ __forceinline__ void sel_mark_tail(const uint32_t *bm_match, const uint32_t *bm_nl, uint32_t steps, uint32_t at, uint32_t nbytes, uint32_t len,
                                              const ZarcSelect &q, uint32_t *red, ZarcSelSlice *__restrict__ out)
{
    const uint32_t tid = threadIdx.x;
    uint32_t mw[8], nw[8];
    lines_load_chunk(bm_match, bm_nl, steps, mw, nw);
    ZsPick k;
    sel_pick(mw, nw, at, nbytes, at + nbytes == len, q, ZL_NONE, 0, 0, ZL_NONE, true, red, k);
    const ZsChunk &c = k.c;
    uint32_t hits, sel, marks;
    (void)lines_block_excl(k.nhits, red, hits);
    (void)lines_block_excl(k.nsel, red, sel);
    (void)lines_block_excl((c.head_low != ZL_NONE && !k.o.nl_before ? 1u : 0u) | (k.v_own ? 1u << 16 : 0u), red, marks);
    const uint32_t first = lines_block_min_after(c.nls ? tid * 256 + c.first : ZL_NONE, red); // (thread 0 sees every other thread's ...
    const uint32_t last = lines_block_max_before(c.nls ? tid * 256 + c.last + 1 : 0u, red);   //  ... and thread 255 every other's)
    const uint32_t first_hit = lines_block_min_after(k.first_hit, red);
    const uint32_t last_hit = lines_block_max_before(k.last_hit, red);
    if (tid == 255) { red[1] = c.nls ? tid * 256 + c.last + 1 : last; red[2] = k.last_hit ? k.last_hit : last_hit; }
    __syncthreads();
    if (tid == 0) {
        ZarcSelSlice S = sel_blank(len);
        const uint32_t fh = k.first_hit != ZL_NONE ? k.first_hit : first_hit;
        S.nl_count = k.total_nl;
        S.first_nl = c.nls ? c.first : first;
        S.last_nl = red[1] ? red[1] - 1 : ZL_NONE;
        S.flags = ((marks & 0xFFFFu) ? ZL_HEAD : 0u) | (k.o.out != ZL_NONE ? ZL_TAIL : 0u) | ((marks >> 16) ? ZS_VIRT : 0u);
        S.hits = hits; S.first_hit = fh != ZL_NONE ? fh : 0u; S.last_hit = red[2]; S.sel = sel;
        S.tail_low = k.o.out;
        *out = S;
    }
}

__global__ void __launch_bounds__(256) zarc_lines_select_mark(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                              const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                              const int32_t *__restrict__ status, const uint8_t *__restrict__ pattern, uint32_t m, uint32_t icase,
                                                              ZarcSelect q, ZarcSelSlice *__restrict__ slices)
{
    __shared__ uint32_t pat[ZARC_SEARCH_MAX_PATTERN / 4];
    __shared__ uint32_t bm_match[ZARC_CHECK_SLICE / 32], bm_nl[ZARC_CHECK_SLICE / 32];
    __shared__ uint32_t red[8];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const int32_t st = status[i];
    const uint64_t len = raw_len[i];
    const uint64_t at = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    if ((st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) || m == 0 || m > ZARC_SEARCH_MAX_PATTERN || at >= len) { // nothing decoded, or an empty frame: no line
        if (threadIdx.x == 0) slices[blockIdx.x] = sel_blank((uint32_t)len);
        return;
    }
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    const uint64_t starts = len >= m && at <= len - m ? len - m + 1 - at : 0;
    const uint32_t cnt = (uint32_t)(starts > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : starts);
    const uint32_t steps = lines_bitmaps(dec_base + dec_off[i] + at, nbytes, cnt, pattern, m, icase != 0, pat, bm_match, bm_nl);
    sel_mark_tail(bm_match, bm_nl, steps, (uint32_t)at, nbytes, (uint32_t)len, q, red, slices + blockIdx.x);
}

__global__ void __launch_bounds__(256) zarc_lines_select_mark_set(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                                  const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                                  const int32_t *__restrict__ status, ZarcSetDesc sd, const uint32_t *__restrict__ set,
                                                                  uint32_t icase, ZarcSelect q, ZarcSelSlice *__restrict__ slices)
{
    HIP_DYNAMIC_SHARED(uint32_t, img)
    __shared__ uint32_t bm_match[ZARC_CHECK_SLICE / 32], bm_nl[ZARC_CHECK_SLICE / 32];
    __shared__ uint32_t red[8];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const int32_t st = status[i];
    const uint64_t len = raw_len[i];
    const uint64_t at = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    if ((st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) || sd.count == 0 || sd.min_len == 0 || at >= len) {
        if (threadIdx.x == 0) slices[blockIdx.x] = sel_blank((uint32_t)len);
        return;
    }
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    ZsetCtx x;
    x.img = img; x.set = set; x.a = dec_base + dec_off[i] + at; x.room = (uint32_t)(len - at); x.fold = icase != 0; x.hits = nullptr;
    const uint32_t steps = lines_bitmaps_set(sd, x, nbytes, img, bm_match, bm_nl);
    sel_mark_tail(bm_match, bm_nl, steps, (uint32_t)at, nbytes, (uint32_t)len, q, red, slices + blockIdx.x);
}

__global__ void __launch_bounds__(256) zarc_lines_select_mark_regex(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                                    const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                                    const int32_t *__restrict__ status, const ZarcRegexDfa *__restrict__ dfa,
                                                                    const uint8_t *__restrict__ entry, ZarcSelect q, ZarcSelSlice *__restrict__ slices)
{
    ZRE_LDS(L);
    __shared__ uint32_t red[8];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const int32_t st = status[i];
    const uint64_t len = raw_len[i];
    const uint64_t at = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    if ((st != ZARC_FRAME_OK && st != ZARC_FRAME_DIGEST) || at >= len) {
        if (threadIdx.x == 0) slices[blockIdx.x] = sel_blank((uint32_t)len);
        return;
    }
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    const uint32_t steps = regex_bitmaps(L, zre_delta, zre_accept, dfa, dec_base + dec_off[i] + at, nbytes, at == 0, slice_prefix[i + 1] - slice0 > 1, entry);
    sel_mark_tail(bm_match, bm_nl, steps, (uint32_t)at, nbytes, (uint32_t)len, q, red, slices + blockIdx.x);
}

// how many of the lines a .. b lie in lo .. hi (64-bit: no sum of a line number and a context wraps)
__device__ __forceinline__ uint64_t sel_clip(uint64_t a, uint64_t b, uint64_t lo, uint64_t hi)
{
    lo = lo > a ? lo : a; hi = hi < b ? hi : b;
    return hi >= lo ? hi - lo + 1 : 0;
}

// one wave per frame (four frames a workgroup), frames of one slice included
__global__ void __launch_bounds__(256) zarc_lines_select_carry(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint64_t *__restrict__ raw_len, ZarcSelect q,
                                                               ZarcSelSlice *__restrict__ slices, uint32_t *__restrict__ lines, uint32_t *__restrict__ selected)
{
    const uint32_t i = blockIdx.x * 4 + (uint32_t)zd::wave_id(), lane = (uint32_t)zd::lane_id();
    if (i >= n) return;
    const uint64_t s0 = slice_prefix[i];
    const uint32_t ns = (uint32_t)(slice_prefix[i + 1] - s0);
    if (ns == 0) { if (lane == 0) { lines[i] = 0; selected[i] = 0; } return; }
    ZarcSelSlice *S = slices + s0;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t c_low = ZL_NONE, c_open = 0, c_nl = 0, c_hits = 0, c_prev = 0;
    for (uint32_t base = 0; base < ns; base += 64) { // forwards: what lies in front of a slice, and with it the verdict on its first line
        const uint32_t j = base + lane;
        const bool valid = j < ns;
        const uint32_t nlc = valid ? S[j].nl_count : 0u, fl = valid ? S[j].flags : 0u, tail_low = valid ? S[j].tail_low : ZL_NONE;
        const uint32_t hits_r = valid ? S[j].hits : 0u, fh_r = valid ? S[j].first_hit : 0u, lh_r = valid ? S[j].last_hit : 0u, sel_r = valid ? S[j].sel : 0u;
        const uint32_t end_of_last = valid && nlc ? j * ZARC_CHECK_SLICE + S[j].last_nl + 1 : 0u; // where the line open at the slice's end starts
        const bool reset = nlc != 0;
        const uint64_t R = zd::ballot(reset), rb = R & below;
        const uint32_t open_low = sel_wave_open(reset, tail_low, c_low);
        const uint32_t from = zd::shfl(end_of_last, rb ? 63 - __clzll((long long)rb) : 0);
        const uint32_t open = rb ? from : c_open;
        const uint32_t top = zd::shfl(end_of_last, R ? 63 - __clzll((long long)R) : 0);
        c_open = R ? top : c_open;
        const uint32_t ends = nlc + ((fl & ZS_VIRT) ? 1u : 0u);
        const uint32_t nl_incl = zd::wave_scan_incl(nlc), nl_base = c_nl + nl_incl - nlc;
        const bool hit0 = ends && ((fl & ZL_HEAD) || open_low != ZL_NONE) != (q.invert != 0);
        const uint32_t hits = hits_r + (hit0 ? 1u : 0u);
        const uint32_t fh = hit0 ? 1u : fh_r, lh = lh_r ? lh_r : (hit0 ? 1u : 0u);
        uint32_t own = sel_r;
        if (hit0) { // ranks 0 .. after of the slice, but for those the other hits reach already: from their first - before on
            const uint64_t reach = (uint64_t)(q.after < ends - 1 ? q.after : ends - 1) + 1;
            const uint64_t open_ranks = fh_r ? (fh_r - 1 > q.before ? fh_r - 1 - q.before : 0u) : reach;
            own += (uint32_t)(reach < open_ranks ? reach : open_ranks);
        }
        const uint32_t F = hits ? nl_base + fh : 0u, Lh = hits ? nl_base + lh : 0u;
        const uint64_t Hb = zd::ballot(hits != 0), hb = Hb & below;
        const uint32_t pfrom = zd::shfl(Lh, hb ? 63 - __clzll((long long)hb) : 0);
        const uint32_t ptop = zd::shfl(Lh, Hb ? 63 - __clzll((long long)Hb) : 0);
        const uint32_t hits_incl = zd::wave_scan_incl(hits);
        if (valid) {
            S[j].flags = fl | (open_low != ZL_NONE ? ZL_IN : 0u);
            S[j].open_start = open; S[j].open_low = open_low; S[j].nl_base = nl_base;
            S[j].hits = hits; S[j].first_hit = F; S[j].last_hit = Lh; S[j].sel = own;
            S[j].prev_hit = hb ? pfrom : c_prev;
        }
        c_prev = Hb ? ptop : c_prev;
        c_nl += zd::shfl(nl_incl, 63);
        c_hits += zd::shfl(hits_incl, 63);
    }
    uint32_t c_next = (uint32_t)raw_len[i], c_nhit = ZL_NONE;
    for (uint32_t base = (ns - 1) / 64 * 64;; base -= 64) { // backwards: what lies behind a slice, and with it the slice's selected lines
        const uint32_t j = base + lane;
        const bool valid = j < ns;
        const bool has = valid && S[j].nl_count != 0;
        const uint32_t hits = valid ? S[j].hits : 0u, F = valid ? S[j].first_hit : 0u;
        const uint32_t first = has ? j * ZARC_CHECK_SLICE + S[j].first_nl : 0u;
        const uint64_t over = lane == 63 ? 0ull : ~((2ull << lane) - 1ull);
        const uint64_t Fn = zd::ballot(has), above = Fn & over;
        const uint32_t from = zd::shfl(first, above ? zd::ctz64(above) : 0);
        const uint32_t low = zd::shfl(first, Fn ? zd::ctz64(Fn) : 0);
        const uint64_t Hb = zd::ballot(hits != 0), habove = Hb & over;
        const uint32_t hfrom = zd::shfl(F, habove ? zd::ctz64(habove) : 0);
        const uint32_t hlow = zd::shfl(F, Hb ? zd::ctz64(Hb) : 0);
        if (valid) {
            const uint32_t N = habove ? hfrom : c_nhit, P = S[j].prev_hit;
            const uint32_t ends = S[j].nl_count + ((S[j].flags & ZS_VIRT) ? 1u : 0u);
            const uint64_t a = (uint64_t)S[j].nl_base + 1, b = (uint64_t)S[j].nl_base + ends; // the lines that end in the slice (ends == 0: none)
            uint64_t sel = 0;
            if (ends) {
                const uint64_t nlo = N != ZL_NONE ? (N > q.before ? (uint64_t)N - q.before : 0) : ~0ull, phi = P ? (uint64_t)P + q.after : 0;
                if (hits) { // context of the neighbours only below the own hits' reach, and above it
                    const uint64_t Lh = S[j].last_hit;
                    const uint64_t under = F > q.before ? (uint64_t)F - q.before : 0; // the first line the own hits select (0: from the frame's start)
                    sel = S[j].sel;
                    if (P && under > 1) sel += sel_clip(a, b, 0, phi < under - 1 ? phi : under - 1);
                    if (N != ZL_NONE) sel += sel_clip(a, b, nlo > Lh + q.after + 1 ? nlo : Lh + q.after + 1, ~0ull);
                } else {
                    sel = (P ? sel_clip(a, b, 0, phi) : 0) + (N != ZL_NONE ? sel_clip(a, b, nlo, ~0ull) : 0);
                    sel = sel < ends ? sel : ends; // a prefix and a suffix of the slice's lines: their union
                }
            }
            S[j].next_end = above ? from : c_next;
            S[j].next_hit = N;
            S[j].sel = (uint32_t)sel;
        }
        c_next = Fn ? low : c_next;
        c_nhit = Hb ? hlow : c_nhit;
        if (base == 0) break;
    }
    uint32_t c_sel = 0;
    for (uint32_t base = 0; base < ns; base += 64) { // forwards again: the selected lines in front of a slice
        const uint32_t j = base + lane;
        const uint32_t sel = j < ns ? S[j].sel : 0u;
        const uint32_t incl = zd::wave_scan_incl(sel);
        if (j < ns) S[j].sel_excl = c_sel + incl - sel;
        c_sel += zd::shfl(incl, 63);
    }
    if (lane == 0) { lines[i] = c_hits; selected[i] = c_sel; }
}

// the records of a thread's chunk, as the walk meets the lines' ends
struct ZsEmit {
    ZarcLineRec *rec;          // the frame's records
    uint32_t deliver, rank;    // how many of them there are; the rank of the chunk's next selected line
    uint32_t frame, pos0;      // the frame (decoder's order); the chunk's first position in the frame
    uint32_t start;            // where the line open at the walk's position starts
    uint32_t number;           // ... and its number
    uint32_t open_low;         // ... and its lowest match in front of the chunk, or ZL_NONE
    uint32_t len, max_line;
    bool v_sel;
    uint32_t cur = ZL_NONE;
    __device__ __forceinline__ void put(uint32_t end)
    {
        if (rank < deliver) {
            const uint32_t match = open_low != ZL_NONE ? open_low : cur;
            ZarcLineRec r;
            r.frame = frame; r.start = start; r.length = end - start; r.number = number; r.match = match != ZL_NONE ? (uint64_t)match : ~0ull; r.text_off = 0;
            r.text_len = r.length < max_line ? r.length : max_line;
            rec[rank] = r;
        }
        rank++;
    }
    __device__ __forceinline__ void low(uint32_t p) { cur = pos0 + p; }
    __device__ __forceinline__ bool nl(uint32_t p, bool, bool selected)
    {
        if (selected) put(pos0 + p);
        start = pos0 + p + 1; number++; open_low = ZL_NONE; cur = ZL_NONE;
        return false;
    }
    __device__ __forceinline__ void end(bool) { if (v_sel) put(len); }
};

// the shared tail of the three emit kernels
__device__ __forceinline__ void sel_emit_tail(const uint32_t *bm_match, const uint32_t *bm_nl, uint32_t steps, uint32_t frame, uint32_t at, uint32_t nbytes, uint32_t len,
                                              const ZarcSelect &q, const ZarcSelSlice &S, uint32_t want, uint32_t max_line, ZarcLineRec *__restrict__ rec, uint32_t *red)
{
    const uint32_t tid = threadIdx.x;
    uint32_t mw[8], nw[8];
    lines_load_chunk(bm_match, bm_nl, steps, mw, nw);
    ZsPick k;
    sel_pick(mw, nw, at, nbytes, at + nbytes == len, q, S.open_low, S.nl_base, S.prev_hit, S.next_hit, false, red, k);
    uint32_t total;
    const uint32_t rank = S.sel_excl + lines_block_excl(k.nsel, red, total);
    const uint32_t prev_end = lines_block_max_before(k.c.nls ? tid * 256 + k.c.last + 1 : 0u, red); // behind the last 0x0A in front of the chunk
    if (!k.nsel || rank >= want) return;
    ZsEmit e;
    e.rec = rec; e.deliver = want; e.rank = rank; e.frame = frame; e.pos0 = at + tid * 256;
    e.start = prev_end ? at + prev_end : S.open_start;
    e.number = k.num0; e.open_low = k.o.low; e.len = len; e.max_line = max_line; e.v_sel = k.v_own && k.v_sel;
    uint32_t unused[8];
    sel_walk(mw, nw, k.sw, unused, e);
}

__global__ void __launch_bounds__(256) zarc_lines_select_emit(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                              const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                              const uint8_t *__restrict__ pattern, uint32_t m, uint32_t icase, ZarcSelect q,
                                                              const ZarcSelSlice *__restrict__ slices, const uint64_t *__restrict__ rec_base,
                                                              const uint32_t *__restrict__ deliver, uint32_t max_line, ZarcLineRec *__restrict__ rec)
{
    __shared__ uint32_t pat[ZARC_SEARCH_MAX_PATTERN / 4];
    __shared__ uint32_t bm_match[ZARC_CHECK_SLICE / 32], bm_nl[ZARC_CHECK_SLICE / 32];
    __shared__ uint32_t red[8];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const uint32_t want = deliver[i];
    const ZarcSelSlice S = slices[blockIdx.x];
    if (S.sel == 0 || S.sel_excl >= want) return; // nothing of this slice is delivered
    const uint64_t len = raw_len[i];
    const uint64_t at = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    const uint64_t starts = len >= m && at <= len - m ? len - m + 1 - at : 0;
    const uint32_t cnt = (uint32_t)(starts > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : starts);
    const uint32_t steps = lines_bitmaps(dec_base + dec_off[i] + at, nbytes, cnt, pattern, m, icase != 0, pat, bm_match, bm_nl);
    sel_emit_tail(bm_match, bm_nl, steps, i, (uint32_t)at, nbytes, (uint32_t)len, q, S, want, max_line, rec + rec_base[i], red);
}

__global__ void __launch_bounds__(256) zarc_lines_select_emit_set(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                                  const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len, ZarcSetDesc sd,
                                                                  const uint32_t *__restrict__ set, uint32_t icase, ZarcSelect q,
                                                                  const ZarcSelSlice *__restrict__ slices, const uint64_t *__restrict__ rec_base,
                                                                  const uint32_t *__restrict__ deliver, uint32_t max_line, ZarcLineRec *__restrict__ rec)
{
    HIP_DYNAMIC_SHARED(uint32_t, img)
    __shared__ uint32_t bm_match[ZARC_CHECK_SLICE / 32], bm_nl[ZARC_CHECK_SLICE / 32];
    __shared__ uint32_t red[8];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const uint32_t want = deliver[i];
    const ZarcSelSlice S = slices[blockIdx.x];
    if (S.sel == 0 || S.sel_excl >= want) return;
    const uint64_t len = raw_len[i];
    const uint64_t at = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    ZsetCtx x;
    x.img = img; x.set = set; x.a = dec_base + dec_off[i] + at; x.room = (uint32_t)(len - at); x.fold = icase != 0; x.hits = nullptr;
    const uint32_t steps = lines_bitmaps_set(sd, x, nbytes, img, bm_match, bm_nl);
    sel_emit_tail(bm_match, bm_nl, steps, i, (uint32_t)at, nbytes, (uint32_t)len, q, S, want, max_line, rec + rec_base[i], red);
}

__global__ void __launch_bounds__(256) zarc_lines_select_emit_regex(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint8_t *__restrict__ dec_base,
                                                                    const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                                    const ZarcRegexDfa *__restrict__ dfa, const uint8_t *__restrict__ entry, ZarcSelect q,
                                                                    const ZarcSelSlice *__restrict__ slices, const uint64_t *__restrict__ rec_base,
                                                                    const uint32_t *__restrict__ deliver, uint32_t max_line, ZarcLineRec *__restrict__ rec)
{
    ZRE_LDS(L);
    __shared__ uint32_t red[8];
    uint32_t i;
    uint64_t slice0;
    if (!lines_locate(n, slice_prefix, i, slice0)) return;
    const uint32_t want = deliver[i];
    const ZarcSelSlice S = slices[blockIdx.x];
    if (S.sel == 0 || S.sel_excl >= want) return;
    const uint64_t len = raw_len[i];
    const uint64_t at = (blockIdx.x - slice0) * (uint64_t)ZARC_CHECK_SLICE;
    const uint32_t nbytes = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    const uint32_t steps = regex_bitmaps(L, zre_delta, zre_accept, dfa, dec_base + dec_off[i] + at, nbytes, at == 0, slice_prefix[i + 1] - slice0 > 1, entry);
    sel_emit_tail(bm_match, bm_nl, steps, i, (uint32_t)at, nbytes, (uint32_t)len, q, S, want, max_line, rec + rec_base[i], red);
}
