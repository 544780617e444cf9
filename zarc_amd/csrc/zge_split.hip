// zarc_amd/csrc/zge_split.hip -- encoder, between the match finder and the entropy stage: where a 64 KiB block is cut (gfx950).
//
// Only launched with ZARC_GPU_PX_BLOCK_SPLIT = 1.  libzstd 1.5 splits a block where its statistics change and gives every part its
// own Huffman table; this kernel makes that decision for the engine's 64 KiB parent blocks.  One wave per parent:
//   1. the parent's sequences are joined (zge_seq_join.h), so that a cut never falls inside one long match;
//   2. the sequences are sorted into ZGE_SPLIT_K chunks by the source position at which their literals start (a prefix sum of the match
//      lengths, 64 sequences per round); a cut can only fall in front of the first sequence of a chunk;
//   3. literal byte histograms per chunk (LDS atomic adds: sums, so their order does not matter), then prefix sums over the chunks --
//      the histogram of any run of chunks is a difference of two rows;
//   4. every run of chunks [i, j) has an estimated cost as one piece, in 1/256 bit (log2_fp8, four symbols per lane, one wave sum):
//      Huffman-coded or raw literals plus ZGE_SPLIT_PIECE_COST bytes of headers, table descriptions and lost repeat codes; the pieces
//      are the partition of least total cost (dynamic programme over the 17 boundaries, 136 runs);
//   5. one record per piece: first sequence / literal / source byte and counts, and where its coded bytes go.
// Everything is a function of the histograms: no result depends on the order in which lanes or atomics run.  The literals are read
// once, the sequences twice.  Bit-identical to tests/support/split_model.c (split_cuts).
// Part of the entropy stage's translation unit: zge_entropy.hip includes this file at its end (it is not compiled on its own) and
// provides log2_fp8, MIN_HUF_LITERALS and the headers, so that the estimate here and the coder there cannot drift apart.

namespace {

constexpr uint32_t K = ZGE_SPLIT_K;
constexpr uint32_t SPLIT_INF = 0xFFFFFFFFu;

struct SplitLds {
    uint32_t pre[K + 1][256]; // pre[j][s]: literals of value s in chunks 0 .. j-1 (row j + 1 first holds chunk j's own histogram)
    uint32_t cb[K + 1], lf[K + 1], sf[K + 1]; // first sequence / literal / source byte of chunk j (entry K: the parent's end)
    uint32_t best[K + 1], from[K + 1], bnd[K + 1];
};

// one piece that is the whole parent
__device__ __forceinline__ void whole_parent(const ZgeBlock &rec, uint32_t nseq, uint32_t slot_bytes, ZgeBlock *pb, ZgePiece *pp, int lane)
{
    if (lane == 0) {
        ZgeBlock r = rec;
        r.nseq = nseq; r.pad = 1;
        pb[0] = r;
        pp[0] = ZgePiece{0, 0, 0, 0, (uint32_t)zge_out_stride(slot_bytes), {0, 0, 0}};
    }
}

} // namespace

__global__ void __launch_bounds__(64) zarc_zge_split(uint32_t n_blocks, uint32_t slot_bytes, const ZgeBlock *__restrict__ blocks, uint64_t *__restrict__ seq_scratch,
                                                     const uint8_t *__restrict__ lit_scratch, ZgeBlock *__restrict__ pblocks, ZgePiece *__restrict__ pieces)
{
    __shared__ SplitLds L;
    const int lane = zd::lane_id();
    const uint32_t bi = blockIdx.x;
    if (bi >= n_blocks) return;
    const ZgeBlock rec = blocks[bi];
    ZgeBlock *const pb = pblocks + (uint64_t)bi * K;
    ZgePiece *const pp = pieces + (uint64_t)bi * K;
    if ((uint32_t)lane < K) { // every slot idle until a piece takes it
        pb[lane] = ZgeBlock{rec.frame, rec.index, 0, 0, 0, ZGE_PIECE_UNUSED, 0, 0};
        pp[lane] = ZgePiece{0, 0, 0, 0, 0, {0, 0, 0}};
    }
    zd::wave_sync_global();
    uint64_t *const seq = seq_scratch + (uint64_t)bi * zge_seq_stride(slot_bytes);
    const uint8_t *const lit = lit_scratch + (uint64_t)bi * zge_lit_stride(slot_bytes);
    uint32_t nseq = rec.nseq;
    if (rec.type == 1 || nseq < 2) { whole_parent(rec, nseq, slot_bytes, pb, pp, lane); return; } // RLE parent, or nothing to cut between
    nseq = zge_join_sequences(seq, nseq, lane);
    zd::wave_sync_global();
    if (nseq < 2) { whole_parent(rec, nseq, slot_bytes, pb, pp, lane); return; }
    const uint32_t nlit = rec.nlit, src_len = rec.src_len, chunk_bytes = ZARC_BLOCK / K;

    // ---- chunk boundaries: chunk of a sequence = source position of its first literal / chunk_bytes
    if (lane == 0) { L.cb[0] = 0; L.lf[0] = 0; L.sf[0] = 0; }
    uint32_t c_lp = 0, c_ml = 0, c_q = 0; // literal position / sum of match lengths / chunk carried over from the previous round
    for (uint32_t base = 0; base < nseq; base += 64) {
        const uint32_t cnt = nseq - base < 64 ? nseq - base : 64;
        const bool valid = (uint32_t)lane < cnt;
        const uint64_t s = valid ? seq[base + (uint32_t)lane] : 0;
        const uint32_t lp = zge_seq_ll(s), ml = valid ? zge_seq_ml(s) : 0u; // lp: literals up to and including this sequence's
        uint32_t plp = zd::shfl_up1(lp);
        if (lane == 0) plp = c_lp;
        const uint32_t mls = zd::wave_scan_incl(ml);
        const uint32_t pos = plp + c_ml + mls - ml; // where this sequence's literals start in the parent
        uint32_t q = pos / chunk_bytes;
        if (q > K - 1) q = K - 1;
        if (!valid) q = 0;
        uint32_t pq = zd::shfl_up1(q);
        if (lane == 0) pq = c_q;
        if (valid) for (uint32_t j = pq + 1; j <= q; j++) { L.cb[j] = base + (uint32_t)lane; L.lf[j] = plp; L.sf[j] = pos; } // positions rise: every j has one writer
        c_lp = zd::readlane(lp, cnt - 1); c_ml += zd::readlane(mls, cnt - 1); c_q = zd::readlane(q, cnt - 1);
    }
    if ((uint32_t)lane > c_q && (uint32_t)lane <= K) { L.cb[lane] = nseq; L.lf[lane] = c_lp; L.sf[lane] = c_lp + c_ml; }
    zd::wave_sync();
    if (lane == 0) { L.lf[K] = nlit; L.sf[K] = src_len; } // the last piece takes the trailing literals
    for (uint32_t i = (uint32_t)lane; i < (K + 1) * 256; i += 64) (&L.pre[0][0])[i] = 0;
    zd::wave_sync();

    // ---- literal histograms per chunk, four bytes per load; a literal's chunk = the number of boundaries 1 .. K-1 at or below it
    {
        uint32_t lfs[K]; // lfs[j] = first literal of chunk j, wave-uniform
#pragma unroll
        for (uint32_t j = 1; j < K; j++) lfs[j] = zd::uniform(L.lf[j]);
        const uint32_t n4 = nlit / 4;
        for (uint32_t i0 = 0; i0 < n4; i0 += 64) {
            const uint32_t i = i0 + (uint32_t)lane;
            if (i >= n4) continue;
            const uint32_t w = zd::load_u32(lit + 4 * (uint64_t)i);
            uint32_t qa = 0, qb = 0;
#pragma unroll
            for (uint32_t j = 1; j < K; j++) { qa += lfs[j] <= 4 * i ? 1u : 0u; qb += lfs[j] <= 4 * i + 3 ? 1u : 0u; }
            if (qa == qb) {
                uint32_t *row = L.pre[qa + 1];
                atomicAdd(&row[w & 0xFF], 1u); atomicAdd(&row[(w >> 8) & 0xFF], 1u); atomicAdd(&row[(w >> 16) & 0xFF], 1u); atomicAdd(&row[w >> 24], 1u);
            } else {
                for (uint32_t b = 0; b < 4; b++) {
                    uint32_t qq = 0;
#pragma unroll
                    for (uint32_t j = 1; j < K; j++) qq += lfs[j] <= 4 * i + b ? 1u : 0u;
                    atomicAdd(&L.pre[qq + 1][(w >> (8 * b)) & 0xFF], 1u);
                }
            }
        }
        const uint32_t p = n4 * 4 + (uint32_t)lane;
        if (p < nlit) {
            uint32_t qq = 0;
#pragma unroll
            for (uint32_t j = 1; j < K; j++) qq += lfs[j] <= p ? 1u : 0u;
            atomicAdd(&L.pre[qq + 1][lit[p]], 1u);
        }
    }
    zd::wave_sync();
    // prefix sums over the chunks: symbol r * 64 + lane, row by row (conflict-free: consecutive lanes, consecutive banks)
#pragma unroll
    for (int r = 0; r < 4; r++) {
        uint32_t run = 0;
        for (uint32_t j = 1; j <= K; j++) { run += L.pre[j][r * 64 + lane]; L.pre[j][r * 64 + lane] = run; }
    }
    zd::wave_sync();

    // ---- the partition of least estimated cost (every lane carries the same scalars; lane 0 keeps the tables)
    if (lane == 0) { L.best[0] = 0; L.from[0] = 0; }
    zd::wave_sync();
    for (uint32_t j = 1; j <= K; j++) {
        uint32_t bj = SPLIT_INF, fj = 0;
        const uint32_t cbj = L.cb[j], lfj = L.lf[j];
        for (uint32_t i = 0; i < j; i++) {
            const uint32_t bi_ = L.best[i];
            if (bi_ == SPLIT_INF || L.cb[i] == cbj) continue; // uniform: no partition ends at i, or the run holds no sequence
            const uint32_t n = lfj - L.lf[i];
            uint32_t cost = n * 8 * 256; // raw; n <= 65 536: below 2^28
            if (n >= MIN_HUF_LITERALS) {
                uint32_t sum = 0, distinct = 0;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const uint32_t c = L.pre[j][r * 64 + lane] - L.pre[i][r * 64 + lane];
                    sum += c ? c * log2_fp8(c) : 0u;
                    distinct += (uint32_t)__popcll(zd::ballot(c != 0));
                }
                sum = zd::readlane(zd::wave_scan_incl(sum), 63); // (six data-parallel adds: no LDS round trips)
                uint32_t ent = n * log2_fp8(n) - sum;
                if (ent < n * 256) ent = n * 256; // a Huffman code spends at least one bit per symbol
                const uint32_t huf = ent + distinct * 8 * 256 + 64 * 256;
                if (huf < cost) cost = huf;
            }
            const uint32_t t = bi_ + cost + ZGE_SPLIT_PIECE_COST * 8 * 256;
            if (t < bj) { bj = t; fj = i; }
        }
        zd::wave_sync();
        if (lane == 0) { L.best[j] = bj; L.from[j] = fj; }
        zd::wave_sync();
    }
    uint32_t np = 0;
    for (uint32_t j = K; j > 0; j = L.from[j]) { if (lane == 0) L.bnd[np] = L.from[j]; np++; } // the pieces' first chunks, last piece first
    zd::wave_sync();
    if (np == 1) { whole_parent(rec, nseq, slot_bytes, pb, pp, lane); return; }
    if ((uint32_t)lane < np) {
        const uint32_t k = (uint32_t)lane, i = L.bnd[np - 1 - k], j = k + 1 < np ? L.bnd[np - 2 - k] : K;
        pb[k] = ZgeBlock{rec.frame, rec.index, L.sf[j] - L.sf[i], L.cb[j] - L.cb[i], L.lf[j] - L.lf[i], 2u, 0u, k == 0 ? np : 0u};
        pp[k] = ZgePiece{L.cb[i], L.lf[i], L.sf[i], L.sf[i] + 64 * k, L.sf[j] - L.sf[i] + 64, {0, 0, 0}};
    }
}
