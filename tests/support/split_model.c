/*
 * tests/support/split_model.c -- TEST INFRASTRUCTURE ONLY.
 * A sequential statement of the encoder with ZARC_GPU_PX_BLOCK_SPLIT = 1: the frozen model (oracle/zstd_enc_model.c, included below
 * for its finder, literal / sequence coders and table choices) plus what the switch adds:
 *   split_cuts()              where a 64 KiB parent block is cut into pieces (zge_split.hip: zarc_zge_split)
 *   split_plan_group()        seq_plan_group() walking pieces instead of blocks, with one more rule at the end of a cut parent
 *   zge_split_encode_frame()  the per-piece loop: every piece is coded like a block (own literals section, repeat-offset history
 *                             unknown at its start); a parent whose pieces cost more than one raw block goes out as one raw block
 * With the switch on, emulator and GPU frames are bit-identical to zge_split_encode_frame(); with it off this file is not involved.
 *
 * The cut rule.  A parent's joined sequences are sorted into `chunks` chunks by the source position at which a sequence's literals
 * start (chunk = position / (64 KiB / chunks)); a cut can only fall in front of the first sequence of a chunk.  A run of chunks
 * [i, j) that holds at least one sequence has an estimated cost as one piece, in 1/256 bit:
 *     literals   fewer than 64: raw, 8 bits each.  Otherwise the smaller of raw and
 *                max(n log2 n - sum c log2 c, n) + 8 bits per distinct symbol + 64 bits   (log2 = log2_fp8, the entropy stage's)
 *     overhead   `piece_cost` bytes: block header, the two section headers, table descriptions, up to three lost repeat codes
 * The pieces are the partition of the chunks into such runs of least total cost (dynamic programme over the chunk boundaries; of
 * two candidates of equal cost for best[j] the one whose last piece starts at the earlier boundary wins): exact under the estimate,
 * and a function of the histograms alone.
 */
#include "../../oracle/zstd_enc_model.c"

#define ZGE_SPLIT_K 16             /* zarc_kernels.h: ZGE_SPLIT_K -- chunks, and so the largest number of pieces, of a parent */
#define ZGE_SPLIT_PIECE_COST 192   /* zarc_kernels.h: ZGE_SPLIT_PIECE_COST, bytes */
#define SPLIT_INF 0xFFFFFFFFu

static int g_chunks = ZGE_SPLIT_K, g_piece_cost = ZGE_SPLIT_PIECE_COST;
/* the sweep of EXPERIMENTS.md moves these; the engine has the defaults compiled in */
void split_model_tune(int chunks, int piece_cost) { g_chunks = chunks < 1 ? 1 : (chunks > ZGE_SPLIT_K ? ZGE_SPLIT_K : chunks); g_piece_cost = piece_cost; }

/* cost of the literals whose histogram is hi[] - lo[] (n of them), 1/256 bit; n <= 65536, so everything stays below 2^28 */
static uint32_t split_lit_cost(const uint32_t *lo, const uint32_t *hi, uint32_t n)
{
    uint32_t s, distinct = 0, sum = 0, ent, huf;
    const uint32_t raw = n * 8 * 256;
    if (n < ZGE_MIN_HUF_LITERALS) return raw;
    for (s = 0; s < 256; s++) {
        const uint32_t c = hi[s] - lo[s];
        if (c) { distinct++; sum += c * log2_fp8(c); }
    }
    ent = n * log2_fp8(n) - sum;
    if (ent < n * 256) ent = n * 256; /* a Huffman code spends at least one bit per symbol */
    huf = ent + distinct * 8 * 256 + 64 * 256;
    return huf < raw ? huf : raw;
}

/* seq[]: the parent's joined sequences (ll / ml).  cut[0 .. np] = first sequence of every piece, then nseq; returns np >= 1. */
static int split_cuts(const zge_seq *seq, uint32_t nseq, const uint8_t *lit, uint32_t nlit, uint32_t *cut)
{
    const int C = g_chunks;
    const uint32_t chunk_bytes = ZGE_BLOCK / (uint32_t)C;
    static uint32_t pre[ZGE_SPLIT_K + 1][256];
    uint32_t cb[ZGE_SPLIT_K + 1], lf[ZGE_SPLIT_K + 1], best[ZGE_SPLIT_K + 1], s, pos = 0, lp = 0;
    int from[ZGE_SPLIT_K + 1], bnd[ZGE_SPLIT_K + 1], i, j, q = 0, np = 0;
    cut[0] = 0; cut[1] = nseq;
    if (nseq < 2 || C < 2) return 1;
    cb[0] = 0; lf[0] = 0;
    for (s = 0; s < nseq; s++) {
        int qs = (int)(pos / chunk_bytes);
        if (qs > C - 1) qs = C - 1;
        while (q < qs) { q++; cb[q] = s; lf[q] = lp; }
        lp += seq[s].ll; pos += seq[s].ll + seq[s].ml;
    }
    while (q < C) { q++; cb[q] = nseq; lf[q] = lp; }
    lf[C] = nlit; /* the last piece takes the trailing literals */
    memset(pre[0], 0, sizeof pre[0]);
    for (j = 0; j < C; j++) {
        memcpy(pre[j + 1], pre[j], sizeof pre[0]);
        for (s = lf[j]; s < lf[j + 1]; s++) pre[j + 1][lit[s]]++;
    }
    best[0] = 0; from[0] = 0;
    for (j = 1; j <= C; j++) {
        best[j] = SPLIT_INF; from[j] = 0;
        for (i = 0; i < j; i++) {
            uint32_t t;
            if (best[i] == SPLIT_INF || cb[i] == cb[j]) continue;
            t = best[i] + split_lit_cost(pre[i], pre[j], lf[j] - lf[i]) + (uint32_t)g_piece_cost * 8 * 256;
            if (t < best[j]) { best[j] = t; from[j] = i; }
        }
    }
    for (j = C; j > 0; j = from[j]) bnd[np++] = from[j];
    for (i = 0; i < np; i++) cut[i] = cb[bnd[np - 1 - i]];
    cut[np] = nseq;
    return np;
}

/* seq_plan_group() over the pieces of a group of parents, in frame order.  first[b] = piece b is the first of its parent, multi[b] =
 * its parent has more than one piece.  The one new rule: a cut parent may still go out as ONE raw block (its pieces together cost more
 * than that), and then none of its pieces reaches the decoder -- so behind a cut parent the decoder is known to hold the group's
 * table only if it held it in front of that parent AND holds it behind the parent's last piece. */
static void split_plan_group(seq_plan *pl, int nb, const uint8_t *first, const uint8_t *multi)
{
    int use_group[3] = {0, 0, 0}, have[3] = {0, 0, 0}, entry[3] = {0, 0, 0}, prev_multi = 0, t, b, s;
    seq_table_choice g[3];
    for (t = 0; t < 3; t++) {
        uint32_t sum[64], total = 0;
        uint64_t cost_own = 0, cost_group;
        int np = 0, distinct = 0, last = 0, al;
        memset(sum, 0, sizeof sum);
        memset(&g[t], 0, sizeof g[t]);
        for (b = 0; b < nb; b++) {
            if (!pl[b].active || pl[b].ch[t].mode == 1) continue;
            for (s = 0; s <= SEQ_MAXSYM[t]; s++) sum[s] += pl[b].count[t][s];
            total += pl[b].nseq; cost_own += pl[b].ch[t].cost; np++;
        }
        if (np < 2) continue;
        for (s = 0; s <= SEQ_MAXSYM[t]; s++) if (sum[s]) { distinct++; last = s; }
        al = hb32(total > 1 ? total - 1 : 1) - 2;
        if (al > SEQ_MAX_AL[t]) al = SEQ_MAX_AL[t];
        if (al < 5) al = 5;
        while ((1 << al) < distinct) al++;
        g[t].mode = 2; g[t].nsym = last + 1; g[t].al = al;
        fse_normalize(sum, g[t].nsym, total, al, g[t].norm);
        g[t].desc_len = fse_write_desc(g[t].desc, sizeof g[t].desc, g[t].norm, g[t].nsym, al);
        if (!g[t].desc_len) continue;
        cost_group = dist_cost(sum, g[t].norm, g[t].nsym, al) + (uint64_t)g[t].desc_len * 8 * 256;
        use_group[t] = cost_group <= cost_own + (cost_own >> 6);
    }
    if (!use_group[0] && !use_group[1] && !use_group[2]) return;
    for (b = 0; b < nb; b++) {
        uint64_t ub_bits = 1; /* the end mark */
        size_t ub;
        seq_plan *p = &pl[b];
        if (first[b]) {
            if (prev_multi) for (t = 0; t < 3; t++) have[t] = have[t] && entry[t];
            for (t = 0; t < 3; t++) entry[t] = have[t];
            prev_multi = multi[b];
        }
        if (!p->active) continue;
        for (t = 0; t < 3; t++) {
            seq_table_choice *c = &p->ch[t];
            if (c->mode == 1 || !use_group[t]) continue;
            { const uint8_t rle = c->rle_sym; *c = g[t]; c->rle_sym = rle; }
            if (have[t]) { c->mode = 3; c->desc_len = 0; }
        }
        for (t = 0; t < 3; t++) {
            const seq_table_choice *c = &p->ch[t];
            if (c->mode == 1) continue;
            for (s = 0; s < c->nsym && s <= SEQ_MAXSYM[t]; s++) if (p->count[t][s]) ub_bits += (uint64_t)p->count[t][s] * fse_max_bits(c->norm[s], c->al);
            ub_bits += (uint64_t)c->al;
        }
        ub_bits += p->extra_bits;
        ub = p->lsz + (p->nseq < 128 ? 1 : (p->nseq < 0x7F00 ? 2 : 3)) + 1 + (size_t)((ub_bits + 7) / 8);
        for (t = 0; t < 3; t++) ub += p->ch[t].mode == 1 ? 1 : p->ch[t].desc_len;
        p->guaranteed = ub < p->blen;
        for (t = 0; t < 3; t++) have[t] = (p->ch[t].mode != 1 && use_group[t]) ? p->guaranteed : 0;
    }
}

typedef struct {
    uint32_t s0, ns, l0, nl, src_off, src_len; /* first sequence / literal of the parent's, counts, source range inside the parent */
    int rle;
    uint8_t *blk;
} split_piece;

#define SPLIT_MAX_PIECES (ZGE_TABLE_GROUP * ZGE_SPLIT_K)

/* returns 0, -1 (capacity), -3 (a `guaranteed` size bound was no bound); *n_blocks = Zstandard blocks written */
int zge_split_encode_frame(const zge_params *P_in, const void *src_, size_t n, void *dst_, size_t cap, size_t *out_len, uint32_t *n_blocks)
{
    zge_params Pn = *P_in;
    const zge_params *P = &Pn;
    const uint8_t *src = (const uint8_t *)src_;
    uint8_t *dst = (uint8_t *)dst_;
    size_t pos = 0, bs, gs;
    mf_ctx c;
    zge_seq *gseq[ZGE_TABLE_GROUP];
    uint8_t *lit;
    seq_plan *plans;
    split_piece *pc;
    uint8_t *pfirst, *pmulti;
    uint32_t blocks_out = 0;
    int wlog, single, bad_bound = 0, g, k;
    if (cap < zge_bound(n)) return -1;
    if (n <= (size_t)Pn.far_min_frame) Pn.far_log = 0;
    dst[pos++] = 0x28; dst[pos++] = 0xB5; dst[pos++] = 0x2F; dst[pos++] = 0xFD;
    wlog = P->window_log;
    single = n <= ((size_t)1 << wlog);
    {
        int fcs_flag = n < 256 ? 0 : (n < 65536 + 256 ? 1 : (n <= 0xFFFFFFFFu ? 2 : 3));
        int i, fcs_bytes = fcs_flag == 0 ? (single ? 1 : 0) : (1 << fcs_flag);
        uint64_t v = fcs_flag == 1 ? n - 256 : n;
        dst[pos++] = (uint8_t)((fcs_flag << 6) | (single << 5) | ((P->checksum ? 1 : 0) << 2));
        if (!single) dst[pos++] = (uint8_t)((wlog - 10) << 3);
        for (i = 0; i < fcs_bytes; i++) dst[pos++] = (uint8_t)(v >> (8 * i));
    }
    c.P = P; c.src = src; c.n = n; c.st = NULL; c.cold = 0; c.skip_left = 0; c.erep0 = 0; c.erep1 = 0; c.far_pending = ZGE_NO_TILE;
    c.window = single ? (n ? n : 1) : ((size_t)1 << wlog);
    {
        const size_t fw = P->far_log ? ((size_t)1 << P->far_log) * (size_t)P->far_ways : 1;
        c.fl = (uint32_t *)calloc(fw, 4);
        c.fs = (uint32_t *)calloc(fw, 4);
        c.farc = (uint32_t *)calloc((size_t)P->tile * ZGE_FAR_MAX, 4);
    }
    c.t16 = (uint16_t *)calloc((size_t)1 << P->short_log, 2);
    c.tl = (uint32_t *)calloc((size_t)1 << P->long_log, 4);
    c.ts = (uint32_t *)calloc((size_t)1 << P->short_log, 4);
    c.M = (cand *)calloc((size_t)P->tile, sizeof(cand));
    c.M2 = (cand *)calloc((size_t)P->tile, sizeof(cand));
    c.next = (uint32_t *)calloc((size_t)P->tile, 4);
    c.take = (uint8_t *)calloc((size_t)P->tile, 1);
    c.mark = (uint8_t *)calloc((size_t)P->tile, 1);
    for (g = 0; g < ZGE_TABLE_GROUP; g++) gseq[g] = (zge_seq *)malloc(sizeof(zge_seq) * (ZGE_BLOCK / 3 + 8));
    plans = (seq_plan *)calloc(SPLIT_MAX_PIECES, sizeof *plans);
    pc = (split_piece *)calloc(SPLIT_MAX_PIECES, sizeof *pc);
    pfirst = (uint8_t *)calloc(SPLIT_MAX_PIECES, 1);
    pmulti = (uint8_t *)calloc(SPLIT_MAX_PIECES, 1);
    for (k = 0; k < SPLIT_MAX_PIECES; k++) pc[k].blk = (uint8_t *)malloc(ZGE_BLOCK + 1024);
    lit = (uint8_t *)malloc(ZGE_BLOCK + 64);
    if (n == 0) { dst[pos++] = 1; dst[pos++] = 0; dst[pos++] = 0; blocks_out++; }
    for (gs = 0; gs < n; gs += (size_t)ZGE_TABLE_GROUP * ZGE_BLOCK) {
      int nb = 0, np = 0, pstart[ZGE_TABLE_GROUP + 1];
      /* first pass: match finding, the cuts, and per piece the literals section, code histograms and own table choices */
      for (bs = gs; bs < n && nb < ZGE_TABLE_GROUP; bs += ZGE_BLOCK, nb++) {
        size_t be = bs + ZGE_BLOCK < n ? bs + ZGE_BLOCK : n, blen = be - bs, nlit = 0, i;
        int all_same = 1, cnt;
        uint32_t cut[ZGE_SPLIT_K + 1], nseq, lp = 0, sp = 0, s;
        if (bs > 0 && (bs & (((size_t)1 << P->seg_log) - 1)) == 0) {
            if (P->far_log) {
                c.far_pending = ZGE_NO_TILE;
                memset(c.fl, 0, (sizeof(uint32_t) << P->far_log) * (size_t)P->far_ways);
                memset(c.fs, 0, (sizeof(uint32_t) << P->far_log) * (size_t)P->far_ways);
            }
            memset(c.tl, 0, sizeof(uint32_t) << P->long_log);
            memset(c.ts, 0, sizeof(uint32_t) << P->short_log);
            memset(c.t16, 0, sizeof(uint16_t) << P->short_log);
            if (n > ZGE_SPLIT_MIN) { c.erep0 = c.erep1 = 0; c.cold = 0; c.skip_left = 0; }
        }
        pstart[nb] = np;
        for (i = 1; i < blen; i++) if (src[bs + i] != src[bs]) { all_same = 0; break; }
        if (all_same && blen >= 2) { /* RLE parent: one piece */
            memset(&plans[np], 0, sizeof plans[np]);
            pc[np].rle = 1; pc[np].src_off = 0; pc[np].src_len = (uint32_t)blen; pfirst[np] = 1; pmulti[np] = 0;
            np++;
            continue;
        }
        nseq = matchfind_block(&c, bs, be, gseq[nb], lit, &nlit);
        cnt = split_cuts(gseq[nb], nseq, lit, (uint32_t)nlit, cut);
        s = 0;
        for (k = 0; k < cnt; k++) {
            split_piece *p = &pc[np];
            uint32_t ll = 0, bytes = 0;
            size_t lsz;
            p->rle = 0; p->s0 = cut[k]; p->ns = cut[k + 1] - cut[k]; p->l0 = lp; p->src_off = sp;
            for (; s < cut[k + 1]; s++) { ll += gseq[nb][s].ll; bytes += gseq[nb][s].ll + gseq[nb][s].ml; }
            if (k + 1 == cnt) { ll = (uint32_t)nlit - lp; bytes = (uint32_t)blen - sp; }
            p->nl = ll; p->src_len = bytes;
            lp += ll; sp += bytes;
            if (cnt > 1) resolve_repcodes(gseq[nb] + p->s0, p->ns, NULL); /* the history starts unknown in every piece */
            lsz = encode_literals(lit + p->l0, p->nl, p->blk, ZGE_BLOCK + 1024, NULL);
            seq_plan_block(&plans[np], gseq[nb] + p->s0, p->ns, lsz, p->src_len);
            pfirst[np] = k == 0; pmulti[np] = cnt > 1;
            np++;
        }
      }
      pstart[nb] = np;
      /* frames of one parent block: every piece keeps its own choices (the engine's one-pass entropy stage) */
      if (P->seq_repeat && n > ZGE_BLOCK) split_plan_group(plans, np, pfirst, pmulti);
      /* second pass: the sequences sections; the pieces of a parent, or the parent as one raw block */
      for (g = 0, bs = gs; g < nb; g++, bs += ZGE_BLOCK) {
        const size_t be = bs + ZGE_BLOCK < n ? bs + ZGE_BLOCK : n, blen = be - bs;
        size_t csz[ZGE_SPLIT_K], total = 0;
        uint32_t hdr;
        for (k = pstart[g]; k < pstart[g + 1]; k++) {
            const split_piece *p = &pc[k];
            size_t ssz = 0, z = 0;
            if (!p->rle) {
                const size_t lsz = plans[k].lsz;
                if (lsz) ssz = encode_sequences(gseq[g] + p->s0, plans[k].nseq, p->blk + lsz, ZGE_BLOCK + 1024 - lsz, NULL, &plans[k]);
                z = lsz && ssz ? lsz + ssz : 0;
                if (!(z && z < p->src_len)) z = 0;
                if (plans[k].guaranteed && !z) bad_bound = 1;
            }
            csz[k - pstart[g]] = z;
            total += 3 + (p->rle ? 1 : (z ? z : p->src_len));
        }
        if (total > blen + 3) { /* the pieces cost more than one raw block: the parent is one */
            hdr = (uint32_t)(be == n) | (0u << 1) | ((uint32_t)blen << 3);
            dst[pos++] = (uint8_t)hdr; dst[pos++] = (uint8_t)(hdr >> 8); dst[pos++] = (uint8_t)(hdr >> 16);
            memcpy(dst + pos, src + bs, blen);
            pos += blen; blocks_out++;
            continue;
        }
        for (k = pstart[g]; k < pstart[g + 1]; k++) {
            const split_piece *p = &pc[k];
            const size_t z = csz[k - pstart[g]];
            const uint32_t last = be == n && k + 1 == pstart[g + 1];
            const uint32_t type = p->rle ? 1u : (z ? 2u : 0u);
            hdr = last | (type << 1) | ((uint32_t)(type == 2 ? z : p->src_len) << 3);
            dst[pos++] = (uint8_t)hdr; dst[pos++] = (uint8_t)(hdr >> 8); dst[pos++] = (uint8_t)(hdr >> 16);
            if (type == 1) dst[pos++] = src[bs + p->src_off];
            else if (type == 2) { memcpy(dst + pos, p->blk, z); pos += z; }
            else { memcpy(dst + pos, src + bs + p->src_off, p->src_len); pos += p->src_len; }
            blocks_out++;
        }
      }
    }
    if (P->checksum) {
        uint32_t x = (uint32_t)oracle_xxh64(src, n, 0);
        dst[pos++] = (uint8_t)x; dst[pos++] = (uint8_t)(x >> 8); dst[pos++] = (uint8_t)(x >> 16); dst[pos++] = (uint8_t)(x >> 24);
    }
    free(c.t16); free(c.fl); free(c.fs); free(c.farc); free(c.tl); free(c.ts); free(c.M); free(c.M2); free(c.next); free(c.take); free(c.mark);
    free(lit); free(plans); free(pfirst); free(pmulti);
    for (k = 0; k < SPLIT_MAX_PIECES; k++) free(pc[k].blk);
    free(pc);
    for (g = 0; g < ZGE_TABLE_GROUP; g++) free(gseq[g]);
    *out_len = pos;
    if (n_blocks) *n_blocks = blocks_out;
    return bad_bound ? -3 : 0;
}
