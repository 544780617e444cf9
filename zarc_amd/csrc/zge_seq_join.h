// zarc_amd/csrc/zge_seq_join.h -- joining the pieces of one long match (encoder; model: merge_sequences).
#pragma once
#include "zarc_device.h"
#include "zarc_kernels.h"

// A sequence without literals that continues its predecessor at the same offset (the finder caps a match at 256 bytes per position and
// at its tile's overrun window) is added to the predecessor's length, so match lengths reach the format's 131 074.  Whole wave, 64
// sequences per round, compacted in place: a head's length is a difference of the round's prefix sums; the last head of a round stays
// pending in scalar registers because its run may go on in the next round.  Returns the number of sequences left; the caller fences
// (wave_sync_global) before other lanes read seq[].  Joining what is joined already changes nothing, so the cut decision
// (zge_split.hip) and the entropy stage behind it both call this.
__device__ __forceinline__ uint32_t zge_join_sequences(uint64_t *seq, uint32_t nseq, int lane)
{
    const uint64_t lt = (1ull << lane) - 1;
    uint32_t out = 0;                       // heads so far, including the pending one
    uint32_t pend_lp = 0, pend_ml = 0, pend_o = 0, c_lp = 0, c_o = 0; // pending head; literal position / offset of the previous round's last sequence
    bool have_pend = false;
    uint64_t s_next = (uint32_t)lane < nseq ? seq[lane] : 0; // every pass over the sequences requests its next round before it works on this one
    for (uint32_t base = 0; base < nseq; base += 64) {
        const uint32_t cnt = nseq - base < 64 ? nseq - base : 64;
        const bool valid = (uint32_t)lane < cnt;
        const uint64_t s = valid ? s_next : 0;
        if (base + 64 + (uint32_t)lane < nseq) s_next = seq[base + 64 + (uint32_t)lane]; // (this round stores below base + 64 only)
        const uint32_t lp = zge_seq_ll(s), ml = valid ? zge_seq_ml(s) : 0u, o = zge_seq_ofv(s);
        uint32_t plp = zd::shfl_up1(lp), po = zd::shfl_up1(o);
        if (lane == 0) { plp = c_lp; po = c_o; }
        const bool cont = valid && (base + (uint32_t)lane) > 0 && lp == plp && o == po;
        const uint64_t hm = zd::ballot(valid && !cont);
        const uint32_t psum = zd::wave_scan_incl(ml); // inclusive prefix sums of the match lengths
        const uint32_t first = hm ? (uint32_t)zd::ctz64(hm) : cnt; // lanes before the first head continue the pending head
        if (first > 0) pend_ml += zd::readlane(psum, first - 1);
        if (hm) {
            if (have_pend && lane == 0) seq[out - 1] = zge_pack_seq(pend_lp, pend_ml, pend_o);
            const uint32_t nh = (uint32_t)__popcll(hm), last = 63u - (uint32_t)__clzll((long long)hm);
            // my run ends in front of the next head (or with the round)
            const uint64_t above = lane == 63 ? 0ull : (hm >> (lane + 1)) << (lane + 1);
            const uint32_t stop = above ? (uint32_t)zd::ctz64(above) : cnt;  // first lane that is not mine
            const uint32_t run = zd::shfl(psum, (int)stop - 1) - psum + ml;
            const uint32_t rank = (uint32_t)__popcll(hm & lt);
            if (((hm >> lane) & 1) && (uint32_t)lane != last) seq[out + rank] = zge_pack_seq(lp, run, o);
            pend_lp = zd::readlane(lp, last); pend_ml = zd::readlane(run, last); pend_o = zd::readlane(o, last);
            have_pend = true;
            out += nh;
        }
        c_lp = zd::readlane(lp, cnt - 1); c_o = zd::readlane(o, cnt - 1);
    }
    if (have_pend && lane == 0) seq[out - 1] = zge_pack_seq(pend_lp, pend_ml, pend_o);
    return out;
}
