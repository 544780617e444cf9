// zarc_amd/csrc/zge_repack.hip -- the join of a repack pass (zarc_gpu_repack_batch*); included by zge_assemble.hip.
//
// The decode half of a repack pass leaves everything it knows in the decoder's order (frames sorted by size and density): where each
// frame's bytes lie in the handle's scratch, its verdict, its XXH64.  The encode half wants the pack pass's per-entry arrays, in the
// caller's order.  This kernel is the permutation between the two, made where the arrays are: a batch is a million small entries as
// readily as a few large ones, and the alternative is three arrays down, a host loop and three arrays up per pass.
//
// A lane per frame, a wave per 64 frames: coalesced loads in the decoder's order, one 8-byte store per array at the entry's own index
// (entry_of is a permutation of 0 .. n-1, so no two lanes meet).  A frame without an OK verdict becomes an entry of no bytes; the
// host leaves such entries out of the size order, so no encoder launch sees them.
__global__ void __launch_bounds__(64) zarc_repack_plan(uint32_t n, const uint32_t *__restrict__ entry_of, const int32_t *__restrict__ status,
                                                       const uint64_t *__restrict__ dec_off, const uint64_t *__restrict__ raw_len,
                                                       const uint64_t *__restrict__ dec_xxh, uint64_t *__restrict__ src_off, uint64_t *__restrict__ src_len,
                                                       uint64_t *__restrict__ xxh)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = entry_of[i];
    if (e >= n) return; // (never: the host made the permutation)
    const bool good = status[i] == ZARC_FRAME_OK;
    src_off[e] = good ? dec_off[i] : 0;
    src_len[e] = good ? raw_len[i] : 0;
    xxh[e] = dec_xxh[i]; // the decoder hashes every frame it decodes: frame assembly takes the trailer from here
}
