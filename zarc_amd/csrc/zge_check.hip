// zarc_amd/csrc/zge_check.hip -- read-back check of a pack call (ZARC_GPU_PX_CHECK_FRAMES); included by zge_assemble.hip.
//
// The frames a pack call has just assembled are decoded by the engine's own decoder into scratch, and this kernel compares the
// decoded bytes with the source bytes, exactly.  It is a bandwidth pass: both sides start 16-byte aligned (source offsets are
// ZARC_GPU_ALIGN multiples by contract, the scratch offsets by construction), so every lane loads 16 bytes of each side per step.
//
// One workgroup per (frame, slice of ZARC_CHECK_SLICE bytes): a batch of a few large entries and a batch of a million small ones
// both fill the chip.  slice_prefix[] (decoder order, like every array the decoder made) says which frame a workgroup belongs to.
// A wave that saw a difference sends ONE atomicMin of the lowest differing byte offset to first_bad[frame]; a clean wave sends
// nothing.  Slice 0 also looks at what cannot be seen in the bytes: a decoder status that is not OK (bad at offset 0) and, with the
// checksum flag, the four trailer bytes of the frame against the low half of the XXH64 pack computed from the source.

__global__ void __launch_bounds__(256) zarc_check_compare(uint32_t n, const uint64_t *__restrict__ slice_prefix, const uint32_t *__restrict__ entry_of,
                                                          uint32_t entry0, const uint8_t *__restrict__ dec_base, const uint64_t *__restrict__ dec_off,
                                                          const int32_t *__restrict__ dec_status, const uint8_t *__restrict__ src_base,
                                                          const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ src_len,
                                                          const uint8_t *__restrict__ frame_base, const uint64_t *__restrict__ frame_off,
                                                          const uint64_t *__restrict__ frame_len, const uint64_t *__restrict__ xxh,
                                                          uint32_t *__restrict__ first_bad)
{
    // the frame of this workgroup: the last i with slice_prefix[i] <= blockIdx.x (wave-uniform: scalar loads)
    const uint64_t wg = blockIdx.x;
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (slice_prefix[mid] <= wg) lo = mid; else hi = mid;
    }
    const uint32_t i = lo;
    if (i >= n || wg >= slice_prefix[i + 1]) return;
    const uint32_t e = entry0 + entry_of[i];
    const uint64_t len = src_len[e];
    const uint64_t at = (wg - slice_prefix[i]) * (uint64_t)ZARC_CHECK_SLICE;
    const uint32_t cnt = (uint32_t)(len - at > ZARC_CHECK_SLICE ? ZARC_CHECK_SLICE : len - at);
    const uint8_t *a = dec_base + dec_off[i] + at, *b = src_base + src_off[e] + at;
    const uint32_t tid = threadIdx.x;
    uint32_t bad = ZARC_CHECK_CLEAN;
    if (dec_status[i] != ZARC_FRAME_OK) {
        if (at == 0 && tid == 0) bad = 0; // nothing to compare with: the decoder left the frame where it found the fault
    } else {
        const uint4 *a16 = (const uint4 *)a, *b16 = (const uint4 *)b;
        const uint32_t n16 = cnt / 16;
#pragma unroll 4
        for (uint32_t v = tid; v < n16; v += 256) {
            const uint4 x = a16[v], y = b16[v];
            const uint32_t d0 = x.x ^ y.x, d1 = x.y ^ y.y, d2 = x.z ^ y.z, d3 = x.w ^ y.w;
            if ((d0 | d1 | d2 | d3) && bad == ZARC_CHECK_CLEAN) { // (v grows: the first hit of a lane is its lowest)
                const uint32_t w = d0 ? 0u : (d1 ? 1u : (d2 ? 2u : 3u)), d = d0 ? d0 : (d1 ? d1 : (d2 ? d2 : d3));
                bad = (uint32_t)at + v * 16 + w * 4 + (uint32_t)zd::ctz32(d) / 8;
            }
        }
        // the byte tail (only a frame's last slice has one)
        const uint32_t t = n16 * 16 + tid;
        if (tid < 16 && t < cnt && a[t] != b[t]) { const uint32_t o = (uint32_t)at + t; bad = o < bad ? o : bad; }
        if (at == 0 && tid == 0 && xxh && bad == ZARC_CHECK_CLEAN) {
            const uint64_t fl = frame_len[e];
            if (fl < 4 || zd::load_u32(frame_base + frame_off[e] + fl - 4) != (uint32_t)xxh[e]) bad = ZARC_CHECK_TRAILER;
        }
    }
    if (zd::ballot(bad != ZARC_CHECK_CLEAN) == 0) return; // the common case: nothing leaves the wave
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = zd::shfl_xor(bad, d); bad = o < bad ? o : bad; }
    if (zd::lane_id() == 0) atomicMin(&first_bad[i], bad);
}
