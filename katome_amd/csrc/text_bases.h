// text_bases.h -- what the kernels that write text partitioned by OUTPUT bytes share (collapse.hip: contigs and FASTA; gfa.hip: GFA):
// the workgroup's search in scanned offsets, 16 bases of a 2-bit label as one 128-bit value, a label's checks, decimal digits.
#pragma once
#include "common.h"

namespace katome {

constexpr uint32_t TEXT_ACGT = 0x54474341u;                 // 'A' 'C' 'G' 'T', code 0 in the low byte
constexpr uint32_t TEXT_MAX_LABEL_BYTES = 1u << 29;         // a label of 2^31 bases: its sizes would not fit 32 bits

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t decimal_digits(uint64_t v) {
    uint32_t d = 1;
    for (uint64_t t = 10; v >= t; t *= 10) { ++d; if (d == 20) break; }      // (10^20 does not fit 64 bits)
    return d;
}

// A label in compress_edge format at bytes [lo, hi) of labels that are label_bytes long: 0 = well-formed, with its bases in *bases
// (4 * (bytes - 1) - pad); 1 = offsets, pad byte or length (shorter than k bases) malformed; 2 = more than 2^31 bases.  Nothing is
// read through an offset before it is checked.
__device__ __forceinline__ int label_check(const uint8_t* __restrict__ label, uint64_t lo, uint64_t hi, uint64_t label_bytes, uint32_t k, uint32_t* bases) {
    if (lo >= hi || hi > label_bytes || hi - lo < 2) return 1;
    if (hi - lo - 1 > TEXT_MAX_LABEL_BYTES) return 2;
    const uint32_t pad = label[lo], packed = 4 * (uint32_t)(hi - lo - 1);
    if (pad > 3 || packed < pad + k) return 1;
    *bases = packed - pad;
    return 0;
}

// the largest p < P with off[p] <= target (off ascending, off[0] = 0 <= target): every round the workgroup probes 256 places at once
__device__ __forceinline__ uint32_t workgroup_search(const uint64_t* __restrict__ off, uint32_t P, uint64_t target) {
    uint32_t lo = 0, n = P;
    while (n > 1) {
        const uint32_t step = (n + BLOCK - 1) / BLOCK, at = threadIdx.x * step;
        const int c = __syncthreads_count(at < n && off[lo + at] <= target);         // (a prefix of the threads: thread 0 always)
        lo += (uint32_t)(c - 1) * step;
        n = min(step, n - (uint32_t)(c - 1) * step);
    }
    return lo;
}

// base b of a label's packed bases as its ASCII letter
__device__ __forceinline__ uint32_t one_base(const uint8_t* src, uint32_t b) {
    return (TEXT_ACGT >> (8 * ((src[b >> 2] >> (6 - 2 * (b & 3))) & 3))) & 0xFF;
}

// 16 bases from base b on, as 16 ASCII bytes: the 32 bits are cut out of the two aligned words that hold them (the second one is
// only read where the bits reach into it), first base in the top bits; four codes then select four bytes of "ACGT" at once
__device__ __forceinline__ uint4 sixteen_bases(const uint8_t* src, uint32_t b) {
    const uintptr_t a = (uintptr_t)(src + (b >> 2));
    const uint32_t bit = 2 * (b & 3);
    const uintptr_t a0 = a & ~(uintptr_t)3, a1 = (a + 3 + (bit ? 1 : 0)) & ~(uintptr_t)3;
    const uint32_t hi = __builtin_bswap32(*(const uint32_t*)a0), lo = __builtin_bswap32(*(const uint32_t*)a1);
    const uint32_t s = 8 * (uint32_t)(a - a0) + bit;                         // 0 .. 30
    const uint32_t v = s ? (hi << s) | (lo >> (32 - s)) : hi;                // (s != 0 here means a1 == a0 + 4: the bits reach into it)
    uint32_t out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t c = (v >> (24 - 8 * j)) & 0xFF;
        const uint32_t sel = (c >> 6) | (((c >> 4) & 3) << 8) | (((c >> 2) & 3) << 16) | ((c & 3) << 24);
        out[j] = __builtin_amdgcn_perm(0u, TEXT_ACGT, sel);
    }
    return make_uint4(out[0], out[1], out[2], out[3]);
}
#endif

}  // namespace katome
