// seq_pair.h -- the two first-seen sequence numbers of a record cut from variable-length reads.  One device function for the
// two kernels that need them: the table's insert (table.hip, the batch's own records) and the sharded build's sender, which
// resolves them before its records leave for their owners (dist.hip, var_pairs_kernel).
#pragma once
#include "common.h"

namespace katome {

// Record g of a batch of variable-length reads: read r is the one with rec_prefix[r] <= g < rec_prefix[r + 1].  Its forward
// windows take 2 * win_prefix[r] + [0, W) after seq_base, the windows of its reverse complement the next W (pt_graph.rs:282-308).
// mode 0: the record is window j of the read; 1: whole tile j of `span` windows; 2: window j after the read's last whole tile.
// P: the number of the record as cut (its first window), Q: that of its reverse complement.
// (var_pair_in_read: the same for a caller that has found the read `lo` itself -- keep_var_kernel runs the searches of a thread's
// records side by side)
__device__ __forceinline__ void var_pair_in_read(const u64* __restrict__ win_prefix, const u64* __restrict__ rec_prefix, u64 lo,
                                                 u32 mode, u32 span, u64 seq_base, u64 g, u64& P, u64& Q) {
    const u64 w0 = win_prefix[lo], W = win_prefix[lo + 1] - w0, j = g - rec_prefix[lo];
    const u64 i0 = mode == 1 ? j * span : mode == 2 ? (W / span) * span + j : j;
    const u64 width = mode == 1 ? span : 1;
    P = seq_base + 2 * w0 + i0; Q = seq_base + 2 * w0 + 2 * W - i0 - width;
}
__device__ __forceinline__ void var_seq_pair(const u64* __restrict__ win_prefix, const u64* __restrict__ rec_prefix, u64 n_reads,
                                             u32 mode, u32 span, u64 seq_base, u64 g, u64& P, u64& Q) {
    u64 lo = 0, hi = n_reads;
    while (hi - lo > 1) { const u64 mid = (lo + hi) >> 1; if (rec_prefix[mid] <= g) lo = mid; else hi = mid; }
    var_pair_in_read(win_prefix, rec_prefix, lo, mode, span, seq_base, g, P, Q);
}

}  // namespace katome
