// settile_split.inc -- the merge-path search of one diagonal, the body of
// k_mp_split (settile.hpp) and of k_or_split_batch (sets.hip), included into
// each kernel.  From the kernel:
//   T, Le      : the tile's items; the order, Le::le(A, i, B, j) (TupleLe);
//   A, B       : the sides, na / nb elements (an empty side is never read: its
//                columns may be null);
//   ntiles, t  : the pair's tiles and this 16-lane group's diagonal, t > ntiles
//                searching and storing nothing;
//   grp, gl    : the group's place in its wave (lane >> 4) and the lane's in
//                the group (lane & 15);
//   split      : split[t] = a elements among the first min(t T, n) merged items.
// Every lane of a wave runs it: the ballots are wave-wide, four diagonals a
// wave, 16 per 256-thread workgroup.
// One text, not a __device__ function: as a function (by reference, by value,
// with the order passed as a callable) it left k_mp_split's instruction counts
// but reordered instructions of its keys-only form (DESIGN.md §5.18, §5.14).
    const uint64_t n = na + nb;
    const uint64_t d = t < ntiles ? t * T : n;
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    bool done = t > ntiles || hi <= lo;
    // P(i) = A[i] <= B[d-1-i]: true below the split, false from it
    while (__ballot(!done)) {
        const uint64_t span = hi - lo;
        const bool small = span <= 16;
        const uint64_t c = small ? lo + (uint64_t)gl : lo + ((uint64_t)gl * span) / 16;
        const bool valid = !done && (small ? (uint64_t)gl < span : true);
        const bool p = valid && Le::le(A, c, B, d - 1 - c);
        const unsigned m = (unsigned)((__ballot(p) >> (grp * 16)) & 0xFFFF);
        const unsigned cnt = (unsigned)__popc(m);
        if (!done) {
            if (small) {
                lo += cnt;
                done = true;
            } else {
                const uint64_t nlo = cnt > 0 ? lo + (((uint64_t)(cnt - 1)) * span) / 16 + 1 : lo;
                const uint64_t nhi = cnt < 16 ? lo + ((uint64_t)cnt * span) / 16 : hi;
                lo = nlo;
                hi = nhi;
                done = hi <= lo;
            }
        }
    }
    if (gl == 0 && t <= ntiles) split[t] = lo;
