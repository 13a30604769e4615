// sets.hip -- LWW-Element-Set and OR-Set merge.
//
// Build-defined semantics (no reference code), tie rule from the reference:
// on an exactly equal timestamp the local/left value is kept (main.go:54-65).
// Inputs A (local) and B (remote) are SoA tuples (key u64, ts u64, rep u32,
// tomb u8) sorted ascending by (key, ts, rep).  The merged order is the
// STABLE merge: on an equal tuple A's element precedes B's.
//   LWW    : one output per distinct key = the first element (in merged
//            order) carrying the key's maximal (ts, rep); tombstoned winners
//            are kept (they are state).
//   OR-Set : one output per distinct tag (key, ts, rep); tomb = OR over the
//            tag's elements.
//
// GPU structure: two passes over merge-order bitmaps, no cross-workgroup
// waiting:
//   split  : merge-path splits of every tile (k_mp_split of settile.hpp:
//            16-ary searches, four tile diagonals per wave);
//   count  : per tile the merge in LDS -> two bitmaps in merge order (`isa`:
//            the item is an A element; `emit`: the item is an output) and the
//            tile's output count;
//   scan   : one workgroup turns the counts into output offsets;
//   write  : per part of a tile, the runs staged in LDS by LDS-DMA, every
//            index a prefix popcount of the bitmaps, outputs stored at their
//            rank.
// The tiles run in chunks of at most 16384 (one scan workgroup each): chunk
// c's count, scan and write pass in turn on the context's stream.  (Smaller
// chunks, so that the keys the count pass read were still in the Infinity
// Cache for the write pass, and a second stream running chunk c+1's count
// beside chunk c's write, measured slower: DESIGN.md §5.4.1.  So did one
// pass with a decoupled look-back, §5.4.4.)
// The lengths' checks, the workspace (TileWs), the split and its search are
// settile.hpp's, shared with the set-state ops; both modes run through one
// host driver (merge_two_pass).  The count, scan and write kernels are this
// file's own, and their text is kept as it is: their instructions are the
// measured ones.
#include <algorithm>
#include <atomic>

#include "scan.hpp"
#include "settile.hpp"

namespace crdt {

struct Tag {
    uint64_t k, t;
    uint32_t r;
};
__device__ __forceinline__ bool tag_le(const Tag &a, const Tag &b) {
    if (a.k != b.k) return a.k < b.k;
    if (a.t != b.t) return a.t < b.t;
    return a.r <= b.r;
}
__device__ __forceinline__ bool tag_eq(const Tag &a, const Tag &b) {
    return a.k == b.k && a.t == b.t && a.r == b.r;
}
// Field-wise select (a ternary on Tag objects lowers to a scratch alloca).
__device__ __forceinline__ Tag tag_sel(bool c, const Tag &x, const Tag &y) {
    return Tag{c ? x.k : y.k, c ? x.t : y.t, c ? x.r : y.r};
}
__device__ __forceinline__ Tag gtag(const crdt_tuples &s, size_t i) { return Tag{s.key[i], s.ts[i], s.rep[i]}; }

// A write pass derives every staged run and index from its tile's bitmaps
// (lane w < nw holds word w of each): they must set no bit at or past the
// tile's n items and hold exactly na A items.  Wave-uniform.
__device__ __forceinline__ bool bitmaps_consistent(uint64_t word_a, uint64_t word_e, uint32_t pre_a, int nw,
                                                   uint32_t na, uint32_t n, int lane) {
    const uint32_t lo = 64u * (uint32_t)lane;
    const uint64_t valid = lane >= nw || lo >= n ? 0ull : (n - lo >= 64u ? ~0ull : (1ull << (n - lo)) - 1);
    const bool bad = ((word_a | word_e) & ~valid) != 0;
    // (readlane: scalar, no LDS round trip in front of the staging loads)
    const uint32_t tot_a = (uint32_t)__builtin_amdgcn_readlane((int)(pre_a + (uint32_t)__popcll(word_a)), 63);
    return __ballot(bad) == 0 && tot_a == na;
}

// ---------------------------------------------------------------- LWW by key runs
// LWW needs no tag-ordered merge: its output is one tuple per distinct key,
// in key order, and a key's winner depends only on the END of the key's run
// on each side -- A's run ends at its max (ts, rep) tag, B's likewise; the
// larger tag wins, A on an equal tag (left / local wins, main.go:54-65), and
// the winner's tomb is that of the FIRST copy of its tag on its side (the
// first element in the stable merged order carrying the key's max tag).  So
// the merge runs over KEYS only (A first on an equal key), and only the run
// ends' ts / rep / tomb are ever read:
//   k_mp_split  : merge-path splits of 4096-item tiles over the keys
//                 (settile.hpp, TupleLe<true>);
//   k_lww_count : per tile, the keys staged in LDS by LDS-DMA and merged
//                 (512 threads x 8 items): bitmap `isa` (merge item is an A
//                 element) and `emit` (its key differs from the next merged
//                 key: the last element of the key's merged run -- B's run
//                 end when B holds the key, else A's), 512 B per tile, and
//                 the tile's emit count;
//   k_chunk_scan: the counts of a chunk of tiles -> output offsets;
//   k_lww_write : per quarter tile the runs staged in LDS; an emitting
//                 item's A / B index and output rank are prefix popcounts
//                 of the bitmaps; a B run end looks at A's element just
//                 before it in merged order, picks the winner, steps back
//                 over equal-tag copies for the first one's tomb, and stores
//                 at its rank (consecutive across the emitting lanes).
constexpr int LT = 4096;                 // merge items per LWW tile
constexpr int LCB = 512;                 // count pass threads (8 items each)
constexpr int LNW = LT / 64;             // bitmap words per tile and bitmap
constexpr uint32_t kScanMax = 16384;     // tiles per chunk (one scan workgroup)

// the scaffold's tile count is for 2048-item tiles: LWW's are twice that
struct LwwTiles {
    static __device__ __forceinline__ uint64_t tiles(uint64_t na, uint64_t nb) { return (na + nb + LT - 1) / LT; }
};

// Tile t of TT merge items out of n: A's run [i0, i1) and B's [j0, j1) from the splits.
struct MergeTile {
    size_t i0, i1, j0, j1;
    uint32_t na, nb, n;
};
template <int TT>
__device__ __forceinline__ MergeTile merge_tile(const uint64_t *__restrict__ split, uint64_t t, size_t n) {
    MergeTile b;
    const size_t d0 = (size_t)t * TT, d1 = d0 + TT < n ? d0 + TT : n;
    b.i0 = split[t];
    b.i1 = split[t + 1];
    b.j0 = d0 - b.i0;
    b.j1 = d1 - b.i1;
    b.na = (uint32_t)(b.i1 - b.i0);
    b.nb = (uint32_t)(b.j1 - b.j0);
    b.n = b.na + b.nb;
    return b;
}

__global__ __launch_bounds__(LCB) void k_lww_count(const uint64_t *__restrict__ ka, const uint64_t *__restrict__ kb,
                                                   size_t na, size_t nb, const uint64_t *__restrict__ split,
                                                   uint32_t *__restrict__ tcnt, uint64_t *__restrict__ bits,
                                                   uint64_t t0) {
    constexpr int NI = LT / LCB, LPW = 64 / NI;
    __shared__ alignas(16) uint64_t sk[LT + 8];          // A's run, then B's, each from its 16-byte aligned-down start
    __shared__ uint32_t s_w[LCB / 64];
    const uint64_t t = t0 + blockIdx.x;
    const MergeTile b = merge_tile<LT>(split, t, na + nb);
    const int lane0 = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t at = 0;
    const int oa = dma_run<uint64_t, LCB / 64>(ka, b.i0, b.na, sk, &at, wv, lane0);
    const int ob = dma_run<uint64_t, LCB / 64>(kb, b.j0, b.nb, sk, &at, wv, lane0);
    // the keys after the tile: the next merged key past its last item
    const bool ha_next = b.i1 < na, hb_next = b.j1 < nb;
    const uint64_t ka_next = ha_next ? ka[b.i1] : 0, kb_next = hb_next ? kb[b.j1] : 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA has landed in LDS
    __syncthreads();
    const uint64_t *SA = sk + oa, *SB = sk + ob;
    const uint32_t k0 = threadIdx.x * NI < b.n ? threadIdx.x * NI : b.n;
    const uint32_t k1 = k0 + NI < b.n ? k0 + NI : b.n;
    uint32_t isa = 0, emit = 0;
    if (k0 < k1) {
        uint32_t lo = k0 > b.nb ? k0 - b.nb : 0, hi = k0 < b.na ? k0 : b.na;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (SA[mid] <= SB[k0 - 1 - mid]) lo = mid + 1;
            else hi = mid;
        }
        uint32_t ia = lo, ib = k0 - lo;
        uint64_t ha = ia < b.na ? SA[ia] : 0, hb = ib < b.nb ? SB[ib] : 0;
        uint64_t prev = 0;
        for (uint32_t i = 0; i < k1 - k0; ++i) {
            const bool take_a = ia < b.na && (ib >= b.nb || ha <= hb);
            const uint64_t key = take_a ? ha : hb;
            if (i > 0 && key != prev) emit |= 1u << (i - 1);
            prev = key;
            if (take_a) {
                isa |= 1u << i;
                ++ia;
                if (ia < b.na) ha = SA[ia];
            } else {
                ++ib;
                if (ib < b.nb) hb = SB[ib];
            }
        }
        // the item after the thread's last one: the merge's next head, or
        // past the tile the first of A[i1] / B[j1] (A first on an equal key)
        bool has_next;
        uint64_t nk;
        if (ia < b.na || ib < b.nb) {
            has_next = true;
            nk = (ia < b.na && (ib >= b.nb || ha <= hb)) ? ha : hb;
        } else {
            has_next = ha_next || hb_next;
            nk = (ha_next && (!hb_next || ka_next <= kb_next)) ? ka_next : kb_next;
        }
        if (!has_next || nk != prev) emit |= 1u << (k1 - k0 - 1);
    }
    const int lane = threadIdx.x & 63, sh = (lane % LPW) * NI;
    uint64_t wl = (uint64_t)isa << sh, we = (uint64_t)emit << sh;
#pragma unroll
    for (int o = 1; o < LPW; o <<= 1) {
        wl |= (uint64_t)__shfl_xor((unsigned long long)wl, o);
        we |= (uint64_t)__shfl_xor((unsigned long long)we, o);
    }
    if (lane % LPW == 0) {
        const uint32_t w = threadIdx.x / LPW;
        bits[t * 2 * LNW + w] = wl;
        bits[t * 2 * LNW + LNW + w] = we;
    }
    uint32_t x = (uint32_t)__popc(emit);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if (lane == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int k = 0; k < LCB / 64; ++k) tot += s_w[k];
        tcnt[t] = tot;
    }
}

// Exclusive scan of the n <= kScanMax tile counts of one chunk (tiles t0 ..
// t0 + n) by one workgroup, on top of the offset the previous chunk's scan
// left at ic[t0] (0 for t0 == 0); ic[t0 + n] = the running total, also
// written to *count when count != nullptr.  Over 8k counts, striped rows
// (scan.hpp wg_scan_rows, every access coalesced): 11.7 -> 8.4 us at 9.8k
// tiles; up to 8k a contiguous run per thread in registers is quicker (4.7
// us at 4.9k; striped ~7-10 us at that size).  (16 coalesced rows per wave
// with a serial carry: 11.9 / 12.0 us.)
__global__ __launch_bounds__(1024) void k_chunk_scan(const uint32_t *__restrict__ tcnt, uint64_t t0, uint32_t n,
                                                     uint64_t *__restrict__ ic, uint64_t *__restrict__ count) {
    __shared__ uint64_t s_pre[16 * 16 + 1];
    __shared__ uint64_t s_w[16];
    static_assert(kScanMax <= 16 * 1024, "striped rows: 16 per thread");
    const uint64_t base = t0 ? ic[t0] : 0;               // (read before any thread rewrites ic[t0]: the
    const uint32_t *tc = tcnt + t0;                      //  scan's first barrier lies between)
    uint64_t *o = ic + t0;
    uint64_t tot = 0;
    if (n > 8u * 1024) {                                 // (uniform) striped rows
        tot = wg_scan_rows<1024, 16, uint32_t>([&](uint32_t i) { return tc[i]; }, n,
                                               [&](uint32_t i, uint64_t x) { o[i] = base + x; }, s_pre);
    } else {                                             // <= 8 counts per thread: a contiguous run each
        const uint32_t per = (n + 1023) / 1024;
        const uint32_t b = threadIdx.x * per < n ? threadIdx.x * per : n;
        const uint32_t e = b + per < n ? b + per : n;
        uint32_t v[8];
        uint64_t sum = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            v[k] = b + k < e ? tc[b + k] : 0u;
            sum += v[k];
        }
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        uint64_t x = sum;
#pragma unroll
        for (int o2 = 1; o2 < 64; o2 <<= 1) {
            const uint64_t y = __shfl_up(x, o2);
            if (lane >= o2) x += y;
        }
        if (lane == 63) s_w[w] = x;
        __syncthreads();
        uint64_t run = base + x - sum;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            run += k < w ? s_w[k] : 0;
            tot += s_w[k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (b + k < e) o[b + k] = run;
            run += v[k];
        }
    }
    if (threadIdx.x == 0) {
        o[n] = base + tot;
        if (count) *count = base + tot;
    }
}

// the first element of a side's run of equal tags ending at index w
__device__ __forceinline__ size_t first_copy(const uint64_t *sk, const uint64_t *st, const uint32_t *sr, size_t w,
                                             uint64_t k, uint64_t ts, uint32_t r) {
    while (w > 0 && sk[w - 1] == k && st[w - 1] == ts && sr[w - 1] == r) --w;
    return w;
}

// k_lww_write: one workgroup per part of a tile (1/P of its 4096 merge
// items, sets.lww_parts).  The part's A run and B run (plus the two A
// elements and the one B element before them) are staged in LDS by LDS-DMA
// -- every field of every input element is read once, in order; per-lane
// gathers of the run ends kept the vector-memory address pipe saturated
// (185 us, 52 % of wave time in issue stalls; a shuffle-window variant
// 216-224 us).  Then, per emitting item, X / Y / their predecessors come
// from LDS.
constexpr int LWH = 2048;                // merge items per write workgroup (template default)
constexpr int LWT = 512;                 // its threads (4 items each)

// WH merge items per workgroup (a 1/P of a tile, P = LT / WH), WT threads
template <int WH = LWH, int WT = LWT>
__global__ __launch_bounds__(WT) void k_lww_write(crdt_tuples A, crdt_tuples B, size_t na, size_t nb,
                                                  const uint64_t *__restrict__ split,
                                                  const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ic,
                                                  crdt_tuples out, uint64_t t0, uint32_t *__restrict__ err) {
    constexpr bool SRC = false;                          // (sets_lww_write.inc: no source indices)
    constexpr int64_t *src = nullptr;
#include "sets_lww_write.inc"
}

// k_lww_write that also stores every output's source index (crdt_lww_merge_src)
template <int WH = LWH, int WT = LWT>
__global__ __launch_bounds__(WT) void k_lww_write_src(crdt_tuples A, crdt_tuples B, size_t na, size_t nb,
                                                      const uint64_t *__restrict__ split,
                                                      const uint64_t *__restrict__ bits,
                                                      const uint64_t *__restrict__ ic, crdt_tuples out,
                                                      int64_t *__restrict__ src, uint64_t t0,
                                                      uint32_t *__restrict__ err) {
    constexpr bool SRC = true;
#include "sets_lww_write.inc"
}

// ---------------------------------------------------------------- OR-Set, two passes
// The same structure for the OR-Set, over TAGS: one output per distinct tag
// (key, ts, rep) in tag order, its tomb the OR over every copy; in the
// stable merge (A first on an equal tag) a tag's copies are consecutive --
// A's, then B's -- so the first copy emits:
//   k_mp_split : merge-path splits of 2048-item tiles over the tags
//                (settile.hpp, TupleLe<false>);
//   k_or_count_dma : per tile the tags merged in LDS (512 threads x 4 items):
//                bitmaps `isa` and `emit` (the item's tag differs from the
//                previous merged tag), 512 B per tile, the emit count;
//   k_chunk_scan;
//   k_or_write : per part of a tile (sets.or_parts), the part's A and B runs
//                staged in LDS by LDS-DMA (every field once); an emitting
//                item ORs the tombs of its tag's copies -- forward over A's,
//                then B's from the B position of the item -- and stores at
//                its rank.
constexpr int OT = 2048;                 // merge items per OR tile
constexpr int OCB = 512;                 // count pass threads (4 items each; 256 x 8: 120 us, 1024 x 2: 153 us, against 111)
constexpr int OWT = 512;                 // write pass threads (4 items each)
constexpr int ONW = OT / 64;             // bitmap words per tile and bitmap

// The count pass.  The tile's key / ts / rep are staged in LDS, each side's
// run from the element before the tile (the first item's merged predecessor
// candidate): element x of the tile's A run (x >= -1) is at field index
// oa_f + x, B's at ob_f + x.
//   DMA (sets.or_count_dma, the default): by LDS-DMA, each run from its
//       16-byte aligned-down start, the element before it only when there is
//       one: no VGPR round trip;
//   else: through registers, A[i0-1], A's run, B[j0-1], B's run at slots 0 ..
//       (a missing predecessor staged as 0, never used).
// One merge, the same bitmaps.
template <int NT, bool DMA>
__global__ __launch_bounds__(NT) void k_or_count_dma(crdt_tuples A, crdt_tuples B, size_t na, size_t nb,
                                                     const uint64_t *__restrict__ split, uint32_t *__restrict__ tcnt,
                                                     uint64_t *__restrict__ bits, uint64_t t0) {
    constexpr int NI = OT / NT, LPW = 64 / NI, CAP = OT + 2;
    __shared__ alignas(16) uint64_t sk[CAP + 8], st[CAP + 8];
    __shared__ alignas(16) uint32_t sr[CAP + 16];
    __shared__ uint32_t s_w[NT / 64];
    const uint64_t t = t0 + blockIdx.x;
    const MergeTile b = merge_tile<OT>(split, t, na + nb);
    int oa_k, ob_k, oa_t, ob_t, oa_r, ob_r;
    if constexpr (DMA) {
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), ln = threadIdx.x & 63;
        const uint32_t pa = b.i0 > 0 ? 1u : 0u, pb = b.j0 > 0 ? 1u : 0u;
        uint32_t at = 0;
        oa_k = dma_run<uint64_t, NT / 64>(A.key, b.i0 - pa, b.na + pa, sk, &at, wv, ln) + (int)pa;
        ob_k = dma_run<uint64_t, NT / 64>(B.key, b.j0 - pb, b.nb + pb, sk, &at, wv, ln) + (int)pb;
        at = 0;
        oa_t = dma_run<uint64_t, NT / 64>(A.ts, b.i0 - pa, b.na + pa, st, &at, wv, ln) + (int)pa;
        ob_t = dma_run<uint64_t, NT / 64>(B.ts, b.j0 - pb, b.nb + pb, st, &at, wv, ln) + (int)pb;
        at = 0;
        oa_r = dma_run<uint32_t, NT / 64>(A.rep, b.i0 - pa, b.na + pa, sr, &at, wv, ln) + (int)pa;
        ob_r = dma_run<uint32_t, NT / 64>(B.rep, b.j0 - pb, b.nb + pb, sr, &at, wv, ln) + (int)pb;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA has landed in LDS
    } else {
        const uint32_t nsa = b.na + 1, nst = nsa + b.nb + 1;
        uint64_t k[NI + 1], ts[NI + 1];
        uint32_t r[NI + 1];
#pragma unroll
        for (int j = 0; j <= NI; ++j) {                  // every staging load issued before the first store
            const uint32_t x = threadIdx.x + (uint32_t)j * NT;
            const bool on_a = x < nsa;
            const size_t g = on_a ? b.i0 - 1 + x : b.j0 - 1 + (x - nsa);
            const bool v = x < nst && (on_a ? b.i0 + x >= 1 : b.j0 + (x - nsa) >= 1);
            k[j] = v ? (on_a ? A.key : B.key)[g] : 0;
            ts[j] = v ? (on_a ? A.ts : B.ts)[g] : 0;
            r[j] = v ? (on_a ? A.rep : B.rep)[g] : 0;
        }
#pragma unroll
        for (int j = 0; j <= NI; ++j) {
            const uint32_t x = threadIdx.x + (uint32_t)j * NT;
            if (x < nst) {
                sk[x] = k[j];
                st[x] = ts[j];
                sr[x] = r[j];
            }
        }
        oa_k = oa_t = oa_r = 1;
        ob_k = ob_t = ob_r = (int)nsa + 1;
    }
    __syncthreads();
#define OA(x) Tag{sk[oa_k + (int)(x)], st[oa_t + (int)(x)], sr[oa_r + (int)(x)]}
#define OB(x) Tag{sk[ob_k + (int)(x)], st[ob_t + (int)(x)], sr[ob_r + (int)(x)]}
    const uint32_t k0 = threadIdx.x * NI < b.n ? threadIdx.x * NI : b.n;
    const uint32_t k1 = k0 + NI < b.n ? k0 + NI : b.n;
    uint32_t isa = 0, emit = 0;
    if (k0 < k1) {
        uint32_t lo = k0 > b.nb ? k0 - b.nb : 0, hi = k0 < b.na ? k0 : b.na;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            const uint64_t ka = sk[oa_k + (int)mid], kb = sk[ob_k + (int)(k0 - 1 - mid)];
            const bool le = ka != kb ? ka < kb : tag_le(OA(mid), OB(k0 - 1 - mid));
            if (le) lo = mid + 1;
            else hi = mid;
        }
        uint32_t ia = lo, ib = k0 - lo;
        // the merged predecessor of item k0: the later of A[ia-1], B[ib-1]
        // (A first on an equal tag), each possibly the element before the tile
        const bool hpa = b.i0 + ia > 0, hpb = b.j0 + ib > 0;
        const Tag qa = hpa ? OA((int)ia - 1) : Tag{0, 0, 0}, qb = hpb ? OB((int)ib - 1) : Tag{0, 0, 0};
        bool has_prev = hpa || hpb;
        Tag prev = tag_sel(hpa && hpb ? tag_le(qa, qb) : !hpa, qb, qa);
        Tag ha = ia < b.na ? OA(ia) : Tag{0, 0, 0}, hb = ib < b.nb ? OB(ib) : Tag{0, 0, 0};
        for (uint32_t i = 0; i < k1 - k0; ++i) {
            const bool take_a = ia < b.na && (ib >= b.nb || tag_le(ha, hb));
            const Tag cur = tag_sel(take_a, ha, hb);
            if (!has_prev || !tag_eq(prev, cur)) emit |= 1u << i;
            prev = cur;
            has_prev = true;
            if (take_a) {
                isa |= 1u << i;
                ++ia;
                if (ia < b.na) ha = OA(ia);
            } else {
                ++ib;
                if (ib < b.nb) hb = OB(ib);
            }
        }
    }
#undef OA
#undef OB
    const int lane = threadIdx.x & 63, sh = (lane % LPW) * NI;
    uint64_t wl = (uint64_t)isa << sh, we = (uint64_t)emit << sh;
#pragma unroll
    for (int o = 1; o < LPW; o <<= 1) {
        wl |= (uint64_t)__shfl_xor((unsigned long long)wl, o);
        we |= (uint64_t)__shfl_xor((unsigned long long)we, o);
    }
    if (lane % LPW == 0) {
        const uint32_t w = threadIdx.x / LPW;
        bits[t * 2 * ONW + w] = wl;
        bits[t * 2 * ONW + ONW + w] = we;
    }
    uint32_t x = (uint32_t)__popc(emit);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if (lane == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) tot += s_w[k];
        tcnt[t] = tot;
    }
}

// WH merge items per workgroup (a 1/P of a tile, P = OT / WH), WT threads
template <int WH = OT, int WT = OWT>
__global__ __launch_bounds__(WT) void k_or_write(crdt_tuples A, crdt_tuples B, size_t na, size_t nb,
                                                 const uint64_t *__restrict__ split,
                                                 const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ic,
                                                 crdt_tuples out, uint64_t t0, uint32_t *__restrict__ err) {
    constexpr bool SRC = false;                          // (sets_or_write.inc: no source indices)
    constexpr int64_t *src = nullptr;
#include "sets_or_write.inc"
}

// k_or_write that also stores every output's source index (crdt_orset_merge_src)
template <int WH = OT, int WT = OWT>
__global__ __launch_bounds__(WT) void k_or_write_src(crdt_tuples A, crdt_tuples B, size_t na, size_t nb,
                                                     const uint64_t *__restrict__ split,
                                                     const uint64_t *__restrict__ bits,
                                                     const uint64_t *__restrict__ ic, crdt_tuples out,
                                                     int64_t *__restrict__ src, uint64_t t0,
                                                     uint32_t *__restrict__ err) {
    constexpr bool SRC = true;
#include "sets_or_write.inc"
}

// The chunked two-pass schedule.  count(t0, n, s) / scan(t0, n, count_out,
// s) / write(t0, n, s) enqueue one chunk's pass on the context's stream; a
// chunk is at most kScanMax tiles (one scan workgroup), or `chunk` tiles
// (sets.lww_chunk / sets.or_chunk, diagnostic build: smaller chunks measured
// slower; so did a second stream for the counts).
template <class CountF, class ScanF, class WriteF>
static int two_pass(crdt_ctx *ctx, size_t ntiles, uint64_t *out_count, CountF count, ScanF scan, WriteF write,
                    size_t chunk, bool fail_bits, uint64_t *bits, size_t bits_bytes) {
    if (chunk == 0 || chunk > kScanMax) chunk = kScanMax;
    const hipStream_t s = ctx->stream;
    if (fail_bits) {                                     // failpoint: one chunk, bitmaps zeroed before the writes
        for (size_t t0 = 0; t0 < ntiles; t0 += chunk) {
            const uint32_t n = (uint32_t)std::min(chunk, ntiles - t0);
            count(t0, n, s);
            scan(t0, n, t0 + n == ntiles ? out_count : nullptr, s);
        }
        hipError_t e = hipMemsetAsync(bits, 0, bits_bytes, s);
        if (e != hipSuccess) return hip_fail(ctx, e);
        for (size_t t0 = 0; t0 < ntiles; t0 += chunk) write(t0, (uint32_t)std::min(chunk, ntiles - t0), s);
        return check_launch(ctx);
    }
    for (size_t t0 = 0; t0 < ntiles; t0 += chunk) {
        const uint32_t n = (uint32_t)std::min(chunk, ntiles - t0);
        count(t0, n, s);
        scan(t0, n, t0 + n == ntiles ? out_count : nullptr, s);
        write(t0, n, s);
    }
    return check_launch(ctx);
}

// What the passes of one merge call take (src != nullptr: the _src write
// kernels, every output's source index beside it).
struct MergeCall {
    crdt_tuples A, B, O;
    size_t na, nb;
    int64_t *src;
    uint32_t *err;
    TileWs w;
};

// The two modes of the two-pass merge.  A mode gives its tile (kT merge items,
// kNW words per bitmap), the split's order and tile count, its chunk knob, and
// the count and write launches of the tiles t0 .. t0 + nt.  A write pass takes
// 1/P of a tile per workgroup (sets.lww_parts / sets.or_parts), 4 items per thread.
struct LwwMode {
    static constexpr int kT = LT, kNW = LNW;
    using Le = TupleLe<true>;
    using Tiles = LwwTiles;
    static size_t chunk() { return (size_t)g_lww_chunk; }
    static void count(const MergeCall &m, size_t t0, uint32_t nt, hipStream_t s) {
        k_lww_count<<<nt, LCB, 0, s>>>(m.A.key, m.B.key, m.na, m.nb, m.w.split, m.w.tcnt, m.w.bits, t0);
    }
    template <int WH, int WT>
    static void part(const MergeCall &m, size_t t0, unsigned g, hipStream_t s) {
        if (m.src)
            k_lww_write_src<WH, WT><<<g, WT, 0, s>>>(m.A, m.B, m.na, m.nb, m.w.split, m.w.bits, m.w.ic, m.O, m.src, t0,
                                                     m.err);
        else k_lww_write<WH, WT><<<g, WT, 0, s>>>(m.A, m.B, m.na, m.nb, m.w.split, m.w.bits, m.w.ic, m.O, t0, m.err);
    }
    static void write(const MergeCall &m, size_t t0, uint32_t nt, hipStream_t s) {
        const unsigned P = (unsigned)g_lww_parts, g = P * nt;
        if (P == 2) part<2048, 512>(m, t0, g, s);
        else if (P == 8) part<512, 128>(m, t0, g, s);
        else if (P == 16) part<256, 64>(m, t0, g, s);
        else part<1024, 256>(m, t0, g, s);
    }
};

struct OrMode {
    static constexpr int kT = OT, kNW = ONW;
    using Le = TupleLe<false>;
    using Tiles = PlainTiles;
    static size_t chunk() { return (size_t)g_or_chunk; }
    static void count(const MergeCall &m, size_t t0, uint32_t nt, hipStream_t s) {
        if (g_or_count_dma)
            k_or_count_dma<OCB, true><<<nt, OCB, 0, s>>>(m.A, m.B, m.na, m.nb, m.w.split, m.w.tcnt, m.w.bits, t0);
        else k_or_count_dma<OCB, false><<<nt, OCB, 0, s>>>(m.A, m.B, m.na, m.nb, m.w.split, m.w.tcnt, m.w.bits, t0);
    }
    template <int WH, int WT>
    static void part(const MergeCall &m, size_t t0, unsigned g, hipStream_t s) {
        if (m.src)
            k_or_write_src<WH, WT><<<g, WT, 0, s>>>(m.A, m.B, m.na, m.nb, m.w.split, m.w.bits, m.w.ic, m.O, m.src, t0,
                                                    m.err);
        else k_or_write<WH, WT><<<g, WT, 0, s>>>(m.A, m.B, m.na, m.nb, m.w.split, m.w.bits, m.w.ic, m.O, t0, m.err);
    }
    static void write(const MergeCall &m, size_t t0, uint32_t nt, hipStream_t s) {
        const unsigned P = (unsigned)g_or_parts, g = P * nt;
        if (P == 2) part<1024, 256>(m, t0, g, s);
        else if (P == 4) part<512, 128>(m, t0, g, s);
        else part<2048, 512>(m, t0, g, s);
    }
};
static_assert(OT == kTile, "PlainTiles counts the OR-Set's tiles");

// One merge: the splits of every tile, then the chunked count / scan / write.
// (An empty side's columns are null: never dereferenced.)
template <class M>
static int merge_two_pass(crdt_ctx *ctx, const crdt_tuples &A, size_t na, const crdt_tuples &B, size_t nb,
                          const crdt_tuples &O, int64_t *src, uint64_t *out_count) {
    const size_t n = na + nb;
    const size_t ntiles = (n + M::kT - 1) / M::kT;
    if (ntiles >= 0x7fffffffULL || n >= (1ULL << 62)) return CRDT_E_RANGE;
    MergeCall m{A, B, O, na, nb, src, ctx->dev_status, {}};
    const int rc = m.w.reserve(ctx, ntiles, true, false, 2 * M::kNW);
    if (rc) return rc;
    k_mp_split<M::kT, typename M::Le, typename M::Tiles>
        <<<mp_split_grid(ntiles), 256, 0, ctx->stream>>>(A, na, nullptr, B, nb, nullptr, m.w.split);
    auto cnt = [&](size_t t0, uint32_t nt, hipStream_t s) { M::count(m, t0, nt, s); };
    auto scn = [&](size_t t0, uint32_t nt, uint64_t *c, hipStream_t s) {
        k_chunk_scan<<<1, 1024, 0, s>>>(m.w.tcnt, t0, nt, m.w.ic, c);
    };
    auto wr = [&](size_t t0, uint32_t nt, hipStream_t s) { M::write(m, t0, nt, s); };
    return two_pass(ctx, ntiles, out_count, cnt, scn, wr, M::chunk(), take_fail_zero_bits(), m.w.bits,
                    ntiles * 2 * M::kNW * 8);
}

// ---------------------------------------------------------------- stable merge (no dedup)
// out = the stable merge of A and B (every tuple kept; on an equal tag A's
// copies first) -- the rank-order merge of the runs a key-range owner
// receives in crdt_shard_*_merge_local.  Its length is na + nb, known on the
// host, so a tree of these merges needs no read-back between levels.  Tiles
// of OT merge items from k_mp_split; per tile both runs staged in LDS, every
// item's output position = its index in its run + its rank in the other run
// (B elements strictly below an A tag, A elements at or below a B tag).
template <int NT>
__device__ __forceinline__ void tmerge_tile(const crdt_tuples &A, const crdt_tuples &B, size_t na, size_t nb,
                                            const uint64_t *__restrict__ split, const crdt_tuples &out, uint64_t t,
                                            uint64_t *sk, uint64_t *st, uint32_t *sr, uint8_t *sm) {
    // both runs staged in LDS (A at slots [0, na), B at [na, n)); thread k
    // merges items [k NI, (k+1) NI) of the tile after a merge-path search
    // of its diagonal (A first on an equal tag), the merged tuples are put
    // back into LDS in merged order, then stored coalesced.  (Round 4's form
    // -- every item binary-searched its rank in the other run, ~11 dependent
    // 3-field LDS compares per item -- ran at ~1.6 TB/s.)
    constexpr int NI = OT / NT;
    const MergeTile b = merge_tile<OT>(split, t, na + nb);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const uint32_t x = threadIdx.x + (uint32_t)j * NT;
        if (x >= b.n) continue;
        const bool on_a = x < b.na;
        const size_t g = on_a ? b.i0 + x : b.j0 + (x - b.na);
        const crdt_tuples &S = on_a ? A : B;
        sk[x] = S.key[g];
        st[x] = S.ts[g];
        sr[x] = S.rep[g];
        sm[x] = S.tomb[g];
    }
    __syncthreads();
    auto tg = [&](uint32_t x) { return Tag{sk[x], st[x], sr[x]}; };
    const uint32_t k0 = threadIdx.x * NI < b.n ? threadIdx.x * NI : b.n;
    const uint32_t k1 = k0 + NI < b.n ? k0 + NI : b.n;
    uint64_t ok[NI], ot[NI];
    uint32_t orr[NI];
    uint8_t om[NI];
    {
        uint32_t lo = k0 > b.nb ? k0 - b.nb : 0, hi = k0 < b.na ? k0 : b.na;
        while (lo < hi) {                                // P(i) = A[i] <= B[k0-1-i]: true below the split
            const uint32_t mid = (lo + hi) >> 1;
            if (tag_le(tg(mid), tg(b.na + (k0 - 1 - mid)))) lo = mid + 1;
            else hi = mid;
        }
        uint32_t ia = lo, ib = k0 - lo;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            if ((uint32_t)j >= k1 - k0) break;
            const bool take_a = ia < b.na && (ib >= b.nb || tag_le(tg(ia), tg(b.na + ib)));
            const uint32_t x = take_a ? ia : b.na + ib;
            ok[j] = sk[x];
            ot[j] = st[x];
            orr[j] = sr[x];
            om[j] = sm[x];
            ia += take_a ? 1u : 0u;
            ib += take_a ? 0u : 1u;
        }
    }
    __syncthreads();                                     // every staged input read
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        if ((uint32_t)j >= k1 - k0) break;
        const uint32_t x = k0 + (uint32_t)j;
        sk[x] = ok[j];
        st[x] = ot[j];
        sr[x] = orr[j];
        sm[x] = om[j];
    }
    __syncthreads();
    const size_t o0 = (size_t)t * OT;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const uint32_t x = threadIdx.x + (uint32_t)j * NT;
        if (x >= b.n) continue;
        out.key[o0 + x] = sk[x];
        out.ts[o0 + x] = st[x];
        out.rep[o0 + x] = sr[x];
        out.tomb[o0 + x] = sm[x];
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_tmerge(crdt_tuples A, crdt_tuples B, size_t na, size_t nb,
                                               const uint64_t *__restrict__ split, crdt_tuples out) {
    __shared__ uint64_t sk[OT], st[OT];
    __shared__ uint32_t sr[OT];
    __shared__ uint8_t sm[OT];
    tmerge_tile<NT>(A, B, na, nb, split, out, blockIdx.x, sk, st, sr, sm);
}

// Up to kMergeBatch independent stable merges in ONE split launch and ONE
// merge launch (a level of the key-range owner's rank-order merge tree, both
// sides: crdt_shard_*_merge_local).  Pair p's tiles are tile0[p] ..
// tile0[p+1]; its split entries (ntiles_p + 1 of them) start at tile0[p] + p.
// (One crdt_tuples_merge per pair paid ~27 us of fixed split + merge latency
// each: 112 of them per distributed set merge at R = 8.)
constexpr int kMergeBatch = 16;
struct MergeBatch {
    crdt_tuples A[kMergeBatch], B[kMergeBatch], O[kMergeBatch];
    uint64_t na[kMergeBatch], nb[kMergeBatch];
    uint32_t tile0[kMergeBatch + 1];
    uint32_t np;
};

__device__ __forceinline__ uint32_t batch_pair(const MergeBatch &mb, uint64_t x, uint32_t per_pair_extra) {
    uint32_t p = 0;                                      // the last p with tile0[p] + p * extra <= x
    for (uint32_t q = 1; q < mb.np; ++q)
        if ((uint64_t)mb.tile0[q] + (uint64_t)q * per_pair_extra <= x) p = q;
    return p;
}

__global__ __launch_bounds__(256) void k_or_split_batch(MergeBatch mb, uint64_t *__restrict__ splits) {
    constexpr int T = OT;
    using Le = TupleLe<false>;
    const int lane = threadIdx.x & 63, grp = lane >> 4, gl = lane & 15;
    const uint64_t e = ((((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6) << 2) + (uint64_t)grp;
    const uint32_t p = batch_pair(mb, e, 1);
    const uint64_t s0 = (uint64_t)mb.tile0[p] + p, ntiles = mb.tile0[p + 1] - mb.tile0[p];
    // entries past the last pair's (ntiles + 1) compute nothing: t > ntiles
    const uint64_t t = e - s0, na = mb.na[p], nb = mb.nb[p];
    const crdt_tuples &A = mb.A[p], &B = mb.B[p];
    uint64_t *const split = splits + s0;
#include "settile_split.inc"
}

template <int NT>
__global__ __launch_bounds__(NT) void k_tmerge_batch(MergeBatch mb, const uint64_t *__restrict__ split) {
    __shared__ uint64_t sk[OT], st[OT];
    __shared__ uint32_t sr[OT];
    __shared__ uint8_t sm[OT];
    const uint32_t p = batch_pair(mb, blockIdx.x, 0);
    tmerge_tile<NT>(mb.A[p], mb.B[p], mb.na[p], mb.nb[p], split + mb.tile0[p] + p, mb.O[p],
                    blockIdx.x - mb.tile0[p], sk, st, sr, sm);
}

// Every pair's stable merge (tuples_merge_stable of each), kMergeBatch pairs
// per pair of launches.
int tuples_merge_stable_batch(crdt_ctx *ctx, const std::vector<MergePairArg> &pairs) {
    for (size_t p0 = 0; p0 < pairs.size(); p0 += kMergeBatch) {
        MergeBatch mb{};
        uint64_t tiles = 0;
        const size_t np = std::min(pairs.size() - p0, (size_t)kMergeBatch);
        for (size_t q = 0; q < np; ++q) {
            const MergePairArg &x = pairs[p0 + q];
            const crdt_tuples empty{nullptr, nullptr, nullptr, nullptr};
            mb.A[q] = x.na ? x.A : empty;
            mb.B[q] = x.nb ? x.B : empty;
            mb.O[q] = x.O;
            mb.na[q] = x.na;
            mb.nb[q] = x.nb;
            mb.tile0[q] = (uint32_t)tiles;
            tiles += (x.na + x.nb + OT - 1) / OT;
            if (tiles >= 0x7fffffffULL) return CRDT_E_RANGE;
        }
        mb.tile0[np] = (uint32_t)tiles;
        mb.np = (uint32_t)np;
        if (tiles == 0) continue;
        const uint64_t entries = tiles + np;
        int rc = ws_reserve(ctx, Carve::round(entries * 8) + 1024);
        if (rc) return rc;
        uint64_t *split = (uint64_t *)ctx->ws;
        k_or_split_batch<<<(unsigned)((entries + 15) / 16), 256, 0, ctx->stream>>>(mb, split);
        k_tmerge_batch<512><<<(unsigned)tiles, 512, 0, ctx->stream>>>(mb, split);
        rc = check_launch(ctx);
        if (rc) return rc;
    }
    return CRDT_OK;
}

int tuples_merge_stable(crdt_ctx *ctx, const crdt_tuples &A, size_t na, const crdt_tuples &B, size_t nb,
                        const crdt_tuples &O) {
    const size_t n = na + nb;
    if (n == 0) return CRDT_OK;
    const size_t ntiles = (n + OT - 1) / OT;
    if (ntiles >= 0x7fffffffULL || n >= (1ULL << 62)) return CRDT_E_RANGE;
    int rc = ws_reserve(ctx, Carve::round((ntiles + 1) * 8) + 1024);
    if (rc) return rc;
    Carve w(ctx->ws);
    uint64_t *split = w.take<uint64_t>(ntiles + 1);
    const crdt_tuples empty{nullptr, nullptr, nullptr, nullptr};
    const crdt_tuples &a = na ? A : empty, &b = nb ? B : empty;
    k_mp_split<OT, TupleLe<false>, PlainTiles>
        <<<mp_split_grid(ntiles), 256, 0, ctx->stream>>>(a, na, nullptr, b, nb, nullptr, split);
    k_tmerge<512><<<(unsigned)ntiles, 512, 0, ctx->stream>>>(a, b, na, nb, split, O);
    return check_launch(ctx);
}

// Adjacent pairs out of (key, ts, rep) order.
__global__ void k_count_unsorted(crdt_tuples T, size_t n, unsigned long long *bad) {
    unsigned long long c = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i + 1 < n; i += (size_t)gridDim.x * 256)
        c += tag_le(gtag(T, i), gtag(T, i + 1)) ? 0 : 1;
    if (c) atomicAdd(bad, c);
}

// WITH_SRC: the _src entry points (src_out: na + nb int64, the source index of every output).
// A side of no elements may be a null pointer; the checks are settile.hpp's.
// (The passes stage every field by LDS-DMA from element offsets: key / ts /
// rep must be naturally aligned, as any element offset of an allocation is.)
template <bool LWW, bool WITH_SRC = false>
static int set_merge(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b, size_t nb,
                     crdt_tuples *out, uint64_t *out_count, int64_t *src_out = nullptr) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out_count || !out || tuples_null(out)) return CRDT_E_INVAL;
    if ((na && (!a || tuples_null(a))) || (nb && (!b || tuples_null(b)))) return CRDT_E_INVAL;
    if ((na && tuples_misaligned(a)) || (nb && tuples_misaligned(b))) return CRDT_E_INVAL;
    if (WITH_SRC && na + nb) {
        if (na + nb >= (1ULL << 62)) return CRDT_E_RANGE;
        const size_t sb = (na + nb) * 8;
        if (!src_out || ((uintptr_t)src_out & 7)) return CRDT_E_INVAL;
        // (every pointer compared here is non-null: spans_overlap's null rule never applies)
        if ((na && tuples_overlap(a, na, src_out, sb)) || (nb && tuples_overlap(b, nb, src_out, sb)) ||
            tuples_overlap(out, na + nb, src_out, sb))
            return CRDT_E_INVAL;
    }
    if (na + nb == 0) {
        hipError_t e = hipMemsetAsync(out_count, 0, sizeof(uint64_t), ctx->stream);
        return e == hipSuccess ? CRDT_OK : hip_fail(ctx, e);
    }
    crdt_tuples empty{nullptr, nullptr, nullptr, nullptr};
    const crdt_tuples &A = na ? *a : empty;
    const crdt_tuples &B = nb ? *b : empty;
    int64_t *src = WITH_SRC ? src_out : nullptr;
    return LWW ? merge_two_pass<LwwMode>(ctx, A, na, B, nb, *out, src, out_count)
               : merge_two_pass<OrMode>(ctx, A, na, B, nb, *out, src, out_count);
}

// out_col[i] = the element src[i] names -- a_col[src[i]] (src[i] >= 0) or
// b_col[-(src[i] + 1)] -- for i < n, n from n_max / n_dev as in setread.hip.
// One lane per element, grid-stride.  A merge's src is ascending within each
// side, so a wave's reads of a side fall in a few neighbouring cache lines
// (near-sequential: no LDS staging would read fewer lines); the stores are
// coalesced.  An index outside its side is never dereferenced: the element
// keeps its value and CRDT_DEV_RANGE is raised.
template <typename E>
__global__ __launch_bounds__(256) void k_src_gather(const int64_t *__restrict__ src, uint64_t n_max,
                                                    const uint64_t *__restrict__ n_dev, const E *__restrict__ a,
                                                    uint64_t na, const E *__restrict__ b, uint64_t nb,
                                                    E *__restrict__ out, uint32_t *__restrict__ err) {
    const uint64_t n = n_dev ? *n_dev : n_max;
    if (n > n_max) {                                     // (a plan miss's ~0 included) nothing touched
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, CRDT_DEV_RANGE);
        return;
    }
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const int64_t s = src[i];
        const bool on_a = s >= 0;
        const uint64_t j = on_a ? (uint64_t)s : ~(uint64_t)s;   // -(s + 1)
        if (j < (on_a ? na : nb)) out[i] = (on_a ? a : b)[j];
        else bad = true;
    }
    if (bad) atomicOr(err, CRDT_DEV_RANGE);
}

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_lww_merge(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b, size_t nb,
                              crdt_tuples *out, uint64_t *out_count_dev) {
    return set_merge<true>(ctx, a, na, b, nb, out, out_count_dev);
}

extern "C" int crdt_orset_merge(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b, size_t nb,
                                crdt_tuples *out, uint64_t *out_count_dev) {
    return set_merge<false>(ctx, a, na, b, nb, out, out_count_dev);
}

extern "C" int crdt_lww_merge_src(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b, size_t nb,
                                  crdt_tuples *out, int64_t *src_out_dev, uint64_t *out_count_dev) {
    return set_merge<true, true>(ctx, a, na, b, nb, out, out_count_dev, src_out_dev);
}

extern "C" int crdt_orset_merge_src(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b, size_t nb,
                                    crdt_tuples *out, int64_t *src_out_dev, uint64_t *out_count_dev) {
    return set_merge<false, true>(ctx, a, na, b, nb, out, out_count_dev, src_out_dev);
}

extern "C" int crdt_src_gather(crdt_ctx *ctx, const int64_t *src_dev, size_t n_max, const uint64_t *n_dev,
                               const void *a_col_dev, size_t na, const void *b_col_dev, size_t nb, void *out_col_dev,
                               size_t elem_size) {
    int rc = bind(ctx);
    if (rc) return rc;
    const size_t es = elem_size;
    if (es != 1 && es != 2 && es != 4 && es != 8 && es != 16) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62) || na >= (1ULL << 59) || nb >= (1ULL << 59)) return CRDT_E_RANGE;
    if (n_max == 0) return CRDT_OK;
    if (!src_dev || !out_col_dev || (na && !a_col_dev) || (nb && !b_col_dev)) return CRDT_E_INVAL;
    if (((uintptr_t)src_dev & 7) || ((uintptr_t)n_dev & 7) ||
        (((uintptr_t)out_col_dev | (uintptr_t)a_col_dev | (uintptr_t)b_col_dev) & (es - 1)))
        return CRDT_E_INVAL;
    if (mul_overflows(n_max, es)) return CRDT_E_RANGE;
    const size_t ob = n_max * es;
    // (a null side has no elements: it met nothing before spans_overlap's null rule, too)
    if (spans_overlap(out_col_dev, ob, src_dev, n_max * 8) || spans_overlap(out_col_dev, ob, a_col_dev, na * es) ||
        spans_overlap(out_col_dev, ob, b_col_dev, nb * es))
        return CRDT_E_INVAL;
    const unsigned g = grid_for(n_max, 256, (unsigned)ctx->num_cus * 8);
    const hipStream_t s = ctx->stream;
    uint32_t *err = ctx->dev_status;
#define GATHER(E)                                                                                                   \
    k_src_gather<E><<<g, 256, 0, s>>>(src_dev, n_max, n_dev, (const E *)a_col_dev, na, (const E *)b_col_dev, nb, \
                                      (E *)out_col_dev, err)
    switch (es) {
    case 1: GATHER(uint8_t); break;
    case 2: GATHER(uint16_t); break;
    case 4: GATHER(uint32_t); break;
    case 8: GATHER(uint64_t); break;
    default: GATHER(uint4); break;                       // 16 bytes: one dwordx4 load and store per element
    }
#undef GATHER
    return check_launch(ctx);
}

extern "C" int crdt_tuples_merge(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b, size_t nb,
                                 const crdt_tuples *out) {
    int rc = bind(ctx);
    if (rc) return rc;
    if ((na + nb && (!out || tuples_null(out))) || (na && (!a || tuples_null(a))) || (nb && (!b || tuples_null(b))))
        return CRDT_E_INVAL;
    const crdt_tuples empty{nullptr, nullptr, nullptr, nullptr};
    return tuples_merge_stable(ctx, na ? *a : empty, na, nb ? *b : empty, nb, na + nb ? *out : empty);
}

extern "C" int crdt_tuples_count_unsorted(crdt_ctx *ctx, const crdt_tuples *t, size_t n, uint64_t *bad) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!bad) return CRDT_E_INVAL;
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(uint64_t), ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e);
    if (n < 2) return CRDT_OK;
    if (!t || tuples_null(t)) return CRDT_E_INVAL;
    k_count_unsorted<<<grid_for(n, 256, (unsigned)ctx->num_cus * 8), 256, 0, ctx->stream>>>(
        *t, n, (unsigned long long *)bad);
    return check_launch(ctx);
}
