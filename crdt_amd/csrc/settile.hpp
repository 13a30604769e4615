// settile.hpp -- the tile scaffold of the set-state ops (setread, setdelta,
// setcompact, setdigest, setcausal, setapply .hip) and of the
// set merges it was first copied from (sets.hip: the argument checks, the
// workspace and the split; LWW tiles there are 4096 items and the scan is
// k_chunk_scan, over chunks of tiles).  Every one of them
// is count / scan / write over tiles of 2048 items with one workspace shape:
//   tcnt[t]  the tile's output count (under an empty carry)
//   rec[t]   the tile's carry record (ops whose decisions cross tiles)
//   ic[t]    the tile's output offset, ic[tiles] = the total
//   bits     bitmaps of 32 words per tile, one bit per item
//   split[t] (two-sided ops) first-side elements before merged item t * 2048
// This file holds what the ops share: the lengths and argument checks, the
// workspace, the one-workgroup scan, the merge-path split, the by-position
// write pass and the rank selection of the by-rank write passes.  An op keeps
// its record encoding, its decisions and its entry points.
// Two-sided passes name the sides a and b, a the first (tie-winning) one.
#pragma once
#include "common.hpp"

namespace crdt {

constexpr int kTile = 2048;               // items per tile
constexpr int kTileNW = kTile / 64;       // words per tile and bitmap
constexpr int kTileB = 256;               // threads of a by-position pass (4 waves)
constexpr int kTileWW = kTile / kTileB;   // 64-item mask words per wave (consecutive: 512 items)

// ---------------------------------------------------------------- lengths
// the call's item count: n_max, or the device count when it is in range
__device__ __forceinline__ bool tile_len(uint64_t n_max, const uint64_t *__restrict__ n_dev, uint64_t *n) {
    *n = n_dev ? *n_dev : n_max;
    return *n <= n_max;
}
// both lengths; false when either is out of range
__device__ __forceinline__ bool tile_len(uint64_t na_max, const uint64_t *__restrict__ na_dev, uint64_t nb_max,
                                         const uint64_t *__restrict__ nb_dev, uint64_t *na, uint64_t *nb) {
    *na = na_dev ? *na_dev : na_max;
    *nb = nb_dev ? *nb_dev : nb_max;
    return *na <= na_max && *nb <= nb_max;
}
// tiles of a call (a one-sided op passes nb = 0)
struct PlainTiles {
    static __device__ __forceinline__ uint64_t tiles(uint64_t na, uint64_t nb) { return (na + nb + kTile - 1) / kTile; }
};

// ---------------------------------------------------------------- argument checks
static bool tuples_null(const crdt_tuples *t) { return !t->key || !t->ts || !t->rep || !t->tomb; }
static bool tuples_misaligned(const crdt_tuples *t) {
    return ((((uintptr_t)t->key | (uintptr_t)t->ts) & 7) | ((uintptr_t)t->rep & 3)) != 0;
}
// [p, p + pn) meets [q, q + qn); a null pointer or no bytes meet nothing
static bool spans_overlap(const void *p, size_t pn, const void *q, size_t qn) {
    const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
    return p && q && pn && qn && x < y + qn && y < x + pn;
}
// any field of t (n elements) meets [p, p + bytes)
static bool tuples_overlap(const crdt_tuples *t, size_t n, const void *p, size_t bytes) {
    return spans_overlap(t->key, n * 8, p, bytes) || spans_overlap(t->ts, n * 8, p, bytes) ||
           spans_overlap(t->rep, n * 4, p, bytes) || spans_overlap(t->tomb, n, p, bytes);
}
// any field of o (no elements) meets any field of t (n elements)
static bool tuples_overlap(const crdt_tuples *o, size_t no, const crdt_tuples *t, size_t n) {
    return tuples_overlap(t, n, o->key, no * 8) || tuples_overlap(t, n, o->ts, no * 8) ||
           tuples_overlap(t, n, o->rep, no * 4) || tuples_overlap(t, n, o->tomb, no);
}

// ---------------------------------------------------------------- carry + scan
// A Carry policy describes an op's tile records to the scan:
//   tiles(na, nb)   the call's tile count
//   kHas            false: no records, the scan carries the offset base alone
//   kId             the record of an empty segment
//   kStride, kEmit, kAux  the bitmap words per tile, its first emit and auxiliary word
//   part(r)         the bits of a record that take part in the scan
//   then(x, y)      part x, then part y (associative)
//   seed(s)         what the round's prefixes start from, the round entered in state s
//   enter(p, s)     the state after the prefix p of a round entered in state s
//   step(s, r)      the state after the tile of record r, entered in state s
//   redecide(r, s)  what the state s before the tile changes at the tile's first
//                   run end: a redo() word, 0 for nothing
// The state before the first tile is 0.
// redecide's answer: the run end's item in the tile; its emit bit / auxiliary
// bit flips; the tile's count goes up (with emit: else down).  0: no change.
__device__ __forceinline__ uint32_t redo(uint32_t pos, bool emit, bool aux, bool up) {
    return (emit ? 1u : 0u) | (aux ? 2u : 0u) | (up ? 4u : 0u) | (pos << 16);
}
template <class Tiles = PlainTiles>
struct NoCarry : Tiles {
    static constexpr bool kHas = false;
};

// One workgroup, rounds of 1024 K tiles, a contiguous run of K tiles per
// thread (k_chunk_scan's scheme): with records, the carry into every tile as a
// scan of the records' parts, the first run end of each tile re-decided under
// its carry (the emit and auxiliary bit in bits, when given -- kStride words
// per tile, the emit words from kEmit, the auxiliary ones from kAux -- and the
// count); then the counts to offsets (ic, when given; ic[tiles] = the total)
// and the total to *count.
template <class Carry, int K>
__global__ __launch_bounds__(1024) void k_tile_scan(uint64_t na_max, const uint64_t *__restrict__ na_dev,
                                                    uint64_t nb_max, const uint64_t *__restrict__ nb_dev,
                                                    const uint32_t *__restrict__ tcnt, const uint32_t *__restrict__ rec,
                                                    uint64_t *__restrict__ bits, uint64_t *__restrict__ ic,
                                                    uint64_t *__restrict__ count, uint32_t *__restrict__ err) {
    constexpr uint32_t kRound = 1024u * K;
    __shared__ uint32_t s_f[Carry::kHas ? 16 : 1];
    __shared__ uint64_t s_c[16];
    uint64_t na, nb;
    if (!tile_len(na_max, na_dev, nb_max, nb_dev, &na, &nb)) {
        if (threadIdx.x == 0) {
            *count = ~0ull;
            atomicOr(err, CRDT_DEV_RANGE);
        }
        return;
    }
    const uint64_t nt = Carry::tiles(na, nb);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t state = 0;                                  // the carry into the round's first tile
    uint64_t base = 0;
    for (uint64_t c0 = 0; c0 < nt; c0 += kRound) {
        const uint64_t b = c0 + (uint64_t)threadIdx.x * K;
        uint32_t v[K];
#pragma unroll
        for (int q = 0; q < K; ++q) v[q] = b + q < nt ? tcnt[b + q] : 0u;
        if constexpr (Carry::kHas) {
            uint32_t rr[K], f = Carry::kId;
#pragma unroll
            for (int q = 0; q < K; ++q) {
                rr[q] = b + q < nt ? rec[b + q] : Carry::kId;
                f = Carry::then(f, Carry::part(rr[q]));
            }
            uint32_t x = f;                              // inclusive scan over the wave's threads
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(x, o, 64);
                if (lane >= o) x = Carry::then(y, x);
            }
            if (lane == 63) s_f[w] = x;
            uint32_t ex = __shfl_up(x, 1, 64);
            if (lane == 0) ex = Carry::kId;
            __syncthreads();
            uint32_t pre = Carry::seed(state), tot = pre;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (q < w) pre = Carry::then(pre, s_f[q]);
                tot = Carry::then(tot, s_f[q]);
            }
            uint32_t s = Carry::enter(Carry::then(pre, ex), state);
#pragma unroll
            for (int q = 0; q < K; ++q) {
                const uint32_t d = Carry::redecide(rr[q], s);
                if (d & 3u) {
                    const uint32_t p = d >> 16;
                    const uint64_t at = (b + q) * Carry::kStride + (p >> 6);
                    if (d & 1u) {
                        if (bits) bits[at + Carry::kEmit] ^= 1ull << (p & 63);
                        v[q] += (d & 4u) ? 1u : 0xffffffffu;
                    }
                    if (bits && (d & 2u)) bits[at + Carry::kAux] ^= 1ull << (p & 63);
                }
                s = Carry::step(s, rr[q]);
            }
            state = Carry::enter(tot, state);
        }
        uint64_t sum = 0;
#pragma unroll
        for (int q = 0; q < K; ++q) sum += v[q];
        uint64_t x = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_c[w] = x;
        __syncthreads();
        uint64_t run = base + x - sum, tot = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            run += q < w ? s_c[q] : 0;
            tot += s_c[q];
        }
        if (ic) {
#pragma unroll
            for (int q = 0; q < K; ++q) {
                if (b + q < nt) ic[b + q] = run;
                run += v[q];
            }
        }
        base += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (ic) ic[nt] = base;
        *count = base;
    }
}

// ---------------------------------------------------------------- workspace
struct TileWs {
    uint64_t *split = nullptr;
    uint32_t *tcnt = nullptr, *rec = nullptr;
    uint64_t *ic = nullptr, *bits = nullptr;
    // what reserve() asks of the workspace (an op that carves more behind the tiles starts there)
    static size_t bytes(size_t ntiles, bool with_split, bool with_rec, size_t wpt) {
        return (with_split ? Carve::round((ntiles + 2) * 8) + 256 : 0) +
               (with_rec ? 2 : 1) * Carve::round((ntiles + 1) * 4) + Carve::round((ntiles + 1) * 8) +
               Carve::round((ntiles * wpt + 1) * 8) + 1024;
    }
    // grows the context's workspace to hold ntiles tiles with wpt bitmap words each, and carves it
    int reserve(crdt_ctx *ctx, size_t ntiles, bool with_split, bool with_rec, size_t wpt, size_t extra = 0) {
        const size_t need = bytes(ntiles, with_split, with_rec, wpt) + extra;
        const int rc = ws_reserve(ctx, need);
        if (rc) return rc;
        Carve w(ctx->ws);
        if (with_split) split = w.take<uint64_t>(ntiles + 2);
        tcnt = w.take<uint32_t>(ntiles + 1);
        if (with_rec) rec = w.take<uint32_t>(ntiles + 1);
        ic = w.take<uint64_t>(ntiles + 1);
        bits = w.take<uint64_t>(ntiles * wpt + 1);
        return CRDT_OK;
    }
    // k_tile_scan over the call's tiles, in rounds of g_tile_scan_round tiles
    // ("settile.scan_round"; the product build: 16384).  wr: the write pass
    // follows, so the bitmaps are patched and ic is stored.
    template <class Carry>
    void scan(crdt_ctx *ctx, uint64_t na_max, const uint64_t *na_dev, uint64_t nb_max, const uint64_t *nb_dev, bool wr,
              uint64_t *count) const {
        uint64_t *const b = wr ? bits : nullptr, *const o = wr ? ic : nullptr;
#ifdef CRDT_DIAG
        if (g_tile_scan_round == 1024) {
            k_tile_scan<Carry, 1><<<1, 1024, 0, ctx->stream>>>(na_max, na_dev, nb_max, nb_dev, tcnt, rec, b, o, count,
                                                               ctx->dev_status);
            return;
        }
#endif
        k_tile_scan<Carry, 16><<<1, 1024, 0, ctx->stream>>>(na_max, na_dev, nb_max, nb_dev, tcnt, rec, b, o, count,
                                                            ctx->dev_status);
    }
};

// ---------------------------------------------------------------- split
// A[i] <= B[j] in merge order (KEYS: keys only; else ts / rep read only on a key tie)
template <bool KEYS>
struct TupleLe {
    static __device__ __forceinline__ bool le(const crdt_tuples &A, uint64_t i, const crdt_tuples &B, uint64_t j) {
        const uint64_t ka = A.key[i], kb = B.key[j];
        if (KEYS || ka != kb) return ka <= kb;
        const uint64_t ta = A.ts[i], tb = B.ts[j];
        if (ta != tb) return ta < tb;
        return A.rep[i] <= B.rep[j];
    }
};

// split[t] = a elements among the first min(t T, n) merged items, t = 0 ..
// tiles: one 16-lane group per diagonal, four per wave, each a 16-ary search
// (settile_split.inc), the lengths read on the device.
template <int T, class Le, class Tiles>
__global__ __launch_bounds__(256) void k_mp_split(crdt_tuples A, uint64_t na_max, const uint64_t *__restrict__ na_dev,
                                                  crdt_tuples B, uint64_t nb_max, const uint64_t *__restrict__ nb_dev,
                                                  uint64_t *__restrict__ split) {
    uint64_t na, nb;
    if (!tile_len(na_max, na_dev, nb_max, nb_dev, &na, &nb)) return;
    const uint64_t ntiles = Tiles::tiles(na, nb);
    if (ntiles == 0) return;
    const int lane = threadIdx.x & 63, grp = lane >> 4, gl = lane & 15;
    const uint64_t t = ((((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6) << 2) + (uint64_t)grp;
#include "settile_split.inc"
}
inline unsigned mp_split_grid(size_t ntiles) { return (unsigned)((ntiles + 1 + 15) / 16); }   // 16 diagonals per workgroup

// ---------------------------------------------------------------- write, by position
// Every set bit of the tile's emit words (AUX: a second bitmap kTileNW words
// on, whose bit travels along): store(i, at, aux) for item i of the state and
// its output rank at.  Positions at or past the length, or ranks at or past
// n_max, raise CRDT_DEV_RANGE and store nothing (a bitmap of the same call's
// count pass never does).
template <bool AUX, class Store>
__device__ __forceinline__ void tile_emit_by_position(uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                      const uint64_t *__restrict__ bits,
                                                      const uint64_t *__restrict__ ic, uint32_t *__restrict__ err,
                                                      Store store) {
    constexpr int BS = AUX ? 2 * kTileNW : kTileNW;
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = blockIdx.x, tb = t * kTile;
    if (tb >= n) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // every wave holds the tile's words, lane w word w
    const uint64_t wd = lane < kTileNW ? bits[t * BS + lane] : 0ull;
    const uint64_t wt = AUX && lane < kTileNW ? bits[t * BS + kTileNW + lane] : 0ull;
    const uint32_t pc = (uint32_t)__popcll(wd);
    uint32_t x = pc;
#pragma unroll
    for (int o = 1; o < kTileNW; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    const uint32_t ex = x - pc;
    const uint64_t base = ic[t];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kTileWW; ++j) {
        const int q = wv * kTileWW + j;
        const uint64_t wq = (uint64_t)__shfl((unsigned long long)wd, q, 64);
        const uint64_t tq = AUX ? (uint64_t)__shfl((unsigned long long)wt, q, 64) : 0ull;
        const uint32_t pq = __shfl(ex, q, 64);
        if ((wq >> lane) & 1) {
            const uint64_t i = tb + (uint64_t)q * 64 + lane;
            const uint64_t at = base + pq + (uint32_t)__popcll(wq & ((1ull << lane) - 1));
            if (i < n && at < n_max) store(i, at, (uint8_t)((tq >> lane) & 1));
            else bad = true;
        }
    }
    if (bad) atomicOr(err, CRDT_DEV_RANGE);
}

// one field of the emitting tuples (crdt_set_elements: the keys)
template <class E>
__global__ __launch_bounds__(kTileB) void k_tile_write_field(const E *__restrict__ key, uint64_t n_max,
                                                             const uint64_t *__restrict__ n_dev,
                                                             const uint64_t *__restrict__ bits,
                                                             const uint64_t *__restrict__ ic, E *__restrict__ out,
                                                             uint32_t *__restrict__ err) {
    tile_emit_by_position<false>(n_max, n_dev, bits, ic, err, [&](uint64_t i, uint64_t at, uint8_t) { out[at] = key[i]; });
}

// The four fields of the emitting tuples, and the source index when asked:
// the index of the first copy of the tuple's tag (the walk back over equal-tag
// copies goes through global memory, as k_lww_write's does).  OR-Set: the tomb
// is the auxiliary bit; LWW: the first copy's.
template <bool LWW, bool SRC>
__global__ __launch_bounds__(kTileB) void k_tile_write(crdt_tuples T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                       const uint64_t *__restrict__ bits,
                                                       const uint64_t *__restrict__ ic, crdt_tuples out,
                                                       int64_t *__restrict__ src, uint32_t *__restrict__ err) {
    tile_emit_by_position<!LWW>(n_max, n_dev, bits, ic, err, [&](uint64_t i, uint64_t at, uint8_t aux) {
        const uint64_t key = T.key[i], ts = T.ts[i];
        const uint32_t rep = T.rep[i];
        uint8_t tomb = LWW ? T.tomb[i] : aux;
        uint64_t f = i;
        if (LWW || SRC) {
            const uint64_t p = i > 0 ? i - 1 : 0;
            const uint64_t pk = T.key[p], pts = T.ts[p];
            const uint32_t pr = T.rep[p];
            if (i > 0 && pk == key && pts == ts && pr == rep) {
                f = p;
                while (f > 0 && T.key[f - 1] == key && T.ts[f - 1] == ts && T.rep[f - 1] == rep) --f;
                if (LWW) tomb = T.tomb[f];
            }
        }
        out.key[at] = key;
        out.ts[at] = ts;
        out.rep[at] = rep;
        out.tomb[at] = tomb;
        if (SRC) src[at] = (int64_t)f;
    });
}
template <class... A>
static void tile_write(bool lww, bool src, unsigned g, hipStream_t s, A... a) {
    if (lww && src) k_tile_write<true, true><<<g, kTileB, 0, s>>>(a...);
    else if (lww) k_tile_write<true, false><<<g, kTileB, 0, s>>>(a...);
    else if (src) k_tile_write<false, true><<<g, kTileB, 0, s>>>(a...);
    else k_tile_write<false, false><<<g, kTileB, 0, s>>>(a...);
}

// ---------------------------------------------------------------- write, by rank
// A two-sided tile's bitmaps are in merged order: `isb` (a b item) in the
// tile's first kTileNW words, `emit` in the next.  Every wave holds them,
// lane w word w, with their exclusive prefix counts.
struct RankWords {
    uint64_t wb, we;
    uint32_t xb, xe;
    uint32_t ne;           // the tile's outputs
};
__device__ __forceinline__ RankWords rank_words(const uint64_t *__restrict__ b, int lane) {
    RankWords k;
    k.wb = lane < kTileNW ? b[lane] : 0ull;
    k.we = lane < kTileNW ? b[kTileNW + lane] : 0ull;
    const uint32_t pb = (uint32_t)__popcll(k.wb), pe = (uint32_t)__popcll(k.we);
    k.xb = pb;
    k.xe = pe;
#pragma unroll
    for (int o = 1; o < kTileNW; o <<= 1) {
        const uint32_t yb = __shfl_up(k.xb, o, 64), ye = __shfl_up(k.xe, o, 64);
        if (lane >= o) {
            k.xb += yb;
            k.xe += ye;
        }
    }
    k.ne = (uint32_t)__builtin_amdgcn_readlane((int)k.xe, kTileNW - 1);
    k.xb -= pb;
    k.xe -= pe;
    return k;
}
// Output r < ne of the tile: the word w holding its emit bit, the bit's
// position there (always < 64), the words' values and the b items merged
// before it.  Every lane of the wave must call it (shuffles).
struct RankHit {
    int w;
    uint32_t pos, nb;
    uint64_t qb, qe;
};
__device__ __forceinline__ RankHit rank_select(const RankWords &k, uint32_t r) {
    RankHit h;
    h.w = 0;                                             // the last word with xe <= r: the one holding output r
#pragma unroll
    for (int o = kTileNW / 2; o > 0; o >>= 1)
        if (__shfl(k.xe, h.w + o, 64) <= r) h.w += o;
    h.qb = (uint64_t)__shfl((unsigned long long)k.wb, h.w, 64);
    h.qe = (uint64_t)__shfl((unsigned long long)k.we, h.w, 64);
    uint32_t c = r - __shfl(k.xe, h.w, 64);              // its set bit of qe, counted from bit 0
    h.pos = 0;
    uint64_t m = h.qe;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t below = (uint32_t)__popcll(m & ((1ull << o) - 1));
        if (c >= below) {
            c -= below;
            m >>= o;
            h.pos += o;
        }
    }
    h.nb = __shfl(k.xb, h.w, 64) + (uint32_t)__popcll(h.qb & ((1ull << h.pos) - 1));
    return h;
}

}  // namespace crdt
