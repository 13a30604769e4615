// setcompact.hip -- tombstone compaction of a sorted LWW / OR-Set state under a
// causal-stability cut (crdt_set_compact).
//
// Semantics, pinned to the merges of sets.hip.  A tag (key, ts, rep) is STABLE
// under cut[0 .. n_cut) iff rep < n_cut and ts <= cut[rep] (unsigned); with
// n_cut == 0 nothing is.  For tuples t[0 .. n) sorted ascending by (key, ts,
// rep), copies of one tag in any order, compact(t, cut) is merge(t, {}) with
// the stable dead tuples removed:
//   OR-Set : per distinct tag, tomb = the OR over its copies; the tag is
//            dropped iff that OR is 1 and the tag is stable, else written once
//            with that OR.
//   LWW    : per distinct key, the winner = the maximal (ts, rep) tag with the
//            tomb of that tag's FIRST copy (crdt_lww_merge's winner); the key
//            is dropped iff the winner's tomb is 1 and the winner is stable,
//            else the winner is written.
// Output in ascending tuple order, its length to *count; optionally, per output
// tuple, the index in t of the tuple it is (LWW: the first copy of the winner
// tag; OR-Set: the first copy of the tag -- crdt_*_merge_src(t, {})'s a-side).
//
// GPU structure: setread.hip's -- a streaming job over tiles of 2048 tuples,
// one workgroup of four waves each, every decision a wave64 ballot word.
//   count : per tile the `emit` bitmap (bit set at the LAST copy of a kept
//           tag's run; LWW: at the last tuple of a kept key's run), OR-Set
//           also the `tomb` bitmap (the tomb-OR of the emitted tag), the
//           tile's count and, OR-Set only, a carry record.  No tile waits for
//           another: each evaluates with an empty carry; what a carry can
//           change is one decision, the tile's first tag end.  cut[rep] is
//           loaded only at a deciding position whose tomb-OR is 1, or may
//           become 1 by the carry, and whose rep < n_cut.
//   scan  : k_tile_scan<CmpCarry> (settile.hpp; LWW: <NoCarry>).  The carry
//           state is one bit (a tombstone seen in the open tag run), a tile's
//           record the 2-entry function it applies to it plus both outcomes of
//           its first tag end; composing functions is associative, so the
//           carries into all tiles are a prefix scan -- linear however many
//           tiles one tag spans.  The scan patches the at most one affected
//           emit / tomb bit and count per tile.
//   write : k_tile_write (settile.hpp): the four fields of each emitting tuple
//           at its rank, and the source index when asked.
// LWW needs no carry: the last tuple of a key's run holds the key's maximal tag.
//
// The tuple count may stay on the device (n_dev): every kernel reads it, tiles
// at or past min(*n_dev, n_max) do nothing, and *n_dev > n_max touches no
// tuple, stores a count of ~0 and raises CRDT_DEV_RANGE.  No kernel reads a
// tuple index at or past that length or before 0 -- the write pass checks every
// bitmap position against it before its first load -- nor cut at or past n_cut.
#include "settile.hpp"

namespace crdt {

constexpr int CT = kTile, CB = kTileB, CWW = kTileWW, CNW = kTileNW;   // tile, its threads, words per wave and tile

// ---- carry records (OR-Set).  State s = a tombstone seen in the open tag run.
//   bits 0-1   F: the state after the segment, per state before it
//   bits 2-3   E: whether the segment's first tag end is emitted, per state before
//   bits 4-5   T: that tag's tomb-OR, per state before
//   bit  6     the segment holds a tag end
//   bits 16-   its position in the segment
constexpr uint32_t kCmpId = 0x2u;        // F = identity, no tag end
constexpr uint32_t kCmpTE = 1u << 6;
__device__ __forceinline__ uint32_t cmp_f(uint32_t r, uint32_t s) { return (r >> s) & 1u; }
__device__ __forceinline__ uint32_t cmp_e(uint32_t r, uint32_t s) { return (r >> (2 + s)) & 1u; }
__device__ __forceinline__ uint32_t cmp_t(uint32_t r, uint32_t s) { return (r >> (4 + s)) & 1u; }
__device__ __forceinline__ uint32_t cmp_pos(uint32_t r) { return r >> 16; }
// segment a, then segment b (which starts off_b tuples after a's start)
__device__ __forceinline__ uint32_t cmp_then(uint32_t a, uint32_t b, uint32_t off_b) {
    uint32_t f = 0, et = 0;
#pragma unroll
    for (uint32_t s = 0; s < 2; ++s) {
        const uint32_t as = cmp_f(a, s);
        f |= cmp_f(b, as) << s;
        et |= (cmp_e(b, as) << (2 + s)) | (cmp_t(b, as) << (4 + s));
    }
    if (a & kCmpTE) return f | (a & 0xffff007cu);
    if (b & kCmpTE) return f | et | kCmpTE | ((cmp_pos(b) + off_b) << 16);
    return f;
}
// F alone (the scan's operator)
__device__ __forceinline__ uint32_t cmp_fn_then(uint32_t a, uint32_t b) {
    return cmp_f(b, cmp_f(a, 0)) | (cmp_f(b, cmp_f(a, 1)) << 1);
}

// One mask word of an OR-Set state: V valid tuples (low bits), ST the tuple has
// a successor with the same tag, TB its tomb, SB the tuple's tag is stable
// (given at every tag end that `dead` or the carry can make dead), pt the
// word's first tuple continues the tag run before it.  *emit0 / *tomb0 = the
// emitted tag ends and their tomb-ORs under an empty carry.
__device__ __forceinline__ uint32_t cmp_word_rec(uint64_t V, uint64_t ST, uint64_t TB, uint64_t SB, bool pt,
                                                 uint64_t *emit0, uint64_t *tomb0) {
    *emit0 = 0;
    *tomb0 = 0;
    if (V == 0) return kCmpId;
    const uint64_t TE = V & ~ST;                         // tag run ends
    // segmented any(): the carry of an add runs from a set bit up to its run's end bit and stops there
    const uint64_t dead = TE & (((V & ~TE) + (TB & ~TE)) | TB);
    *emit0 = TE & ~(dead & SB);
    *tomb0 = dead & *emit0;
    if (TE == 0) {                                       // no tag end: the open run goes on
        const uint32_t t = TB != 0 ? 1u : 0u;
        return t | ((t | (pt ? 1u : 0u)) << 1);
    }
    const uint64_t f_te = TE & (0 - TE);
    const uint64_t h = 1ull << (63 - __builtin_clzll(TE));
    const uint32_t trail = (TB & ~(h | (h - 1))) != 0 ? 1u : 0u;
    const bool lead = (dead & f_te) != 0, stab = (SB & f_te) != 0;
    uint32_t r = kCmpTE | ((uint32_t)__builtin_ctzll(TE) << 16) | trail | (trail << 1);
#pragma unroll
    for (uint32_t s = 0; s < 2; ++s) {
        const bool tor = lead || (pt && s);
        r |= ((tor && stab) ? 0u : 1u) << (2 + s);
        r |= (tor ? 1u : 0u) << (4 + s);
    }
    return r;
}

// the scan's view of a record: F composes; the first tag end's emit and tomb are E and T at the carry, not at 0
struct CmpCarry : PlainTiles {
    static constexpr bool kHas = true;
    static constexpr uint32_t kId = kCmpId, kStride = 2 * CNW, kEmit = 0, kAux = CNW;   // (`emit`, then `tomb`)
    static __device__ __forceinline__ uint32_t part(uint32_t r) { return r & 3u; }
    static __device__ __forceinline__ uint32_t then(uint32_t a, uint32_t b) { return cmp_fn_then(a, b); }
    static __device__ __forceinline__ uint32_t seed(uint32_t) { return kCmpId; }
    static __device__ __forceinline__ uint32_t enter(uint32_t p, uint32_t s) { return cmp_f(p, s); }
    static __device__ __forceinline__ uint32_t step(uint32_t s, uint32_t r) { return cmp_f(r, s); }
    static __device__ __forceinline__ uint32_t redecide(uint32_t r, uint32_t s) {
        if (!((r & kCmpTE) && s != 0)) return 0;
        const bool e0 = cmp_e(r, 0) != 0, e1 = cmp_e(r, s) != 0;
        const bool t0 = e0 && cmp_t(r, 0) != 0, t1 = e1 && cmp_t(r, s) != 0;
        return redo(cmp_pos(r), e0 != e1, t0 != t1, e1);
    }
};

// ---------------------------------------------------------------- OR-Set count pass
template <bool BITS>
__global__ __launch_bounds__(CB) void k_cmp_or_count(crdt_tuples T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                     const uint64_t *__restrict__ cut, uint32_t n_cut,
                                                     uint32_t *__restrict__ tcnt, uint32_t *__restrict__ rec,
                                                     uint64_t *__restrict__ bits) {
    __shared__ uint32_t s_rec[CB / 64], s_cnt[CB / 64];
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = blockIdx.x, tb = t * CT;
    if (tb >= n) return;                                 // (uniform; so n > 0 below)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i0 = tb + (uint64_t)wv * (64 * CWW);
    // every tuple load up front, indices clamped into [0, n): nothing at or past n is read
    uint64_t k[CWW], kn[CWW], ts[CWW], tn[CWW];
    uint32_t r[CWW], rn[CWW];
    uint8_t tm[CWW];
#pragma unroll
    for (int j = 0; j < CWW; ++j) {
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        const uint64_t a = i < n ? i : n - 1, b = i + 1 < n ? i + 1 : n - 1;
        k[j] = T.key[a];
        kn[j] = T.key[b];
        ts[j] = T.ts[a];
        tn[j] = T.ts[b];
        r[j] = T.rep[a];
        rn[j] = T.rep[b];
        tm[j] = T.tomb[a];
    }
    // the tuple before the wave's first: does it open the wave's first tag run?
    bool pt0 = false;
    if (lane == 0 && i0 > 0 && i0 < n) pt0 = T.key[i0 - 1] == k[0] && T.ts[i0 - 1] == ts[0] && T.rep[i0 - 1] == r[0];
    const bool ptw = __ballot(pt0) != 0;
    // the masks of every word, and which lanes need their tag's stability
    uint64_t V[CWW], ST[CWW], TB[CWW];
    uint32_t need = 0;
    {
        bool pt = ptw;
#pragma unroll
        for (int j = 0; j < CWW; ++j) {
            const uint64_t i = i0 + (uint64_t)j * 64 + lane;
            const bool v = i < n;
            const bool st = i + 1 < n && k[j] == kn[j] && ts[j] == tn[j] && r[j] == rn[j];
            V[j] = __ballot(v);
            ST[j] = __ballot(st);
            TB[j] = __ballot(v && tm[j] != 0);
            const uint64_t TE = V[j] & ~ST[j];
            uint64_t may = TE & (((V[j] & ~TE) + (TB[j] & ~TE)) | TB[j]);
            if (pt) may |= TE & (0 - TE);                // the carry may bring a tombstone to the first tag end
            if (((may >> lane) & 1) && r[j] < n_cut) need |= 1u << j;
            pt = (ST[j] >> 63) != 0;
        }
    }
    uint64_t c[CWW];
#pragma unroll
    for (int j = 0; j < CWW; ++j) c[j] = (need >> j) & 1 ? cut[r[j]] : 0;   // (all in flight together)
    uint32_t wr[CWW], agg = kCmpId;
    uint64_t e0[CWW], t0[CWW];
    {
        bool pt = ptw;
#pragma unroll
        for (int j = 0; j < CWW; ++j) {
            const uint64_t SB = __ballot(((need >> j) & 1) && ts[j] <= c[j]);
            wr[j] = cmp_word_rec(V[j], ST[j], TB[j], SB, pt, &e0[j], &t0[j]);
            agg = cmp_then(agg, wr[j], (uint32_t)j * 64);
            pt = (ST[j] >> 63) != 0;
        }
    }
    if (lane == 0) s_rec[wv] = agg;
    __syncthreads();
    // the state the tile's earlier waves leave (under the tile's empty carry)
    uint32_t pre = kCmpId;
    for (int w = 0; w < wv; ++w) pre = cmp_fn_then(pre, s_rec[w] & 3u);
    uint32_t s = cmp_f(pre, 0), cnt = 0;
    uint64_t mine_e = 0, mine_t = 0;
#pragma unroll
    for (int j = 0; j < CWW; ++j) {
        uint64_t e = e0[j], tt = t0[j];
        if (wr[j] & kCmpTE) {
            const uint64_t bit = 1ull << cmp_pos(wr[j]);
            const bool em = cmp_e(wr[j], s) != 0, tmb = em && cmp_t(wr[j], s) != 0;
            e = em ? (e | bit) : (e & ~bit);
            tt = tmb ? (tt | bit) : (tt & ~bit);
        }
        s = cmp_f(wr[j], s);
        cnt += (uint32_t)__popcll(e);
        if (lane == j) {
            mine_e = e;
            mine_t = tt;
        }
    }
    if (BITS && lane < CWW) {
        uint64_t *b = bits + t * (2 * CNW) + (uint64_t)wv * CWW + lane;
        b[0] = mine_e;
        b[CNW] = mine_t;
    }
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = kCmpId, cc = 0;
#pragma unroll
        for (int w = 0; w < CB / 64; ++w) {
            a = cmp_then(a, s_rec[w], (uint32_t)w * 64 * CWW);
            cc += s_cnt[w];
        }
        tcnt[t] = cc;
        rec[t] = a;
    }
}

// ---------------------------------------------------------------- LWW count pass
template <bool BITS>
__global__ __launch_bounds__(CB) void k_cmp_lww_count(crdt_tuples T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                      const uint64_t *__restrict__ cut, uint32_t n_cut,
                                                      uint32_t *__restrict__ tcnt, uint64_t *__restrict__ bits) {
    __shared__ uint32_t s_cnt[CB / 64];
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = blockIdx.x, tb = t * CT;
    if (tb >= n) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i0 = tb + (uint64_t)wv * (64 * CWW);
    uint64_t k[CWW], kn[CWW], kp[CWW];
    uint8_t tm[CWW];
#pragma unroll
    for (int j = 0; j < CWW; ++j) {
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        const uint64_t a = i < n ? i : n - 1, b = i + 1 < n ? i + 1 : n - 1;
        k[j] = T.key[a];
        kn[j] = T.key[b];
        kp[j] = T.key[a > 0 ? a - 1 : 0];
        tm[j] = T.tomb[a];
    }
    // the last tuple of a key's run carries the key's maximal tag.  Per lane a
    // bit per word: ke a key end, more the key has more tuples (the tag's FIRST
    // copy decides), dead the winner's tomb
    uint32_t ke = 0, more = 0, dead = 0;
#pragma unroll
    for (int j = 0; j < CWW; ++j) {
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        if (i < n && !(i + 1 < n && k[j] == kn[j])) {
            ke |= 1u << j;
            if (i > 0 && kp[j] == k[j]) more |= 1u << j;
            if (tm[j] != 0) dead |= 1u << j;
        }
    }
    // ts / rep are read only at a key end that is dead or has more tuples: the
    // loads of all words in flight together, then the few walks, then the cut
    const uint32_t need = more | dead;
    uint64_t x[CWW], px[CWW];
    uint32_t y[CWW], py[CWW];
#pragma unroll
    for (int j = 0; j < CWW; ++j) {
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        const bool nd = (need >> j) & 1, mr = (more >> j) & 1;
        x[j] = nd ? T.ts[i] : 0;
        y[j] = nd ? T.rep[i] : 0;
        px[j] = mr ? T.ts[i - 1] : 0;
        py[j] = mr ? T.rep[i - 1] : 0;
    }
#pragma unroll
    for (int j = 0; j < CWW; ++j) {
        if (((more >> j) & 1) && px[j] == x[j] && py[j] == y[j]) {   // more copies of the winner tag
            const uint64_t i = i0 + (uint64_t)j * 64 + lane;
            uint64_t w = i - 1;
            while (w > 0 && T.key[w - 1] == k[j] && T.ts[w - 1] == x[j] && T.rep[w - 1] == y[j]) --w;
            dead = T.tomb[w] != 0 ? (dead | (1u << j)) : (dead & ~(1u << j));
        }
    }
    uint64_t c[CWW];
#pragma unroll
    for (int j = 0; j < CWW; ++j) c[j] = ((dead >> j) & 1) && y[j] < n_cut ? cut[y[j]] : 0;
    uint32_t cnt = 0;
    uint64_t mine = 0;
#pragma unroll
    for (int j = 0; j < CWW; ++j) {
        const bool drop = ((dead >> j) & 1) && y[j] < n_cut && x[j] <= c[j];
        const uint64_t e = __ballot(((ke >> j) & 1) && !drop);
        cnt += (uint32_t)__popcll(e);
        if (lane == j) mine = e;
    }
    if (BITS && lane < CWW) bits[t * CNW + (uint64_t)wv * CWW + lane] = mine;
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t cc = 0;
#pragma unroll
        for (int w = 0; w < CB / 64; ++w) cc += s_cnt[w];
        tcnt[t] = cc;
    }
}

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_set_compact(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                                const uint64_t *cut_dev, size_t n_cut, const crdt_tuples *out, int64_t *src_out_dev,
                                uint64_t *count) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!t || !count || (mode != CRDT_SET_LWW && mode != CRDT_SET_ORSET)) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62) || n_cut >= (1ULL << 32)) return CRDT_E_RANGE;
    if ((n_cut && !cut_dev) || ((uintptr_t)cut_dev & 7)) return CRDT_E_INVAL;
    if (!out && src_out_dev) return CRDT_E_INVAL;
    if (n_max && tuples_null(t)) return CRDT_E_INVAL;
    if (tuples_misaligned(t) || (out && tuples_misaligned(out)) || ((uintptr_t)src_out_dev & 7)) return CRDT_E_INVAL;
    if (out && n_max) {
        if (tuples_null(out)) return CRDT_E_INVAL;
        if (tuples_overlap(out, n_max, t, n_max) || tuples_overlap(out, n_max, cut_dev, n_cut * 8) ||
            tuples_overlap(out, n_max, src_out_dev, n_max * 8) || tuples_overlap(t, n_max, src_out_dev, n_max * 8) ||
            spans_overlap(cut_dev, n_cut * 8, src_out_dev, n_max * 8))
            return CRDT_E_INVAL;
    }
    const size_t ntiles = (n_max + CT - 1) / CT;
    if (ntiles >= 0x7fffffffULL) return CRDT_E_RANGE;
    TileWs w;
    rc = w.reserve(ctx, ntiles, false, true, 2 * CNW);
    if (rc) return rc;
    const bool lww = mode == CRDT_SET_LWW, wr = out != nullptr;
    const uint32_t nc = (uint32_t)n_cut;
    const hipStream_t s = ctx->stream;
    const unsigned g = (unsigned)ntiles;
    if (ntiles) {
        if (lww && wr) k_cmp_lww_count<true><<<g, CB, 0, s>>>(*t, n_max, n_dev, cut_dev, nc, w.tcnt, w.bits);
        else if (lww) k_cmp_lww_count<false><<<g, CB, 0, s>>>(*t, n_max, n_dev, cut_dev, nc, w.tcnt, w.bits);
        else if (wr) k_cmp_or_count<true><<<g, CB, 0, s>>>(*t, n_max, n_dev, cut_dev, nc, w.tcnt, w.rec, w.bits);
        else k_cmp_or_count<false><<<g, CB, 0, s>>>(*t, n_max, n_dev, cut_dev, nc, w.tcnt, w.rec, w.bits);
    }
    if (lww) w.scan<NoCarry<>>(ctx, n_max, n_dev, 0, nullptr, wr, count);
    else w.scan<CmpCarry>(ctx, n_max, n_dev, 0, nullptr, wr, count);
    if (ntiles && wr)
        tile_write(lww, src_out_dev != nullptr, g, s, *t, n_max, n_dev, w.bits, w.ic, *out, src_out_dev, ctx->dev_status);
    return check_launch(ctx);
}
