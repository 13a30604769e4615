// setread.hpp -- what the reads of a sorted LWW / OR-Set state share
// (setread.hip: crdt_set_elements; mapread.hip: crdt_map_read): the OR-Set
// carry records and their scan policy, the mask-word decision, and the LWW
// count pass.  The semantics are pinned in setread.hip's header comment.
#pragma once
#include "settile.hpp"

namespace crdt {

constexpr int RT = kTile, RB = kTileB, RWW = kTileWW, RNW = kTileNW;   // tile, its threads, words per wave and tile

// ---- carry records.  State s = tor | live << 1 (tor: a tombstone seen in
// the open tag run; live: a live tag closed in the open key run).  A record:
//   bits 0-7   F: the state after the segment, 2 bits per state before it
//   bits 8-11  E: whether the segment's first key end emits, per state before
//   bit  12    the segment holds a key end
//   bits 16-   its position in the segment
constexpr uint32_t kRecId = 0xE4u;       // F = identity, no key end
constexpr uint32_t kRecKE = 1u << 12;
__device__ __forceinline__ uint32_t rec_f(uint32_t r, uint32_t s) { return (r >> (2 * s)) & 3u; }
__device__ __forceinline__ uint32_t rec_e(uint32_t r, uint32_t s) { return (r >> (8 + s)) & 1u; }
__device__ __forceinline__ uint32_t rec_pos(uint32_t r) { return r >> 16; }
// segment a, then segment b (which starts off_b tuples after a's start)
__device__ __forceinline__ uint32_t rec_then(uint32_t a, uint32_t b, uint32_t off_b) {
    uint32_t f = 0, e = 0;
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) {
        const uint32_t as = rec_f(a, s);
        f |= rec_f(b, as) << (2 * s);
        e |= rec_e(b, as) << (8 + s);
    }
    if (a & kRecKE) return f | (a & 0xffff1f00u);
    if (b & kRecKE) return f | e | kRecKE | ((rec_pos(b) + off_b) << 16);
    return f;
}
// F alone (the scan's operator)
__device__ __forceinline__ uint32_t fn_then(uint32_t a, uint32_t b) {
    uint32_t f = 0;
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) f |= rec_f(b, rec_f(a, s)) << (2 * s);
    return f;
}

// One mask word of an OR-Set state: V valid tuples (low bits), ST / SK the
// tuple has a successor with the same tag / key, TB its tomb, pt / pk the
// word's first tuple continues the tag / key run before it.  *emit0 = the
// emitting key ends under an empty carry; *lv0 (when asked) = the live tags,
// at their run ends, under an empty carry.
__device__ __forceinline__ uint32_t or_word_rec(uint64_t V, uint64_t ST, uint64_t SK, uint64_t TB, bool pt, bool pk,
                                                uint64_t *emit0, uint64_t *lv0 = nullptr) {
    *emit0 = 0;
    if (lv0) *lv0 = 0;
    if (V == 0) return kRecId;
    const uint64_t TE = V & ~ST, KE = V & ~SK;           // tag run ends, key run ends (a subset)
    // segmented any(): the carry of an add runs from a set bit up to its run's end bit and stops there
    const uint64_t dead = TE & (((V & ~TE) + (TB & ~TE)) | TB);
    const uint64_t LV = TE & ~dead;                      // live tags, at their ends
    if (lv0) *lv0 = LV;
    *emit0 = KE & (((V & ~KE) + (LV & ~KE)) | LV);
    const bool any_te = TE != 0, any_ke = KE != 0;
    const uint64_t f_te = TE & (0 - TE), f_ke = KE & (0 - KE);
    const bool lead_tor = any_te ? (dead & f_te) != 0 : TB != 0;
    const uint64_t up_k = any_ke ? (f_ke | (f_ke - 1)) : ~0ull;
    const bool lead_rest = (LV & ~f_te & up_k) != 0;     // live tags of the leading key run but the first closing tag
    bool trail_tor = false, trail_live = false;          // the open runs' state at the end
    if (any_te) {
        const uint64_t h = 1ull << (63 - __builtin_clzll(TE));
        trail_tor = (TB & ~(h | (h - 1))) != 0;
    }
    if (any_ke) {
        const uint64_t h = 1ull << (63 - __builtin_clzll(KE));
        trail_live = (LV & ~(h | (h - 1))) != 0;
    }
    uint32_t r = any_ke ? (kRecKE | ((uint32_t)__builtin_ctzll(KE) << 16)) : 0u;
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) {
        const bool tin = pt && (s & 1), lin = pk && (s & 2);
        const bool first_live = any_te && !(tin || lead_tor);
        const bool lead_live = lin || first_live || lead_rest;
        const bool tor = any_te ? trail_tor : (tin || lead_tor);
        const bool live = any_ke ? trail_live : lead_live;
        r |= ((tor ? 1u : 0u) | (live ? 2u : 0u)) << (2 * s);
        r |= (lead_live ? 1u : 0u) << (8 + s);
    }
    return r;
}

// the scan's view of a record: F composes, the first key end flips where its
// outcome differs from the empty carry's.  WPT: the bitmap words a tile keeps
// (`emit` first).
template <uint32_t WPT>
struct ReadCarryT : PlainTiles {
    static constexpr bool kHas = true;
    static constexpr uint32_t kId = kRecId, kStride = WPT, kEmit = 0, kAux = 0;   // (`emit` alone is patched)
    static __device__ __forceinline__ uint32_t part(uint32_t r) { return r & 0xffu; }
    static __device__ __forceinline__ uint32_t then(uint32_t a, uint32_t b) { return fn_then(a, b); }
    static __device__ __forceinline__ uint32_t seed(uint32_t) { return kRecId; }
    static __device__ __forceinline__ uint32_t enter(uint32_t p, uint32_t s) { return rec_f(p, s); }
    static __device__ __forceinline__ uint32_t step(uint32_t s, uint32_t r) { return rec_f(r, s); }
    static __device__ __forceinline__ uint32_t redecide(uint32_t r, uint32_t s) {
        if (!((r & kRecKE) && rec_e(r, s) != rec_e(r, 0))) return 0;
        return redo(rec_pos(r), true, false, rec_e(r, s) != 0);
    }
};
using ReadCarry = ReadCarryT<RNW>;

// ---------------------------------------------------------------- LWW count pass
template <bool BITS>
__global__ __launch_bounds__(RB) void k_lww_read(crdt_tuples T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                 uint32_t *__restrict__ tcnt, uint64_t *__restrict__ bits) {
    __shared__ uint32_t s_cnt[RB / 64];
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = blockIdx.x, tb = t * RT;
    if (tb >= n) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i0 = tb + (uint64_t)wv * (64 * RWW);
    uint64_t k[RWW], kn[RWW], kp[RWW];
    uint8_t tm[RWW];
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        const uint64_t a = i < n ? i : n - 1, b = i + 1 < n ? i + 1 : n - 1;
        k[j] = T.key[a];
        kn[j] = T.key[b];
        kp[j] = T.key[a > 0 ? a - 1 : 0];
        tm[j] = T.tomb[a];
    }
    uint32_t cnt = 0;
    uint64_t mine = 0;
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        // the last tuple of a key's run carries the key's maximal tag
        const bool ke = i < n && !(i + 1 < n && k[j] == kn[j]);
        bool live = ke && tm[j] == 0;
        if (ke && i > 0 && kp[j] == k[j]) {              // the key has more tuples: the tag's FIRST copy decides
            const uint64_t x = T.ts[i];
            const uint32_t y = T.rep[i];
            uint64_t w = i;
            while (w > 0 && T.key[w - 1] == k[j] && T.ts[w - 1] == x && T.rep[w - 1] == y) --w;
            live = T.tomb[w] == 0;
        }
        const uint64_t e = __ballot(live);
        cnt += (uint32_t)__popcll(e);
        if (lane == j) mine = e;
    }
    if (BITS && lane < RWW) bits[t * RNW + (uint64_t)wv * RWW + lane] = mine;
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < RB / 64; ++w) c += s_cnt[w];
        tcnt[t] = c;
    }
}

}  // namespace crdt
