// mapread.hip -- reading a map kept as a sorted LWW / OR-Set state with a value
// column beside the tuples: each member key's winning tuple and sibling count
// (crdt_map_read), and a batched point lookup (crdt_map_lookup).  DESIGN.md
// §5.21.
//
// Semantics.  t[0 .. n) sorted ascending by (key, ts, rep), copies of one tag
// in any order and number; n from n_max / n_dev exactly as crdt_set_elements
// takes it.  A causal-form state (all tombs 0) is read in OR-Set mode.
//   member keys : exactly those of crdt_set_elements(mode, t), ascending, one
//                 row each.
//   winner      : OR-Set -- the greatest (ts, rep) LIVE tag of the key (a tag
//                 is live iff none of its copies is tombstoned).
//                 LWW    -- the key's maximal tag; the key is a member iff the
//                 tomb of that tag's FIRST copy is 0.
//   win (int64) : the index in t of the FIRST copy of the winner tag -- the
//                 a-side encoding of crdt_src_gather, so
//                 crdt_src_gather(win, n_max, count_dev, val, n, NULL, 0,
//                 out_val, elem) yields the map's values with no read-back.
//   nsib (u32)  : OR-Set -- the number of distinct live tags of the key (>= 1,
//                 saturating at 2^32 - 1); LWW -- 1.  nsib > 1: concurrent puts
//                 left the key multi-valued.
// The lookup gives, per probe key, the win / nsib the read gives that key, or
// (-1, 0) for a key that is not a member.  To crdt_src_gather -1 is element 0
// of the b side: a one-element b_col is the default of the missing keys.
//
// GPU structure of the read: setread.hip's count / scan / write over tiles of
// 2048 tuples (settile.hpp), one workgroup of four waves per tile.
//   count : LWW -- k_lww_read (setread.hpp), unchanged.  OR-Set -- k_or_read's
//           decision, the `emit` bitmap (a member key's LAST tuple) under an
//           empty carry and the ReadCarry record, plus a second bitmap LV: the
//           live tags at their run ends.  LV is exact when the pass ends: the
//           one LV bit a carry can change is the tile's first tag end, when
//           the tile's first tuple continues a tag, and the one tile that
//           holds that tag's end walks its earlier copies' tombs through
//           global memory (one thread; tiles inside the run walk nothing, so
//           the walks are linear in the copies, as the first-copy walk is).
//   scan  : k_tile_scan<ReadCarry> patches the one emit bit per tile the carry
//           (tomb-OR of the open tag run, a live tag seen in the open key run)
//           can change.  LWW: <NoCarry>.
//   write : per emit bit, at its rank: OR-Set -- the winner's end is the
//           highest LV bit at or below the emit bit, searched 64 tuples a step
//           through the bitmap words in global memory (the tile's own, then
//           earlier tiles'); nsib is the population count of LV over (previous
//           emit bit, this emit bit] -- keys that are not members have no LV
//           bit, the intervals are disjoint, so the word walks are linear in
//           total; without nsib the walk stops at the first LV bit.  Then the
//           walk back over equal-tag copies to the first one, through global
//           memory, as k_tile_write's does.
// The lookup is one thread per probe: an upper-bound binary search on t.key
// clamped to the length, then the walk over the key's tags from the run's end.
//
// No kernel reads a tuple at or past min(*n_dev, n_max) or before 0; *n_dev >
// n_max touches no tuple (read: count = ~0, nothing else written; lookup: every
// win -1, every nsib 0) and raises CRDT_DEV_RANGE.
#include "setread.hpp"

namespace crdt {

__device__ __forceinline__ bool same_tag(const crdt_tuples &T, uint64_t i, uint64_t key, uint64_t ts, uint32_t rep) {
    return T.key[i] == key && T.ts[i] == ts && T.rep[i] == rep;
}

// ---------------------------------------------------------------- OR-Set count pass
// k_or_read<true> with the LV bitmap: a tile's words are `emit` (under an
// empty carry; the scan patches it), then LV (exact).
__global__ __launch_bounds__(RB) void k_map_or_count(crdt_tuples T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                     uint32_t *__restrict__ tcnt, uint32_t *__restrict__ rec,
                                                     uint64_t *__restrict__ bits) {
    __shared__ uint32_t s_rec[RB / 64], s_cnt[RNW], s_tin;
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = blockIdx.x, tb = t * RT;
    if (tb >= n) return;                                 // (uniform; so n > 0 below)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i0 = tb + (uint64_t)wv * (64 * RWW);
    // every load up front, indices clamped into [0, n): nothing at or past n is read
    uint64_t k[RWW], kn[RWW], ts[RWW], tn[RWW];
    uint32_t r[RWW], rn[RWW];
    uint8_t tm[RWW];
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
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
    // the tuple before the wave's first: does it open the wave's first runs?
    bool pk0 = false, pt0 = false;
    if (lane == 0 && i0 > 0 && i0 < n) {
        pk0 = T.key[i0 - 1] == k[0];
        pt0 = pk0 && T.ts[i0 - 1] == ts[0] && T.rep[i0 - 1] == r[0];
    }
    bool pk = __ballot(pk0) != 0, pt = __ballot(pt0) != 0;
    uint32_t wr[RWW], agg = kRecId;
    uint64_t mine = 0, mine_lv = 0;                      // lane j: word j's emit (under the wave's empty carry) and LV
    uint32_t my_fte = 0xffu;                             // lane j: word j's first tag end where the carried tag run reaches it, else 0xff
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        // the word's valid tuples, and those with a successor, as scalar masks (the loads were clamped)
        const uint64_t wb = i0 + (uint64_t)j * 64, nv = wb < n ? n - wb : 0;
        const uint64_t V = nv >= 64 ? ~0ull : (1ull << nv) - 1, V1 = nv > 64 ? ~0ull : V >> 1;
        const bool sk = k[j] == kn[j];
        const uint64_t SK = __ballot(sk) & V1, ST = __ballot(sk && ts[j] == tn[j] && r[j] == rn[j]) & V1;
        const uint64_t TB = __ballot(tm[j] != 0) & V;
        uint64_t e0, lv;
        wr[j] = or_word_rec(V, ST, SK, TB, pt, pk, &e0, &lv);
        const uint64_t TE = V & ~ST;
        if (lane == j) {
            mine = e0;
            mine_lv = lv;
            my_fte = pt && TE != 0 ? (uint32_t)__builtin_ctzll(TE) : 0xffu;
        }
        agg = rec_then(agg, wr[j], (uint32_t)j * 64);
        pt = (ST >> 63) != 0;
        pk = (SK >> 63) != 0;
        // the word's masks are consumed here, not sunk past the barriers: eight words' worth would not fit the SGPRs
        asm volatile("" : "+v"(mine), "+v"(mine_lv), "+v"(my_fte));
    }
    if (lane == 0) s_rec[wv] = agg;
    // The tile's first tuple continues a tag that ends in the tile (the tuple
    // after the tile is not of it): the tomb-OR of its copies before the tile,
    // exactly.  A tile inside the run walks nothing.
    if (threadIdx.x == 0) {
        uint32_t tin = 0;
        if (pt0 && !(tb + RT < n && same_tag(T, tb + RT, k[0], ts[0], r[0]))) {
            uint64_t w = tb;
            while (!tin && w > 0 && same_tag(T, w - 1, k[0], ts[0], r[0])) {
                --w;
                tin = T.tomb[w] != 0 ? 1u : 0u;
            }
        }
        s_tin = tin;
    }
    __syncthreads();
    // the state the tile's earlier waves leave: s under the tile's empty carry
    // (emit; the scan's convention), s2 under the true tomb-OR (LV)
    uint32_t pre = kRecId;
    for (int w = 0; w < wv; ++w) pre = fn_then(pre, s_rec[w] & 0xffu);
    uint32_t s = rec_f(pre, 0), s2 = rec_f(pre, s_tin);
    uint64_t flip = ~0ull;                               // byte j: the bit of word j's emit to flip, else 0xff
    uint32_t kill = 0;                                   // bit j: word j is entered with a tombstone in the open tag run
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        if ((wr[j] & kRecKE) && rec_e(wr[j], s) != rec_e(wr[j], 0)) {   // the word's first key end, re-decided
            flip ^= (uint64_t)(0xffu ^ rec_pos(wr[j])) << (8 * j);
        }
        kill |= (s2 & 1u) << j;
        s = rec_f(wr[j], s);
        s2 = rec_f(wr[j], s2);
    }
    if (lane < RWW) {
        const uint32_t bf = (uint32_t)(flip >> (8 * lane)) & 0xffu;
        if (bf != 0xffu) mine ^= 1ull << bf;
        // a tombstoned earlier copy kills the carried tag
        if (((kill >> lane) & 1u) && my_fte != 0xffu) mine_lv &= ~(1ull << my_fte);
        s_cnt[wv * RWW + lane] = (uint32_t)__popcll(mine);
        bits[t * (2 * RNW) + (uint64_t)wv * RWW + lane] = mine;
        bits[t * (2 * RNW) + RNW + (uint64_t)wv * RWW + lane] = mine_lv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = kRecId, c = 0;
#pragma unroll
        for (int w = 0; w < RB / 64; ++w) a = rec_then(a, s_rec[w], (uint32_t)w * 64 * RWW);
#pragma unroll
        for (int q = 0; q < RNW; ++q) c += s_cnt[q];
        tcnt[t] = c;
        rec[t] = a;
    }
}

// ---------------------------------------------------------------- write pass
// Every emit bit at its rank: the key, the first copy of the winner tag, the
// sibling count.  OR-Set bitmaps: word g of the state (tuples 64 g ..) is the
// tile's g / RNW, its word g % RNW.
template <bool LWW, bool KEYS, bool NSIB>
__global__ __launch_bounds__(kTileB) void k_map_write(crdt_tuples T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                      const uint64_t *__restrict__ bits,
                                                      const uint64_t *__restrict__ ic, uint64_t *__restrict__ keys,
                                                      int64_t *__restrict__ win, uint32_t *__restrict__ nsib,
                                                      uint32_t *__restrict__ err) {
    tile_emit_by_position<!LWW>(n_max, n_dev, bits, ic, err, [&](uint64_t i, uint64_t at, uint8_t aux) {
        uint64_t e = i, sib = 1;                         // the winner tag's last copy; the key's live tags
        if (!LWW && (NSIB || !aux)) {
            uint64_t g = i >> 6;
            const uint64_t upto = (2ull << (i & 63)) - 1;    // bits 0 .. i & 63
            const uint64_t *p = bits + (g / RNW) * (2 * RNW) + (g % RNW);
            uint64_t E = p[0] & (upto >> 1), L = p[RNW] & upto;
            bool found = false;
            sib = 0;
            for (;;) {
                if (E) L &= ~((2ull << (63 - __builtin_clzll(E))) - 1);   // the tags after the previous member key's end
                if (!found && L) {
                    e = g * 64 + (uint64_t)(63 - __builtin_clzll(L));
                    found = true;
                }
                sib += (uint64_t)__popcll(L);
                if (E || g == 0 || (!NSIB && found)) break;
                --g;
                p = bits + (g / RNW) * (2 * RNW) + (g % RNW);
                E = p[0];
                L = p[RNW];
            }
        }
        const uint64_t key = T.key[i];
        uint64_t f = e;
        if (e > 0 && T.key[e - 1] == key) {
            const uint64_t ts = T.ts[e];
            const uint32_t rep = T.rep[e];
            while (f > 0 && same_tag(T, f - 1, key, ts, rep)) --f;
        }
        if (KEYS) keys[at] = key;
        win[at] = (int64_t)f;
        if (NSIB) nsib[at] = sib > 0xffffffffull ? 0xffffffffu : (uint32_t)sib;
    });
}
template <bool LWW, class... A>
static void map_write(bool keys, bool sib, unsigned g, hipStream_t s, A... a) {
    if (keys && sib) k_map_write<LWW, true, true><<<g, kTileB, 0, s>>>(a...);
    else if (keys) k_map_write<LWW, true, false><<<g, kTileB, 0, s>>>(a...);
    else if (sib) k_map_write<LWW, false, true><<<g, kTileB, 0, s>>>(a...);
    else k_map_write<LWW, false, false><<<g, kTileB, 0, s>>>(a...);
}

// ---------------------------------------------------------------- lookup
// One probe per lane: the end of the key's run by binary search (the loads are
// what it costs, as in k_u64_contains), then the key's tags from the run's end.
template <bool LWW, bool NSIB>
__global__ void k_map_lookup(crdt_tuples T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                             const uint64_t *__restrict__ probes, uint64_t m, int64_t *__restrict__ win,
                             uint32_t *__restrict__ nsib, uint32_t *__restrict__ err) {
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) {
        n = 0;
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, CRDT_DEV_RANGE);
    }
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const uint64_t x = probes[i];
        uint64_t lo = 0, hi = n;                         // lo -> the first tuple with a key above x
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (T.key[mid] <= x) lo = mid + 1;
            else hi = mid;
        }
        int64_t w = -1;
        uint64_t sib = 0;
        uint64_t j = lo;                                 // one past the last copy of the tag looked at
        while (j > 0 && T.key[j - 1] == x) {
            const uint64_t ts = T.ts[j - 1];
            const uint32_t rep = T.rep[j - 1];
            uint64_t f = j - 1;
            bool dead = T.tomb[f] != 0;
            while (f > 0 && same_tag(T, f - 1, x, ts, rep)) {
                --f;
                dead = dead || T.tomb[f] != 0;
            }
            if (LWW) {                                   // the maximal tag's first copy decides
                if (T.tomb[f] == 0) {
                    w = (int64_t)f;
                    sib = 1;
                }
                break;
            }
            if (!dead) {
                if (w < 0) w = (int64_t)f;
                ++sib;
                if (!NSIB) break;
            }
            j = f;
        }
        win[i] = w;
        if (NSIB) nsib[i] = sib > 0xffffffffull ? 0xffffffffu : (uint32_t)sib;
    }
}

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_map_read(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                             uint64_t *keys_out, int64_t *win_out, uint32_t *nsib_out, uint64_t *count) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!t || !count || (mode != CRDT_SET_LWW && mode != CRDT_SET_ORSET)) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62)) return CRDT_E_RANGE;
    if (((uintptr_t)keys_out & 7) || ((uintptr_t)win_out & 7) || ((uintptr_t)nsib_out & 3)) return CRDT_E_INVAL;
    if (n_max) {
        if (!win_out || tuples_null(t) || tuples_misaligned(t)) return CRDT_E_INVAL;
        if (tuples_overlap(t, n_max, keys_out, n_max * 8) || tuples_overlap(t, n_max, win_out, n_max * 8) ||
            tuples_overlap(t, n_max, nsib_out, n_max * 4) || spans_overlap(keys_out, n_max * 8, win_out, n_max * 8) ||
            spans_overlap(keys_out, n_max * 8, nsib_out, n_max * 4) ||
            spans_overlap(win_out, n_max * 8, nsib_out, n_max * 4))
            return CRDT_E_INVAL;
    }
    const size_t ntiles = (n_max + RT - 1) / RT;
    if (ntiles >= 0x7fffffffULL) return CRDT_E_RANGE;
    TileWs w;
    rc = w.reserve(ctx, ntiles, false, true, 2 * RNW);
    if (rc) return rc;
    const bool lww = mode == CRDT_SET_LWW, keys = keys_out != nullptr, sib = nsib_out != nullptr;
    const hipStream_t s = ctx->stream;
    const unsigned g = (unsigned)ntiles;
    if (ntiles) {
        if (lww) k_lww_read<true><<<g, RB, 0, s>>>(*t, n_max, n_dev, w.tcnt, w.bits);
        else k_map_or_count<<<g, RB, 0, s>>>(*t, n_max, n_dev, w.tcnt, w.rec, w.bits);
    }
    if (lww) w.scan<NoCarry<>>(ctx, n_max, n_dev, 0, nullptr, true, count);
    else w.scan<ReadCarryT<2 * RNW>>(ctx, n_max, n_dev, 0, nullptr, true, count);
    if (ntiles) {
        if (lww) map_write<true>(keys, sib, g, s, *t, n_max, n_dev, w.bits, w.ic, keys_out, win_out, nsib_out, ctx->dev_status);
        else map_write<false>(keys, sib, g, s, *t, n_max, n_dev, w.bits, w.ic, keys_out, win_out, nsib_out, ctx->dev_status);
    }
    return check_launch(ctx);
}

extern "C" int crdt_map_lookup(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                               const uint64_t *probes, size_t m, int64_t *win_out, uint32_t *nsib_out) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!t || (mode != CRDT_SET_LWW && mode != CRDT_SET_ORSET)) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62) || m >= (1ULL << 60)) return CRDT_E_RANGE;
    if (m == 0) return CRDT_OK;
    if (!probes || !win_out || (n_max && tuples_null(t)) || tuples_misaligned(t)) return CRDT_E_INVAL;
    if (((uintptr_t)probes & 7) || ((uintptr_t)win_out & 7) || ((uintptr_t)nsib_out & 3)) return CRDT_E_INVAL;
    if (tuples_overlap(t, n_max, win_out, m * 8) || tuples_overlap(t, n_max, nsib_out, m * 4) ||
        spans_overlap(probes, m * 8, win_out, m * 8) || spans_overlap(probes, m * 8, nsib_out, m * 4) ||
        spans_overlap(win_out, m * 8, nsib_out, m * 4))
        return CRDT_E_INVAL;
    const unsigned g = grid_for(m, 256, (unsigned)ctx->num_cus * 8);
    const hipStream_t s = ctx->stream;
    const bool lww = mode == CRDT_SET_LWW, sib = nsib_out != nullptr;
    if (lww && sib) k_map_lookup<true, true><<<g, 256, 0, s>>>(*t, n_max, n_dev, probes, m, win_out, nsib_out, ctx->dev_status);
    else if (lww) k_map_lookup<true, false><<<g, 256, 0, s>>>(*t, n_max, n_dev, probes, m, win_out, nsib_out, ctx->dev_status);
    else if (sib) k_map_lookup<false, true><<<g, 256, 0, s>>>(*t, n_max, n_dev, probes, m, win_out, nsib_out, ctx->dev_status);
    else k_map_lookup<false, false><<<g, 256, 0, s>>>(*t, n_max, n_dev, probes, m, win_out, nsib_out, ctx->dev_status);
    return check_launch(ctx);
}
