// setread.hip -- the read side of the keyed sets: live elements, cardinality
// and membership of a sorted LWW / OR-Set state.
//
// Semantics, pinned to the merges of sets.hip.  For tuples t[0 .. n) sorted
// ascending by (key, ts, rep), copies of one tag in any order:
//   OR-Set : a tag is live iff none of its copies is tombstoned; a key is a
//            member iff it has a live tag.
//   LWW    : a key is a member iff the FIRST copy of its maximal (ts, rep)
//            tag has tomb == 0 (the winner rule of sets.hip).
// elements(t) = the member keys, ascending, each once = the keys of
// merge(t, {}) whose (OR-Set: any) output tuple has tomb == 0.
//
// GPU structure: a streaming job over tiles of 2048 tuples, one workgroup of
// four waves each, every decision a wave64 ballot word -- the tile's logic
// runs on 64-bit masks (same-key-as-next, same-tag-as-next, tomb), one mask
// bit per tuple, a segmented OR per mask word being one 64-bit add.
//   count : per tile the `emit` bitmap (bit set at the LAST tuple of a member
//           key's run), the tile's member count and, OR-Set only, a carry
//           record.  No tile waits for another: each evaluates with an empty
//           carry; what a carry can change is one bit, the first key end.
//   scan  : k_tile_scan<ReadCarry> (settile.hpp; LWW: <NoCarry>).  A tile's
//           record is the FUNCTION it applies to the carry state (tomb-OR of
//           the open tag run, live-any of the open key run: 2 bits, so a
//           4-entry table) plus the 4 outcomes of its first key end;
//           composing tables is associative, so the carries into all tiles
//           are a prefix scan of compositions -- linear however many tiles
//           one key or tag spans.  The scan patches the at most one affected
//           emit bit and count per tile.
//   write : (elements only) k_tile_write_field (settile.hpp): each emitting
//           key at its rank.
// LWW needs no carry: the last tuple of a key's run holds the key's maximal
// tag, and the walk back over equal-tag copies to the first one's tomb goes
// through global memory, as k_lww_write's does.
// The carry records, the mask-word decision (or_word_rec), ReadCarry and the
// LWW count pass are in setread.hpp: the map read (mapread.hip) shares them.
//
// The tuple count may stay on the device (n_dev): every kernel reads it,
// tiles at or past min(*n_dev, n_max) do nothing, and *n_dev > n_max touches
// no tuple, stores a count of ~0 and raises CRDT_DEV_RANGE.  No kernel reads
// an index at or past that length or before 0.
#include "setread.hpp"

namespace crdt {

// ---------------------------------------------------------------- OR-Set count pass
template <bool BITS>
__global__ __launch_bounds__(RB) void k_or_read(crdt_tuples T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                uint32_t *__restrict__ tcnt, uint32_t *__restrict__ rec,
                                                uint64_t *__restrict__ bits) {
    __shared__ uint32_t s_rec[RB / 64], s_cnt[RB / 64];
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
    uint64_t e0[RWW];
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        const bool v = i < n, sk = i + 1 < n && k[j] == kn[j];
        const bool st = sk && ts[j] == tn[j] && r[j] == rn[j];
        const uint64_t V = __ballot(v), SK = __ballot(sk), ST = __ballot(st), TB = __ballot(v && tm[j] != 0);
        wr[j] = or_word_rec(V, ST, SK, TB, pt, pk, &e0[j]);
        agg = rec_then(agg, wr[j], (uint32_t)j * 64);
        pt = (ST >> 63) != 0;
        pk = (SK >> 63) != 0;
    }
    if (lane == 0) s_rec[wv] = agg;
    __syncthreads();
    // the state the tile's earlier waves leave (under the tile's empty carry)
    uint32_t pre = kRecId;
    for (int w = 0; w < wv; ++w) pre = fn_then(pre, s_rec[w] & 0xffu);
    uint32_t s = rec_f(pre, 0), cnt = 0;
    uint64_t mine = 0;
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        uint64_t e = e0[j];
        if ((wr[j] & kRecKE) && rec_e(wr[j], s) != rec_e(wr[j], 0)) e ^= 1ull << rec_pos(wr[j]);
        s = rec_f(wr[j], s);
        cnt += (uint32_t)__popcll(e);
        if (lane == j) mine = e;
    }
    if (BITS && lane < RWW) bits[t * RNW + (uint64_t)wv * RWW + lane] = mine;
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = kRecId, c = 0;
#pragma unroll
        for (int w = 0; w < RB / 64; ++w) {
            a = rec_then(a, s_rec[w], (uint32_t)w * 64 * RWW);
            c += s_cnt[w];
        }
        tcnt[t] = c;
        rec[t] = a;
    }
}

// ---------------------------------------------------------------- membership
// out[i] = probes[i] occurs in v[0 .. n): one probe per lane, the binary
// search of crdt_u64_lower_bound and an equality test.  (Its loads are what
// it costs, one cache line each until the last few steps share one: a 4-ary
// step per lane, 3 pivots in flight, measured 1.17x the time at 1M probes
// into 7M keys, a 16-ary one 2.3x -- DESIGN.md §5.12.)
__global__ void k_u64_contains(const uint64_t *__restrict__ v, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                               const uint64_t *__restrict__ probes, uint64_t m, uint8_t *__restrict__ out,
                               uint32_t *__restrict__ err) {
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) {
        n = 0;
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, CRDT_DEV_RANGE);
    }
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const uint64_t x = probes[i];
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (v[mid] < x) lo = mid + 1;
            else hi = mid;
        }
        out[i] = lo < n && v[lo] == x ? 1 : 0;
    }
}

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_set_elements(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                                 uint64_t *keys_out, uint64_t *count) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!t || !count || (mode != CRDT_SET_LWW && mode != CRDT_SET_ORSET)) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62)) return CRDT_E_RANGE;
    if (n_max) {
        if (tuples_null(t) || tuples_misaligned(t)) return CRDT_E_INVAL;
        if (keys_out && (((uintptr_t)keys_out & 7) || tuples_overlap(t, n_max, keys_out, n_max * 8))) return CRDT_E_INVAL;
    }
    const size_t ntiles = (n_max + RT - 1) / RT;
    if (ntiles >= 0x7fffffffULL) return CRDT_E_RANGE;
    TileWs w;
    rc = w.reserve(ctx, ntiles, false, true, RNW);
    if (rc) return rc;
    uint32_t *const tcnt = w.tcnt, *const rec = w.rec;
    uint64_t *const ic = w.ic, *const bits = w.bits;
    const bool lww = mode == CRDT_SET_LWW, wr = keys_out != nullptr;
    const hipStream_t s = ctx->stream;
    if (ntiles) {
        const unsigned g = (unsigned)ntiles;
        if (lww && wr) k_lww_read<true><<<g, RB, 0, s>>>(*t, n_max, n_dev, tcnt, bits);
        else if (lww) k_lww_read<false><<<g, RB, 0, s>>>(*t, n_max, n_dev, tcnt, bits);
        else if (wr) k_or_read<true><<<g, RB, 0, s>>>(*t, n_max, n_dev, tcnt, rec, bits);
        else k_or_read<false><<<g, RB, 0, s>>>(*t, n_max, n_dev, tcnt, rec, bits);
    }
    if (lww) w.scan<NoCarry<>>(ctx, n_max, n_dev, 0, nullptr, wr, count);
    else w.scan<ReadCarry>(ctx, n_max, n_dev, 0, nullptr, wr, count);
    if (ntiles && wr)
        k_tile_write_field<uint64_t><<<(unsigned)ntiles, RB, 0, s>>>(t->key, n_max, n_dev, bits, ic, keys_out,
                                                                     ctx->dev_status);
    return check_launch(ctx);
}

extern "C" int crdt_u64_contains(crdt_ctx *ctx, const uint64_t *sorted, size_t n_max, const uint64_t *n_dev,
                                 const uint64_t *probes, size_t m, uint8_t *out) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (n_max >= (1ULL << 62)) return CRDT_E_RANGE;
    if (m == 0) return CRDT_OK;
    if (!probes || !out || (n_max && !sorted) || ((uintptr_t)sorted & 7) || ((uintptr_t)probes & 7))
        return CRDT_E_INVAL;
    k_u64_contains<<<grid_for(m, 256, (unsigned)ctx->num_cus * 8), 256, 0, ctx->stream>>>(
        sorted, n_max, n_dev, probes, m, out, ctx->dev_status);
    return check_launch(ctx);
}
