// setdelta.hip -- set deltas: the tuples of one sorted LWW / OR-Set state that
// another lacks (crdt_set_delta).
//
// Semantics, pinned to the merges of sets.hip.  delta(src, dst) is the
// smallest D with merge(dst, D) == merge(dst, src), dst the left (tie-winning)
// operand; both sides sorted ascending by (key, ts, rep), copies of one tag in
// any order on either side:
//   OR-Set : per distinct tag g of src, tomb_s / tomb_d = the OR over src's /
//            dst's copies of g; g ships iff dst holds no copy of g, or
//            tomb_s == 1 && tomb_d == 0; once, with tomb = tomb_s.
//   LWW    : per distinct key k of src, src's winner (its maximal (ts, rep)
//            tag, the tomb of that tag's first copy) ships iff dst holds no
//            tuple of k or src's maximal tag is strictly greater than dst's.
// D comes out in ascending tuple order.
//
// GPU structure: the merges' two passes over the stable merged order of
// (dst, src), dst first on an equal tag (LWW: on an equal key), every
// decision taken at the LAST merged item of a tag run (LWW: key run) -- that
// item is a src item exactly when src holds the tag (key):
//   split : k_mp_split (settile.hpp), side a = dst, by keys alone for LWW;
//   count : per tile both runs staged in LDS (plain loads, clamped to each
//           side's length) and merged, 512 threads x 4 items.  OR-Set: a
//           thread carries the open tag run's state (dst copy seen, dst
//           tomb-OR, src tomb-OR: 3 bits); a run end resets it, so a thread's
//           effect on the state is "reset, then OR" -- an associative record
//           scanned over the workgroup; what an earlier thread or tile can
//           change is one decision, the first run end after it.  LWW merges
//           keys only and needs no carry: the run end is src's maximal tag,
//           dst's is the dst element merged just before the key's src items;
//           ts / rep are read only there.  Output: bitmaps in merged order
//           (`iss`: a src item, `emit`, OR-Set `tomb`: the emitted tomb), the
//           tile's count and record;
//   scan  : k_tile_scan<DeltaCarry> (settile.hpp; LWW: <NoCarry>): the records
//           scan as they are, each tile's first run end, when a src item, is
//           re-decided with the carry's bits ORed into its run's own;
//   write : (out != NULL) one output per lane, by rank (rank_words /
//           rank_select, settile.hpp): its src index is the count of src items
//           before it; the four fields stored at the rank (LWW: the tomb of
//           the first copy of the tag, a walk back over src).
//
// Either length may stay on the device.  A value past its n_max touches no
// tuple, stores a count of ~0 and raises CRDT_DEV_RANGE; no kernel reads an
// index at or past min(*n_dev, n_max) of its side, or before 0.
#include "settile.hpp"

namespace crdt {

constexpr int DT = kTile;                 // merge items per tile
constexpr int DCB = 512;                  // count pass threads
constexpr int DNI = DT / DCB;             // merge items per count thread
constexpr int DNW = kTileNW;              // words per tile and bitmap
constexpr int DWB = 256;                  // write pass threads (one output each per round)
constexpr int DCAP = DT + 4;              // staged slots: each side's run, the element before and the one after it

// ---- the open tag run's state and a segment's record (OR-Set)
constexpr uint32_t kHasD = 1, kTorD = 2, kTorS = 4;   // dst copy seen / dst tomb-OR / src tomb-OR
constexpr uint32_t kEnd = 8;                          // the segment holds a run end: the state before it is dropped
// record of a tile: bits 0-3 as above (the state it leaves), bits 4-6 the
// state its items add to the run of its first run end, bit 7 that end is a
// src item, bits 16- its position in the tile
__device__ __forceinline__ uint32_t st_then(uint32_t a, uint32_t b) { return (b & kEnd) ? b : (a | b); }
__device__ __forceinline__ bool st_ships(uint32_t s) { return !(s & kHasD) || ((s & kTorS) && !(s & kTorD)); }

// tiles of the call: none without a src tuple
__device__ __forceinline__ uint64_t delta_tiles(uint64_t ns, uint64_t nd) { return ns ? (ns + nd + DT - 1) / DT : 0; }
// the shared passes' view: side a = dst (it wins ties), side b = src
struct DeltaTiles {
    static __device__ __forceinline__ uint64_t tiles(uint64_t nd, uint64_t ns) { return delta_tiles(ns, nd); }
};
// the scan's view of a record: the state scans as it is; the first run end,
// when a src item, is re-decided with the carry's bits ORed into its run's own
struct DeltaCarry : DeltaTiles {
    static constexpr bool kHas = true;
    static constexpr uint32_t kId = 0, kStride = 3 * DNW, kEmit = DNW, kAux = 2 * DNW;   // (`iss`, `emit`, `tomb`)
    static __device__ __forceinline__ uint32_t part(uint32_t r) { return r & 0xfu; }
    static __device__ __forceinline__ uint32_t then(uint32_t a, uint32_t b) { return st_then(a, b); }
    static __device__ __forceinline__ uint32_t seed(uint32_t s) { return s; }
    static __device__ __forceinline__ uint32_t enter(uint32_t p, uint32_t) { return p; }
    static __device__ __forceinline__ uint32_t step(uint32_t s, uint32_t r) { return st_then(s, r & 0xfu); }
    static __device__ __forceinline__ uint32_t redecide(uint32_t r, uint32_t s) {
        if (!((r & kEnd) && (r & 0x80u))) return 0;      // (a tile past the last holds no end)
        const uint32_t own = (r >> 4) & 7u, all = own | (s & 7u);
        const bool e0 = st_ships(own), e1 = st_ships(all);
        const bool t0 = e0 && (own & kTorS), t1 = e1 && (all & kTorS);
        return redo(r >> 16, e0 != e1, t0 != t1, e1);
    }
};

// ---------------------------------------------------------------- count
template <bool LWW, bool BITS>
__global__ __launch_bounds__(DCB) void k_delta_count(crdt_tuples S, uint64_t ns_max, const uint64_t *__restrict__ ns_dev,
                                                     crdt_tuples D, uint64_t nd_max, const uint64_t *__restrict__ nd_dev,
                                                     const uint64_t *__restrict__ split, uint32_t *__restrict__ tcnt,
                                                     uint32_t *__restrict__ rec, uint64_t *__restrict__ bits) {
    // staged: dst slots 0 .. na + 1 = D[i0 - 1 .. i1], then src slots = S[j0 - 1 .. j1]
    __shared__ uint64_t sk[DCAP];
    __shared__ uint64_t st[LWW ? 1 : DCAP];
    __shared__ uint32_t sr[LWW ? 1 : DCAP];
    __shared__ uint8_t sm[LWW ? 4 : DCAP];
    __shared__ uint32_t s_w[DCB / 64], s_c[DCB / 64], s_first;
    uint64_t ns, nd;
    if (!tile_len(ns_max, ns_dev, nd_max, nd_dev, &ns, &nd)) return;
    const uint64_t t = blockIdx.x;
    if (t >= delta_tiles(ns, nd)) return;                // (uniform)
    const uint64_t n = ns + nd, d0 = t * DT, d1 = d0 + DT < n ? d0 + DT : n;
    const uint64_t i0 = split[t], i1 = split[t + 1], j0 = d0 - i0, j1 = d1 - i1;
    const uint32_t na = (uint32_t)(i1 - i0), nb = (uint32_t)(j1 - j0), tn = na + nb;
    const uint32_t so = na + 2, nst = so + nb + 2;       // first src slot, slots in all
    if (threadIdx.x == 0) s_first = 0;
    {
        constexpr int NL = (DCAP + DCB - 1) / DCB;
        uint64_t k[NL], ts[NL];
        uint32_t r[NL];
        uint8_t m[NL];
#pragma unroll
        for (int j = 0; j < NL; ++j) {                   // every staging load issued before the first store
            const uint32_t x = threadIdx.x + (uint32_t)j * DCB;
            const bool on_d = x < so;
            const uint64_t g = on_d ? i0 + x - 1 : j0 + (x - so) - 1;   // (slot 0 of an unstarted side wraps: not below its length)
            const bool v = x < nst && g < (on_d ? nd : ns);
            k[j] = v ? (on_d ? D.key : S.key)[g] : 0;
            if (!LWW) {
                ts[j] = v ? (on_d ? D.ts : S.ts)[g] : 0;
                r[j] = v ? (on_d ? D.rep : S.rep)[g] : 0;
                m[j] = v ? (on_d ? D.tomb : S.tomb)[g] : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const uint32_t x = threadIdx.x + (uint32_t)j * DCB;
            if (x < nst && x < (uint32_t)DCAP) {
                sk[x] = k[j];
                if (!LWW) {
                    st[x] = ts[j];
                    sr[x] = r[j];
                    sm[x] = m[j];
                }
            }
        }
    }
    __syncthreads();
    // heads run one past each side's tile elements when the side goes on: the
    // item merged after the tile's last is then a head like any other
    const uint32_t nax = na + (i1 < nd ? 1u : 0u), nbx = nb + (j1 < ns ? 1u : 0u);
    // dst element a (slot 1 + a) <= src element b (slot so + 1 + b)
    auto le = [&](uint32_t a, uint32_t b) -> bool {
        const uint32_t xd = 1 + a, xs = so + 1 + b;
        const uint64_t kd = sk[xd], ks = sk[xs];
        if (LWW || kd != ks) return kd <= ks;
        const uint64_t td = st[xd], tss = st[xs];
        if (td != tss) return td < tss;
        return sr[xd] <= sr[xs];
    };
    auto same = [&](uint32_t x, uint32_t y) -> bool {   // slots x, y carry one tag (LWW: key)
        if (sk[x] != sk[y]) return false;
        if (LWW) return true;
        return st[x] == st[y] && sr[x] == sr[y];
    };
    const uint32_t k0 = threadIdx.x * DNI < tn ? threadIdx.x * DNI : tn;
    const uint32_t k1 = k0 + DNI < tn ? k0 + DNI : tn;
    uint32_t iss = 0, emit = 0, tmb = 0;
    uint32_t state = 0, lead = 0, first = 0;             // OR-Set: open run's state; the first run end's state and item
    bool seen = false, first_s = false;
    if (k0 < k1) {
        uint32_t lo = k0 > nb ? k0 - nb : 0, hi = k0 < na ? k0 : na;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (le(mid, k0 - 1 - mid)) lo = mid + 1;
            else hi = mid;
        }
        uint32_t ia = lo, ib = k0 - lo;
        bool take_d = ia < nax && (ib >= nbx || le(ia, ib));
        for (uint32_t i = 0; i < k1 - k0; ++i) {
            const uint32_t cur = take_d ? 1 + ia : so + 1 + ib;
            const bool is_d = take_d;
            if (is_d) ++ia;
            else ++ib;
            const bool hd = ia < nax, hs = ib < nbx;
            take_d = hd && (!hs || le(ia, ib));
            const bool end = !((hd || hs) && same(cur, take_d ? 1 + ia : so + 1 + ib));
            if (!is_d) iss |= 1u << i;
            if (LWW) {
                if (end && !is_d) {                      // src's maximal tag of the key; dst's: the element merged before the key's src items
                    // (batching the thread's run-end loads after the loop measured slower: DESIGN.md §5.13)
                    bool ship = true;
                    if (i0 + ia > 0 && sk[ia] == sk[cur]) {
                        const uint64_t js = j0 + ib - 1, id = i0 + ia - 1;   // (64-bit: ia may be 0 with i0 > 0)
                        const uint64_t a = S.ts[js], b = D.ts[id];
                        ship = a != b ? a > b : S.rep[js] > D.rep[id];
                    }
                    if (ship) emit |= 1u << i;
                }
            } else {
                state |= is_d ? (kHasD | (sm[cur] ? kTorD : 0u)) : (sm[cur] ? kTorS : 0u);
                if (end) {
                    if (!seen) {
                        seen = true;
                        lead = state;
                        first = i;
                        first_s = !is_d;
                    } else if (!is_d && st_ships(state)) {
                        emit |= 1u << i;
                        if (state & kTorS) tmb |= 1u << i;
                    }
                    state = 0;
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!LWW) {
        // the state the tile's earlier threads leave (under the tile's empty carry)
        const uint32_t mine = state | (seen ? kEnd : 0u);
        uint32_t x = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x = st_then(y, x);
        }
        if (lane == 63) s_w[wv] = x;
        uint32_t ex = __shfl_up(x, 1, 64);
        if (lane == 0) ex = 0;
        __syncthreads();
        uint32_t pre = 0;
        for (int w = 0; w < wv; ++w) pre = st_then(pre, s_w[w]);
        pre = st_then(pre, ex);
        if (seen) {
            const uint32_t all = (pre & 7u) | lead;
            if (first_s && st_ships(all)) {
                emit |= 1u << first;
                if (all & kTorS) tmb |= 1u << first;
            }
            if (!(pre & kEnd))                           // the tile's first run end: the scan re-decides it under the carry
                s_first = (all << 4) | (first_s ? 0x80u : 0u) | ((k0 + first) << 16);
        }
    }
    if (BITS) {
        constexpr int LPW = 64 / DNI;
        const int sh = (lane % LPW) * DNI;
        uint64_t ws = (uint64_t)iss << sh, we = (uint64_t)emit << sh, wt = (uint64_t)tmb << sh;
#pragma unroll
        for (int o = 1; o < LPW; o <<= 1) {
            ws |= (uint64_t)__shfl_xor((unsigned long long)ws, o);
            we |= (uint64_t)__shfl_xor((unsigned long long)we, o);
            if (!LWW) wt |= (uint64_t)__shfl_xor((unsigned long long)wt, o);
        }
        if (lane % LPW == 0) {
            const uint32_t w = threadIdx.x / LPW;
            uint64_t *b = bits + t * (3 * DNW);
            b[w] = ws;
            b[DNW + w] = we;
            if (!LWW) b[2 * DNW + w] = wt;
        }
    }
    uint32_t c = (uint32_t)__popc(emit);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) s_c[wv] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0, all = 0;
#pragma unroll
        for (int w = 0; w < DCB / 64; ++w) {
            tot += s_c[w];
            if (!LWW) all = st_then(all, s_w[w]);
        }
        tcnt[t] = tot;
        if (!LWW) rec[t] = all | s_first;
    }
}

// ---------------------------------------------------------------- write pass
template <bool LWW>
__global__ __launch_bounds__(DWB) void k_delta_write(crdt_tuples S, uint64_t ns_max, const uint64_t *__restrict__ ns_dev,
                                                     uint64_t nd_max, const uint64_t *__restrict__ nd_dev,
                                                     const uint64_t *__restrict__ split,
                                                     const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ic,
                                                     crdt_tuples out, uint32_t *__restrict__ err) {
    uint64_t ns, nd;
    if (!tile_len(ns_max, ns_dev, nd_max, nd_dev, &ns, &nd)) return;
    const uint64_t t = blockIdx.x;
    if (t >= delta_tiles(ns, nd)) return;
    const int lane = threadIdx.x & 63;
    const uint64_t *b = bits + t * (3 * DNW);
    const RankWords k = rank_words(b, lane);              // `iss`, `emit` and their prefix counts
    const uint64_t wt = !LWW && lane < DNW ? b[2 * DNW + lane] : 0ull;
    const uint32_t ne = k.ne;
    const uint64_t j0 = t * DT - split[t], base = ic[t];
    bool bad = false;
    // one output per thread and round, by rank: every lane of a wave loads and
    // stores, whatever fraction of the merged items ships
    for (uint32_t r0 = 0; r0 < ne; r0 += DWB) {          // (uniform: the shuffles below read every word's lane)
        const bool valid = r0 + threadIdx.x < ne;
        const uint32_t r = valid ? r0 + threadIdx.x : ne - 1;
        const RankHit h = rank_select(k, r);
        const uint64_t qs = h.qb, qe = h.qe;
        const uint64_t qt = LWW ? 0ull : (uint64_t)__shfl((unsigned long long)wt, h.w, 64);
        const uint32_t pos = h.pos;
        const uint64_t i = j0 + h.nb;                    // the src item's index
        const uint64_t at = base + r;
        if (!valid) continue;
        // (the bitmaps of this call's count pass never fail this)
        if (!(pos < 64 && ((qe >> pos) & (qs >> pos) & 1) && i < ns && at < ns_max)) {
            bad = true;
            continue;
        }
        const uint64_t key = S.key[i], ts = S.ts[i];
        const uint32_t rep = S.rep[i];
        uint8_t tomb = (uint8_t)((qt >> pos) & 1);
        if (LWW) {
            const uint64_t p = i > 0 ? i - 1 : 0;
            const uint64_t pk = S.key[p], pts = S.ts[p];
            const uint32_t pr = S.rep[p];
            tomb = S.tomb[i];
            if (i > 0 && pk == key && pts == ts && pr == rep) {
                // more copies of the key's maximal tag: the tomb of the first one
                uint64_t f = p;
                while (f > 0 && S.key[f - 1] == key && S.ts[f - 1] == ts && S.rep[f - 1] == rep) --f;
                tomb = S.tomb[f];
            }
        }
        out.key[at] = key;
        out.ts[at] = ts;
        out.rep[at] = rep;
        out.tomb[at] = tomb;
    }
    if (bad) atomicOr(err, CRDT_DEV_RANGE);
}

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_set_delta(crdt_ctx *ctx, int mode, const crdt_tuples *src, size_t ns_max, const uint64_t *ns_dev,
                              const crdt_tuples *dst, size_t nd_max, const uint64_t *nd_dev, const crdt_tuples *out,
                              uint64_t *count) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!src || !dst || !count || (mode != CRDT_SET_LWW && mode != CRDT_SET_ORSET)) return CRDT_E_INVAL;
    if (ns_max >= (1ULL << 62) || nd_max >= (1ULL << 62)) return CRDT_E_RANGE;
    if (ns_max && tuples_null(src)) return CRDT_E_INVAL;
    if (nd_max && tuples_null(dst)) return CRDT_E_INVAL;
    if (tuples_misaligned(src) || tuples_misaligned(dst) || (out && tuples_misaligned(out))) return CRDT_E_INVAL;
    if (out && ns_max) {
        if (tuples_null(out)) return CRDT_E_INVAL;
        if (tuples_overlap(out, ns_max, src, ns_max) || tuples_overlap(out, ns_max, dst, nd_max)) return CRDT_E_INVAL;
    }
    const size_t ntiles = ns_max ? (ns_max + nd_max + DT - 1) / DT : 0;
    if (ntiles >= 0x7fffffffULL) return CRDT_E_RANGE;
    TileWs w;
    rc = w.reserve(ctx, ntiles, true, true, 3 * DNW);
    if (rc) return rc;
    const bool lww = mode == CRDT_SET_LWW, wr = out != nullptr;
    const hipStream_t s = ctx->stream;
    const crdt_tuples &S = *src, &D = *dst;
    if (ntiles) {
        const unsigned g = (unsigned)ntiles, gs = mp_split_grid(ntiles);
        if (lww) k_mp_split<DT, TupleLe<true>, DeltaTiles><<<gs, 256, 0, s>>>(D, nd_max, nd_dev, S, ns_max, ns_dev, w.split);
        else k_mp_split<DT, TupleLe<false>, DeltaTiles><<<gs, 256, 0, s>>>(D, nd_max, nd_dev, S, ns_max, ns_dev, w.split);
        if (lww && wr)
            k_delta_count<true, true><<<g, DCB, 0, s>>>(S, ns_max, ns_dev, D, nd_max, nd_dev, w.split, w.tcnt, w.rec, w.bits);
        else if (lww)
            k_delta_count<true, false><<<g, DCB, 0, s>>>(S, ns_max, ns_dev, D, nd_max, nd_dev, w.split, w.tcnt, w.rec, w.bits);
        else if (wr)
            k_delta_count<false, true><<<g, DCB, 0, s>>>(S, ns_max, ns_dev, D, nd_max, nd_dev, w.split, w.tcnt, w.rec, w.bits);
        else
            k_delta_count<false, false><<<g, DCB, 0, s>>>(S, ns_max, ns_dev, D, nd_max, nd_dev, w.split, w.tcnt, w.rec, w.bits);
    }
    if (lww) w.scan<NoCarry<DeltaTiles>>(ctx, nd_max, nd_dev, ns_max, ns_dev, wr, count);
    else w.scan<DeltaCarry>(ctx, nd_max, nd_dev, ns_max, ns_dev, wr, count);
    if (ntiles && wr) {
        const unsigned g = (unsigned)ntiles;
        if (lww)
            k_delta_write<true><<<g, DWB, 0, s>>>(S, ns_max, ns_dev, nd_max, nd_dev, w.split, w.bits, w.ic, *out, ctx->dev_status);
        else
            k_delta_write<false><<<g, DWB, 0, s>>>(S, ns_max, ns_dev, nd_max, nd_dev, w.split, w.bits, w.ic, *out, ctx->dev_status);
    }
    return check_launch(ctx);
}
