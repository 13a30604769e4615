// setcausal.hip -- the tombstone-free OR-Set: the causal merge of two states
// under their version vectors (crdt_orset_merge_causal).
//
// Semantics.  A causal state is (tuples, context): tuples sorted ascending by
// (key, ts, rep), copies of one tag in any order and number; the context n_ctx
// uint64, ctx[r] = the events of replica r the state has seen.  Side X holds
// tag g PRESENT iff it holds a copy of g and the OR of its copies' tombs is 0
// (crdt_set_elements' live tag; a tombstoned tag counts as absent).  g is
// COVERED by (v, n) iff g.rep < n and g.ts <= v[g.rep] (unsigned;
// crdt_set_compact's "stable").  g is in merge(a, b) iff
//   present in a and in b, or
//   present in a and not covered by b's context, or
//   present in b and not covered by a's context
// -- a side whose context covers a tag it does not hold has seen and removed
// it.  Each surviving tag is written once, tomb = 0, in ascending tuple order.
// Its source index names the first copy, in the stable merged order (a's
// copies of a tag before b's, each side in input order), on a side where the
// tag is present: a's first copy when a holds it present, else b's first copy.
// ctx_out = the element-wise maximum of the contexts, the shorter one padded
// with zeros.
//
// GPU structure: setdelta.hip's, over the stable merged order of (a, b), every
// decision taken at the LAST merged item of a tag run (an a item exactly when
// b holds no copy of the tag):
//   ctx   : ctx_out alone, whatever the lengths are;
//   split : k_mp_split (settile.hpp) by the full tag;
//   count : per tile both runs staged in LDS (plain loads, clamped to each
//           side's length) and merged, 512 threads x 4 items.  A thread
//           carries the open tag run's state (a copy seen, a tomb-OR, b copy
//           seen, b tomb-OR: 4 bits); a run end resets it, so a thread's effect
//           on the state is "reset, then OR" -- an associative record scanned
//           over the workgroup; what an earlier thread or tile can change is
//           one decision, the first run end after it.  A context is read only
//           at a run end with exactly one side present (the other side's, at
//           the tag's rep when rep < n_ctx); the tile's first run end, which
//           the scan re-decides, records both covered bits.  Output: bitmaps
//           in merged order (`isb`: a b item, `emit`, `srca`: the emitted tag
//           is present in a), the tile's count and record;
//   scan  : k_tile_scan<CausalCarry> (settile.hpp): the records scan as they
//           are, each tile's first run end is re-decided with the carry's
//           bits ORed into its run's own, under the recorded covered bits;
//   write : (out != NULL) one output per lane, by rank (rank_words /
//           rank_select, settile.hpp): its side and index there follow from
//           the count of b items before it; key / ts / rep of the run end stored at
//           the rank with tomb = 0, and, when asked, the source index: the
//           walk back over the present side's equal-tag copies to the first
//           one goes through global memory, as k_tile_write's does (from a's
//           last copy, the a item merged just before b's copies, when the run
//           ends on b).
//
// Either length may stay on the device.  A value past its n_max touches no
// tuple, stores a count of ~0 and raises CRDT_DEV_RANGE; no kernel reads an
// index at or past min(*n_dev, n_max) of its side, or before 0, nor a context
// at or past its n_ctx.
//
// The ranged form (crdt_orset_merge_causal_ranges) merges a
// whole state a with what a peer shipped for the buckets of crdt_set_digest
// whose digests differ.  The merge is not monotone -- a tag a holds and b's
// context covers is dropped unless b's copy is in the operand -- so in an
// unflagged bucket, where equal digests say both replicas hold the same
// canonical tuples, "present in both" is "present in a": the tag survives iff
// a holds it present, b's copies there are ignored and no context is read.
// One predicate of the count pass (k_causal_count<*, true>); a tag lies in one
// bucket, so every tile masks its copies alike and the scan, the write pass
// and the split run unchanged: a run that ends on an ignored b copy loads the
// same tag there, `srca` is set, and the source walk goes to a's first copy.
// No kernel reads a splitter at or past m or a flag at or past m + 1.
#include "settile.hpp"

namespace crdt {

constexpr int UT = kTile;                  // merge items per tile
constexpr int UCB = 512;                   // count pass threads
constexpr int UNI = UT / UCB;              // merge items per count thread
constexpr int UNW = kTileNW;               // words per tile and bitmap
constexpr int UWB = 256;                   // write pass threads (one output each per round)
constexpr int UCAP = UT + 4;               // staged slots: each side's run, the element before and the one after it
constexpr size_t kCausalMaxSplit = (size_t)1 << 24;   // (crdt_set_digest's bound on m)

// ---- the open tag run's state and a segment's record
constexpr uint32_t kUHasA = 1, kUTorA = 2, kUHasB = 4, kUTorB = 8;   // a / b: copy seen, tomb-OR
constexpr uint32_t kURun = 15;
constexpr uint32_t kUEnd = 16;             // the segment holds a run end: the state before it is dropped
// record of a tile: bits 0-4 as above (the state it leaves), bits 5-8 the
// state its items add to the run of its first run end, bit 9 / 10 that tag is
// covered by a's / b's context, bits 16- its position in the tile
__device__ __forceinline__ uint32_t cz_then(uint32_t a, uint32_t b) { return (b & kUEnd) ? b : (a | b); }
__device__ __forceinline__ bool cz_pa(uint32_t s) { return (s & (kUHasA | kUTorA)) == kUHasA; }
__device__ __forceinline__ bool cz_pb(uint32_t s) { return (s & (kUHasB | kUTorB)) == kUHasB; }
__device__ __forceinline__ bool cz_cov(const uint64_t *__restrict__ v, uint32_t n, uint32_t rep, uint64_t ts) {
    return rep < n && ts <= v[rep];
}
// bit 0: the tag survives; bit 1: it does and a holds it present
__device__ __forceinline__ uint32_t cz_keep(uint32_t s, bool cov_a, bool cov_b) {
    const bool pa = cz_pa(s), pb = cz_pb(s);
    const bool keep = (pa && pb) || (pa && !cov_b) || (pb && !cov_a);
    return (keep ? 1u : 0u) | (keep && pa ? 2u : 0u);
}
// the same, a context read only where exactly one side is present
__device__ __forceinline__ uint32_t cz_decide(uint32_t s, uint64_t ts, uint32_t rep, const uint64_t *__restrict__ ca,
                                              uint32_t nca, const uint64_t *__restrict__ cb, uint32_t ncb) {
    const bool pa = cz_pa(s), pb = cz_pb(s);
    bool keep = pa && pb;
    if (pa != pb) keep = !(pa ? cz_cov(cb, ncb, rep, ts) : cz_cov(ca, nca, rep, ts));
    return (keep ? 1u : 0u) | (keep && pa ? 2u : 0u);
}

// the scan's view of a record: the state scans as it is; the first run end is
// re-decided with the carry's bits ORed into its run's own, under the recorded covered bits
struct CausalCarry : PlainTiles {
    static constexpr bool kHas = true;
    static constexpr uint32_t kId = 0, kStride = 3 * UNW, kEmit = UNW, kAux = 2 * UNW;   // (`isb`, `emit`, `srca`)
    static __device__ __forceinline__ uint32_t part(uint32_t r) { return r & 0x1fu; }
    static __device__ __forceinline__ uint32_t then(uint32_t a, uint32_t b) { return cz_then(a, b); }
    static __device__ __forceinline__ uint32_t seed(uint32_t s) { return s; }
    static __device__ __forceinline__ uint32_t enter(uint32_t p, uint32_t) { return p; }
    static __device__ __forceinline__ uint32_t step(uint32_t s, uint32_t r) { return cz_then(s, r & 0x1fu); }
    static __device__ __forceinline__ uint32_t redecide(uint32_t r, uint32_t s) {
        if (!((r & kUEnd) && (s & kURun))) return 0;     // (an empty carry changes nothing)
        const uint32_t own = (r >> 5) & kURun, all = own | (s & kURun);
        const bool cva = (r >> 9) & 1, cvb = (r >> 10) & 1;
        const uint32_t d0 = cz_keep(own, cva, cvb), d1 = cz_keep(all, cva, cvb);
        return redo(r >> 16, ((d0 ^ d1) & 1) != 0, ((d0 ^ d1) & 2) != 0, (d1 & 1) != 0);
    }
};

// ---------------------------------------------------------------- ctx_out
__global__ __launch_bounds__(256) void k_causal_ctx(const uint64_t *__restrict__ ca, uint32_t nca,
                                                    const uint64_t *__restrict__ cb, uint32_t ncb,
                                                    uint64_t *__restrict__ out) {
    const uint32_t n = nca > ncb ? nca : ncb;
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const uint64_t x = c < nca ? ca[c] : 0ull, y = c < ncb ? cb[c] : 0ull;
    out[c] = x > y ? x : y;
}

// lo + #{ j in [lo, hi) : sp[j] <= key } for ascending sp (setdigest.hip's
// dig_ub): always a value in [lo, max(lo, hi)], and only sp[lo .. hi) is read
__device__ __forceinline__ uint32_t cz_ub(const uint64_t *__restrict__ sp, uint32_t lo, uint32_t hi, uint64_t key) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sp[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The same count over sp[0 .. m) for a wave-uniform key by a whole wave (every
// lane active): 64 probes a round, so 255 splitters take two dependent loads
// where the binary search takes eight.  Reads sp[lo .. hi) only and returns a
// value in [0, m], whatever sp holds.
__device__ __forceinline__ uint32_t cz_ub_wave(const uint64_t *__restrict__ sp, uint32_t m, uint64_t key, uint32_t lane) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) {                                    // (uniform)
        const uint32_t span = hi - lo;
        if (span <= 64) {
            const bool p = lane < span && sp[lo + lane] <= key;
            return lo + (uint32_t)__popcll(__ballot(p));
        }
        // probe c_l = lo + floor(l span / 64), ascending from lo: the first cnt hold (ascending sp)
        const uint32_t c = lo + (uint32_t)(((uint64_t)lane * span) >> 6);
        const uint32_t cnt = (uint32_t)__popcll(__ballot(sp[c] <= key));
        const uint32_t nlo = cnt ? lo + (uint32_t)(((uint64_t)(cnt - 1) * span) >> 6) + 1 : lo;
        hi = cnt < 64 ? lo + (uint32_t)(((uint64_t)cnt * span) >> 6) : hi;
        lo = nlo;
    }
    return lo;
}

// ---------------------------------------------------------------- count
// RANGED (crdt_orset_merge_causal_ranges): sp[0 .. m) and flags[0 .. m] are
// crdt_set_digest's buckets.  In an unflagged bucket b is taken to hold what a
// holds: a b item keeps its `isb` bit and adds nothing to the run state, a run
// end decides by a's bits alone (covered by b: false) and reads no context.
// Every wave searches the splitters for its tile's first and last key (uniform,
// 64 probes a round); one bucket, the common case, is one flag load, else an
// item searches between the two.  Every search is an upper bound inside [0, m].
template <bool BITS, bool RANGED>
__global__ __launch_bounds__(UCB) void k_causal_count(crdt_tuples A, uint64_t na_max, const uint64_t *__restrict__ na_dev,
                                                      const uint64_t *__restrict__ ca, uint32_t nca, crdt_tuples B,
                                                      uint64_t nb_max, const uint64_t *__restrict__ nb_dev,
                                                      const uint64_t *__restrict__ cb, uint32_t ncb,
                                                      const uint64_t *__restrict__ split, uint32_t *__restrict__ tcnt,
                                                      uint32_t *__restrict__ rec, uint64_t *__restrict__ bits,
                                                      const uint64_t *__restrict__ sp, uint32_t m,
                                                      const uint8_t *__restrict__ flags) {
    // staged: a slots 0 .. ta + 1 = A[i0 - 1 .. i1], then b slots = B[j0 - 1 .. j1]
    __shared__ uint64_t sk[UCAP];
    __shared__ uint64_t st[UCAP];
    __shared__ uint32_t sr[UCAP];
    __shared__ uint8_t sm[UCAP];
    __shared__ uint32_t s_w[UCB / 64], s_c[UCB / 64], s_first;
    uint64_t na, nb;
    if (!tile_len(na_max, na_dev, nb_max, nb_dev, &na, &nb)) return;
    const uint64_t t = blockIdx.x;
    if (t >= PlainTiles::tiles(na, nb)) return;                   // (uniform)
    const uint64_t n = na + nb, d0 = t * UT, d1 = d0 + UT < n ? d0 + UT : n;
    const uint64_t i0 = split[t], i1 = split[t + 1], j0 = d0 - i0, j1 = d1 - i1;
    const uint32_t ta = (uint32_t)(i1 - i0), tb = (uint32_t)(j1 - j0), tn = ta + tb;
    const uint32_t so = ta + 2, nst = so + tb + 2;       // first b slot, slots in all
    if (threadIdx.x == 0) s_first = 0;
    {
        constexpr int NL = (UCAP + UCB - 1) / UCB;
        uint64_t k[NL], ts[NL];
        uint32_t r[NL];
        uint8_t m[NL];
#pragma unroll
        for (int j = 0; j < NL; ++j) {                   // every staging load issued before the first store
            const uint32_t x = threadIdx.x + (uint32_t)j * UCB;
            const bool on_a = x < so;
            const uint64_t g = on_a ? i0 + x - 1 : j0 + (x - so) - 1;   // (slot 0 of an unstarted side wraps: not below its length)
            const bool v = x < nst && g < (on_a ? na : nb);
            k[j] = v ? (on_a ? A.key : B.key)[g] : 0;
            ts[j] = v ? (on_a ? A.ts : B.ts)[g] : 0;
            r[j] = v ? (on_a ? A.rep : B.rep)[g] : 0;
            m[j] = v ? (on_a ? A.tomb : B.tomb)[g] : 0;
        }
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const uint32_t x = threadIdx.x + (uint32_t)j * UCB;
            if (x < nst && x < (uint32_t)UCAP) {
                sk[x] = k[j];
                st[x] = ts[j];
                sr[x] = r[j];
                sm[x] = m[j];
            }
        }
    }
    __syncthreads();
    // heads run one past each side's tile elements when the side goes on: the
    // item merged after the tile's last is then a head like any other
    const uint32_t tax = ta + (i1 < na ? 1u : 0u), tbx = tb + (j1 < nb ? 1u : 0u);
    // a element x (slot 1 + x) <= b element y (slot so + 1 + y)
    auto le = [&](uint32_t x, uint32_t y) -> bool {
        const uint32_t xa = 1 + x, xb = so + 1 + y;
        const uint64_t ka = sk[xa], kb = sk[xb];
        if (ka != kb) return ka < kb;
        const uint64_t tsa = st[xa], tsb = st[xb];
        if (tsa != tsb) return tsa < tsb;
        return sr[xa] <= sr[xb];
    };
    auto same = [&](uint32_t x, uint32_t y) -> bool {   // slots x, y carry one tag
        return sk[x] == sk[y] && st[x] == st[y] && sr[x] == sr[y];
    };
    // RANGED: the tile's bucket span [blo, bhi] from its first and last key; one bucket: its flag
    uint32_t blo = 0, bhi = 0;
    bool one = true, f1 = true;
    if constexpr (RANGED) {
        const uint64_t fa = sk[1], la = sk[ta], fb = sk[so + 1], lb = sk[so + tb];   // (a side with no item in the tile is not taken)
        const uint64_t kf = ta && (!tb || fa < fb) ? fa : fb, kl = ta && (!tb || la > lb) ? la : lb;
        blo = __builtin_amdgcn_readfirstlane(cz_ub_wave(sp, m, kf, threadIdx.x & 63));
        bhi = __builtin_amdgcn_readfirstlane(cz_ub_wave(sp, m, kl, threadIdx.x & 63));
        one = blo == bhi;
        f1 = one && flags[blo] != 0;
    }
    const uint32_t k0 = threadIdx.x * UNI < tn ? threadIdx.x * UNI : tn;
    const uint32_t k1 = k0 + UNI < tn ? k0 + UNI : tn;
    uint32_t isb = 0, emit = 0, sa = 0;
    uint32_t state = 0, lead = 0, first = 0, fslot = 0;  // open run's state; the first run end's state, item and slot
    bool seen = false, ffl = true;                       // RANGED: the first run end's bucket is flagged
    if (k0 < k1) {
        uint32_t lo = k0 > tb ? k0 - tb : 0, hi = k0 < ta ? k0 : ta;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (le(mid, k0 - 1 - mid)) lo = mid + 1;
            else hi = mid;
        }
        uint32_t ia = lo, ib = k0 - lo;
        bool take_a = ia < tax && (ib >= tbx || le(ia, ib));
        for (uint32_t i = 0; i < k1 - k0; ++i) {
            const uint32_t cur = take_a ? 1 + ia : so + 1 + ib;
            const bool is_a = take_a;
            if (is_a) ++ia;
            else ++ib;
            const bool ha = ia < tax, hb = ib < tbx;
            take_a = ha && (!hb || le(ia, ib));
            const bool end = !((ha || hb) && same(cur, take_a ? 1 + ia : so + 1 + ib));
            if (!is_a) isb |= 1u << i;
            bool fl = true;                              // RANGED: the item's bucket is flagged (wanted at a b item and a run end)
            if constexpr (RANGED) {
                fl = f1;
                if (!one && (!is_a || end)) fl = flags[cz_ub(sp, blo, bhi, sk[cur])] != 0;
            }
            state |= is_a ? (kUHasA | (sm[cur] ? kUTorA : 0u)) : (fl ? (kUHasB | (sm[cur] ? kUTorB : 0u)) : 0u);
            if (end) {
                if (!seen) {
                    seen = true;
                    lead = state;
                    first = i;
                    fslot = cur;
                    if constexpr (RANGED) ffl = fl;
                } else {
                    const uint32_t d = fl ? cz_decide(state, st[cur], sr[cur], ca, nca, cb, ncb) : (cz_pa(state) ? 3u : 0u);
                    if (d & 1) emit |= 1u << i;
                    if (d & 2) sa |= 1u << i;
                }
                state = 0;
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    {
        // the state the tile's earlier threads leave (under the tile's empty carry)
        const uint32_t mine = state | (seen ? kUEnd : 0u);
        uint32_t x = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x = cz_then(y, x);
        }
        if (lane == 63) s_w[wv] = x;
        uint32_t ex = __shfl_up(x, 1, 64);
        if (lane == 0) ex = 0;
        __syncthreads();
        uint32_t pre = 0;
        for (int w = 0; w < wv; ++w) pre = cz_then(pre, s_w[w]);
        pre = cz_then(pre, ex);
        if (seen) {
            const uint32_t all = (pre & kURun) | lead;
            const uint64_t fts = st[fslot];
            const uint32_t frep = sr[fslot];
            if (!(pre & kUEnd)) {                        // the tile's first run end: the scan re-decides it under the carry
                // (an unflagged bucket: neither context is read, both bits 0 -- no b bit reaches the run's state)
                const bool cva = ffl && cz_cov(ca, nca, frep, fts), cvb = ffl && cz_cov(cb, ncb, frep, fts);
                const uint32_t d = cz_keep(all, cva, cvb);
                if (d & 1) emit |= 1u << first;
                if (d & 2) sa |= 1u << first;
                s_first = (all << 5) | (cva ? 1u << 9 : 0u) | (cvb ? 1u << 10 : 0u) | ((k0 + first) << 16);
            } else {
                const uint32_t d = ffl ? cz_decide(all, fts, frep, ca, nca, cb, ncb) : (cz_pa(all) ? 3u : 0u);
                if (d & 1) emit |= 1u << first;
                if (d & 2) sa |= 1u << first;
            }
        }
    }
    if (BITS) {
        constexpr int LPW = 64 / UNI;
        const int sh = (lane % LPW) * UNI;
        uint64_t wb = (uint64_t)isb << sh, we = (uint64_t)emit << sh, wa = (uint64_t)sa << sh;
#pragma unroll
        for (int o = 1; o < LPW; o <<= 1) {
            wb |= (uint64_t)__shfl_xor((unsigned long long)wb, o);
            we |= (uint64_t)__shfl_xor((unsigned long long)we, o);
            wa |= (uint64_t)__shfl_xor((unsigned long long)wa, o);
        }
        if (lane % LPW == 0) {
            const uint32_t w = threadIdx.x / LPW;
            uint64_t *b = bits + t * (3 * UNW);
            b[w] = wb;
            b[UNW + w] = we;
            b[2 * UNW + w] = wa;
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
        for (int w = 0; w < UCB / 64; ++w) {
            tot += s_c[w];
            all = cz_then(all, s_w[w]);
        }
        tcnt[t] = tot;
        rec[t] = all | s_first;
    }
}

// ---------------------------------------------------------------- write pass
template <bool SRC>
__global__ __launch_bounds__(UWB) void k_causal_write(crdt_tuples A, uint64_t na_max, const uint64_t *__restrict__ na_dev,
                                                      crdt_tuples B, uint64_t nb_max, const uint64_t *__restrict__ nb_dev,
                                                      const uint64_t *__restrict__ split,
                                                      const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ic,
                                                      crdt_tuples out, int64_t *__restrict__ src,
                                                      uint32_t *__restrict__ err) {
    uint64_t na, nb;
    if (!tile_len(na_max, na_dev, nb_max, nb_dev, &na, &nb)) return;
    const uint64_t t = blockIdx.x;
    if (t >= PlainTiles::tiles(na, nb)) return;
    const int lane = threadIdx.x & 63;
    const uint64_t *b = bits + t * (3 * UNW);
    const RankWords k = rank_words(b, lane);              // `isb`, `emit` and their prefix counts
    const uint64_t wa = SRC && lane < UNW ? b[2 * UNW + lane] : 0ull;
    const uint32_t ne = k.ne;
    const uint64_t i0 = split[t], j0 = t * UT - i0, base = ic[t], cap = na_max + nb_max;
    bool bad = false;
    // one output per thread and round, by rank: every lane of a wave loads and
    // stores, whatever fraction of the merged items survives
    for (uint32_t r0 = 0; r0 < ne; r0 += UWB) {          // (uniform: the shuffles below read every word's lane)
        const bool valid = r0 + threadIdx.x < ne;
        const uint32_t r = valid ? r0 + threadIdx.x : ne - 1;
        const RankHit h = rank_select(k, r);
        const uint64_t qb = h.qb, qe = h.qe;
        const uint64_t qa = SRC ? (uint64_t)__shfl((unsigned long long)wa, h.w, 64) : 0ull;
        const uint32_t pos = h.pos;
        if (!valid) continue;
        // (the bitmaps of this call's count pass never fail the checks below)
        if (!((qe >> pos) & 1)) {
            bad = true;
            continue;
        }
        const uint32_t bb = h.nb;                            // b items merged before this one
        const uint32_t ab = (uint32_t)h.w * 64 + pos - bb;   // a items
        const bool is_b = (qb >> pos) & 1;
        const uint64_t i = is_b ? j0 + bb : i0 + ab;     // the run end's index on its side
        const uint64_t at = base + r;
        if (!(i < (is_b ? nb : na) && at < cap)) {
            bad = true;
            continue;
        }
        const uint64_t key = (is_b ? B.key : A.key)[i], ts = (is_b ? B.ts : A.ts)[i];
        const uint32_t rep = (is_b ? B.rep : A.rep)[i];
        int64_t s = 0;
        if (SRC) {                                       // the first copy on the present side, a before b
            const bool from_a = (qa >> pos) & 1;
            if (from_a) {
                uint64_t f = i;
                if (is_b) {                              // a's last copy: the a item merged just before b's copies
                    f = i0 + ab - 1;
                    if (i0 + ab == 0 || f >= na) {
                        bad = true;
                        continue;
                    }
                }
                while (f > 0 && A.key[f - 1] == key && A.ts[f - 1] == ts && A.rep[f - 1] == rep) --f;
                s = (int64_t)f;
            } else {
                if (!is_b) {
                    bad = true;
                    continue;
                }
                uint64_t f = i;
                while (f > 0 && B.key[f - 1] == key && B.ts[f - 1] == ts && B.rep[f - 1] == rep) --f;
                s = -(int64_t)f - 1;
            }
        }
        out.key[at] = key;
        out.ts[at] = ts;
        out.rep[at] = rep;
        out.tomb[at] = 0;
        if (SRC) src[at] = s;
    }
    if (bad) atomicOr(err, CRDT_DEV_RANGE);
}

struct CausalSpan {
    const void *p;
    size_t bytes;
};
static int causal_fields(const crdt_tuples *t, size_t n, CausalSpan *s) {
    s[0] = {t->key, n * 8};
    s[1] = {t->ts, n * 8};
    s[2] = {t->rep, n * 4};
    s[3] = {t->tomb, n};
    return 4;
}

}  // namespace crdt

using namespace crdt;

// both entry points: ranged takes crdt_set_digest's buckets (sp, m, flags)
static int causal_merge(crdt_ctx *ctx, const crdt_tuples *a, size_t na_max, const uint64_t *na_dev,
                        const uint64_t *ctx_a_dev, size_t n_ctx_a, const crdt_tuples *b, size_t nb_max,
                        const uint64_t *nb_dev, const uint64_t *ctx_b_dev, size_t n_ctx_b, bool ranged,
                        const uint64_t *sp, size_t m, const uint8_t *flags, const crdt_tuples *out,
                        int64_t *src_out_dev, uint64_t *ctx_out_dev, uint64_t *count) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!a || !b || !count) return CRDT_E_INVAL;
    if (na_max >= (1ULL << 62) || nb_max >= (1ULL << 62)) return CRDT_E_RANGE;
    if (ranged) {
        if (m >= kCausalMaxSplit) return CRDT_E_RANGE;
        if (!flags || (m && !sp) || ((uintptr_t)sp & 7)) return CRDT_E_INVAL;
    }
    if (n_ctx_a >= (1ULL << 32) || n_ctx_b >= (1ULL << 32)) return CRDT_E_RANGE;
    if ((n_ctx_a && !ctx_a_dev) || (n_ctx_b && !ctx_b_dev)) return CRDT_E_INVAL;
    if (!out && src_out_dev) return CRDT_E_INVAL;
    if (na_max && tuples_null(a)) return CRDT_E_INVAL;
    if (nb_max && tuples_null(b)) return CRDT_E_INVAL;
    if (tuples_misaligned(a) || tuples_misaligned(b) || (out && tuples_misaligned(out))) return CRDT_E_INVAL;
    if ((((uintptr_t)ctx_a_dev | (uintptr_t)ctx_b_dev | (uintptr_t)ctx_out_dev | (uintptr_t)src_out_dev |
          (uintptr_t)na_dev | (uintptr_t)nb_dev | (uintptr_t)count) & 7) != 0)
        return CRDT_E_INVAL;
    const size_t cap = na_max + nb_max, n_ctx = n_ctx_a > n_ctx_b ? n_ctx_a : n_ctx_b;
    if (out && cap && tuples_null(out)) return CRDT_E_INVAL;
    const size_t ntiles = (cap + UT - 1) / UT;
    if (ntiles >= 0x7fffffffULL) return CRDT_E_RANGE;
    {
        CausalSpan in[14], o[6];
        int ni = causal_fields(a, na_max, in), no = 0;
        ni += causal_fields(b, nb_max, in + ni);
        in[ni++] = {ctx_a_dev, n_ctx_a * 8};
        in[ni++] = {ctx_b_dev, n_ctx_b * 8};
        in[ni++] = {na_dev, 8};
        in[ni++] = {nb_dev, 8};
        if (ranged) {
            in[ni++] = {sp, m * 8};
            in[ni++] = {flags, m + 1};
        }
        if (out) no = causal_fields(out, cap, o);
        o[no++] = {src_out_dev, cap * 8};
        o[no++] = {ctx_out_dev, n_ctx * 8};
        for (int x = 0; x < no; ++x) {
            for (int y = 0; y < ni; ++y)
                if (spans_overlap(o[x].p, o[x].bytes, in[y].p, in[y].bytes)) return CRDT_E_INVAL;
            for (int y = x + 1; y < no; ++y)
                if (spans_overlap(o[x].p, o[x].bytes, o[y].p, o[y].bytes)) return CRDT_E_INVAL;
        }
    }
    TileWs w;
    rc = w.reserve(ctx, ntiles, true, true, 3 * UNW);
    if (rc) return rc;
    const bool wr = out != nullptr;
    const uint32_t nca = (uint32_t)n_ctx_a, ncb = (uint32_t)n_ctx_b;
    const hipStream_t s = ctx->stream;
    if (ctx_out_dev && n_ctx)
        k_causal_ctx<<<(unsigned)((n_ctx + 255) / 256), 256, 0, s>>>(ctx_a_dev, nca, ctx_b_dev, ncb, ctx_out_dev);
    if (ntiles) {
        const unsigned g = (unsigned)ntiles;
        k_mp_split<UT, TupleLe<false>, PlainTiles><<<mp_split_grid(ntiles), 256, 0, s>>>(*a, na_max, na_dev, *b, nb_max,
                                                                                        nb_dev, w.split);
        const uint32_t mm = (uint32_t)m;
        if (ranged && wr)
            k_causal_count<true, true><<<g, UCB, 0, s>>>(*a, na_max, na_dev, ctx_a_dev, nca, *b, nb_max, nb_dev, ctx_b_dev,
                                                         ncb, w.split, w.tcnt, w.rec, w.bits, sp, mm, flags);
        else if (ranged)
            k_causal_count<false, true><<<g, UCB, 0, s>>>(*a, na_max, na_dev, ctx_a_dev, nca, *b, nb_max, nb_dev, ctx_b_dev,
                                                          ncb, w.split, w.tcnt, w.rec, w.bits, sp, mm, flags);
        else if (wr)
            k_causal_count<true, false><<<g, UCB, 0, s>>>(*a, na_max, na_dev, ctx_a_dev, nca, *b, nb_max, nb_dev, ctx_b_dev,
                                                          ncb, w.split, w.tcnt, w.rec, w.bits, nullptr, 0u, nullptr);
        else
            k_causal_count<false, false><<<g, UCB, 0, s>>>(*a, na_max, na_dev, ctx_a_dev, nca, *b, nb_max, nb_dev, ctx_b_dev,
                                                           ncb, w.split, w.tcnt, w.rec, w.bits, nullptr, 0u, nullptr);
    }
    w.scan<CausalCarry>(ctx, na_max, na_dev, nb_max, nb_dev, wr, count);
    if (ntiles && wr) {
        if (src_out_dev)
            k_causal_write<true><<<(unsigned)ntiles, UWB, 0, s>>>(*a, na_max, na_dev, *b, nb_max, nb_dev, w.split, w.bits,
                                                                  w.ic, *out, src_out_dev, ctx->dev_status);
        else
            k_causal_write<false><<<(unsigned)ntiles, UWB, 0, s>>>(*a, na_max, na_dev, *b, nb_max, nb_dev, w.split, w.bits,
                                                                   w.ic, *out, src_out_dev, ctx->dev_status);
    }
    return check_launch(ctx);
}

extern "C" int crdt_orset_merge_causal(crdt_ctx *ctx, const crdt_tuples *a, size_t na_max, const uint64_t *na_dev,
                                       const uint64_t *ctx_a_dev, size_t n_ctx_a, const crdt_tuples *b, size_t nb_max,
                                       const uint64_t *nb_dev, const uint64_t *ctx_b_dev, size_t n_ctx_b,
                                       const crdt_tuples *out, int64_t *src_out_dev, uint64_t *ctx_out_dev,
                                       uint64_t *count) {
    return causal_merge(ctx, a, na_max, na_dev, ctx_a_dev, n_ctx_a, b, nb_max, nb_dev, ctx_b_dev, n_ctx_b, false, nullptr,
                        0, nullptr, out, src_out_dev, ctx_out_dev, count);
}

extern "C" int crdt_orset_merge_causal_ranges(crdt_ctx *ctx, const crdt_tuples *a, size_t na_max, const uint64_t *na_dev,
                                              const uint64_t *ctx_a_dev, size_t n_ctx_a, const crdt_tuples *b,
                                              size_t nb_max, const uint64_t *nb_dev, const uint64_t *ctx_b_dev,
                                              size_t n_ctx_b, const uint64_t *splitters_dev, size_t m,
                                              const uint8_t *flags_dev, const crdt_tuples *out, int64_t *src_out_dev,
                                              uint64_t *ctx_out_dev, uint64_t *count_dev) {
    return causal_merge(ctx, a, na_max, na_dev, ctx_a_dev, n_ctx_a, b, nb_max, nb_dev, ctx_b_dev, n_ctx_b, true,
                        splitters_dev, m, flags_dev, out, src_out_dev, ctx_out_dev, count_dev);
}
