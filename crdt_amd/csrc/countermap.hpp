// countermap.hpp -- the kernels of the keyed PN-Counter map (crdt_cmap_*, the
// entry points in counters.hip).  Device code only.
//
// A state is cells (key, rep, p, n), strictly ascending by (key, rep), both
// unsigned, each cell at most once: replica rep's increments p and decrements
// n of key.  All sums are mod 2^64.
//
// Two-sided passes (merge, apply, delta): settile.hpp's split -> count -> scan
// -> write over the stable merged order of (a, b), a first on an equal cell.
// Under the precondition a run of equal cells is at most two items, a's then
// b's; every decision is taken at the run's last item and needs only the a
// element merged before it, which the staged "element before" covers when the
// pair straddles a tile boundary: no tile carries a record (NoCarry).
//   split : k_mp_split through a crdt_tuples view (key, rep), order CellLe;
//   count : per tile both runs' key / rep staged in LDS (every load issued
//           before the first store, clamped to each side's length) and merged,
//           512 threads x 4 items.  Bitmaps in merged order: `isb` (a b item),
//           `emit`, `pair` (a b item whose cell a holds too).
//           merge / apply: every run end emits.  delta (a = dst, b = src): a
//           src run end emits when dst has no such cell, or p_s > p_d, or n_s >
//           n_d -- p / n are read from global memory at the pairs alone;
//   scan  : k_tile_scan<NoCarry>;
//   write : one output per lane, by rank (rank_words / rank_select).  merge /
//           apply: the item's four fields, a `pair` combined with a's p / n by
//           the policy (max: merge; wrapping add: apply).  delta: src's fields.
// One-sided: values = heads (key[i] != key[i - 1]) through the by-position
// scaffold, then a segmented sum per tile; lookup = one probe per lane, a long
// key run finished by the whole wave.
// Combine (crdt_cmap_combine, the back end of crdt_cmap_from_ops; DESIGN.md
// §5.25): cells ascending by (key, rep) with repeats -> one cell per run, values'
// scaffold with a head at every change of (key, rep), the key columns written
// by the sums pass, the amounts optionally gathered through an index column.
// The additive join (crdt_cmap_add) is merge's passes with the CmAdd policy.
// Range digests (digest, select): by position over tiles of
// 2048 cells, a wave 8 consecutive 64-cell words, buckets and accumulation
// digest.hpp's.  Every cell is a deciding position: nothing walks back.
//
// No kernel reads a cell at or past min(*n_dev, n_max) of its side or before
// 0, whatever the cells hold; a length past its n_max touches nothing (the
// scan stores the count ~0 and raises CRDT_DEV_RANGE).
#pragma once
#include "digest.hpp"
#include "setread.hpp"

namespace crdt {

constexpr int CT = kTile;                 // merge items per tile
constexpr int CCB = 512;                  // count pass threads
constexpr int CNI = CT / CCB;             // merge items per count thread
constexpr int CNW = kTileNW;              // words per tile and bitmap
constexpr int CWB = 256;                  // write pass threads (one output each per round)
constexpr int CCAP = CT + 4;              // staged slots: each side's run, the element before and the one after it
constexpr int CBS = 3 * CNW;              // bitmap words per tile: `isb`, `emit`, `pair`

// A[i] <= B[j] by (key, rep), through the split's crdt_tuples view (ts and tomb are never dereferenced)
struct CellLe {
    static __device__ __forceinline__ bool le(const crdt_tuples &A, uint64_t i, const crdt_tuples &B, uint64_t j) {
        const uint64_t ka = A.key[i], kb = B.key[j];
        if (ka != kb) return ka < kb;
        return A.rep[i] <= B.rep[j];
    }
};
// delta: side a = dst, side b = src; no tile without a src cell
struct CmDeltaTiles {
    static __device__ __forceinline__ uint64_t tiles(uint64_t nd, uint64_t ns) { return ns ? (ns + nd + CT - 1) / CT : 0; }
};
// what a cell held by both sides becomes
struct CmMax {
    static __device__ __forceinline__ uint64_t f(uint64_t a, uint64_t b) { return a > b ? a : b; }
};
struct CmAdd {
    static __device__ __forceinline__ uint64_t f(uint64_t a, uint64_t b) { return a + b; }
};

// ---------------------------------------------------------------- count (two-sided)
template <bool DELTA, bool BITS, class Tiles>
__global__ __launch_bounds__(CCB) void k_cmap_count(crdt_cmap A, uint64_t na_max, const uint64_t *__restrict__ na_dev,
                                                    crdt_cmap B, uint64_t nb_max, const uint64_t *__restrict__ nb_dev,
                                                    const uint64_t *__restrict__ split, uint32_t *__restrict__ tcnt,
                                                    uint64_t *__restrict__ bits) {
    // staged: a slots 0 .. ta + 1 = A[i0 - 1 .. i1], then b slots = B[j0 - 1 .. j1]
    __shared__ uint64_t sk[CCAP];
    __shared__ uint32_t sr[CCAP];
    __shared__ uint32_t s_c[CCB / 64];
    uint64_t na, nb;
    if (!tile_len(na_max, na_dev, nb_max, nb_dev, &na, &nb)) return;
    const uint64_t t = blockIdx.x;
    if (t >= Tiles::tiles(na, nb)) return;               // (uniform)
    const uint64_t n = na + nb, d0 = t * CT, d1 = d0 + CT < n ? d0 + CT : n;
    const uint64_t i0 = split[t], i1 = split[t + 1], j0 = d0 - i0, j1 = d1 - i1;
    // (sides that break the order can leave splits that run backwards: such a tile emits nothing)
    const bool sane = i1 >= i0 && j1 >= j0 && i1 <= na && j1 <= nb && i1 - i0 <= (uint64_t)CT && j1 - j0 <= (uint64_t)CT;
    const uint32_t ta = sane ? (uint32_t)(i1 - i0) : 0u, tb = sane ? (uint32_t)(j1 - j0) : 0u, tn = ta + tb;
    const uint32_t so = ta + 2, nst = so + tb + 2;       // first b slot, slots in all
    {
        constexpr int NL = (CCAP + CCB - 1) / CCB;
        uint64_t k[NL];
        uint32_t r[NL];
#pragma unroll
        for (int j = 0; j < NL; ++j) {                   // every staging load issued before the first store
            const uint32_t x = threadIdx.x + (uint32_t)j * CCB;
            const bool on_a = x < so;
            const uint64_t g = on_a ? i0 + x - 1 : j0 + (x - so) - 1;   // (slot 0 of an unstarted side wraps: not below its length)
            const bool v = x < nst && g < (on_a ? na : nb);
            k[j] = v ? (on_a ? A.key : B.key)[g] : 0;
            r[j] = v ? (on_a ? A.rep : B.rep)[g] : 0;
        }
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const uint32_t x = threadIdx.x + (uint32_t)j * CCB;
            if (x < nst && x < (uint32_t)CCAP) {
                sk[x] = k[j];
                sr[x] = r[j];
            }
        }
    }
    __syncthreads();
    // heads run one past each side's tile elements when the side goes on: the
    // item merged after the tile's last is then a head like any other
    const uint32_t tax = ta + (sane && i1 < na ? 1u : 0u), tbx = tb + (sane && j1 < nb ? 1u : 0u);
    // a element x (slot 1 + x) <= b element y (slot so + 1 + y)
    auto le = [&](uint32_t x, uint32_t y) -> bool {
        const uint32_t xa = 1 + x, xb = so + 1 + y;
        const uint64_t ka = sk[xa], kb = sk[xb];
        if (ka != kb) return ka < kb;
        return sr[xa] <= sr[xb];
    };
    auto same = [&](uint32_t x, uint32_t y) -> bool { return sk[x] == sk[y] && sr[x] == sr[y]; };   // slots x, y: one cell
    const uint32_t k0 = threadIdx.x * CNI < tn ? threadIdx.x * CNI : tn;
    const uint32_t k1 = k0 + CNI < tn ? k0 + CNI : tn;
    uint32_t isb = 0, emit = 0, pair = 0;
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
            if (!end) continue;
            // a's copy of a b item's cell is the a element merged before it: slot ia
            const bool both = !is_a && i0 + ia > 0 && same(ia, cur);
            if (!DELTA) {
                emit |= 1u << i;
                if (both) pair |= 1u << i;
            } else if (!is_a) {
                bool ship = true;
                const uint64_t js = j0 + ib - 1, id = i0 + ia - 1;   // (64-bit: ia may be 0 with i0 > 0)
                if (both && js < nb && id < na) ship = B.p[js] > A.p[id] || B.n[js] > A.n[id];
                if (ship) emit |= 1u << i;
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (BITS) {
        constexpr int LPW = 64 / CNI;
        const int sh = (lane % LPW) * CNI;
        uint64_t wb = (uint64_t)isb << sh, we = (uint64_t)emit << sh, wp = (uint64_t)pair << sh;
#pragma unroll
        for (int o = 1; o < LPW; o <<= 1) {
            wb |= (uint64_t)__shfl_xor((unsigned long long)wb, o);
            we |= (uint64_t)__shfl_xor((unsigned long long)we, o);
            if (!DELTA) wp |= (uint64_t)__shfl_xor((unsigned long long)wp, o);
        }
        if (lane % LPW == 0) {
            const uint32_t w = threadIdx.x / LPW;
            uint64_t *b = bits + t * CBS;
            b[w] = wb;
            b[CNW + w] = we;
            if (!DELTA) b[2 * CNW + w] = wp;
        }
    }
    uint32_t c = (uint32_t)__popc(emit);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) s_c[wv] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int w = 0; w < CCB / 64; ++w) tot += s_c[w];
        tcnt[t] = tot;
    }
}

// ---------------------------------------------------------------- write (merge, apply)
template <class Comb>
__global__ __launch_bounds__(CWB) void k_cmap_write(crdt_cmap A, uint64_t na_max, const uint64_t *__restrict__ na_dev,
                                                    crdt_cmap B, uint64_t nb_max, const uint64_t *__restrict__ nb_dev,
                                                    const uint64_t *__restrict__ split,
                                                    const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ic,
                                                    crdt_cmap out, uint32_t *__restrict__ err) {
    uint64_t na, nb;
    if (!tile_len(na_max, na_dev, nb_max, nb_dev, &na, &nb)) return;
    const uint64_t t = blockIdx.x;
    if (t >= PlainTiles::tiles(na, nb)) return;
    const int lane = threadIdx.x & 63;
    const uint64_t *b = bits + t * CBS;
    const RankWords k = rank_words(b, lane);              // `isb`, `emit` and their prefix counts
    const uint64_t wp = lane < CNW ? b[2 * CNW + lane] : 0ull;
    const uint32_t ne = k.ne;
    const uint64_t i0 = split[t], j0 = t * CT - i0, base = ic[t], cap = na_max + nb_max;
    bool bad = false;
    for (uint32_t r0 = 0; r0 < ne; r0 += CWB) {          // (uniform: the shuffles below read every word's lane)
        const bool valid = r0 + threadIdx.x < ne;
        const uint32_t r = valid ? r0 + threadIdx.x : ne - 1;
        const RankHit h = rank_select(k, r);
        const uint64_t qb = h.qb, qe = h.qe;
        const uint64_t qp = (uint64_t)__shfl((unsigned long long)wp, h.w, 64);
        const uint32_t pos = h.pos;
        if (!valid) continue;
        // (the bitmaps of this call's count pass never fail the checks below)
        if (!((qe >> pos) & 1)) {
            bad = true;
            continue;
        }
        const uint32_t bb = h.nb;                            // b items merged before this one
        const uint32_t ab = (uint32_t)h.w * 64 + pos - bb;   // a items
        const bool is_b = (qb >> pos) & 1, both = (qp >> pos) & 1;
        const uint64_t i = is_b ? j0 + bb : i0 + ab;     // the item's index on its side
        const uint64_t ia = i0 + ab;                     // a elements merged before it: a's copy is the last of them
        const uint64_t at = base + r;
        if (!(i < (is_b ? nb : na) && at < cap) || (both && !(is_b && ia > 0 && ia <= na))) {
            bad = true;
            continue;
        }
        const uint64_t key = (is_b ? B.key : A.key)[i];
        const uint32_t rp = (is_b ? B.rep : A.rep)[i];
        uint64_t p = (is_b ? B.p : A.p)[i], q = (is_b ? B.n : A.n)[i];
        if (both) {
            const uint64_t pa = A.p[ia - 1], qa = A.n[ia - 1];
            p = Comb::f(pa, p);
            q = Comb::f(qa, q);
        }
        out.key[at] = key;
        out.rep[at] = rp;
        out.p[at] = p;
        out.n[at] = q;
    }
    if (bad) atomicOr(err, CRDT_DEV_RANGE);
}

// ---------------------------------------------------------------- write (delta): src's cells
__global__ __launch_bounds__(CWB) void k_cmap_delta_write(crdt_cmap S, uint64_t ns_max, const uint64_t *__restrict__ ns_dev,
                                                          uint64_t nd_max, const uint64_t *__restrict__ nd_dev,
                                                          const uint64_t *__restrict__ split,
                                                          const uint64_t *__restrict__ bits,
                                                          const uint64_t *__restrict__ ic, crdt_cmap out,
                                                          uint32_t *__restrict__ err) {
    uint64_t ns, nd;
    if (!tile_len(ns_max, ns_dev, nd_max, nd_dev, &ns, &nd)) return;
    const uint64_t t = blockIdx.x;
    if (t >= CmDeltaTiles::tiles(nd, ns)) return;
    const int lane = threadIdx.x & 63;
    const RankWords k = rank_words(bits + t * CBS, lane);   // `isb` (a src item), `emit` and their prefix counts
    const uint32_t ne = k.ne;
    const uint64_t j0 = t * CT - split[t], base = ic[t];
    bool bad = false;
    for (uint32_t r0 = 0; r0 < ne; r0 += CWB) {          // (uniform: the shuffles below read every word's lane)
        const bool valid = r0 + threadIdx.x < ne;
        const uint32_t r = valid ? r0 + threadIdx.x : ne - 1;
        const RankHit h = rank_select(k, r);
        const uint64_t i = j0 + h.nb;                    // the src item's index
        const uint64_t at = base + r;
        if (!valid) continue;
        // (the bitmaps of this call's count pass never fail this)
        if (!(((h.qe >> h.pos) & (h.qb >> h.pos) & 1) && i < ns && at < ns_max)) {
            bad = true;
            continue;
        }
        const uint64_t key = S.key[i], p = S.p[i], q = S.n[i];
        const uint32_t rp = S.rep[i];
        out.key[at] = key;
        out.rep[at] = rp;
        out.p[at] = p;
        out.n[at] = q;
    }
    if (bad) atomicOr(err, CRDT_DEV_RANGE);
}

// ---------------------------------------------------------------- values: heads
// The first cell of each key's run, as the tile's emit words; one global
// look-back at a tile's first cell.
template <bool BITS>
__global__ __launch_bounds__(RB) void k_cmap_heads(const uint64_t *__restrict__ key, uint64_t n_max,
                                                   const uint64_t *__restrict__ n_dev, uint32_t *__restrict__ tcnt,
                                                   uint64_t *__restrict__ bits) {
    __shared__ uint32_t s_cnt[RB / 64];
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = blockIdx.x, tb = t * RT;
    if (tb >= n) return;                                 // (uniform; so n > 0 below)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i0 = tb + (uint64_t)wv * (64 * RWW);
    uint64_t k[RWW], kp[RWW];
#pragma unroll
    for (int j = 0; j < RWW; ++j) {                      // indices clamped into [0, n)
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        const uint64_t a = i < n ? i : n - 1;
        k[j] = key[a];
        kp[j] = key[a > 0 ? a - 1 : 0];
    }
    uint32_t cnt = 0;
    uint64_t mine = 0;
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        const uint64_t e = __ballot(i < n && (i == 0 || k[j] != kp[j]));
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

// ---------------------------------------------------------------- values: sums
// A key run that crosses a tile boundary is summed by atomics, one per (tile,
// run piece) and column; its row is the one before the first row of every tile
// it runs into: zeroed here, ahead of the sums.  (Several tiles may zero one
// row: the same store.)
__global__ __launch_bounds__(256) void k_cmap_zero(uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                   const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ic,
                                                   uint64_t *__restrict__ p_out, uint64_t *__restrict__ n_out,
                                                   int64_t *__restrict__ v_out) {
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0 || t * RT >= n) return;
    if (bits[t * RNW] & 1) return;                       // the tile starts a key
    const uint64_t row = ic[t] - 1;
    if (row >= n_max) return;                            // (never: cell 0 is a head)
    if (p_out) p_out[row] = 0;
    if (n_out) n_out[row] = 0;
    if (v_out) v_out[row] = 0;
}

// One workgroup per tile, a lane per cell: a segmented inclusive scan of (p, n)
// inside each 64-cell word, the words' open tails chained through LDS, and at
// the last cell of each run piece the piece's sums: one plain store per column
// when the run lies wholly inside the tile, else one atomic add per column
// (integer sums mod 2^64 do not depend on the order).  A row gets plain stores
// alone or atomics alone.
__global__ __launch_bounds__(RB) void k_cmap_sums(const uint64_t *__restrict__ p, const uint64_t *__restrict__ q,
                                                  uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                  const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ic,
                                                  uint64_t *__restrict__ p_out, uint64_t *__restrict__ n_out,
                                                  int64_t *__restrict__ v_out, uint32_t *__restrict__ err) {
    __shared__ uint64_t s_tp[RNW], s_tn[RNW];            // per word: the sums from its last head (else its start) to its end
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = blockIdx.x, tb = t * RT;
    if (tb >= n) return;                                 // (uniform)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t xp[RWW], xn[RWW];
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        const uint64_t i = tb + (uint64_t)(wv * RWW + j) * 64 + lane;
        xp[j] = i < n ? p[i] : 0;
        xn[j] = i < n ? q[i] : 0;
    }
    // every wave holds the tile's head words, lane w word w, and the heads before each word
    const uint64_t wd = lane < RNW ? bits[t * RNW + lane] : 0ull;
    // the cell after the tile starts a key (the end of the state counts as one)
    const bool nh = tb + RT < n ? (bits[(t + 1) * RNW] & 1) != 0 : true;
    const uint32_t pc = (uint32_t)__popcll(wd);
    uint32_t hx = pc;
#pragma unroll
    for (int o = 1; o < RNW; o <<= 1) {
        const uint32_t y = __shfl_up(hx, o, 64);
        if (lane >= o) hx += y;
    }
    hx -= pc;
    const uint64_t hm = __ballot(wd != 0);               // bit w: word w holds a head
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        const int w = wv * RWW + j;
        const uint64_t H = (uint64_t)__shfl((unsigned long long)wd, w, 64);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t yp = (uint64_t)__shfl_up((unsigned long long)xp[j], o, 64);
            const uint64_t yn = (uint64_t)__shfl_up((unsigned long long)xn[j], o, 64);
            // no head in (lane - o, lane]: the cell o back is of this cell's run
            if (lane >= o && ((H >> (lane - o + 1)) & ((1ull << o) - 1)) == 0) {
                xp[j] += yp;
                xn[j] += yn;
            }
        }
        if (lane == 63) {
            s_tp[w] = xp[j];
            s_tn[w] = xn[j];
        }
    }
    __syncthreads();
    const uint64_t base = ic[t];
    // What the words before word w leave open, lane w: the tails back to the nearest word with a head, that
    // word's included -- one segmented scan of the 32 tails per wave (a word with a head starts a segment),
    // then one lane up.
    uint64_t cpl = lane < RNW ? s_tp[lane] : 0ull, cnl = lane < RNW ? s_tn[lane] : 0ull;
#pragma unroll
    for (int o = 1; o < RNW; o <<= 1) {
        const uint64_t yp = (uint64_t)__shfl_up((unsigned long long)cpl, o, 64);
        const uint64_t yn = (uint64_t)__shfl_up((unsigned long long)cnl, o, 64);
        if (lane >= o && ((hm >> (lane - o + 1)) & ((1ull << o) - 1)) == 0) {
            cpl += yp;
            cnl += yn;
        }
    }
    cpl = (uint64_t)__shfl_up((unsigned long long)cpl, 1, 64);
    cnl = (uint64_t)__shfl_up((unsigned long long)cnl, 1, 64);
    if (lane == 0) cpl = cnl = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        const int w = wv * RWW + j;
        const uint64_t i = tb + (uint64_t)w * 64 + lane;
        const uint64_t H = (uint64_t)__shfl((unsigned long long)wd, w, 64);
        const uint32_t hb = __shfl(hx, w, 64);
        const uint64_t Hn = w + 1 < RNW ? (uint64_t)__shfl((unsigned long long)wd, (w + 1) & (RNW - 1), 64) : 0ull;
        const uint64_t cp = (uint64_t)__shfl((unsigned long long)cpl, w, 64);
        const uint64_t cn = (uint64_t)__shfl((unsigned long long)cnl, w, 64);
        const uint64_t upto = (2ull << lane) - 1;        // bits 0 .. lane
        const bool last = w == RNW - 1 && lane == 63;    // the tile's last cell
        const bool nxt = lane < 63 ? ((H >> (lane + 1)) & 1) != 0 : (last ? nh : (Hn & 1) != 0);
        if (!(i < n && (i + 1 >= n || nxt || last))) continue;   // the last cell of a run piece
        const bool open = (H & upto) == 0;               // the piece began before this word
        const uint32_t heads = hb + (uint32_t)__popcll(H & upto);   // the tile's heads up to this cell
        const uint64_t sp = xp[j] + (open ? cp : 0), sn = xn[j] + (open ? cn : 0);
        const uint64_t row = base + heads - 1;
        if (base + heads == 0 || row >= n_max) {         // (the bitmaps of this call's heads pass never do this)
            bad = true;
            continue;
        }
        if (heads > 0 && (i + 1 >= n || nxt)) {          // the run lies inside the tile
            if (p_out) p_out[row] = sp;
            if (n_out) n_out[row] = sn;
            if (v_out) v_out[row] = (int64_t)(sp - sn);
        } else {
            if (p_out) atomicAdd((unsigned long long *)&p_out[row], (unsigned long long)sp);
            if (n_out) atomicAdd((unsigned long long *)&n_out[row], (unsigned long long)sn);
            if (v_out) atomicAdd((unsigned long long *)&v_out[row], (unsigned long long)(sp - sn));
        }
    }
    if (bad) atomicOr(err, CRDT_DEV_RANGE);
}

// ---------------------------------------------------------------- combine (crdt_cmap_combine)
// Sorted cells with repeats -> one cell per distinct (key, rep), p and n summed
// over the run: values' by-position scaffold with a head at every change of
// (key, rep).  R: the rep column's element (uint32_t; uint64_t for the sorted
// view of crdt_cmap_from_ops, whose ts column holds rep widened).
//
// Heads: a cell's predecessor comes from the lane below (the word before for
// lane 0); each wave's first cell looks back once in global memory, in both
// columns (four look-backs a tile, the first of them across the tile edge).
template <bool BITS, class R>
__global__ __launch_bounds__(RB) void k_cmap_cheads(const uint64_t *__restrict__ key, const R *__restrict__ rep,
                                                    uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                    uint32_t *__restrict__ tcnt, uint64_t *__restrict__ bits) {
    __shared__ uint32_t s_cnt[RB / 64];
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = blockIdx.x, tb = t * RT;
    if (tb >= n) return;                                 // (uniform; so n > 0 below)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i0 = tb + (uint64_t)wv * (64 * RWW);
    uint64_t k[RWW];
    R r[RWW];
#pragma unroll
    for (int j = 0; j < RWW; ++j) {                      // indices clamped into [0, n)
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        const uint64_t a = i < n ? i : n - 1;
        k[j] = key[a];
        r[j] = rep[a];
    }
    const uint64_t b = i0 > 0 ? (i0 - 1 < n ? i0 - 1 : n - 1) : 0;   // the cell before the wave's first (uniform)
    uint64_t ck = key[b];
    R cr = rep[b];
    uint32_t cnt = 0;
    uint64_t mine = 0;
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        uint64_t kp = (uint64_t)__shfl_up((unsigned long long)k[j], 1, 64);
        R rp = __shfl_up(r[j], 1, 64);
        if (lane == 0) {
            kp = ck;
            rp = cr;
        }
        const uint64_t e = __ballot(i < n && (i == 0 || k[j] != kp || r[j] != rp));
        cnt += (uint32_t)__popcll(e);
        if (lane == j) mine = e;
        ck = (uint64_t)__shfl((unsigned long long)k[j], 63, 64);
        cr = __shfl(r[j], 63, 64);
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

// k_cmap_sums' pass over two policies (k_cmap_sums itself is kept as it was
// written: through the policies the compiler schedules its loads differently,
// and crdt_cmap_values' code objects are not to change).  Src: where cell i's
// (p, n) come from -- load() fills the wave's RWW words, zeros at and past n,
// and answers whether a contribution had to be refused.  Sink: where a run
// piece's sums go (plain() / atomic()) and what is stored at each head cell
// beside them (head(i, row): the row's key columns).
struct CmSrcDirect {                                     // cell i contributes p[i], q[i]
    const uint64_t *__restrict__ p, *__restrict__ q;
    __device__ __forceinline__ bool load(uint64_t tb, int wv, int lane, uint64_t n, uint64_t *xp, uint64_t *xn) const {
#pragma unroll
        for (int j = 0; j < RWW; ++j) {
            const uint64_t i = tb + (uint64_t)(wv * RWW + j) * 64 + lane;
            xp[j] = i < n ? p[i] : 0;
            xn[j] = i < n ? q[i] : 0;
        }
        return false;
    }
};
template <class Src, class Sink>
__device__ __forceinline__ void cmap_sums_tile(const Src &src, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                               const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ic,
                                               const Sink &sink, uint32_t *__restrict__ err, uint64_t *s_tp,
                                               uint64_t *s_tn) {
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = blockIdx.x, tb = t * RT;
    if (tb >= n) return;                                 // (uniform)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t xp[RWW], xn[RWW];
    bool bad = src.load(tb, wv, lane, n, xp, xn);
    // every wave holds the tile's head words, lane w word w, and the heads before each word
    const uint64_t wd = lane < RNW ? bits[t * RNW + lane] : 0ull;
    // the cell after the tile starts a key (the end of the state counts as one)
    const bool nh = tb + RT < n ? (bits[(t + 1) * RNW] & 1) != 0 : true;
    const uint32_t pc = (uint32_t)__popcll(wd);
    uint32_t hx = pc;
#pragma unroll
    for (int o = 1; o < RNW; o <<= 1) {
        const uint32_t y = __shfl_up(hx, o, 64);
        if (lane >= o) hx += y;
    }
    hx -= pc;
    const uint64_t hm = __ballot(wd != 0);               // bit w: word w holds a head
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        const int w = wv * RWW + j;
        const uint64_t H = (uint64_t)__shfl((unsigned long long)wd, w, 64);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t yp = (uint64_t)__shfl_up((unsigned long long)xp[j], o, 64);
            const uint64_t yn = (uint64_t)__shfl_up((unsigned long long)xn[j], o, 64);
            // no head in (lane - o, lane]: the cell o back is of this cell's run
            if (lane >= o && ((H >> (lane - o + 1)) & ((1ull << o) - 1)) == 0) {
                xp[j] += yp;
                xn[j] += yn;
            }
        }
        if (lane == 63) {
            s_tp[w] = xp[j];
            s_tn[w] = xn[j];
        }
    }
    __syncthreads();
    const uint64_t base = ic[t];
    // What the words before word w leave open, lane w: the tails back to the nearest word with a head, that
    // word's included -- one segmented scan of the 32 tails per wave (a word with a head starts a segment),
    // then one lane up.
    uint64_t cpl = lane < RNW ? s_tp[lane] : 0ull, cnl = lane < RNW ? s_tn[lane] : 0ull;
#pragma unroll
    for (int o = 1; o < RNW; o <<= 1) {
        const uint64_t yp = (uint64_t)__shfl_up((unsigned long long)cpl, o, 64);
        const uint64_t yn = (uint64_t)__shfl_up((unsigned long long)cnl, o, 64);
        if (lane >= o && ((hm >> (lane - o + 1)) & ((1ull << o) - 1)) == 0) {
            cpl += yp;
            cnl += yn;
        }
    }
    cpl = (uint64_t)__shfl_up((unsigned long long)cpl, 1, 64);
    cnl = (uint64_t)__shfl_up((unsigned long long)cnl, 1, 64);
    if (lane == 0) cpl = cnl = 0;
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        const int w = wv * RWW + j;
        const uint64_t i = tb + (uint64_t)w * 64 + lane;
        const uint64_t H = (uint64_t)__shfl((unsigned long long)wd, w, 64);
        const uint32_t hb = __shfl(hx, w, 64);
        const uint64_t Hn = w + 1 < RNW ? (uint64_t)__shfl((unsigned long long)wd, (w + 1) & (RNW - 1), 64) : 0ull;
        const uint64_t cp = (uint64_t)__shfl((unsigned long long)cpl, w, 64);
        const uint64_t cn = (uint64_t)__shfl((unsigned long long)cnl, w, 64);
        const uint64_t upto = (2ull << lane) - 1;        // bits 0 .. lane
        const bool last = w == RNW - 1 && lane == 63;    // the tile's last cell
        const bool nxt = lane < 63 ? ((H >> (lane + 1)) & 1) != 0 : (last ? nh : (Hn & 1) != 0);
        if (i < n && ((H >> lane) & 1)) {                // a head: its row is the run's
            const uint64_t hrow = base + hb + (uint32_t)__popcll(H & upto) - 1;
            if (hrow < n_max) sink.head(i, hrow);
            else bad = true;
        }
        if (!(i < n && (i + 1 >= n || nxt || last))) continue;   // the last cell of a run piece
        const bool open = (H & upto) == 0;               // the piece began before this word
        const uint32_t heads = hb + (uint32_t)__popcll(H & upto);   // the tile's heads up to this cell
        const uint64_t sp = xp[j] + (open ? cp : 0), sn = xn[j] + (open ? cn : 0);
        const uint64_t row = base + heads - 1;
        if (base + heads == 0 || row >= n_max) {         // (the bitmaps of this call's heads pass never do this)
            bad = true;
            continue;
        }
        if (heads > 0 && (i + 1 >= n || nxt)) sink.plain(row, sp, sn);   // the run lies inside the tile
        else sink.atomic(row, sp, sn);
    }
    if (bad) atomicOr(err, CRDT_DEV_RANGE);
}

// Cell i contributes p[idx[i]], q[idx[i]] (columns of n_src > 0 elements): the
// gather fused behind an index-carrying sort.  No load is predicated: positions
// are clamped into [0, n) and a refused index to element 0, so all 8 index
// loads go out together, then all 16 gathers, and the selects follow; an index
// at or past n_src contributes 0 and is reported.
struct CmSrcIndexed {
    const uint64_t *__restrict__ p, *__restrict__ q;
    const uint32_t *__restrict__ idx;
    uint64_t n_src;
    __device__ __forceinline__ bool load(uint64_t tb, int wv, int lane, uint64_t n, uint64_t *xp, uint64_t *xn) const {
        uint32_t at[RWW];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < RWW; ++j) {                  // (the caller's tb < n: so n > 0)
            const uint64_t i = tb + (uint64_t)(wv * RWW + j) * 64 + lane;
            at[j] = idx[i < n ? i : n - 1];
        }
        uint64_t gp[RWW], gq[RWW];
#pragma unroll
        for (int j = 0; j < RWW; ++j) {
            const uint32_t a = (uint64_t)at[j] < n_src ? at[j] : 0u;
            gp[j] = p[a];
            gq[j] = q[a];
        }
#pragma unroll
        for (int j = 0; j < RWW; ++j) {
            const uint64_t i = tb + (uint64_t)(wv * RWW + j) * 64 + lane;
            const bool in = (uint64_t)at[j] < n_src;
            bad |= i < n && !in;
            xp[j] = i < n && in ? gp[j] : 0;
            xn[j] = i < n && in ? gq[j] : 0;
        }
        return bad;
    }
};
// the combined cells: each row's key and rep from its head cell, its sums
template <class R>
struct CmSinkCells {
    const uint64_t *__restrict__ key;
    const R *__restrict__ rep;
    crdt_cmap out;
    __device__ __forceinline__ void head(uint64_t i, uint64_t row) const {
        const uint64_t k = key[i];
        const R r = rep[i];
        out.key[row] = k;
        out.rep[row] = (uint32_t)r;
    }
    __device__ __forceinline__ void plain(uint64_t row, uint64_t sp, uint64_t sn) const {
        out.p[row] = sp;
        out.n[row] = sn;
    }
    __device__ __forceinline__ void atomic(uint64_t row, uint64_t sp, uint64_t sn) const {
        atomicAdd((unsigned long long *)&out.p[row], (unsigned long long)sp);
        atomicAdd((unsigned long long *)&out.n[row], (unsigned long long)sn);
    }
};
// values' sums pass over the combine's heads (k_cmap_zero in front, as there)
template <class Src, class R>
__global__ __launch_bounds__(RB) void k_cmap_csums(Src src, const uint64_t *__restrict__ key, const R *__restrict__ rep,
                                                   uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                   const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ic,
                                                   crdt_cmap out, uint32_t *__restrict__ err) {
    __shared__ uint64_t s_tp[RNW], s_tn[RNW];
    cmap_sums_tile(src, n_max, n_dev, bits, ic, CmSinkCells<R>{key, rep, out}, err, s_tp, s_tn);
}

// crdt_cmap_from_ops: the operations as the sort's tuples (key, ts = rep
// widened, rep = the operation's index, tomb = 0) -- the three columns the
// caller does not hold
__global__ __launch_bounds__(256) void k_cmap_ops_view(const uint32_t *__restrict__ op_rep, uint64_t m,
                                                       uint64_t *__restrict__ ts, uint32_t *__restrict__ index,
                                                       uint8_t *__restrict__ tomb) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        ts[i] = (uint64_t)op_rep[i];
        index[i] = (uint32_t)i;
        tomb[i] = 0;
    }
}

// ---------------------------------------------------------------- lookup
// One probe per lane: the first cell of the key by binary search, then the
// key's run.  A lane walks up to kLookupWalk cells of its run itself; a longer
// run (one key may have thousands of replicas) is finished by the whole wave:
// its end by one more binary search, the rest summed 64 cells a step and
// reduced, one such run after another.  The loop is wave-uniform, so that
// every lane takes part in the shuffles.  A length out of range: every value
// 0, every found 0.
constexpr uint32_t kLookupWalk = 32;
__global__ __launch_bounds__(256) void k_cmap_lookup(crdt_cmap T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                     const uint64_t *__restrict__ probes, uint64_t m,
                                                     int64_t *__restrict__ value, uint8_t *__restrict__ found,
                                                     uint32_t *__restrict__ err) {
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) {
        n = 0;
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, CRDT_DEV_RANGE);
    }
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < m; i0 += (uint64_t)gridDim.x * 256) {
        const uint64_t i = i0 + lane;
        const bool valid = i < m;
        const uint64_t x = valid ? probes[i] : 0;
        uint64_t lo = 0, hi = valid ? n : 0;             // lo -> the first cell with a key at or above x
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (T.key[mid] < x) lo = mid + 1;
            else hi = mid;
        }
        uint64_t s = 0, j = lo;
        const uint64_t stop = valid ? (n - lo < kLookupWalk ? n : lo + kLookupWalk) : 0;
        for (; j < stop && T.key[j] == x; ++j) s += T.p[j] - T.n[j];
        const bool hit = j > lo;
        // the run goes on past the lane's own walk: its end, the first cell from j on with a key above x
        const bool more = valid && j == lo + kLookupWalk && j < n && T.key[j] == x;
        uint64_t ub = j;
        if (more) {
            uint64_t h = n;
            while (ub < h) {
                const uint64_t mid = ub + ((h - ub) >> 1);
                if (T.key[mid] <= x) ub = mid + 1;
                else h = mid;
            }
        }
        for (uint64_t pend = __ballot(more); pend; pend &= pend - 1) {   // (uniform)
            const int l = __builtin_ctzll(pend);
            const uint64_t b = (uint64_t)__shfl((unsigned long long)j, l, 64);
            const uint64_t e = (uint64_t)__shfl((unsigned long long)ub, l, 64);
            uint64_t part = 0;
            for (uint64_t c = b + lane; c < e; c += 64) part += T.p[c] - T.n[c];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part += (uint64_t)__shfl_xor((unsigned long long)part, o, 64);
            if ((int)lane == l) s += part;
        }
        if (valid) {
            value[i] = (int64_t)s;
            if (found) found[i] = hit ? 1 : 0;
        }
    }
}

// ---------------------------------------------------------------- range digests
// h(key, rep, p, n) = sm(sm(sm(sm(key) ^ rep) ^ p) ^ n), sm = SplitMix64's output function
__device__ __forceinline__ uint64_t cm_hash(uint64_t key, uint32_t rep, uint64_t p, uint64_t n) {
    return splitmix64(splitmix64(splitmix64(splitmix64(key) ^ (uint64_t)rep) ^ p) ^ n);
}

// hash[b] += the cells' hashes, count[b] += their number, per bucket (both
// zeroed by k_dig_init ahead of this kernel).  No LDS, no barrier, no waiting
// between workgroups.
__global__ __launch_bounds__(RB) void k_cmap_digest(crdt_cmap T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                    const uint64_t *__restrict__ sp, uint32_t m,
                                                    uint64_t *__restrict__ hash, uint64_t *__restrict__ count) {
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t tb = (uint64_t)blockIdx.x * RT;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i0 = tb + (uint64_t)wv * (64 * RWW);
    if (i0 >= n) return;                                 // (wave-uniform; so n > 0 below)
    uint64_t k[RWW], p[RWW], q[RWW];
    uint32_t r[RWW];
#pragma unroll
    for (int j = 0; j < RWW; ++j) {                      // all four columns in flight; indices clamped into [0, n)
        const uint64_t i = i0 + (uint64_t)j * 64 + lane;
        const uint64_t a = i < n ? i : n - 1;
        k[j] = T.key[a];
        r[j] = T.rep[a];
        p[j] = T.p[a];
        q[j] = T.n[a];
    }
    uint32_t blo, bhi;
    dig_wave_buckets(sp, m, k, &blo, &bhi);
    if (blo == bhi) {                                    // the whole wave in one bucket
        uint64_t h = 0;
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < RWW; ++j) {
            if (i0 + (uint64_t)j * 64 + lane < n) {
                h += cm_hash(k[j], r[j], p[j], q[j]);
                ++c;
            }
        }
        dig_add_wave(h, c, lane, blo, hash, count);
        return;
    }
#pragma unroll
    for (int j = 0; j < RWW; ++j) {
        const bool v = i0 + (uint64_t)j * 64 + lane < n;
        if (__ballot(v) == 0) continue;
        const uint32_t b = dig_ub(sp, blo, bhi, k[j]);   // (a clamped lane: the last cell's bucket, with nothing to add)
        dig_add_runs(v ? cm_hash(k[j], r[j], p[j], q[j]) : 0ull, v ? 1u : 0u, lane, b, hash, count);
    }
}

// select, count pass: the cells whose bucket is flagged, as the tile's emit
// words and count.  Only keys, splitters and flags are read.
template <bool BITS>
__global__ __launch_bounds__(RB) void k_cmap_sel_count(const uint64_t *__restrict__ key, uint64_t n_max,
                                                       const uint64_t *__restrict__ n_dev,
                                                       const uint64_t *__restrict__ sp, uint32_t m,
                                                       const uint8_t *__restrict__ flags, uint32_t *__restrict__ tcnt,
                                                       uint64_t *__restrict__ bits) {
    __shared__ uint32_t s_cnt[RB / 64];
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = blockIdx.x, tb = t * RT;
    if (tb >= n) return;                                 // (uniform; so n > 0 below)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i0 = tb + (uint64_t)wv * (64 * RWW);
    uint32_t cnt = 0;
    uint64_t mine = 0;
    if (i0 < n) {                                        // (wave-uniform)
        uint64_t k[RWW];
#pragma unroll
        for (int j = 0; j < RWW; ++j) {                  // indices clamped into [0, n)
            const uint64_t i = i0 + (uint64_t)j * 64 + lane;
            k[j] = key[i < n ? i : n - 1];
        }
        uint32_t blo, bhi;
        dig_wave_buckets(sp, m, k, &blo, &bhi);
        const bool one = blo == bhi;
        const bool f1 = one && flags[blo] != 0;
#pragma unroll
        for (int j = 0; j < RWW; ++j) {
            const bool v = i0 + (uint64_t)j * 64 + lane < n;
            bool f = f1;
            if (!one && v) f = flags[dig_ub(sp, blo, bhi, k[j])] != 0;
            const uint64_t e = __ballot(v && f);
            cnt += (uint32_t)__popcll(e);
            if (lane == j) mine = e;
        }
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

// select, write pass: the four columns of the emitting cells in one kernel
// (the bitmap and its prefix counts are read once, not once per column)
__global__ __launch_bounds__(kTileB) void k_cmap_sel_write(crdt_cmap T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                           const uint64_t *__restrict__ bits,
                                                           const uint64_t *__restrict__ ic, crdt_cmap out,
                                                           uint32_t *__restrict__ err) {
    tile_emit_by_position<false>(n_max, n_dev, bits, ic, err, [&](uint64_t i, uint64_t at, uint8_t) {
        const uint64_t key = T.key[i], p = T.p[i], q = T.n[i];
        const uint32_t rp = T.rep[i];
        out.key[at] = key;
        out.rep[at] = rp;
        out.p[at] = p;
        out.n[at] = q;
    });
}

}  // namespace crdt
