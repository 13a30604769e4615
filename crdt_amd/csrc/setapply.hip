// setapply.hip -- the OR-Set mutators: a batch of local adds and removes applied
// to a sorted state on the device (crdt_set_apply).
//
// Semantics.  t[0 .. n) is sorted ascending by (key, ts, rep), copies of one tag
// in any order and number; the applying replica rep holds the clock row
// clock[0 .. n_clock); the batch is m operations (op_key non-decreasing, op_kind
// 0 = add, else remove).  With ts0 = clock[rep], operation i is event e_i = ts0
// + 1 + i of rep -- add and remove alike, in both forms -- and the result is the
// batch applied one operation at a time in index order:
//   add(k)     inserts the tag (k, e_i, rep), tomb 0;
//   remove(k)  tombstone form: tomb = 1 on every tag of k held at that point;
//              causal form: every tag of k held at that point is deleted.
// In closed form: a tag of t is tombstoned / dropped iff the batch holds any
// remove of its key; the tag of add i iff a remove of its key sits at an index
// > i; the output is the sorted union, each tag once, tombstone form with tomb =
// the OR over the tag's copies then the removes, causal form with a tag whose
// tomb-OR is 1 in t dropped and every output tomb 0.
//
// GPU structure: setcausal.hip's, over the merged order of (t, the batch's tags):
//   scan   : R[i] = the removes among operations [0, i) (scan_lb, scan.hpp);
//   tags   : per operation its event as a tag (ts, rep) and three bits: `dead`,
//            a remove of the key sits at a later index (R between i + 1 and the
//            end of the key's run of operations), `rm`, the key's run holds a
//            remove, and `notag`, the operation is a remove (it takes its place
//            in the merged order and is never emitted);
//   split  : k_mp_split (settile.hpp) by the full tag over (t, tags);
//   count  : per tile both runs staged in LDS and merged, 512 threads x 4 items.
//            A batch item decides by its own bits.  A state item decides at the
//            LAST copy of its tag in t: the tomb-OR walks back over the copies
//            (LDS, then global memory when the run began in an earlier tile, as
//            k_tile_write's source walk does; every copy is visited by its own
//            run end alone, so the work stays linear), and the "key is removed"
//            bit is the `rm` bit of the key's first operation, found by a lower
//            bound in the operations between the tile's first and last state key:
//            inside the tile's own staged run of operations when its neighbours
//            show that no key's operations cross the tile's edge (LDS alone),
//            else by two wave-wide searches per tile (64 probes a round) and a
//            search in global memory per item; a span with no remove (R) and a
//            batch with none search nothing.  A remove
//            may be merged into a later tile than the tags it kills: no decision
//            depends on another tile, so there is no carry record;
//   scan   : k_tile_scan<NoCarry> (settile.hpp);
//   write  : (out != NULL) one output per lane, by rank (rank_words /
//            rank_select): the four fields, tomb from the third bitmap, and the
//            source index when asked (the walk back to the tag's first copy goes
//            through global memory);
//   finish : clock_out, or the poison when the length or the events are out of
//            range.
//
// The state's length may stay on the device.  *n_dev > n_max, or ts0 + m
// wrapping past 2^64, touches no tuple, stores a count of ~0 and raises
// CRDT_DEV_RANGE; out, src and clock_out stay as they were.  No kernel reads t
// at or past min(*n_dev, n_max), an operation at or past m or the clock at or
// past n_clock, whatever the operation keys hold.
#include "scan.hpp"
#include "settile.hpp"

namespace crdt {

constexpr int AT = kTile;                  // merge items per tile
constexpr int ACB = 512;                   // count pass threads
constexpr int ANI = AT / ACB;              // merge items per count thread
constexpr int ANW = kTileNW;               // words per tile and bitmap
constexpr int AWB = 256;                   // write pass threads (one output each per round)
constexpr int ACAP = AT + 4;               // staged slots: each side's run, the element before and the one after it
// a batch item's bits: killed by a later remove; its key's run holds a remove; it is a remove (an event with no tag)
constexpr uint8_t kApDead = 1, kApRm = 2, kApNoTag = 4;

// the state's length and the replica's clock entry; false: a length out of range, or the batch's events wrap
__device__ __forceinline__ bool apply_len(uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                          const uint64_t *__restrict__ clock, uint32_t rep, uint64_t m, uint64_t *n,
                                          uint64_t *ts0) {
    *ts0 = clock[rep];
    return tile_len(n_max, n_dev, n) && *ts0 + m >= *ts0;
}

// the removes as scan items
struct KindSrc {
    const uint8_t *kind;
    struct Item {
        uint64_t len = 0;
    };
    __device__ Item load(uint64_t i) const { return Item{kind[i] != 0 ? 1ull : 0ull}; }
};

// lo + #{ j in [lo, hi) : sp[j] < key (UB: <= key) } for ascending sp: always
// a value in [lo, max(lo, hi)], and only sp[lo .. hi) is read
template <bool UB>
__device__ __forceinline__ uint64_t ap_bound(const uint64_t *__restrict__ sp, uint64_t lo, uint64_t hi, uint64_t key) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = sp[mid];
        if (UB ? v <= key : v < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The same count over sp[0 .. m) for a wave-uniform key by a whole wave (every
// lane active; setcausal.hip's cz_ub_wave with 64-bit bounds): reads sp[0 .. m)
// only and returns a value in [0, m], whatever sp holds.
template <bool UB>
__device__ __forceinline__ uint64_t ap_bound_wave(const uint64_t *__restrict__ sp, uint64_t m, uint64_t key,
                                                  uint32_t lane) {
    uint64_t lo = 0, hi = m;
    while (lo < hi) {                                    // (uniform)
        const uint64_t span = hi - lo;
        if (span <= 64) {
            bool p = false;
            if (lane < span) {
                const uint64_t v = sp[lo + lane];
                p = UB ? v <= key : v < key;
            }
            return lo + (uint64_t)__popcll(__ballot(p));
        }
        const uint64_t v = sp[lo + (((uint64_t)lane * span) >> 6)];   // (span < 2^58: the host bounds the tiles)
        const uint64_t cnt = (uint64_t)__popcll(__ballot(UB ? v <= key : v < key));
        const uint64_t nlo = cnt ? lo + (((cnt - 1) * span) >> 6) + 1 : lo;
        hi = cnt < 64 ? lo + ((cnt * span) >> 6) : hi;
        lo = nlo;
    }
    return lo;
}

// ---------------------------------------------------------------- the batch's tags
// ts / rep / bits of operation i's tag (key: op_key itself).  R[i] = removes
// among operations [0, i).  The key's run of operations [lb, ub) by two searches
// on either side of i: lb in [0, i], ub in [i + 1, m], whatever the keys hold.
__global__ __launch_bounds__(256) void k_apply_tags(const uint64_t *__restrict__ op_key, uint64_t m,
                                                    const uint64_t *__restrict__ clock, uint32_t rep,
                                                    const uint64_t *__restrict__ R, uint64_t *__restrict__ bts,
                                                    uint32_t *__restrict__ brep, uint8_t *__restrict__ binfo) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const uint64_t k = op_key[i];
    const uint64_t lb = ap_bound<false>(op_key, 0, i, k), ub = ap_bound<true>(op_key, i + 1, m, k);
    const uint64_t r_ub = R[ub], r_i = R[i], r_n = R[i + 1];
    bts[i] = clock[rep] + 1 + i;
    brep[i] = rep;
    binfo[i] = (uint8_t)((r_ub != r_n ? kApDead : 0) | (r_ub != R[lb] ? kApRm : 0) | (r_n != r_i ? kApNoTag : 0));
}

// ---------------------------------------------------------------- count
// A = the state, B = the batch's tags (B.tomb: the kAp bits), nb = m.
template <bool BITS, bool CAUSAL>
__global__ __launch_bounds__(ACB) void k_apply_count(crdt_tuples A, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                     crdt_tuples B, uint64_t m, const uint64_t *__restrict__ clock,
                                                     uint32_t rep, const uint64_t *__restrict__ R,
                                                     const uint64_t *__restrict__ split, uint32_t *__restrict__ tcnt,
                                                     uint64_t *__restrict__ bits) {
    // staged: a slots 0 .. ta + 1 = A[i0 - 1 .. i1], then b slots = B[j0 - 1 .. j1]
    __shared__ uint64_t sk[ACAP];
    __shared__ uint64_t st[ACAP];
    __shared__ uint32_t sr[ACAP];
    __shared__ uint8_t sm[ACAP];
    __shared__ uint32_t s_c[ACB / 64];
    uint64_t na, ts0;
    if (!apply_len(n_max, n_dev, clock, rep, m, &na, &ts0)) return;
    const uint64_t nb = m, t = blockIdx.x;
    if (t >= PlainTiles::tiles(na, nb)) return;                   // (uniform)
    const uint64_t n = na + nb, d0 = t * AT, d1 = d0 + AT < n ? d0 + AT : n;
    const uint64_t i0 = split[t], i1 = split[t + 1], j0 = d0 - i0, j1 = d1 - i1;
    const uint32_t ta = (uint32_t)(i1 - i0), tb = (uint32_t)(j1 - j0), tn = ta + tb;
    const uint32_t so = ta + 2, nst = so + tb + 2;       // first b slot, slots in all
    {
        constexpr int NL = (ACAP + ACB - 1) / ACB;
        uint64_t k[NL], ts[NL];
        uint32_t r[NL];
        uint8_t f[NL];
#pragma unroll
        for (int j = 0; j < NL; ++j) {                   // every staging load issued before the first store
            const uint32_t x = threadIdx.x + (uint32_t)j * ACB;
            const bool on_a = x < so;
            const uint64_t g = on_a ? i0 + x - 1 : j0 + (x - so) - 1;   // (slot 0 of an unstarted side wraps: not below its length)
            const bool v = x < nst && g < (on_a ? na : nb);
            k[j] = v ? (on_a ? A.key : B.key)[g] : 0;
            ts[j] = v ? (on_a ? A.ts : B.ts)[g] : 0;
            r[j] = v ? (on_a ? A.rep : B.rep)[g] : 0;
            f[j] = v ? (on_a ? A.tomb : B.tomb)[g] : 0;
        }
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const uint32_t x = threadIdx.x + (uint32_t)j * ACB;
            if (x < nst && x < (uint32_t)ACAP) {
                sk[x] = k[j];
                st[x] = ts[j];
                sr[x] = r[j];
                sm[x] = f[j];
            }
        }
    }
    __syncthreads();
    // heads run one past each side's tile elements when the side goes on
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
    // The operations a state key of this tile can meet, [blo, bhi), and whether any is a remove (a batch with no
    // remove at all, R[m] == 0, searches nothing).  The keys are sorted: when B[j0 - 1], the operation before
    // the tile's own run B[j0 .. j1), has a key below the tile's first state key, so has every earlier one, and
    // when B[j1] has a key above the last state key, so has every later one -- the span then lies inside the
    // staged run: `inl`, found in LDS as b elements [slo, shi), no global load.  Else (the operations of the
    // tile's first or last key cross its edge) two wave-wide searches of all m operations.
    uint64_t blo = 0, bhi = 0;
    uint32_t slo = 0, shi = 0;
    bool anyrm = false, inl = false;
    if (ta && m && R[m] != 0) {                          // (uniform)
        const uint64_t fa = sk[1], la = sk[ta];
        inl = (j0 == 0 || sk[so] < fa) && (j1 >= nb || sk[so + tb + 1] > la);
        if (inl) {
            uint32_t hi = tb;
            while (slo < hi) {                           // the first b element with key >= fa
                const uint32_t mid = (slo + hi) >> 1;
                if (sk[so + 1 + mid] < fa) slo = mid + 1;
                else hi = mid;
            }
            shi = slo;
            hi = tb;
            while (shi < hi) {                           // the first with key > la
                const uint32_t mid = (shi + hi) >> 1;
                if (sk[so + 1 + mid] <= la) shi = mid + 1;
                else hi = mid;
            }
            anyrm = shi > slo;
        } else {
            blo = ap_bound_wave<false>(B.key, m, fa, threadIdx.x & 63);
            bhi = ap_bound_wave<true>(B.key, m, la, threadIdx.x & 63);
            anyrm = bhi > blo && R[bhi] != R[blo];
        }
    }
    const uint32_t k0 = threadIdx.x * ANI < tn ? threadIdx.x * ANI : tn;
    const uint32_t k1 = k0 + ANI < tn ? k0 + ANI : tn;
    uint32_t isb = 0, emit = 0, tmb = 0;
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
            bool keep, dead;
            if (!is_a) {
                isb |= 1u << i;
                dead = (sm[cur] & kApDead) != 0;
                keep = (sm[cur] & kApNoTag) == 0;        // a remove is an event of its own and leaves no tag
            } else {
                keep = !(ha && same(cur, 1 + ia));       // the last copy of its tag in the state
                dead = false;
                if (keep) {
                    // the tomb-OR over the tag's copies: back through the tile, then through global memory
                    uint32_t x = cur;
                    dead = sm[x] != 0;
                    while (!dead && x > 1 && same(x - 1, x)) {
                        --x;
                        dead = sm[x] != 0;
                    }
                    if (!dead && x == 1 && i0 > 0 && same(0, 1)) {
                        dead = sm[0] != 0;
                        const uint64_t key = sk[cur], ts = st[cur];
                        const uint32_t r = sr[cur];
                        uint64_t g = i0 - 1;
                        while (!dead && g > 0 && A.key[g - 1] == key && A.ts[g - 1] == ts && A.rep[g - 1] == r) {
                            --g;
                            dead = A.tomb[g] != 0;
                        }
                    }
                    if (!dead && anyrm) {                // the key's first operation carries its run's `rm` bit
                        const uint64_t key = sk[cur];
                        if (inl) {
                            uint32_t lo2 = slo, hi2 = shi;
                            while (lo2 < hi2) {
                                const uint32_t mid = (lo2 + hi2) >> 1;
                                if (sk[so + 1 + mid] < key) lo2 = mid + 1;
                                else hi2 = mid;
                            }
                            dead = lo2 < shi && sk[so + 1 + lo2] == key && (sm[so + 1 + lo2] & kApRm) != 0;
                        } else {
                            const uint64_t p = ap_bound<false>(B.key, blo, bhi, key);
                            dead = p < bhi && B.key[p] == key && (B.tomb[p] & kApRm) != 0;
                        }
                    }
                }
            }
            if (keep && !(CAUSAL && dead)) {
                emit |= 1u << i;
                if (!CAUSAL && dead) tmb |= 1u << i;
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (BITS) {
        constexpr int LPW = 64 / ANI;
        const int sh = (lane % LPW) * ANI;
        uint64_t wb = (uint64_t)isb << sh, we = (uint64_t)emit << sh, wt = (uint64_t)tmb << sh;
#pragma unroll
        for (int o = 1; o < LPW; o <<= 1) {
            wb |= (uint64_t)__shfl_xor((unsigned long long)wb, o);
            we |= (uint64_t)__shfl_xor((unsigned long long)we, o);
            wt |= (uint64_t)__shfl_xor((unsigned long long)wt, o);
        }
        if (lane % LPW == 0) {
            const uint32_t w = threadIdx.x / LPW;
            uint64_t *b = bits + t * (3 * ANW);
            b[w] = wb;
            b[ANW + w] = we;
            b[2 * ANW + w] = wt;
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
        for (int w = 0; w < ACB / 64; ++w) tot += s_c[w];
        tcnt[t] = tot;
    }
}

// ---------------------------------------------------------------- write pass
template <bool SRC>
__global__ __launch_bounds__(AWB) void k_apply_write(crdt_tuples A, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                     crdt_tuples B, uint64_t m, const uint64_t *__restrict__ clock,
                                                     uint32_t rep, const uint64_t *__restrict__ split,
                                                     const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ic,
                                                     crdt_tuples out, int64_t *__restrict__ src,
                                                     uint32_t *__restrict__ err) {
    uint64_t na, ts0;
    if (!apply_len(n_max, n_dev, clock, rep, m, &na, &ts0)) return;
    const uint64_t nb = m, t = blockIdx.x;
    if (t >= PlainTiles::tiles(na, nb)) return;
    const int lane = threadIdx.x & 63;
    const uint64_t *b = bits + t * (3 * ANW);
    const RankWords k = rank_words(b, lane);              // `isb`, `emit` and their prefix counts
    const uint64_t wt = lane < ANW ? b[2 * ANW + lane] : 0ull;
    const uint32_t ne = k.ne;
    const uint64_t i0 = split[t], j0 = t * AT - i0, base = ic[t], cap = n_max + m;
    bool bad = false;
    for (uint32_t r0 = 0; r0 < ne; r0 += AWB) {          // (uniform: the shuffles below read every word's lane)
        const bool valid = r0 + threadIdx.x < ne;
        const uint32_t r = valid ? r0 + threadIdx.x : ne - 1;
        const RankHit h = rank_select(k, r);
        const uint64_t qb = h.qb, qe = h.qe;
        const uint64_t qt = (uint64_t)__shfl((unsigned long long)wt, h.w, 64);
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
        const uint64_t i = is_b ? j0 + bb : i0 + ab;     // the item's index on its side
        const uint64_t at = base + r;
        if (!(i < (is_b ? nb : na) && at < cap)) {
            bad = true;
            continue;
        }
        const uint64_t key = (is_b ? B.key : A.key)[i], ts = (is_b ? B.ts : A.ts)[i];
        const uint32_t rp = (is_b ? B.rep : A.rep)[i];
        int64_t s = 0;
        if (SRC) {
            if (is_b) {
                s = -(int64_t)i - 1;
            } else {                                     // the tag's first copy in the state
                uint64_t f = i;
                while (f > 0 && A.key[f - 1] == key && A.ts[f - 1] == ts && A.rep[f - 1] == rp) --f;
                s = (int64_t)f;
            }
        }
        out.key[at] = key;
        out.ts[at] = ts;
        out.rep[at] = rp;
        out.tomb[at] = (uint8_t)((qt >> pos) & 1);
        if (SRC) src[at] = s;
    }
    if (bad) atomicOr(err, CRDT_DEV_RANGE);
}

// ---------------------------------------------------------------- clock_out / poison
__global__ __launch_bounds__(256) void k_apply_finish(uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                      const uint64_t *__restrict__ clock, uint32_t n_clock, uint32_t rep,
                                                      uint64_t m, uint64_t *__restrict__ clock_out,
                                                      uint64_t *__restrict__ count, uint32_t *__restrict__ err) {
    uint64_t na, ts0;
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (!apply_len(n_max, n_dev, clock, rep, m, &na, &ts0)) {
        if (c == 0) {
            *count = ~0ull;
            atomicOr(err, CRDT_DEV_RANGE);
        }
        return;
    }
    if (clock_out && c < n_clock) clock_out[c] = c == rep ? ts0 + m : clock[c];
}

struct ApplySpan {
    const void *p;
    size_t bytes;
};
static int apply_fields(const crdt_tuples *t, size_t n, ApplySpan *s) {
    s[0] = {t->key, n * 8};
    s[1] = {t->ts, n * 8};
    s[2] = {t->rep, n * 4};
    s[3] = {t->tomb, n};
    return 4;
}

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_set_apply(crdt_ctx *ctx, int form, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                              const uint64_t *clock_dev, size_t n_clock, uint32_t rep, const uint64_t *op_key_dev,
                              const uint8_t *op_kind_dev, size_t m, const crdt_tuples *out, int64_t *src_out_dev,
                              uint64_t *clock_out_dev, uint64_t *count) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!t || !count || !clock_dev) return CRDT_E_INVAL;
    if (form != CRDT_APPLY_TOMBSTONE && form != CRDT_APPLY_CAUSAL) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62) || m >= (1ULL << 62) || n_clock >= (1ULL << 32)) return CRDT_E_RANGE;
    if ((size_t)rep >= n_clock) return CRDT_E_INVAL;
    if (!out && src_out_dev) return CRDT_E_INVAL;
    if (n_max && tuples_null(t)) return CRDT_E_INVAL;
    if (m && (!op_key_dev || !op_kind_dev)) return CRDT_E_INVAL;
    if (tuples_misaligned(t) || (out && tuples_misaligned(out))) return CRDT_E_INVAL;
    if ((((uintptr_t)op_key_dev | (uintptr_t)clock_dev | (uintptr_t)clock_out_dev | (uintptr_t)src_out_dev |
          (uintptr_t)n_dev | (uintptr_t)count) & 7) != 0)
        return CRDT_E_INVAL;
    const size_t cap = n_max + m;
    if (out && cap && tuples_null(out)) return CRDT_E_INVAL;
    const size_t ntiles = (cap + AT - 1) / AT;
    if (ntiles >= 0x7fffffffULL) return CRDT_E_RANGE;
    {
        ApplySpan in[8], o[7];
        int ni = apply_fields(t, n_max, in), no = 0;
        in[ni++] = {clock_dev, n_clock * 8};
        in[ni++] = {n_dev, 8};
        in[ni++] = {op_key_dev, m * 8};
        in[ni++] = {op_kind_dev, m};
        if (out) no = apply_fields(out, cap, o);
        o[no++] = {src_out_dev, cap * 8};
        o[no++] = {clock_out_dev, n_clock * 8};
        o[no++] = {count, 8};
        for (int x = 0; x < no; ++x) {
            for (int y = 0; y < ni; ++y)
                if (spans_overlap(o[x].p, o[x].bytes, in[y].p, in[y].bytes)) return CRDT_E_INVAL;
            for (int y = x + 1; y < no; ++y)
                if (spans_overlap(o[x].p, o[x].bytes, o[y].p, o[y].bytes)) return CRDT_E_INVAL;
        }
    }
    // behind the tiles: R, the tags' ts / rep / bits, the scan's tile sums
    const size_t extra = Carve::round((m + 1) * 8) + Carve::round(m * 8) + Carve::round(m * 4) + Carve::round(m) +
                         scan_lb_tmp_bytes(m) + 1024;
    TileWs w;
    rc = w.reserve(ctx, ntiles, true, false, 3 * ANW, extra);
    if (rc) return rc;
    Carve x((char *)ctx->ws + TileWs::bytes(ntiles, true, false, 3 * ANW));
    uint64_t *const R = x.take<uint64_t>(m + 1);
    crdt_tuples B;
    B.key = const_cast<uint64_t *>(op_key_dev);
    B.ts = x.take<uint64_t>(m);
    B.rep = x.take<uint32_t>(m);
    B.tomb = x.take<uint8_t>(m);
    void *const tmp = x.take<uint64_t>(scan_lb_tmp_bytes(m) / 8);
    const bool wr = out != nullptr, causal = form == CRDT_APPLY_CAUSAL;
    const uint32_t nc = (uint32_t)n_clock;
    const hipStream_t s = ctx->stream;
    if (m) {
        rc = scan_lb(ctx, KindSrc{op_kind_dev}, NoAct{}, m, 0, R, tmp);
        if (rc) return rc;
        k_apply_tags<<<(unsigned)((m + 255) / 256), 256, 0, s>>>(op_key_dev, m, clock_dev, rep, R, B.ts, B.rep, B.tomb);
    }
    if (ntiles) {
        const unsigned g = (unsigned)ntiles;
        k_mp_split<AT, TupleLe<false>, PlainTiles><<<mp_split_grid(ntiles), 256, 0, s>>>(*t, n_max, n_dev, B, m, nullptr,
                                                                                        w.split);
        if (causal && wr)
            k_apply_count<true, true><<<g, ACB, 0, s>>>(*t, n_max, n_dev, B, m, clock_dev, rep, R, w.split, w.tcnt, w.bits);
        else if (causal)
            k_apply_count<false, true><<<g, ACB, 0, s>>>(*t, n_max, n_dev, B, m, clock_dev, rep, R, w.split, w.tcnt, w.bits);
        else if (wr)
            k_apply_count<true, false><<<g, ACB, 0, s>>>(*t, n_max, n_dev, B, m, clock_dev, rep, R, w.split, w.tcnt, w.bits);
        else
            k_apply_count<false, false><<<g, ACB, 0, s>>>(*t, n_max, n_dev, B, m, clock_dev, rep, R, w.split, w.tcnt,
                                                          w.bits);
    }
    w.scan<NoCarry<>>(ctx, n_max, n_dev, m, nullptr, wr, count);
    if (ntiles && wr) {
        if (src_out_dev)
            k_apply_write<true><<<(unsigned)ntiles, AWB, 0, s>>>(*t, n_max, n_dev, B, m, clock_dev, rep, w.split, w.bits,
                                                                 w.ic, *out, src_out_dev, ctx->dev_status);
        else
            k_apply_write<false><<<(unsigned)ntiles, AWB, 0, s>>>(*t, n_max, n_dev, B, m, clock_dev, rep, w.split, w.bits,
                                                                  w.ic, *out, src_out_dev, ctx->dev_status);
    }
    k_apply_finish<<<(unsigned)((n_clock + 255) / 256), 256, 0, s>>>(n_max, n_dev, clock_dev, nc, rep, m, clock_out_dev,
                                                                    count, ctx->dev_status);
    return check_launch(ctx);
}
