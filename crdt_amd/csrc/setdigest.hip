// setdigest.hip -- range digests of a sorted LWW / OR-Set state and the
// selection of the key ranges whose digests differ (crdt_set_digest,
// crdt_set_digest_diff, crdt_set_select).
//
// Semantics, pinned to the merges of sets.hip.  For tuples t[0 .. n) sorted
// ascending by (key, ts, rep), copies of one tag in any order, canon(t) is the
// tuples of merge(t, {}):
//   OR-Set : each distinct tag once, tomb = the OR over its copies.
//   LWW    : per distinct key the maximal (ts, rep) tag with the tomb of that
//            tag's FIRST copy (crdt_lww_merge's winner).
// m ascending uint64 splitters cut the key space into m + 1 buckets, bucket(key)
// = #{ j : splitters[j] <= key } (unsigned; equal neighbours give empty buckets).
// With sm(x) = SplitMix64's output function (x += 0x9E3779B97F4A7C15; x = (x ^
// x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x
// >> 31) the hash of a tuple is
//   h(key, ts, rep, tomb) = sm( sm( sm(key) ^ ts ) ^ ((uint64)rep << 1 | tomb) )
// and the digest of bucket b is hash[b] = the sum mod 2^64 of h over canon(t)'s
// tuples in b, count[b] = their number.  Wrapping adds commute, so the result
// is bit-exact however the adds are ordered.
// select(t, flags) = canon(t) restricted to the buckets with flags[b] != 0, in
// ascending order, optionally with crdt_set_compact's source indices.
//
// GPU structure: setcompact.hip's -- a streaming job over tiles of 2048
// tuples, one workgroup of four waves each, a wave 8 consecutive 64-tuple
// words, every decision a wave64 ballot word.  The deciding position of a
// canonical tuple is the LAST copy of its tag's run (OR-Set) or the last tuple
// of its key's run (LWW: it holds the key's maximal tag).
//   tomb   : OR-Set: the OR over the run's copies inside the mask word is a
//            segmented any() of the ballot words; a run that began before the
//            word and shows no tombstone inside it is walked back through
//            global memory by the one lane at its end, until a tombstone or the
//            run's first copy.  LWW: the lane at a key end whose predecessor
//            carries the same tag walks back to the tag's first copy and takes
//            its tomb (k_cmp_lww_count's walk).  Only a run's END walks, and
//            only over its own copies: the work is linear in n however many
//            tiles one tag spans, and no workgroup waits on another -- no
//            carry, no look-back, no flags.
//   bucket, digest : digest.hpp's, shared with the counter map's digest -- the
//            wave's bucket range from its first and last key, hashes at the
//            deciding positions, one atomicAdd pair per wave (word) and bucket
//            run.
//   select : compaction with another drop predicate (the bucket is unflagged):
//            count (emit / tomb bitmaps and tile counts), then the scan and the
//            write pass of settile.hpp: k_tile_scan<NoCarry> -- the tomb is
//            settled in the count pass, so the scan carries counts alone --
//            and crdt_set_compact's k_tile_write.
//
// The tuple count may stay on the device (n_dev) exactly as in setcompact.hip:
// tiles at or past min(*n_dev, n_max) do nothing; *n_dev > n_max touches no
// tuple and raises CRDT_DEV_RANGE (digest: every entry of both outputs ~0;
// select: a count of ~0).  No kernel reads a tuple at or past that length or
// before 0, a splitter at or past m, or a flag at or past m + 1.
#include "digest.hpp"

namespace crdt {

constexpr int GT = kTile, GB = kTileB, GWW = kTileWW, GNW = kTileNW;   // tile, its threads, words per wave and tile

__device__ __forceinline__ uint64_t dig_hash(uint64_t key, uint64_t ts, uint32_t rep, uint32_t tomb) {
    return splitmix64(splitmix64(splitmix64(key) ^ ts) ^ (((uint64_t)rep << 1) | (uint64_t)(tomb & 1u)));
}

// The canonical tuples of one wave's 8 words from i0 on (i0 < n).  Per lane a
// bit per word: dec the lane's tuple is a deciding position, dead the canonical
// tuple's tomb.  k is loaded at every position (index clamped into [0, n)); ts
// and r are valid at the deciding positions.
template <bool LWW>
__device__ __forceinline__ void dig_decide(const crdt_tuples &T, uint64_t n, uint64_t i0, int lane,
                                           uint64_t (&k)[GWW], uint64_t (&ts)[GWW], uint32_t (&r)[GWW],
                                           uint32_t *dec_out, uint32_t *dead_out) {
    uint32_t dec = 0, dead = 0;
    if (LWW) {
        uint64_t kn[GWW];
        uint8_t tm[GWW];
#pragma unroll
        for (int j = 0; j < GWW; ++j) {
            const uint64_t i = i0 + (uint64_t)j * 64 + lane;
            const uint64_t a = i < n ? i : n - 1, b = i + 1 < n ? i + 1 : n - 1;
            k[j] = T.key[a];
            kn[j] = T.key[b];
            tm[j] = T.tomb[a];
        }
#pragma unroll
        for (int j = 0; j < GWW; ++j) {
            const uint64_t i = i0 + (uint64_t)j * 64 + lane;
            if (i < n && !(i + 1 < n && k[j] == kn[j])) {
                dec |= 1u << j;
                if (tm[j] != 0) dead |= 1u << j;
            }
        }
        // ts / rep at the key ends, with the predecessor's tag; all in flight together
        uint64_t pk[GWW], px[GWW];
        uint32_t py[GWW];
#pragma unroll
        for (int j = 0; j < GWW; ++j) {
            const uint64_t i = i0 + (uint64_t)j * 64 + lane;
            const bool d = (dec >> j) & 1, p = d && i > 0;
            ts[j] = d ? T.ts[i] : 0;
            r[j] = d ? T.rep[i] : 0;
            pk[j] = p ? T.key[i - 1] : 0;
            px[j] = p ? T.ts[i - 1] : 0;
            py[j] = p ? T.rep[i - 1] : 0;
        }
#pragma unroll
        for (int j = 0; j < GWW; ++j) {
            const uint64_t i = i0 + (uint64_t)j * 64 + lane;
            if (((dec >> j) & 1) && i > 0 && pk[j] == k[j] && px[j] == ts[j] && py[j] == r[j]) {
                uint64_t w = i - 1;                          // more copies of the winner tag: the first decides
                while (w > 0 && T.key[w - 1] == k[j] && T.ts[w - 1] == ts[j] && T.rep[w - 1] == r[j]) --w;
                dead = T.tomb[w] != 0 ? (dead | (1u << j)) : (dead & ~(1u << j));
            }
        }
    } else {
        uint64_t kn[GWW], tn[GWW];
        uint32_t rn[GWW];
        uint8_t tm[GWW];
#pragma unroll
        for (int j = 0; j < GWW; ++j) {
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
        if (lane == 0 && i0 > 0) pt0 = T.key[i0 - 1] == k[0] && T.ts[i0 - 1] == ts[0] && T.rep[i0 - 1] == r[0];
        bool pt = __ballot(pt0) != 0;
#pragma unroll
        for (int j = 0; j < GWW; ++j) {
            const uint64_t wb = i0 + (uint64_t)j * 64, i = wb + lane;
            const bool v = i < n;
            const bool st = i + 1 < n && k[j] == kn[j] && ts[j] == tn[j] && r[j] == rn[j];
            const uint64_t V = __ballot(v), ST = __ballot(st), TB = __ballot(v && tm[j] != 0);
            const uint64_t TE = V & ~ST;                     // tag run ends
            // segmented any(): the carry of an add runs from a set bit up to its run's end bit and stops there
            const uint64_t dd = TE & (((V & ~TE) + (TB & ~TE)) | TB);
            const bool mine = (TE >> lane) & 1;
            bool d = (dd >> lane) & 1;
            // the word's first tag end closes a run from before the word that shows no tombstone in it
            if (pt && mine && !d && (TE & ((1ull << lane) - 1)) == 0) {
                uint64_t w = wb;                             // (pt: wb > 0 and tuple wb - 1 carries the tag)
                while (w > 0 && T.key[w - 1] == k[j] && T.ts[w - 1] == ts[j] && T.rep[w - 1] == r[j]) {
                    --w;
                    if (T.tomb[w] != 0) {
                        d = true;
                        break;
                    }
                }
            }
            if (mine) dec |= 1u << j;
            if (mine && d) dead |= 1u << j;
            pt = (ST >> 63) != 0;
        }
    }
    *dec_out = dec;
    *dead_out = dead;
}

// ---------------------------------------------------------------- digest
template <bool LWW>
__global__ __launch_bounds__(GB) void k_dig_digest(crdt_tuples T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                   const uint64_t *__restrict__ sp, uint32_t m,
                                                   uint64_t *__restrict__ hash, uint64_t *__restrict__ count) {
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t tb = (uint64_t)blockIdx.x * GT;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i0 = tb + (uint64_t)wv * (64 * GWW);
    if (i0 >= n) return;                                     // (wave-uniform; no barrier in this kernel)
    uint64_t k[GWW], ts[GWW];
    uint32_t r[GWW], dec, dead;
    dig_decide<LWW>(T, n, i0, lane, k, ts, r, &dec, &dead);
    uint32_t blo, bhi;
    dig_wave_buckets(sp, m, k, &blo, &bhi);
    if (blo == bhi) {                                        // the whole wave in one bucket
        uint64_t h = 0;
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < GWW; ++j) {
            if ((dec >> j) & 1) {
                h += dig_hash(k[j], ts[j], r[j], (dead >> j) & 1);
                ++c;
            }
        }
        dig_add_wave(h, c, lane, blo, hash, count);
        return;
    }
#pragma unroll
    for (int j = 0; j < GWW; ++j) {
        const bool d = (dec >> j) & 1;
        if (__ballot(d) == 0) continue;
        const uint32_t b = dig_ub(sp, blo, bhi, k[j]);
        uint64_t h = d ? dig_hash(k[j], ts[j], r[j], (dead >> j) & 1) : 0ull;
        uint32_t c = d ? 1u : 0u;
        dig_add_runs(h, c, lane, b, hash, count);
    }
}

// ---------------------------------------------------------------- digest diff
// (a kernel, not a memset: the count is zeroed the same way eagerly and in a captured graph)
__global__ void k_dig_zero(uint64_t *__restrict__ p) {
    if (threadIdx.x == 0) *p = 0;
}

__global__ __launch_bounds__(256) void k_dig_diff(const uint64_t *__restrict__ ha, const uint64_t *__restrict__ ca,
                                                  const uint64_t *__restrict__ hb, const uint64_t *__restrict__ cb,
                                                  uint64_t nb, uint8_t *__restrict__ flags,
                                                  uint64_t *__restrict__ n_diff) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool f = false;
    if (i < nb) {
        const uint64_t x = ca[i], y = cb[i];
        f = ha[i] != hb[i] || x != y || x == ~0ull || y == ~0ull;
        flags[i] = f ? 1 : 0;
    }
    const uint64_t B = __ballot(f);
    if ((threadIdx.x & 63) == 0 && B != 0)
        atomicAdd((unsigned long long *)n_diff, (unsigned long long)__popcll(B));
}

// ---------------------------------------------------------------- select: count pass
template <bool LWW, bool BITS>
__global__ __launch_bounds__(GB) void k_sel_count(crdt_tuples T, uint64_t n_max, const uint64_t *__restrict__ n_dev,
                                                  const uint64_t *__restrict__ sp, uint32_t m,
                                                  const uint8_t *__restrict__ flags, uint32_t *__restrict__ tcnt,
                                                  uint64_t *__restrict__ bits) {
    constexpr int BS = LWW ? GNW : 2 * GNW;
    __shared__ uint32_t s_cnt[GB / 64];
    uint64_t n;
    if (!tile_len(n_max, n_dev, &n)) return;
    const uint64_t t = blockIdx.x, tb = t * GT;
    if (tb >= n) return;                                     // (uniform)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i0 = tb + (uint64_t)wv * (64 * GWW);
    uint32_t cnt = 0;
    uint64_t mine_e = 0, mine_t = 0;
    if (i0 < n) {                                            // (wave-uniform)
        uint64_t k[GWW], ts[GWW];
        uint32_t r[GWW], dec, dead;
        dig_decide<LWW>(T, n, i0, lane, k, ts, r, &dec, &dead);
        uint32_t blo, bhi;
        dig_wave_buckets(sp, m, k, &blo, &bhi);
        const bool one = blo == bhi;
        const bool f1 = one && flags[blo] != 0;
#pragma unroll
        for (int j = 0; j < GWW; ++j) {
            const bool d = (dec >> j) & 1;
            bool f = f1;
            if (!one && d) f = flags[dig_ub(sp, blo, bhi, k[j])] != 0;
            const uint64_t e = __ballot(d && f), tt = __ballot(d && f && ((dead >> j) & 1));
            cnt += (uint32_t)__popcll(e);
            if (lane == j) {
                mine_e = e;
                mine_t = tt;
            }
        }
    }
    if (BITS && lane < GWW) {
        uint64_t *b = bits + t * BS + (uint64_t)wv * GWW + lane;
        b[0] = mine_e;
        if (!LWW) b[GNW] = mine_t;
    }
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t cc = 0;
#pragma unroll
        for (int w = 0; w < GB / 64; ++w) cc += s_cnt[w];
        tcnt[t] = cc;
    }
}

// the checks the digest and the selection share: mode, t, n_max, splitters
static int dig_check_in(int mode, const crdt_tuples *t, size_t n_max, const uint64_t *sp, size_t m) {
    if (!t || (mode != CRDT_SET_LWW && mode != CRDT_SET_ORSET)) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62) || m >= kDigMaxSplit) return CRDT_E_RANGE;
    if ((m && !sp) || ((uintptr_t)sp & 7)) return CRDT_E_INVAL;
    if (n_max && tuples_null(t)) return CRDT_E_INVAL;
    if (tuples_misaligned(t)) return CRDT_E_INVAL;
    if ((n_max + GT - 1) / GT >= 0x7fffffffULL) return CRDT_E_RANGE;
    return CRDT_OK;
}

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_set_digest(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                               const uint64_t *splitters_dev, size_t m, uint64_t *hash_out_dev,
                               uint64_t *count_out_dev) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!hash_out_dev || !count_out_dev) return CRDT_E_INVAL;
    rc = dig_check_in(mode, t, n_max, splitters_dev, m);
    if (rc) return rc;
    if ((((uintptr_t)hash_out_dev | (uintptr_t)count_out_dev | (uintptr_t)n_dev) & 7) != 0) return CRDT_E_INVAL;
    const size_t ob = (m + 1) * 8;
    uint64_t *const outs[2] = {hash_out_dev, count_out_dev};
    if (spans_overlap(hash_out_dev, ob, count_out_dev, ob)) return CRDT_E_INVAL;
    for (int a = 0; a < 2; ++a) {
        if (tuples_overlap(t, n_max, outs[a], ob) || spans_overlap(splitters_dev, m * 8, outs[a], ob) ||
            spans_overlap(n_dev, 8, outs[a], ob))
            return CRDT_E_INVAL;
    }
    const hipStream_t s = ctx->stream;
    const size_t ntiles = (n_max + GT - 1) / GT;
    dig_init(ctx, n_max, n_dev, m, hash_out_dev, count_out_dev);
    if (ntiles) {
        const unsigned g = (unsigned)ntiles;
        if (mode == CRDT_SET_LWW)
            k_dig_digest<true><<<g, GB, 0, s>>>(*t, n_max, n_dev, splitters_dev, (uint32_t)m, hash_out_dev, count_out_dev);
        else
            k_dig_digest<false><<<g, GB, 0, s>>>(*t, n_max, n_dev, splitters_dev, (uint32_t)m, hash_out_dev, count_out_dev);
    }
    return check_launch(ctx);
}

extern "C" int crdt_set_digest_diff(crdt_ctx *ctx, const uint64_t *hash_a_dev, const uint64_t *count_a_dev,
                                    const uint64_t *hash_b_dev, const uint64_t *count_b_dev, size_t n_buckets,
                                    uint8_t *flags_out_dev, uint64_t *n_diff_dev) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!n_diff_dev) return CRDT_E_INVAL;
    if (n_buckets > kDigMaxSplit) return CRDT_E_RANGE;
    if (n_buckets && (!hash_a_dev || !count_a_dev || !hash_b_dev || !count_b_dev || !flags_out_dev)) return CRDT_E_INVAL;
    if ((((uintptr_t)hash_a_dev | (uintptr_t)count_a_dev | (uintptr_t)hash_b_dev | (uintptr_t)count_b_dev |
          (uintptr_t)n_diff_dev) & 7) != 0)
        return CRDT_E_INVAL;
    const void *in[4] = {hash_a_dev, count_a_dev, hash_b_dev, count_b_dev};
    for (int a = 0; a < 4; ++a) {
        if (spans_overlap(in[a], n_buckets * 8, flags_out_dev, n_buckets) || spans_overlap(in[a], n_buckets * 8, n_diff_dev, 8))
            return CRDT_E_INVAL;
    }
    if (spans_overlap(flags_out_dev, n_buckets, n_diff_dev, 8)) return CRDT_E_INVAL;
    const hipStream_t s = ctx->stream;
    k_dig_zero<<<1, 64, 0, s>>>(n_diff_dev);
    if (n_buckets)
        k_dig_diff<<<(unsigned)((n_buckets + 255) / 256), 256, 0, s>>>(hash_a_dev, count_a_dev, hash_b_dev, count_b_dev,
                                                                       n_buckets, flags_out_dev, n_diff_dev);
    return check_launch(ctx);
}

extern "C" int crdt_set_select(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                               const uint64_t *splitters_dev, size_t m, const uint8_t *flags_dev,
                               const crdt_tuples *out, int64_t *src_out_dev, uint64_t *count_dev) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!count_dev || !flags_dev) return CRDT_E_INVAL;
    rc = dig_check_in(mode, t, n_max, splitters_dev, m);
    if (rc) return rc;
    if (!out && src_out_dev) return CRDT_E_INVAL;
    if ((out && tuples_misaligned(out)) || (((uintptr_t)src_out_dev | (uintptr_t)count_dev | (uintptr_t)n_dev) & 7) != 0)
        return CRDT_E_INVAL;
    if (out && n_max) {
        if (tuples_null(out)) return CRDT_E_INVAL;
        const void *o[5] = {out->key, out->ts, out->rep, out->tomb, src_out_dev};   // (src_out_dev: null meets nothing)
        const size_t ob[5] = {n_max * 8, n_max * 8, n_max * 4, n_max, n_max * 8};
        for (int a = 0; a < 5; ++a) {
            if (tuples_overlap(t, n_max, o[a], ob[a]) || spans_overlap(splitters_dev, m * 8, o[a], ob[a]) ||
                spans_overlap(flags_dev, m + 1, o[a], ob[a]) || spans_overlap(count_dev, 8, o[a], ob[a]) ||
                (a < 4 && spans_overlap(src_out_dev, n_max * 8, o[a], ob[a])))
                return CRDT_E_INVAL;
        }
    }
    const size_t ntiles = (n_max + GT - 1) / GT;
    TileWs w;
    rc = w.reserve(ctx, ntiles, false, false, 2 * GNW);
    if (rc) return rc;
    const bool lww = mode == CRDT_SET_LWW, wr = out != nullptr;
    const uint32_t mm = (uint32_t)m;
    const hipStream_t s = ctx->stream;
    const unsigned g = (unsigned)ntiles;
    if (ntiles) {
        if (lww && wr) k_sel_count<true, true><<<g, GB, 0, s>>>(*t, n_max, n_dev, splitters_dev, mm, flags_dev, w.tcnt, w.bits);
        else if (lww) k_sel_count<true, false><<<g, GB, 0, s>>>(*t, n_max, n_dev, splitters_dev, mm, flags_dev, w.tcnt, w.bits);
        else if (wr) k_sel_count<false, true><<<g, GB, 0, s>>>(*t, n_max, n_dev, splitters_dev, mm, flags_dev, w.tcnt, w.bits);
        else k_sel_count<false, false><<<g, GB, 0, s>>>(*t, n_max, n_dev, splitters_dev, mm, flags_dev, w.tcnt, w.bits);
    }
    w.scan<NoCarry<>>(ctx, n_max, n_dev, 0, nullptr, wr, count_dev);   // (the count pass settled every bit)
    if (ntiles && wr)
        tile_write(lww, src_out_dev != nullptr, g, s, *t, n_max, n_dev, w.bits, w.ic, *out, src_out_dev, ctx->dev_status);
    return check_launch(ctx);
}
