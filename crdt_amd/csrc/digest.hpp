// digest.hpp -- what the range digests of the keyed state types share
// (setdigest.hip: crdt_set_digest / crdt_set_select over tuples, DESIGN.md
// §5.16; countermap.hpp: crdt_cmap_digest / crdt_cmap_select over counter-map
// cells): the buckets and the accumulation of a digest.  Device
// code only; what is hashed and which positions count is each state type's own.
//
// m ascending uint64 splitters cut the key space into m + 1 buckets, bucket(key)
// = #{ j : splitters[j] <= key } (unsigned; equal neighbours give empty buckets).
// hash[b] is the sum mod 2^64 of the hashes in bucket b, count[b] their number:
// wrapping adds commute, so the result is bit-exact however the adds are ordered.
//   bucket : the wave searches the splitters for its first and last key
//            (uniform loads); when both fall into one bucket, the common case,
//            no lane searches.  Otherwise each lane searches between the two.
//            Every search is an upper bound inside [0, m], whatever the
//            splitters hold: unsorted splitters give unspecified digests, never
//            an access out of range.
//   digest : a reduction within the wave over runs of equal bucket (one run per
//            wave in the common case, else a segmented shuffle scan per word),
//            one 64-bit global atomicAdd pair per wave (word) and bucket run.
#pragma once
#include "settile.hpp"

namespace crdt {

constexpr size_t kDigMaxSplit = (size_t)1 << 24;

// lo + #{ j in [lo, hi) : sp[j] <= key } for ascending sp; always a value in
// [lo, max(lo, hi)], and only sp[lo .. hi) is read
__device__ __forceinline__ uint32_t dig_ub(const uint64_t *__restrict__ sp, uint32_t lo, uint32_t hi, uint64_t key) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sp[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The bucket range of the wave's keys: [*blo, *bhi] from its first and its
// last (clamped) key, both wave-uniform.
__device__ __forceinline__ void dig_wave_buckets(const uint64_t *__restrict__ sp, uint32_t m,
                                                 const uint64_t (&k)[kTileWW], uint32_t *blo, uint32_t *bhi) {
    const uint64_t kf = (uint64_t)__shfl((unsigned long long)k[0], 0, 64);
    const uint64_t kl = (uint64_t)__shfl((unsigned long long)k[kTileWW - 1], 63, 64);
    *blo = __builtin_amdgcn_readfirstlane(dig_ub(sp, 0, m, kf));
    *bhi = __builtin_amdgcn_readfirstlane(dig_ub(sp, 0, m, kl));
}

// hash / count [0 .. m1) zeroed, or poisoned when the device count is out of range
// (a template: the header goes into more than one translation unit)
template <int TB>
__global__ __launch_bounds__(TB) void k_dig_init(uint64_t n_max, const uint64_t *__restrict__ n_dev, uint64_t m1,
                                                 uint64_t *__restrict__ hash, uint64_t *__restrict__ count,
                                                 uint32_t *__restrict__ err) {
    uint64_t n;
    const bool ok = tile_len(n_max, n_dev, &n);
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i < m1) {
        hash[i] = ok ? 0ull : ~0ull;
        count[i] = ok ? 0ull : ~0ull;
    }
    if (!ok && i == 0) atomicOr(err, CRDT_DEV_RANGE);
}
inline void dig_init(crdt_ctx *ctx, uint64_t n_max, const uint64_t *n_dev, size_t m, uint64_t *hash, uint64_t *count) {
    k_dig_init<256><<<(unsigned)((m + 1 + 255) / 256), 256, 0, ctx->stream>>>(n_max, n_dev, m + 1, hash, count,
                                                                             ctx->dev_status);
}

// the whole wave in bucket b: every lane's sum (h, c) of its own positions, one atomic pair from lane 0
__device__ __forceinline__ void dig_add_wave(uint64_t h, uint32_t c, int lane, uint32_t b,
                                             uint64_t *__restrict__ hash, uint64_t *__restrict__ count) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        h += (uint64_t)__shfl_down((unsigned long long)h, o, 64);
        c += __shfl_down(c, o, 64);
    }
    if (lane == 0 && c != 0) {
        atomicAdd((unsigned long long *)hash + b, (unsigned long long)h);
        atomicAdd((unsigned long long *)count + b, (unsigned long long)c);
    }
}

// one word, the lane's position in bucket b with (h, c) = (its hash, 1) or (0, 0):
// runs of equal bucket by a segmented inclusive scan, the run's last lane adds.
// Every lane of the wave must call it (shuffles).
__device__ __forceinline__ void dig_add_runs(uint64_t h, uint32_t c, int lane, uint32_t b,
                                             uint64_t *__restrict__ hash, uint64_t *__restrict__ count) {
    const uint32_t bp = __shfl_up(b, 1, 64);
    const uint64_t HD = __ballot(lane == 0 || b != bp);
    const int seg = 63 - __builtin_clzll(HD & ((2ull << lane) - 1));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t yh = (uint64_t)__shfl_up((unsigned long long)h, o, 64);
        const uint32_t yc = __shfl_up(c, o, 64);
        if (lane - o >= seg) {
            h += yh;
            c += yc;
        }
    }
    const bool tail = lane == 63 || ((HD >> (lane + 1)) & 1);
    if (tail && c != 0) {
        atomicAdd((unsigned long long *)hash + b, (unsigned long long)h);
        atomicAdd((unsigned long long *)count + b, (unsigned long long)c);
    }
}

}  // namespace crdt
