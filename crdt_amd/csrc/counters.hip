// counters.hip -- dense and keyed counters: the G-Counter / PN-Counter /
// vector-clock join kernels and the entry points of the keyed
// PN-Counter map (crdt_cmap_*; kernels in countermap.hpp, DESIGN.md §5.23, its
// range digests §5.24).
//
// No reference code exists for these types: they are the
// standard state-based CRDT joins (elementwise unsigned max) over a replica
// population stored row-major [rows x nodes] uint64 in HBM.  Everything dense
// here is HBM-bound integer streaming: 16-byte (dwordx4) loads per lane,
// several independent loads in flight per lane, no LDS, no MFMA.
#include "countermap.hpp"

namespace crdt {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

template <bool NT> __device__ __forceinline__ u64x2 ld(const u64x2 *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT> __device__ __forceinline__ void st(u64x2 *p, u64x2 v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}
__device__ __forceinline__ u64x2 vmax(u64x2 x, u64x2 y) {
    return __builtin_elementwise_max(x, y);  // unsigned 64-bit max per lane
}

// out = max(a, b) elementwise over n2 16-byte vectors.  Grid-stride: at each
// step the whole grid touches one contiguous window of U * grid * 4 KiB.
template <int U, bool NT>
__global__ __launch_bounds__(256) void k_join(const u64x2 *__restrict__ a,
                                              const u64x2 *__restrict__ b,
                                              u64x2 *__restrict__ o, size_t n2) {
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + (size_t)(U - 1) * stride < n2; i += (size_t)U * stride) {
        u64x2 x[U], y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = ld<NT>(a + i + (size_t)u * stride);
#pragma unroll
        for (int u = 0; u < U; ++u) y[u] = ld<NT>(b + i + (size_t)u * stride);
#pragma unroll
        for (int u = 0; u < U; ++u) st<NT>(o + i + (size_t)u * stride, vmax(x[u], y[u]));
    }
    for (; i < n2; i += stride) st<NT>(o + i, vmax(ld<NT>(a + i), ld<NT>(b + i)));
}

// Scalar tail (odd element count).
__global__ void k_join_tail(const uint64_t *a, const uint64_t *b, uint64_t *o, size_t idx) {
    uint64_t x = a[idx], y = b[idx];
    o[idx] = x > y ? x : y;
}

// ---------------------------------------------------------------- fold
// Column max over rows.  Fast path: nodes a power of two in [2, 512], so a
// 256-lane block covers 512 uint64 = 512/nodes whole rows per load and every
// lane keeps the same column pair for the whole grid-stride loop.
template <int U, bool NT>
__global__ __launch_bounds__(256) void k_fold_pow2(const u64x2 *__restrict__ a, size_t n2,
                                                   int nodes, uint64_t *__restrict__ partial) {
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    u64x2 m = {0, 0};
    for (; i + (size_t)(U - 1) * stride < n2; i += (size_t)U * stride) {
        u64x2 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = ld<NT>(a + i + (size_t)u * stride);
#pragma unroll
        for (int u = 0; u < U; ++u) m = vmax(m, x[u]);
    }
    for (; i < n2; i += stride) m = vmax(m, ld<NT>(a + i));
    __shared__ u64x2 red[256];
    red[threadIdx.x] = m;
    __syncthreads();
    const int lanes_per_row = nodes >> 1;          // vectors per row
    if ((int)threadIdx.x < lanes_per_row) {
        u64x2 r = red[threadIdx.x];
        for (int t = threadIdx.x + lanes_per_row; t < 256; t += lanes_per_row) r = vmax(r, red[t]);
        partial[(size_t)blockIdx.x * nodes + 2 * threadIdx.x] = r.x;
        partial[(size_t)blockIdx.x * nodes + 2 * threadIdx.x + 1] = r.y;
    }
}

// Generic nodes: lanes stride over columns, blocks over rows.
__global__ __launch_bounds__(256) void k_fold_generic(const uint64_t *__restrict__ a, size_t rows,
                                                      size_t nodes, uint64_t *__restrict__ partial) {
    for (size_t c = threadIdx.x; c < nodes; c += 256) {
        uint64_t m = 0;
        for (size_t r = blockIdx.x; r < rows; r += gridDim.x) {
            uint64_t v = a[r * nodes + c];
            m = v > m ? v : m;
        }
        partial[(size_t)blockIdx.x * nodes + c] = m;
    }
}

// partial [g x nodes] -> out[nodes] via unsigned 64-bit atomicMax (out pre-zeroed).
__global__ __launch_bounds__(256) void k_fold_finish(const uint64_t *__restrict__ partial, size_t g,
                                                     size_t nodes, uint64_t *__restrict__ out) {
    for (size_t c = threadIdx.x; c < nodes; c += 256) {
        uint64_t m = 0;
        for (size_t r = blockIdx.x; r < g; r += gridDim.x) {
            uint64_t v = partial[r * nodes + c];
            m = v > m ? v : m;
        }
        if (m) atomicMax((unsigned long long *)&out[c], (unsigned long long)m);
    }
}

// ---------------------------------------------------------------- row sums
// out[r] = sum_n a[r][n] (- sum_n n[r][n] for PN), uint64 wrap.  NODES/2 lanes
// per row (16 B each), 64/(NODES/2) rows per wave-load, butterfly reduction
// inside the row's lane group.
template <int NODES, bool PN>
__global__ __launch_bounds__(256) void k_rowsum(const u64x2 *__restrict__ p,
                                                const u64x2 *__restrict__ n, uint64_t *__restrict__ out,
                                                size_t rows) {
    constexpr int LPR = NODES / 2;               // lanes per row
    constexpr int RPW = kWave / LPR;             // rows per wave per step
    const int lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const size_t nwaves = ((size_t)gridDim.x * 256) >> 6;
    const int sub = lane / LPR, col = lane % LPR;
    for (size_t r0 = wave * RPW; r0 < rows; r0 += nwaves * RPW) {
        const size_t r = r0 + sub;
        uint64_t s = 0;
        if (r < rows) {
            u64x2 v = ld<true>(p + r * LPR + col);
            s = v.x + v.y;
            if constexpr (PN) {
                u64x2 w = ld<true>(n + r * LPR + col);
                s -= w.x + w.y;
            }
        }
#pragma unroll
        for (int m = LPR / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m, LPR);
        if (col == 0 && r < rows) out[r] = s;
    }
}

// Generic nodes: one wave per row, lanes stride over columns.
template <bool PN>
__global__ __launch_bounds__(256) void k_rowsum_generic(const uint64_t *__restrict__ p,
                                                        const uint64_t *__restrict__ n,
                                                        uint64_t *__restrict__ out, size_t rows,
                                                        size_t nodes) {
    const int lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const size_t nwaves = ((size_t)gridDim.x * 256) >> 6;
    for (size_t r = wave; r < rows; r += nwaves) {
        uint64_t s = 0;
        for (size_t c = lane; c < nodes; c += 64) {
            s += p[r * nodes + c];
            if constexpr (PN) s -= n[r * nodes + c];
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        if (lane == 0) out[r] = s;
    }
}

// ---------------------------------------------------------------- order maps
__global__ void k_u64_to_i64(const uint64_t *in, int64_t *out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = (int64_t)(in[i] ^ 0x8000000000000000ULL);
}
__global__ void k_i64_to_u64(const int64_t *in, uint64_t *out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = (uint64_t)in[i] ^ 0x8000000000000000ULL;
}

// ---------------------------------------------------------------- launchers
template <int U, bool NT>
static void launch_join(unsigned grid, hipStream_t s, const u64x2 *a, const u64x2 *b, u64x2 *o,
                        size_t n2) {
    k_join<U, NT><<<grid, 256, 0, s>>>(a, b, o, n2);
}

static int join_impl(crdt_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *o, size_t n) {
    const size_t n2 = n / 2;
    const unsigned grid = grid_for(n2, 256, (unsigned)(ctx->num_cus * g_join_blocks_per_cu));
    const hipStream_t s = ctx->stream;
    if (n2) {
        const u64x2 *va = (const u64x2 *)a, *vb = (const u64x2 *)b;
        u64x2 *vo = (u64x2 *)o;
        const bool nt = g_join_nontemporal != 0;
        switch (g_join_unroll) {
            case 1: nt ? launch_join<1, true>(grid, s, va, vb, vo, n2) : launch_join<1, false>(grid, s, va, vb, vo, n2); break;
            case 2: nt ? launch_join<2, true>(grid, s, va, vb, vo, n2) : launch_join<2, false>(grid, s, va, vb, vo, n2); break;
            case 8: nt ? launch_join<8, true>(grid, s, va, vb, vo, n2) : launch_join<8, false>(grid, s, va, vb, vo, n2); break;
            default: nt ? launch_join<4, true>(grid, s, va, vb, vo, n2) : launch_join<4, false>(grid, s, va, vb, vo, n2); break;
        }
    }
    if (n & 1) k_join_tail<<<1, 1, 0, s>>>(a, b, o, n - 1);
    return check_launch(ctx);
}

// ---------------------------------------------------------------- streaming peaks
// the bench reports each kernel's fraction of a SELF-MEASURED
// copy-kernel peak beside the 8 TB/s spec.  A plain copy (16-B loads and
// stores, U vectors in flight per lane) and a read-only sweep (xor-reduced
// over the workgroup, one store per workgroup) of the same form as the join / fold loops.
template <int U>
__global__ __launch_bounds__(256) void k_stream_copy(const u64x2 *__restrict__ a, u64x2 *__restrict__ o, size_t n2) {
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + (size_t)(U - 1) * stride < n2; i += (size_t)U * stride) {
        u64x2 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = ld<true>(a + i + (size_t)u * stride);
#pragma unroll
        for (int u = 0; u < U; ++u) st<true>(o + i + (size_t)u * stride, x[u]);
    }
    for (; i < n2; i += stride) st<true>(o + i, ld<true>(a + i));
}

template <int U>
__global__ __launch_bounds__(256) void k_stream_read(const u64x2 *__restrict__ a, size_t n2,
                                                     uint64_t *__restrict__ sink) {
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    u64x2 m = {0, 0};
    for (; i + (size_t)(U - 1) * stride < n2; i += (size_t)U * stride) {
        u64x2 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = ld<true>(a + i + (size_t)u * stride);
#pragma unroll
        for (int u = 0; u < U; ++u) m ^= x[u];
    }
    for (; i < n2; i += stride) m ^= ld<true>(a + i);
    // xor over the workgroup (every lane's loads feed the stored word)
    uint64_t v = m.x ^ m.y;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o);
    __shared__ uint64_t red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) sink[blockIdx.x] = red[0] ^ red[1] ^ red[2] ^ red[3];
}

}  // namespace crdt

using namespace crdt;

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int crdt_stream_copy(crdt_ctx *ctx, const void *src, void *dst, size_t bytes, int unroll,
                                int blocks_per_cu) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!src || !dst || !aligned16(src) || !aligned16(dst) || (bytes & 15)) return CRDT_E_INVAL;
    if (blocks_per_cu < 1 || blocks_per_cu > 64) return CRDT_E_INVAL;
    const size_t n2 = bytes / 16;
    if (n2 == 0) return CRDT_OK;
    const unsigned grid = grid_for(n2, 256, (unsigned)(ctx->num_cus * blocks_per_cu));
    const u64x2 *a = (const u64x2 *)src;
    u64x2 *o = (u64x2 *)dst;
    const hipStream_t s = ctx->stream;
    switch (unroll) {
        case 1: k_stream_copy<1><<<grid, 256, 0, s>>>(a, o, n2); break;
        case 2: k_stream_copy<2><<<grid, 256, 0, s>>>(a, o, n2); break;
        case 4: k_stream_copy<4><<<grid, 256, 0, s>>>(a, o, n2); break;
        case 8: k_stream_copy<8><<<grid, 256, 0, s>>>(a, o, n2); break;
        default: return CRDT_E_INVAL;
    }
    return check_launch(ctx);
}

extern "C" int crdt_stream_read(crdt_ctx *ctx, const void *src, size_t bytes, uint64_t *sink_dev, size_t sink_words,
                                int unroll, int blocks_per_cu) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!src || !sink_dev || !aligned16(src) || (bytes & 15)) return CRDT_E_INVAL;
    if (blocks_per_cu < 1 || blocks_per_cu > 64) return CRDT_E_INVAL;
    const size_t n2 = bytes / 16;
    if (n2 == 0) return CRDT_OK;
    const unsigned grid = grid_for(n2, 256, (unsigned)(ctx->num_cus * blocks_per_cu));
    if (sink_words < grid) return CRDT_E_INVAL;         // one word per workgroup
    const u64x2 *a = (const u64x2 *)src;
    const hipStream_t s = ctx->stream;
    switch (unroll) {
        case 1: k_stream_read<1><<<grid, 256, 0, s>>>(a, n2, sink_dev); break;
        case 2: k_stream_read<2><<<grid, 256, 0, s>>>(a, n2, sink_dev); break;
        case 4: k_stream_read<4><<<grid, 256, 0, s>>>(a, n2, sink_dev); break;
        case 8: k_stream_read<8><<<grid, 256, 0, s>>>(a, n2, sink_dev); break;
        default: return CRDT_E_INVAL;
    }
    return check_launch(ctx);
}

extern "C" int crdt_gcounter_join(crdt_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out,
                                  size_t rows, size_t nodes) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (mul_overflows(rows, nodes)) return CRDT_E_INVAL;
    const size_t n = rows * nodes;
    if (n == 0) return CRDT_OK;
    if (!a || !b || !out || !aligned16(a) || !aligned16(b) || !aligned16(out)) return CRDT_E_INVAL;
    return join_impl(ctx, a, b, out, n);
}

extern "C" int crdt_pncounter_join(crdt_ctx *ctx, const uint64_t *pa, const uint64_t *na,
                                   const uint64_t *pb, const uint64_t *nb, uint64_t *po,
                                   uint64_t *no, size_t rows, size_t nodes) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (mul_overflows(rows, nodes)) return CRDT_E_INVAL;
    const size_t n = rows * nodes;
    if (n == 0) return CRDT_OK;
    const void *ps[6] = {pa, na, pb, nb, po, no};
    for (const void *p : ps)
        if (!p || !aligned16(p)) return CRDT_E_INVAL;
    // the P and N halves as two passes of the tuned G-Counter join: a fused
    // single pass keeps four 16-B loads per lane in flight, past the ~16 KiB
    // per CU the HBM system prefers (measured 65% vs 80% of peak)
    rc = join_impl(ctx, pa, pb, po, n);
    if (rc) return rc;
    return join_impl(ctx, na, nb, no, n);
}

extern "C" int crdt_gcounter_fold(crdt_ctx *ctx, const uint64_t *a, size_t rows, size_t nodes,
                                  uint64_t *out) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out || nodes == 0 || mul_overflows(rows, nodes)) return CRDT_E_INVAL;
    hipError_t e = hipMemsetAsync(out, 0, nodes * sizeof(uint64_t), ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e);
    if (rows == 0) return CRDT_OK;
    if (!a) return CRDT_E_INVAL;
    const bool pow2 = nodes >= 2 && nodes <= 512 && (nodes & (nodes - 1)) == 0 && aligned16(a);
    unsigned grid;
    const unsigned bpc = (unsigned)g_fold_blocks_per_cu;
    if (pow2) grid = grid_for(rows * nodes / 2, 256 * (unsigned)g_fold_unroll, (unsigned)ctx->num_cus * bpc);
    else grid = grid_for(rows, 1, (unsigned)(ctx->num_cus * 4));
    const size_t part_bytes = (size_t)grid * nodes * sizeof(uint64_t);
    rc = ws_reserve(ctx, part_bytes);
    if (rc) return rc;
    uint64_t *partial = (uint64_t *)ctx->ws;
    if (pow2) {
        const u64x2 *va = (const u64x2 *)a;
        const size_t n2 = rows * nodes / 2;
        const hipStream_t s = ctx->stream;
        const bool nt = g_fold_nontemporal != 0;
#define FOLD(U) (nt ? k_fold_pow2<U, true><<<grid, 256, 0, s>>>(va, n2, (int)nodes, partial) \
                    : k_fold_pow2<U, false><<<grid, 256, 0, s>>>(va, n2, (int)nodes, partial))
        switch (g_fold_unroll) {
            case 1: FOLD(1); break;
            case 2: FOLD(2); break;
            case 8: FOLD(8); break;
            case 16: FOLD(16); break;
            default: FOLD(4); break;
        }
#undef FOLD
    } else {
        k_fold_generic<<<grid, 256, 0, ctx->stream>>>(a, rows, nodes, partial);
    }
    rc = check_launch(ctx);
    if (rc) return rc;
    const unsigned g2 = grid < 32 ? grid : 32;
    k_fold_finish<<<g2, 256, 0, ctx->stream>>>(partial, grid, nodes, out);
    return check_launch(ctx);
}

template <bool PN>
static int rowsum(crdt_ctx *ctx, const uint64_t *p, const uint64_t *n, uint64_t *out, size_t rows,
                  size_t nodes) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (mul_overflows(rows, nodes)) return CRDT_E_INVAL;
    if (rows == 0) return CRDT_OK;
    if (!p || !out || (PN && !n)) return CRDT_E_INVAL;
    const bool vec = aligned16(p) && (!PN || aligned16(n));
    const unsigned grid = grid_for(rows * 64, 256, (unsigned)(ctx->num_cus * 8));
    const hipStream_t s = ctx->stream;
    const u64x2 *vp = (const u64x2 *)p, *vn = (const u64x2 *)n;
    if (vec && nodes == 64) k_rowsum<64, PN><<<grid, 256, 0, s>>>(vp, vn, out, rows);
    else if (vec && nodes == 128) k_rowsum<128, PN><<<grid, 256, 0, s>>>(vp, vn, out, rows);
    else if (vec && nodes == 32) k_rowsum<32, PN><<<grid, 256, 0, s>>>(vp, vn, out, rows);
    else if (vec && nodes == 16) k_rowsum<16, PN><<<grid, 256, 0, s>>>(vp, vn, out, rows);
    else k_rowsum_generic<PN><<<grid, 256, 0, s>>>(p, n, out, rows, nodes);
    return check_launch(ctx);
}

extern "C" int crdt_gcounter_value(crdt_ctx *ctx, const uint64_t *a, size_t rows, size_t nodes,
                                   uint64_t *out) {
    return rowsum<false>(ctx, a, nullptr, out, rows, nodes);
}

extern "C" int crdt_pncounter_value(crdt_ctx *ctx, const uint64_t *p, const uint64_t *n, int64_t *out,
                                    size_t rows, size_t nodes) {
    return rowsum<true>(ctx, p, n, (uint64_t *)out, rows, nodes);
}

extern "C" int crdt_u64_to_ordered_i64(crdt_ctx *ctx, const uint64_t *in, int64_t *out, size_t n) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (n == 0) return CRDT_OK;
    if (!in || !out) return CRDT_E_INVAL;
    k_u64_to_i64<<<grid_for(n, 256, 4096), 256, 0, ctx->stream>>>(in, out, n);
    return check_launch(ctx);
}

extern "C" int crdt_ordered_i64_to_u64(crdt_ctx *ctx, const int64_t *in, uint64_t *out, size_t n) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (n == 0) return CRDT_OK;
    if (!in || !out) return CRDT_E_INVAL;
    k_i64_to_u64<<<grid_for(n, 256, 4096), 256, 0, ctx->stream>>>(in, out, n);
    return check_launch(ctx);
}

// ---------------------------------------------------------------- keyed PN-Counter map
// Entry points of crdt_cmap_* (include/crdt_amd.h; kernels and pass structure:
// countermap.hpp).  Every length may stay on the device; every call is
// stream-ordered with no host synchronisation.
static bool cmap_null(const crdt_cmap *t) { return !t->key || !t->rep || !t->p || !t->n; }
static bool cmap_misaligned(const crdt_cmap *t) {
    return ((((uintptr_t)t->key | (uintptr_t)t->p | (uintptr_t)t->n) & 7) | ((uintptr_t)t->rep & 3)) != 0;
}
struct CmSpan {
    const void *p;
    size_t bytes;
};
static int cmap_fields(const crdt_cmap *t, size_t n, CmSpan *s) {
    s[0] = {t->key, n * 8};
    s[1] = {t->rep, n * 4};
    s[2] = {t->p, n * 8};
    s[3] = {t->n, n * 8};
    return 4;
}
// an output meets an input or another output
static bool cmap_clash(const CmSpan *o, int no, const CmSpan *in, int ni) {
    for (int x = 0; x < no; ++x) {
        for (int y = 0; y < ni; ++y)
            if (spans_overlap(o[x].p, o[x].bytes, in[y].p, in[y].bytes)) return true;
        for (int y = x + 1; y < no; ++y)
            if (spans_overlap(o[x].p, o[x].bytes, o[y].p, o[y].bytes)) return true;
    }
    return false;
}
// the split's view of a side: key and rep (the other two fields are never dereferenced)
static crdt_tuples cmap_view(const crdt_cmap &c) {
    crdt_tuples v;
    v.key = c.key;
    v.ts = nullptr;
    v.rep = c.rep;
    v.tomb = nullptr;
    return v;
}

// split -> count -> scan -> write of one two-sided call over the carved tiles.
// DELTA: side a = dst, b = src, out holds src cells; else out = the union, a
// cell of both sides combined by Comb.
template <bool DELTA, class Comb>
static int cmap_two_sided(crdt_ctx *ctx, const TileWs &w, size_t ntiles, const crdt_cmap &A, size_t na_max,
                          const uint64_t *na_dev, const crdt_cmap &B, size_t nb_max, const uint64_t *nb_dev,
                          const crdt_cmap *out, uint64_t *count) {
    using Tiles = typename std::conditional<DELTA, CmDeltaTiles, PlainTiles>::type;
    const bool wr = out != nullptr;
    const hipStream_t s = ctx->stream;
    if (ntiles) {
        const unsigned g = (unsigned)ntiles;
        k_mp_split<CT, CellLe, Tiles><<<mp_split_grid(ntiles), 256, 0, s>>>(cmap_view(A), na_max, na_dev, cmap_view(B),
                                                                           nb_max, nb_dev, w.split);
        if (wr)
            k_cmap_count<DELTA, true, Tiles><<<g, CCB, 0, s>>>(A, na_max, na_dev, B, nb_max, nb_dev, w.split, w.tcnt, w.bits);
        else
            k_cmap_count<DELTA, false, Tiles><<<g, CCB, 0, s>>>(A, na_max, na_dev, B, nb_max, nb_dev, w.split, w.tcnt, w.bits);
    }
    w.scan<NoCarry<Tiles>>(ctx, na_max, na_dev, nb_max, nb_dev, wr, count);
    if (ntiles && wr) {
        const unsigned g = (unsigned)ntiles;
        if (DELTA)
            k_cmap_delta_write<<<g, CWB, 0, s>>>(B, nb_max, nb_dev, na_max, na_dev, w.split, w.bits, w.ic, *out,
                                                 ctx->dev_status);
        else
            k_cmap_write<Comb><<<g, CWB, 0, s>>>(A, na_max, na_dev, B, nb_max, nb_dev, w.split, w.bits, w.ic, *out,
                                                 ctx->dev_status);
    }
    return check_launch(ctx);
}

// the union of two states, a cell of both sides combined by Comb: the checks, the workspace, the passes
template <class Comb>
static int cmap_union(crdt_ctx *ctx, const crdt_cmap *a, size_t na_max, const uint64_t *na_dev, const crdt_cmap *b,
                      size_t nb_max, const uint64_t *nb_dev, const crdt_cmap *out, uint64_t *count_dev) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!a || !b || !count_dev) return CRDT_E_INVAL;
    if (na_max >= (1ULL << 62) || nb_max >= (1ULL << 62)) return CRDT_E_RANGE;
    if ((na_max && cmap_null(a)) || (nb_max && cmap_null(b))) return CRDT_E_INVAL;
    if (cmap_misaligned(a) || cmap_misaligned(b) || (out && cmap_misaligned(out))) return CRDT_E_INVAL;
    if ((((uintptr_t)na_dev | (uintptr_t)nb_dev | (uintptr_t)count_dev) & 7) != 0) return CRDT_E_INVAL;
    const size_t cap = na_max + nb_max;
    const size_t ntiles = (cap + CT - 1) / CT;
    if (ntiles >= 0x7fffffffULL) return CRDT_E_RANGE;   // (so no byte count below wraps)
    if (out && cap && cmap_null(out)) return CRDT_E_INVAL;
    {
        CmSpan in[10], o[5];
        int ni = cmap_fields(a, na_max, in), no = 0;
        ni += cmap_fields(b, nb_max, in + ni);
        in[ni++] = {na_dev, 8};
        in[ni++] = {nb_dev, 8};
        if (out) no = cmap_fields(out, cap, o);
        o[no++] = {count_dev, 8};
        if (cmap_clash(o, no, in, ni)) return CRDT_E_INVAL;
    }
    TileWs w;
    rc = w.reserve(ctx, ntiles, true, false, CBS);
    if (rc) return rc;
    return cmap_two_sided<false, Comb>(ctx, w, ntiles, *a, na_max, na_dev, *b, nb_max, nb_dev, out, count_dev);
}

extern "C" int crdt_cmap_merge(crdt_ctx *ctx, const crdt_cmap *a, size_t na_max, const uint64_t *na_dev,
                               const crdt_cmap *b, size_t nb_max, const uint64_t *nb_dev, const crdt_cmap *out,
                               uint64_t *count_dev) {
    return cmap_union<CmMax>(ctx, a, na_max, na_dev, b, nb_max, nb_dev, out, count_dev);
}

extern "C" int crdt_cmap_add(crdt_ctx *ctx, const crdt_cmap *t, size_t nt_max, const uint64_t *nt_dev,
                             const crdt_cmap *d, size_t nd_max, const uint64_t *nd_dev, const crdt_cmap *out,
                             uint64_t *count_dev) {
    return cmap_union<CmAdd>(ctx, t, nt_max, nt_dev, d, nd_max, nd_dev, out, count_dev);
}

extern "C" int crdt_cmap_apply(crdt_ctx *ctx, const crdt_cmap *t, size_t n_max, const uint64_t *n_dev, uint32_t rep,
                               const uint64_t *op_key_dev, const uint64_t *op_dp_dev, const uint64_t *op_dn_dev,
                               size_t m, const crdt_cmap *out, uint64_t *count_dev) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!t || !count_dev) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62) || m >= (1ULL << 62)) return CRDT_E_RANGE;
    if (n_max && cmap_null(t)) return CRDT_E_INVAL;
    if (m && (!op_key_dev || !op_dp_dev || !op_dn_dev)) return CRDT_E_INVAL;
    if (cmap_misaligned(t) || (out && cmap_misaligned(out))) return CRDT_E_INVAL;
    if ((((uintptr_t)op_key_dev | (uintptr_t)op_dp_dev | (uintptr_t)op_dn_dev | (uintptr_t)n_dev |
          (uintptr_t)count_dev) & 7) != 0)
        return CRDT_E_INVAL;
    const size_t cap = n_max + m;
    const size_t ntiles = (cap + CT - 1) / CT;
    if (ntiles >= 0x7fffffffULL) return CRDT_E_RANGE;   // (so no byte count below wraps)
    if (out && cap && cmap_null(out)) return CRDT_E_INVAL;
    {
        CmSpan in[8], o[5];
        int ni = cmap_fields(t, n_max, in), no = 0;
        in[ni++] = {n_dev, 8};
        in[ni++] = {op_key_dev, m * 8};
        in[ni++] = {op_dp_dev, m * 8};
        in[ni++] = {op_dn_dev, m * 8};
        if (out) no = cmap_fields(out, cap, o);
        o[no++] = {count_dev, 8};
        if (cmap_clash(o, no, in, ni)) return CRDT_E_INVAL;
    }
    // behind the tiles: the batch's rep column, so that the batch is an ordinary side
    TileWs w;
    rc = w.reserve(ctx, ntiles, true, false, CBS, Carve::round(m * 4) + 256);
    if (rc) return rc;
    Carve x((char *)ctx->ws + TileWs::bytes(ntiles, true, false, CBS));
    crdt_cmap B;
    B.key = const_cast<uint64_t *>(op_key_dev);
    B.rep = x.take<uint32_t>(m);
    B.p = const_cast<uint64_t *>(op_dp_dev);
    B.n = const_cast<uint64_t *>(op_dn_dev);
    if (m) {
        const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)B.rep, (int)rep, m, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e);
    }
    return cmap_two_sided<false, CmAdd>(ctx, w, ntiles, *t, n_max, n_dev, B, m, nullptr, out, count_dev);
}

extern "C" int crdt_cmap_delta(crdt_ctx *ctx, const crdt_cmap *src, size_t ns_max, const uint64_t *ns_dev,
                               const crdt_cmap *dst, size_t nd_max, const uint64_t *nd_dev, const crdt_cmap *out,
                               uint64_t *count_dev) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!src || !dst || !count_dev) return CRDT_E_INVAL;
    if (ns_max >= (1ULL << 62) || nd_max >= (1ULL << 62)) return CRDT_E_RANGE;
    if ((ns_max && cmap_null(src)) || (nd_max && cmap_null(dst))) return CRDT_E_INVAL;
    if (cmap_misaligned(src) || cmap_misaligned(dst) || (out && cmap_misaligned(out))) return CRDT_E_INVAL;
    if ((((uintptr_t)ns_dev | (uintptr_t)nd_dev | (uintptr_t)count_dev) & 7) != 0) return CRDT_E_INVAL;
    const size_t ntiles = ns_max ? (ns_max + nd_max + CT - 1) / CT : 0;
    if (ntiles >= 0x7fffffffULL) return CRDT_E_RANGE;   // (so no byte count below wraps)
    if (out && ns_max && cmap_null(out)) return CRDT_E_INVAL;
    {
        CmSpan in[10], o[5];
        int ni = cmap_fields(src, ns_max, in), no = 0;
        ni += cmap_fields(dst, nd_max, in + ni);
        in[ni++] = {ns_dev, 8};
        in[ni++] = {nd_dev, 8};
        if (out) no = cmap_fields(out, ns_max, o);
        o[no++] = {count_dev, 8};
        if (cmap_clash(o, no, in, ni)) return CRDT_E_INVAL;
    }
    TileWs w;
    rc = w.reserve(ctx, ntiles, true, false, CBS);
    if (rc) return rc;
    // side a = dst: its copy of a shared cell is merged first
    return cmap_two_sided<true, CmMax>(ctx, w, ntiles, *dst, nd_max, nd_dev, *src, ns_max, ns_dev, out, count_dev);
}

extern "C" int crdt_cmap_values(crdt_ctx *ctx, const crdt_cmap *t, size_t n_max, const uint64_t *n_dev,
                                uint64_t *keys_out, uint64_t *p_out, uint64_t *n_out, int64_t *value_out,
                                uint64_t *count_dev) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!t || !count_dev) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62)) return CRDT_E_RANGE;
    if (n_max && cmap_null(t)) return CRDT_E_INVAL;
    if (cmap_misaligned(t)) return CRDT_E_INVAL;
    if ((((uintptr_t)keys_out | (uintptr_t)p_out | (uintptr_t)n_out | (uintptr_t)value_out | (uintptr_t)n_dev |
          (uintptr_t)count_dev) & 7) != 0)
        return CRDT_E_INVAL;
    const size_t ntiles = (n_max + RT - 1) / RT;
    if (ntiles >= 0x7fffffffULL) return CRDT_E_RANGE;   // (so no byte count below wraps)
    {
        CmSpan in[5], o[5];
        int ni = cmap_fields(t, n_max, in);
        in[ni++] = {n_dev, 8};
        o[0] = {keys_out, n_max * 8};
        o[1] = {p_out, n_max * 8};
        o[2] = {n_out, n_max * 8};
        o[3] = {value_out, n_max * 8};
        o[4] = {count_dev, 8};
        if (cmap_clash(o, 5, in, ni)) return CRDT_E_INVAL;
    }
    TileWs w;
    rc = w.reserve(ctx, ntiles, false, false, RNW);
    if (rc) return rc;
    const bool sums = p_out || n_out || value_out, wr = sums || keys_out;
    const hipStream_t s = ctx->stream;
    const unsigned g = (unsigned)ntiles;
    if (ntiles) {
        if (wr) k_cmap_heads<true><<<g, RB, 0, s>>>(t->key, n_max, n_dev, w.tcnt, w.bits);
        else k_cmap_heads<false><<<g, RB, 0, s>>>(t->key, n_max, n_dev, w.tcnt, w.bits);
    }
    w.scan<NoCarry<>>(ctx, n_max, n_dev, 0, nullptr, wr, count_dev);
    if (ntiles && keys_out)
        k_tile_write_field<uint64_t><<<g, kTileB, 0, s>>>(t->key, n_max, n_dev, w.bits, w.ic, keys_out, ctx->dev_status);
    if (ntiles && sums) {
        if (ntiles > 1)
            k_cmap_zero<<<(unsigned)((ntiles + 255) / 256), 256, 0, s>>>(n_max, n_dev, w.bits, w.ic, p_out, n_out, value_out);
        k_cmap_sums<<<g, RB, 0, s>>>(t->p, t->n, n_max, n_dev, w.bits, w.ic, p_out, n_out, value_out, ctx->dev_status);
    }
    return check_launch(ctx);
}

extern "C" int crdt_cmap_lookup(crdt_ctx *ctx, const crdt_cmap *t, size_t n_max, const uint64_t *n_dev,
                                const uint64_t *probes_dev, size_t m, int64_t *value_out, uint8_t *found_out) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!t) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62) || m >= (1ULL << 60)) return CRDT_E_RANGE;
    if (m == 0) return CRDT_OK;
    if (!probes_dev || !value_out || (n_max && cmap_null(t)) || cmap_misaligned(t)) return CRDT_E_INVAL;
    if ((((uintptr_t)probes_dev | (uintptr_t)value_out | (uintptr_t)n_dev) & 7) != 0) return CRDT_E_INVAL;
    {
        CmSpan in[6], o[2];
        int ni = cmap_fields(t, n_max, in);
        in[ni++] = {n_dev, 8};
        in[ni++] = {probes_dev, m * 8};
        o[0] = {value_out, m * 8};
        o[1] = {found_out, m};
        if (cmap_clash(o, 2, in, ni)) return CRDT_E_INVAL;
    }
    k_cmap_lookup<<<grid_for(m, 256, (unsigned)ctx->num_cus * 8), 256, 0, ctx->stream>>>(*t, n_max, n_dev, probes_dev, m,
                                                                                       value_out, found_out,
                                                                                       ctx->dev_status);
    return check_launch(ctx);
}

// what the digest and the selection check alike: t, n_max, the splitters
static int cmap_dig_check_in(const crdt_cmap *t, size_t n_max, const uint64_t *n_dev, const uint64_t *sp, size_t m) {
    if (!t) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62) || m >= kDigMaxSplit) return CRDT_E_RANGE;
    if ((m && !sp) || (((uintptr_t)sp | (uintptr_t)n_dev) & 7) != 0) return CRDT_E_INVAL;
    if ((n_max && cmap_null(t)) || cmap_misaligned(t)) return CRDT_E_INVAL;
    if ((n_max + RT - 1) / RT >= 0x7fffffffULL) return CRDT_E_RANGE;   // (so no byte count below wraps)
    return CRDT_OK;
}

extern "C" int crdt_cmap_digest(crdt_ctx *ctx, const crdt_cmap *t, size_t n_max, const uint64_t *n_dev,
                                const uint64_t *splitters_dev, size_t m, uint64_t *hash_out_dev,
                                uint64_t *count_out_dev) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!hash_out_dev || !count_out_dev) return CRDT_E_INVAL;
    rc = cmap_dig_check_in(t, n_max, n_dev, splitters_dev, m);
    if (rc) return rc;
    if ((((uintptr_t)hash_out_dev | (uintptr_t)count_out_dev) & 7) != 0) return CRDT_E_INVAL;
    {
        CmSpan in[6], o[2];
        int ni = cmap_fields(t, n_max, in);
        in[ni++] = {n_dev, 8};
        in[ni++] = {splitters_dev, m * 8};
        o[0] = {hash_out_dev, (m + 1) * 8};
        o[1] = {count_out_dev, (m + 1) * 8};
        if (cmap_clash(o, 2, in, ni)) return CRDT_E_INVAL;
    }
    const size_t ntiles = (n_max + RT - 1) / RT;
    dig_init(ctx, n_max, n_dev, m, hash_out_dev, count_out_dev);
    if (ntiles)
        k_cmap_digest<<<(unsigned)ntiles, RB, 0, ctx->stream>>>(*t, n_max, n_dev, splitters_dev, (uint32_t)m, hash_out_dev,
                                                                count_out_dev);
    return check_launch(ctx);
}

extern "C" int crdt_cmap_select(crdt_ctx *ctx, const crdt_cmap *t, size_t n_max, const uint64_t *n_dev,
                                const uint64_t *splitters_dev, size_t m, const uint8_t *flags_dev,
                                const crdt_cmap *out, uint64_t *count_dev) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!count_dev || !flags_dev) return CRDT_E_INVAL;
    rc = cmap_dig_check_in(t, n_max, n_dev, splitters_dev, m);
    if (rc) return rc;
    if (((uintptr_t)count_dev & 7) != 0 || (out && cmap_misaligned(out))) return CRDT_E_INVAL;
    if (out && n_max && cmap_null(out)) return CRDT_E_INVAL;
    {
        CmSpan in[7], o[5];
        int ni = cmap_fields(t, n_max, in), no = 0;
        in[ni++] = {n_dev, 8};
        in[ni++] = {splitters_dev, m * 8};
        in[ni++] = {flags_dev, m + 1};
        if (out) no = cmap_fields(out, n_max, o);
        o[no++] = {count_dev, 8};
        if (cmap_clash(o, no, in, ni)) return CRDT_E_INVAL;
    }
    const size_t ntiles = (n_max + RT - 1) / RT;
    TileWs w;
    rc = w.reserve(ctx, ntiles, false, false, RNW);
    if (rc) return rc;
    const bool wr = out != nullptr;
    const hipStream_t s = ctx->stream;
    const unsigned g = (unsigned)ntiles;
    if (ntiles) {
        if (wr) k_cmap_sel_count<true><<<g, RB, 0, s>>>(t->key, n_max, n_dev, splitters_dev, (uint32_t)m, flags_dev, w.tcnt, w.bits);
        else k_cmap_sel_count<false><<<g, RB, 0, s>>>(t->key, n_max, n_dev, splitters_dev, (uint32_t)m, flags_dev, w.tcnt, w.bits);
    }
    w.scan<NoCarry<>>(ctx, n_max, n_dev, 0, nullptr, wr, count_dev);
    if (ntiles && wr) k_cmap_sel_write<<<g, kTileB, 0, s>>>(*t, n_max, n_dev, w.bits, w.ic, *out, ctx->dev_status);
    return check_launch(ctx);
}

// ---------------------------------------------------------------- combine, from_ops
// heads -> scan -> zero -> sums over the carved tiles; R: the rep column's element; IDX: idx is always given
// (from_ops), so that no direct sums kernel is built for that R
template <class R, bool IDX>
static int cmap_combine_passes(crdt_ctx *ctx, const TileWs &w, size_t ntiles, const uint64_t *key, const R *rep,
                               const uint64_t *p, const uint64_t *q, size_t n_max, const uint64_t *n_dev,
                               const uint32_t *idx, size_t n_src, const crdt_cmap *out, uint64_t *count_dev) {
    const bool wr = out != nullptr;
    const hipStream_t s = ctx->stream;
    const unsigned g = (unsigned)ntiles;
    if (ntiles) {
        if (wr) k_cmap_cheads<true, R><<<g, RB, 0, s>>>(key, rep, n_max, n_dev, w.tcnt, w.bits);
        else k_cmap_cheads<false, R><<<g, RB, 0, s>>>(key, rep, n_max, n_dev, w.tcnt, w.bits);
    }
    w.scan<NoCarry<>>(ctx, n_max, n_dev, 0, nullptr, wr, count_dev);
    if (ntiles && wr) {
        if (ntiles > 1)
            k_cmap_zero<<<(unsigned)((ntiles + 255) / 256), 256, 0, s>>>(n_max, n_dev, w.bits, w.ic, out->p, out->n, nullptr);
        if (IDX || idx)
            k_cmap_csums<CmSrcIndexed, R><<<g, RB, 0, s>>>(CmSrcIndexed{p, q, idx, n_src}, key, rep, n_max, n_dev, w.bits,
                                                           w.ic, *out, ctx->dev_status);
        else if constexpr (!IDX)
            k_cmap_csums<CmSrcDirect, R><<<g, RB, 0, s>>>(CmSrcDirect{p, q}, key, rep, n_max, n_dev, w.bits, w.ic, *out,
                                                          ctx->dev_status);
    }
    return check_launch(ctx);
}

extern "C" int crdt_cmap_combine(crdt_ctx *ctx, const crdt_cmap *in, size_t n_max, const uint64_t *n_dev,
                                 const uint32_t *idx_dev, size_t n_src, const crdt_cmap *out, uint64_t *count_dev) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!in || !count_dev) return CRDT_E_INVAL;
    if (n_max >= (1ULL << 62) || (idx_dev && n_src >= (1ULL << 62))) return CRDT_E_RANGE;
    if (n_max && (cmap_null(in) || (idx_dev && !n_src))) return CRDT_E_INVAL;
    if (cmap_misaligned(in) || (out && cmap_misaligned(out))) return CRDT_E_INVAL;
    if ((((uintptr_t)n_dev | (uintptr_t)count_dev) & 7) != 0 || ((uintptr_t)idx_dev & 3) != 0) return CRDT_E_INVAL;
    const size_t ntiles = (n_max + RT - 1) / RT;
    if (ntiles >= 0x7fffffffULL) return CRDT_E_RANGE;   // (so no byte count below wraps)
    if (out && n_max && cmap_null(out)) return CRDT_E_INVAL;
    {
        const size_t nv = idx_dev ? n_src : n_max;       // elements of the p / n columns
        CmSpan i[6], o[5];
        int ni = 0, no = 0;
        i[ni++] = {in->key, n_max * 8};
        i[ni++] = {in->rep, n_max * 4};
        i[ni++] = {in->p, nv * 8};
        i[ni++] = {in->n, nv * 8};
        i[ni++] = {n_dev, 8};
        i[ni++] = {idx_dev, n_max * 4};
        if (out) no = cmap_fields(out, n_max, o);
        o[no++] = {count_dev, 8};
        if (cmap_clash(o, no, i, ni)) return CRDT_E_INVAL;
    }
    TileWs w;
    rc = w.reserve(ctx, ntiles, false, false, RNW);
    if (rc) return rc;
    return cmap_combine_passes<uint32_t, false>(ctx, w, ntiles, in->key, in->rep, in->p, in->n, n_max, n_dev, idx_dev, n_src, out,
                                         count_dev);
}

extern "C" int crdt_cmap_from_ops(crdt_ctx *ctx, const uint64_t *op_key_dev, const uint32_t *op_rep_dev,
                                  const uint64_t *op_dp_dev, const uint64_t *op_dn_dev, size_t m, const crdt_cmap *out,
                                  uint64_t *count_dev) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out || !count_dev) return CRDT_E_INVAL;
    if (m >= (1ULL << 32)) return CRDT_E_RANGE;         // the sort's limit, and the index column's width
    if (m && (!op_key_dev || !op_rep_dev || !op_dp_dev || !op_dn_dev || cmap_null(out))) return CRDT_E_INVAL;
    if (cmap_misaligned(out) || ((uintptr_t)op_rep_dev & 3) != 0) return CRDT_E_INVAL;
    if ((((uintptr_t)op_key_dev | (uintptr_t)op_dp_dev | (uintptr_t)op_dn_dev | (uintptr_t)count_dev) & 7) != 0)
        return CRDT_E_INVAL;
    {
        CmSpan i[4], o[5];
        i[0] = {op_key_dev, m * 8};
        i[1] = {op_rep_dev, m * 4};
        i[2] = {op_dp_dev, m * 8};
        i[3] = {op_dn_dev, m * 8};
        int no = cmap_fields(out, m, o);
        o[no++] = {count_dev, 8};
        if (cmap_clash(o, no, i, 4)) return CRDT_E_INVAL;
    }
    // The workspace, reserved once for the whole call so that neither the sort's own reserve nor the tiles' moves
    // it: [the sort's share | the tiles' share] from the start, both carved by their owners, and behind the larger
    // of the two the view's three columns and the sorted tuples, which live from the sort to the last pass.
    const size_t ntiles = (m + RT - 1) / RT;
    const size_t b_tiles = TileWs::bytes(ntiles, false, false, RNW);
    const size_t b_sort = m ? tuples_sort_ws_bytes(m) : 0;
    const size_t front = Carve::round(b_sort > b_tiles ? b_sort : b_tiles);
    const size_t b_cols = 3 * Carve::round(m * 8) + 2 * Carve::round(m * 4) + 2 * Carve::round(m) + 2048;
    rc = ws_reserve(ctx, front + b_cols);
    if (rc) return rc;
    Carve x((char *)ctx->ws + front);
    crdt_tuples view, sorted;
    view.key = const_cast<uint64_t *>(op_key_dev);
    view.ts = x.take<uint64_t>(m);
    view.rep = x.take<uint32_t>(m);
    view.tomb = x.take<uint8_t>(m);
    sorted.key = x.take<uint64_t>(m);
    sorted.ts = x.take<uint64_t>(m);
    sorted.rep = x.take<uint32_t>(m);
    sorted.tomb = x.take<uint8_t>(m);
    if (m) {
        k_cmap_ops_view<<<grid_for(m, 256, (unsigned)ctx->num_cus * 8), 256, 0, ctx->stream>>>(op_rep_dev, m, view.ts,
                                                                                             view.rep, view.tomb);
        rc = check_launch(ctx);
        if (rc) return rc;
        void *const ws = ctx->ws;
        rc = crdt_tuples_sort(ctx, &view, m, &sorted);  // (synchronises once: its plan's read-back)
        if (rc) return rc;
        if (ctx->ws != ws) return CRDT_E_HIP;           // (never: the reserve above covers the sort's)
    }
    TileWs w;
    rc = w.reserve(ctx, ntiles, false, false, RNW);
    if (rc) return rc;
    // sorted by (key, rep, index): the combine over the sorted key / widened rep, p and n gathered through the index
    return cmap_combine_passes<uint64_t, true>(ctx, w, ntiles, sorted.key, sorted.ts, op_dp_dev, op_dn_dev, m, nullptr,
                                         sorted.rep, m, out, count_dev);
}
