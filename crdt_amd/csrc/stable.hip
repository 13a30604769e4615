// stable.hip -- the causal-stability cut of a vector-clock population
// (crdt_vclock_stable_cut): out[c] = min over rows of
// clocks[r][c], unsigned -- the number of node c's events every replica has
// seen.  The column-MIN twin of crdt_gcounter_fold (counters.hip), whose
// kernels stay as they are: the same two paths, the same launch geometry, the
// same 16-byte nontemporal loads, at the fold's product shape (unroll 8, one
// workgroup per CU) as compile-time constants -- no knob.  The identity of a
// minimum is 2^64 - 1: out is pre-filled with it and the finish step joins
// the partials by atomicMin (a partial that is still the identity is skipped).
#include "common.hpp"

namespace crdt {

typedef uint64_t cut_u64x2 __attribute__((ext_vector_type(2)));

constexpr int kCutUnroll = 8;            // the fold's product shape (knobs.inc fold.unroll)
constexpr unsigned kCutBlocksPerCu = 1;  // ... fold.blocks_per_cu
constexpr uint64_t kCutId = ~0ull;

__device__ __forceinline__ cut_u64x2 cut_vmin(cut_u64x2 x, cut_u64x2 y) {
    return __builtin_elementwise_min(x, y);  // unsigned 64-bit min per lane
}

// nodes a power of two in [2, 512]: a 256-lane block covers 512 uint64 =
// 512/nodes whole rows per load, every lane keeps one column pair.
template <int U>
__global__ __launch_bounds__(256) void k_cut_pow2(const cut_u64x2 *__restrict__ a, size_t n2, int nodes,
                                                  uint64_t *__restrict__ partial) {
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    cut_u64x2 m = {kCutId, kCutId};
    for (; i + (size_t)(U - 1) * stride < n2; i += (size_t)U * stride) {
        cut_u64x2 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = __builtin_nontemporal_load(a + i + (size_t)u * stride);
#pragma unroll
        for (int u = 0; u < U; ++u) m = cut_vmin(m, x[u]);
    }
    for (; i < n2; i += stride) m = cut_vmin(m, __builtin_nontemporal_load(a + i));
    __shared__ cut_u64x2 red[256];
    red[threadIdx.x] = m;
    __syncthreads();
    const int lanes_per_row = nodes >> 1;          // vectors per row
    if ((int)threadIdx.x < lanes_per_row) {
        cut_u64x2 r = red[threadIdx.x];
        for (int t = threadIdx.x + lanes_per_row; t < 256; t += lanes_per_row) r = cut_vmin(r, red[t]);
        partial[(size_t)blockIdx.x * nodes + 2 * threadIdx.x] = r.x;
        partial[(size_t)blockIdx.x * nodes + 2 * threadIdx.x + 1] = r.y;
    }
}

// Any other nodes or alignment: lanes stride over columns, blocks over rows.
__global__ __launch_bounds__(256) void k_cut_generic(const uint64_t *__restrict__ a, size_t rows, size_t nodes,
                                                     uint64_t *__restrict__ partial) {
    for (size_t c = threadIdx.x; c < nodes; c += 256) {
        uint64_t m = kCutId;
        for (size_t r = blockIdx.x; r < rows; r += gridDim.x) {
            const uint64_t v = a[r * nodes + c];
            m = v < m ? v : m;
        }
        partial[(size_t)blockIdx.x * nodes + c] = m;
    }
}

// partial [g x nodes] -> out[nodes] via unsigned 64-bit atomicMin (out pre-filled with 2^64 - 1).
__global__ __launch_bounds__(256) void k_cut_finish(const uint64_t *__restrict__ partial, size_t g, size_t nodes,
                                                    uint64_t *__restrict__ out) {
    for (size_t c = threadIdx.x; c < nodes; c += 256) {
        uint64_t m = kCutId;
        for (size_t r = blockIdx.x; r < g; r += gridDim.x) {
            const uint64_t v = partial[r * nodes + c];
            m = v < m ? v : m;
        }
        if (m != kCutId) atomicMin((unsigned long long *)&out[c], (unsigned long long)m);
    }
}

}  // namespace crdt

using namespace crdt;

extern "C" int crdt_vclock_stable_cut(crdt_ctx *ctx, const uint64_t *clocks, size_t rows, size_t nodes,
                                      uint64_t *out) {
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out || nodes == 0 || mul_overflows(rows, nodes)) return CRDT_E_INVAL;
    // the minimum over no replica is all-ones: a cut that would make every tombstone droppable
    if (rows == 0 || !clocks) return CRDT_E_INVAL;
    hipError_t e = hipMemsetAsync(out, 0xff, nodes * sizeof(uint64_t), ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e);
    const bool pow2 = nodes >= 2 && nodes <= 512 && (nodes & (nodes - 1)) == 0 && ((uintptr_t)clocks & 15) == 0;
    unsigned grid;
    if (pow2) grid = grid_for(rows * nodes / 2, 256 * (unsigned)kCutUnroll, (unsigned)ctx->num_cus * kCutBlocksPerCu);
    else grid = grid_for(rows, 1, (unsigned)(ctx->num_cus * 4));
    rc = ws_reserve(ctx, (size_t)grid * nodes * sizeof(uint64_t));
    if (rc) return rc;
    uint64_t *partial = (uint64_t *)ctx->ws;
    if (pow2)
        k_cut_pow2<kCutUnroll><<<grid, 256, 0, ctx->stream>>>((const cut_u64x2 *)clocks, rows * nodes / 2, (int)nodes,
                                                              partial);
    else
        k_cut_generic<<<grid, 256, 0, ctx->stream>>>(clocks, rows, nodes, partial);
    rc = check_launch(ctx);
    if (rc) return rc;
    const unsigned g2 = grid < 32 ? grid : 32;
    k_cut_finish<<<g2, 256, 0, ctx->stream>>>(partial, grid, nodes, out);
    return check_launch(ctx);
}
