// sets_or_write.inc -- the body of k_or_write and k_or_write_src (sets.hip),
// included into each kernel: the kernel's parameters and, from the kernel,
//   constexpr bool SRC : also store every output's source index;
//   src                : int64_t[na + nb], written at the output's rank when SRC
//                        (>= 0 an A index, < 0 B index j as -(j + 1)).
// One text, two kernels: the plain kernel's instructions are those it had
// before the _src form existed (DESIGN.md §5.14; a shared __device__ function
// reordered them).
    constexpr int NWV = WT / 64, P = OT / WH, WPP = ONW / P, FI = WPP / NWV, CAP = WH + 2;
    static_assert(FI * NWV == WPP && WH * P == OT && ONW <= 64 && WH == 4 * WT, "shape");
    __shared__ alignas(16) uint64_t s_key[CAP + 8];
    __shared__ alignas(16) uint64_t s_ts[CAP + 8];
    __shared__ alignas(16) uint32_t s_rep[CAP + 16];
    __shared__ alignas(16) uint8_t s_tomb[CAP + 64];
    const uint64_t t = t0 + blockIdx.x / P;
    const uint32_t h = blockIdx.x % P;
    const MergeTile b = merge_tile<OT>(split, t, na + nb);
    const int lane = threadIdx.x & 63;
    const bool wl_ok = lane < ONW;
    // split, bitmap words and offset loads issued together (none after the barrier)
    const uint64_t word_a = wl_ok ? bits[t * 2 * ONW + lane] : 0, word_e = wl_ok ? bits[t * 2 * ONW + ONW + lane] : 0;
    const uint64_t ob = ic[t];
    uint32_t pre_a = (uint32_t)__popcll(word_a), pre_e = (uint32_t)__popcll(word_e);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t ya = __shfl_up(pre_a, o), ye = __shfl_up(pre_e, o);
        if (lane >= o) {
            pre_a += ya;
            pre_e += ye;
        }
    }
    pre_a -= (uint32_t)__popcll(word_a);
    pre_e -= (uint32_t)__popcll(word_e);
    if (!bitmaps_consistent(word_a, word_e, pre_a, ONW, b.na, b.n, lane)) {   // (see k_lww_write)
        if (threadIdx.x == 0 && blockIdx.x % P == 0) atomicOr(err, CRDT_DEV_RANGE);
        return;
    }
    // the part's runs: A [pa0, pa0 + ca), B [pb0, pb0 + cb) (tile-relative)
    const uint32_t d0 = WH * h;
    const uint32_t hn = b.n > d0 ? (b.n - d0 < (uint32_t)WH ? b.n - d0 : (uint32_t)WH) : 0;   // items in the part
    if (hn == 0) return;
    const uint32_t pa0 = P == 1 ? 0u : (uint32_t)__builtin_amdgcn_readlane(pre_a, WPP * h);
    const uint32_t pa1 = h + 1 == P ? b.na : (uint32_t)__builtin_amdgcn_readlane(pre_a, WPP * (h + 1));
    const uint32_t ca = pa1 - pa0, cb = hn - ca, pb0 = d0 - pa0;
    const size_t ga = b.i0 + pa0, gb = b.j0 + pb0;       // global index of each run's first element
    // staged by LDS-DMA: A run (slots 0 .. ca-1), then B run (slots ca ..),
    // every field once; slot x of field f at LDS element x + (x < ca ? oa[f] : ob[f])
    int oa_k, ob_k, oa_t, ob_t, oa_r, ob_r, oa_m, ob_m;
    {
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int sb = (int)ca;
        uint32_t at = 0;
        oa_k = dma_run<uint64_t, NWV>(A.key, ga, ca, s_key, &at, wv, lane);
        ob_k = dma_run<uint64_t, NWV>(B.key, gb, cb, s_key, &at, wv, lane) - sb;
        at = 0;
        oa_t = dma_run<uint64_t, NWV>(A.ts, ga, ca, s_ts, &at, wv, lane);
        ob_t = dma_run<uint64_t, NWV>(B.ts, gb, cb, s_ts, &at, wv, lane) - sb;
        at = 0;
        oa_r = dma_run<uint32_t, NWV>(A.rep, ga, ca, s_rep, &at, wv, lane);
        ob_r = dma_run<uint32_t, NWV>(B.rep, gb, cb, s_rep, &at, wv, lane) - sb;
        at = 0;
        oa_m = dma_run<uint8_t, NWV>(A.tomb, ga, ca, s_tomb, &at, wv, lane);
        ob_m = dma_run<uint8_t, NWV>(B.tomb, gb, cb, s_tomb, &at, wv, lane) - sb;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA has landed in LDS
    }
    __syncthreads();
    const int wvu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto below = [&](uint64_t msk) -> uint32_t {        // set bits of msk below this lane
        return __builtin_amdgcn_mbcnt_hi((uint32_t)(msk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)msk, 0u));
    };
#pragma unroll
    for (int f = 0; f < FI; ++f) {
        const int w = WPP * (int)h + wvu + NWV * f;      // the tile's word
        // (readlane returns int: widen through uint32_t, never sign-extend)
        const uint64_t wa = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(word_a >> 32), w) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((uint32_t)word_a, w);
        const uint64_t we = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(word_e >> 32), w) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((uint32_t)word_e, w);
        if (!((we >> lane) & 1)) continue;
        const uint32_t la = (uint32_t)__builtin_amdgcn_readlane(pre_a, w) + below(wa) - pa0;   // A items before (part)
        const uint32_t rk = (uint32_t)__builtin_amdgcn_readlane(pre_e, w) + below(we);         // output rank (tile)
        const uint32_t k = 64u * (uint32_t)w + (uint32_t)lane - d0;
        const uint32_t lb = k - la;                      // B items before (part)
        const bool is_a = (wa >> lane) & 1;
        const uint32_t xs = is_a ? la : ca + lb;         // the first copy's slot
        const int xo = is_a ? 0 : 1;
        const uint64_t key = s_key[(int)xs + (xo ? ob_k : oa_k)], ts = s_ts[(int)xs + (xo ? ob_t : oa_t)];
        const uint32_t rep = s_rep[(int)xs + (xo ? ob_r : oa_r)];
        uint32_t tomb = 0;
        // A's copies (an A first copy only), then B's from position lb:
        // in the staging, then past the part in global memory (rare)
        if (is_a) {
            uint32_t s = la;
            while (s < ca && s_key[(int)s + oa_k] == key && s_ts[(int)s + oa_t] == ts && s_rep[(int)s + oa_r] == rep)
                tomb |= s_tomb[(int)(s++) + oa_m];
            if (s == ca)
                for (size_t g = ga + ca; g < na && A.key[g] == key && A.ts[g] == ts && A.rep[g] == rep; ++g)
                    tomb |= A.tomb[g];
        }
        {
            uint32_t s = lb;
            while (s < cb && s_key[(int)(ca + s) + ob_k] == key && s_ts[(int)(ca + s) + ob_t] == ts &&
                   s_rep[(int)(ca + s) + ob_r] == rep)
                tomb |= s_tomb[(int)(ca + s++) + ob_m];
            if (s == cb)
                for (size_t g = gb + cb; g < nb && B.key[g] == key && B.ts[g] == ts && B.rep[g] == rep; ++g)
                    tomb |= B.tomb[g];
        }
        const uint64_t o = ob + rk;
        if (o >= na + nb) {                              // (consistent bitmaps never get here)
            atomicOr(err, CRDT_DEV_RANGE);
            continue;
        }
        out.key[o] = key;
        out.ts[o] = ts;
        out.rep[o] = rep;
        out.tomb[o] = (uint8_t)tomb;
        // (an emitting item is its tag's first copy in merged order)
        if constexpr (SRC) src[o] = is_a ? (int64_t)(ga + la) : -(int64_t)(gb + lb) - 1;
    }
