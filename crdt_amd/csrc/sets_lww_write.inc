// sets_lww_write.inc -- the body of k_lww_write and k_lww_write_src (sets.hip),
// included into each kernel: the kernel's parameters and, from the kernel,
//   constexpr bool SRC : also store every output's source index;
//   src                : int64_t[na + nb], written at the output's rank when SRC
//                        (>= 0 an A index, < 0 B index j as -(j + 1)).
// One text, two kernels: the plain kernel's instructions are those it had
// before the _src form existed (DESIGN.md §5.14; a shared __device__ function
// reordered them).
    constexpr int NWV = WT / 64, FI = (WH / 64) / NWV, CAP = WH + 3, P = LT / WH, WPP = LNW / P;
    static_assert(LNW == 64 && WH * P == LT && FI * NWV * 64 == WH && WH == 4 * WT, "shape");
    // (each field holds A's run then B's, each from its 16-byte aligned-down
    // start by LDS-DMA: up to 64 bytes more than the elements)
    __shared__ alignas(16) uint64_t s_key[CAP + 8];
    __shared__ alignas(16) uint64_t s_ts[CAP + 8];
    __shared__ alignas(16) uint32_t s_rep[CAP + 16];
    __shared__ alignas(16) uint8_t s_tomb[CAP + 64];
    const uint64_t t = t0 + blockIdx.x / P;
    const uint32_t h = blockIdx.x % P;
    const MergeTile b = merge_tile<LT>(split, t, na + nb);
    const int lane = threadIdx.x & 63;
    const uint64_t word_a = bits[t * 2 * LNW + lane], word_e = bits[t * 2 * LNW + LNW + lane];
    const uint64_t ob = ic[t];                           // (with the split and bitmaps: no load after the barrier)
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
    // every index below derives from the bitmaps: a tile whose bitmaps do not
    // describe its counts raises CRDT_DEV_RANGE instead of reading out of range
    if (!bitmaps_consistent(word_a, word_e, pre_a, LNW, b.na, b.n, lane)) {
        if (threadIdx.x == 0 && blockIdx.x % P == 0) atomicOr(err, CRDT_DEV_RANGE);
        return;
    }
    // the half's runs: A [ra, ra + ca), B [rb, rb + cb); staged from ra - 2 / rb - 1
    const uint32_t ha = (uint32_t)__builtin_amdgcn_readlane(pre_a, WPP * h);       // A items before the part
    const uint32_t ha1 = h + 1 == P ? b.na : (uint32_t)__builtin_amdgcn_readlane(pre_a, WPP * (h + 1));  // ... before its end
    const uint32_t d0 = WH * h;
    const uint32_t hn = b.n > d0 ? (b.n - d0 < (uint32_t)WH ? b.n - d0 : (uint32_t)WH) : 0;   // items in the part
    if (hn == 0) return;
    const size_t ra = b.i0 + ha, rb = b.j0 + (d0 - ha);
    const uint32_t ca = ha1 - ha, cb = hn - ca;
    const uint32_t na2 = ca + 2;                         // staged A: ra-2 .. ra+ca-1 (slots 0 .. ca+1)
    // slot x of field f sits at LDS element x + (x < na2 ? oa[f] : ob[f])
    int oa_k, ob_k, oa_t, ob_t, oa_r, ob_r, oa_m, ob_m;
    {
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const size_t ga = ra >= 2 ? ra - 2 : 0, gb = rb >= 1 ? rb - 1 : 0;   // first staged element of each side
        const uint32_t ka = (uint32_t)(ra + ca - ga), kb = (uint32_t)(rb + cb - gb);
        const int sa = (int)(ga - (ra - 2)), sb = (int)(gb - (rb - 1)) + (int)na2;   // their slots
        uint32_t at = 0;
        oa_k = dma_run<uint64_t, NWV>(A.key, ga, ka, s_key, &at, wv, lane) - sa;
        ob_k = dma_run<uint64_t, NWV>(B.key, gb, kb, s_key, &at, wv, lane) - sb;
        at = 0;
        // (ts / rep / tomb read once, nontemporal: they do not evict the keys
        // the count pass left in the Infinity Cache)
        oa_t = dma_run<uint64_t, NWV, 2>(A.ts, ga, ka, s_ts, &at, wv, lane) - sa;
        ob_t = dma_run<uint64_t, NWV, 2>(B.ts, gb, kb, s_ts, &at, wv, lane) - sb;
        at = 0;
        oa_r = dma_run<uint32_t, NWV, 2>(A.rep, ga, ka, s_rep, &at, wv, lane) - sa;
        ob_r = dma_run<uint32_t, NWV, 2>(B.rep, gb, kb, s_rep, &at, wv, lane) - sb;
        at = 0;
        oa_m = dma_run<uint8_t, NWV, 2>(A.tomb, ga, ka, s_tomb, &at, wv, lane) - sa;
        ob_m = dma_run<uint8_t, NWV, 2>(B.tomb, gb, kb, s_tomb, &at, wv, lane) - sb;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA has landed in LDS
    }
    __syncthreads();
    const int wvu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto below = [&](uint64_t msk) -> uint32_t {        // set bits of msk below this lane
        return __builtin_amdgcn_mbcnt_hi((uint32_t)(msk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)msk, 0u));
    };
    // staged fields of slot sl
    auto tag_at = [&](uint32_t sl, uint64_t &k, uint64_t &ts, uint32_t &r) {
        const bool sa = sl < na2;
        k = s_key[(int)sl + (sa ? oa_k : ob_k)];
        ts = s_ts[(int)sl + (sa ? oa_t : ob_t)];
        r = s_rep[(int)sl + (sa ? oa_r : ob_r)];
    };
    auto tomb_at = [&](uint32_t sl) -> uint8_t { return s_tomb[(int)sl + (sl < na2 ? oa_m : ob_m)]; };
#pragma unroll
    for (int f = 0; f < FI; ++f) {
        const int w = WPP * (int)h + wvu + NWV * f;      // the tile's word
        const uint64_t wa = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(word_a >> 32), w) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((uint32_t)word_a, w);
        const uint64_t we = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(word_e >> 32), w) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((uint32_t)word_e, w);
        if (!((we >> lane) & 1)) continue;
        const uint32_t pa = (uint32_t)__builtin_amdgcn_readlane(pre_a, w) + below(wa);   // A items before (tile)
        const uint32_t rk = (uint32_t)__builtin_amdgcn_readlane(pre_e, w) + below(we);   // output rank
        const uint32_t k = 64u * (uint32_t)w + (uint32_t)lane;                          // tile merge item
        const uint32_t la = pa - ha, lb = (k - d0) - la; // A / B items of the half before this one
        const bool is_a = (wa >> lane) & 1;
        const size_t ai = ra + la;                       // A elements merged before this item
        uint64_t key, ts;
        uint32_t rep, xs;                                // the winner's staging slot
        bool on_a;
        size_t wi;
        if (is_a) {                                      // an A run end whose key B does not hold
            xs = la + 2;
            tag_at(xs, key, ts, rep);
            on_a = true;
            wi = ai;
        } else {                                         // B's run end; A's run end of the key just before it
            const uint32_t bs = na2 + 1 + lb;
            uint64_t kb_, tb, ka_ = 0, ta = 0;
            uint32_t rb_, ra_ = 0;
            tag_at(bs, kb_, tb, rb_);
            const bool a_has = ai > 0 && (tag_at(la + 1, ka_, ta, ra_), ka_ == kb_);
            const bool ya = a_has && (ta > tb || (ta == tb && ra_ >= rb_));   // A wins an equal tag
            key = kb_;
            on_a = ya;
            xs = ya ? la + 1 : bs;
            ts = ya ? ta : tb;
            rep = ya ? ra_ : rb_;
            wi = ya ? ai - 1 : rb + lb;
        }
        // the first copy of the winner's tag on its side: its staged
        // predecessor, then (rare) global memory before the staging
        uint8_t tomb = tomb_at(xs);
        const uint32_t lo = on_a ? 0u : na2;             // first staged slot of the side
        bool more = wi > 0;
        uint32_t sl = xs;
        while (more && sl > lo) {
            uint64_t pk, pt;
            uint32_t pr;
            tag_at(sl - 1, pk, pt, pr);
            if (pk != key || pt != ts || pr != rep) {
                more = false;
                break;
            }
            --sl;
            --wi;
            tomb = tomb_at(sl);
            more = wi > 0;
        }
        if (more && sl == lo) {                          // the run of copies reaches past the staging
            const size_t fc = first_copy(on_a ? A.key : B.key, on_a ? A.ts : B.ts, on_a ? A.rep : B.rep, wi, key, ts,
                                         rep);
            tomb = (on_a ? A.tomb : B.tomb)[fc];
            if constexpr (SRC) wi = fc;
        }
        const uint64_t o = ob + rk;
        if (o >= na + nb) {                              // (consistent bitmaps never get here)
            atomicOr(err, CRDT_DEV_RANGE);
            continue;
        }
        out.key[o] = key;
        out.ts[o] = ts;
        out.rep[o] = rep;
        out.tomb[o] = tomb;
        // (wi: the first copy of the winner's tag on its side, after the walk back)
        if constexpr (SRC) src[o] = on_a ? (int64_t)wi : -(int64_t)wi - 1;
    }
