//go:build cgo && rocm

// The keyed PN-Counter map on device pointers (crdt_cmap_*, include/crdt_amd.h):
// the convergent form of the per-key curr + change fold of the reference's
// replay (main.go:75-98).  A state is cells (key, rep, p, n) strictly ascending
// by (key, rep) in HBM; CMapDigest / CMapSelect are its range digests for
// replicas that share no memory.  Uncompiled in the build image (no Go toolchain).
package crdt

/*
#include "crdt_amd.h"
*/
import "C"

// CMapMerge: the join of two counter maps -- the union of their cells, a cell
// held by both with the unsigned maximum of p and of n -- into out (capacity
// naMax + nbMax cells; nil: the count alone), its length into countDev.  naDev /
// nbDev (nil: all nMax cells of the side) chain the call off device counts
// with no read-back.  Enqueued: crdt_ctx_sync before reading.
func CMapMerge(a *C.crdt_cmap, naMax int, naDev *C.uint64_t, b *C.crdt_cmap, nbMax int, nbDev *C.uint64_t,
	out *C.crdt_cmap, countDev *C.uint64_t) error {
	if a == nil || b == nil || countDev == nil || naMax < 0 || nbMax < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_cmap_merge(gpuCtx, a, C.size_t(naMax), naDev, b, C.size_t(nbMax), nbDev, out, countDev))
}

// CMapApply: replica rep's batch of m increments (opKeyDev strictly ascending)
// applied to t -- cell (opKey[i], rep) becomes (p + opDp[i], n + opDn[i]) mod
// 2^64, an absent cell is created from (0, 0) -- into out (capacity nMax + m;
// nil: the count alone).  The integer AddCommand (main.go:173-207) as a state
// change that commutes.  Enqueued.
func CMapApply(t *C.crdt_cmap, nMax int, nDev *C.uint64_t, rep uint32, opKeyDev, opDpDev, opDnDev *C.uint64_t, m int,
	out *C.crdt_cmap, countDev *C.uint64_t) error {
	if t == nil || countDev == nil || nMax < 0 || m < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_cmap_apply(gpuCtx, t, C.size_t(nMax), nDev, C.uint32_t(rep), opKeyDev, opDpDev, opDnDev,
		C.size_t(m), out, countDev))
}

// CMapValues: one row per distinct key of t, in key order -- the key, P and N
// (the sums of the key's p and n cells mod 2^64) and value = int64(P - N), the
// number the replay of main.go:75-98 arrives at -- each output of capacity nMax
// rows and optional (all nil: the number of distinct keys alone).  Enqueued.
func CMapValues(t *C.crdt_cmap, nMax int, nDev, keysOutDev, pOutDev, nOutDev *C.uint64_t, valueOutDev *C.int64_t,
	countDev *C.uint64_t) error {
	if t == nil || countDev == nil || nMax < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_cmap_values(gpuCtx, t, C.size_t(nMax), nDev, keysOutDev, pOutDev, nOutDev, valueOutDev, countDev))
}

// CMapLookup: the counter of each of the m probe keys (any order, repeats
// allowed) into valueOutDev, 0 where the key is absent; foundOutDev (may be
// nil) 1 / 0.  No probes enqueue nothing.
func CMapLookup(t *C.crdt_cmap, nMax int, nDev, probesDev *C.uint64_t, m int, valueOutDev *C.int64_t,
	foundOutDev *C.uint8_t) error {
	if t == nil || nMax < 0 || m < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_cmap_lookup(gpuCtx, t, C.size_t(nMax), nDev, probesDev, C.size_t(m), valueOutDev, foundOutDev))
}

// CMapDelta: the smallest D with merge(dst, D) == merge(dst, src) -- the cells
// of src that dst lacks or holds with a smaller p or n, with src's own p and n
// -- into out (capacity nsMax; nil: the count alone, 0 iff dst already holds
// all of src).  What a pull needs to ship instead of the entire Diff
// (main.go:153-170).  Enqueued.
func CMapDelta(src *C.crdt_cmap, nsMax int, nsDev *C.uint64_t, dst *C.crdt_cmap, ndMax int, ndDev *C.uint64_t,
	out *C.crdt_cmap, countDev *C.uint64_t) error {
	if src == nil || dst == nil || countDev == nil || nsMax < 0 || ndMax < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_cmap_delta(gpuCtx, src, C.size_t(nsMax), nsDev, dst, C.size_t(ndMax), ndDev, out, countDev))
}

// CMapDigest: one order-independent fingerprint per key range of t into
// hashOutDev / countOutDev, m + 1 entries each -- the buckets are SetDigest's
// (bucket(key) = #{ j : splitters[j] <= key }, unsigned), hash[b] the wrapping
// sum over the cells in b of sm(sm(sm(sm(key) ^ rep) ^ p) ^ n), count[b] their
// number.  Two replicas exchange these 16 bytes a bucket instead of the entire
// Diff of a gossip pull (main.go:153-170, :245-256); SetDigestDiff flags the
// buckets that differ.  Enqueued.
func CMapDigest(t *C.crdt_cmap, nMax int, nDev, splittersDev *C.uint64_t, m int,
	hashOutDev, countOutDev *C.uint64_t) error {
	if t == nil || hashOutDev == nil || countOutDev == nil || nMax < 0 || m < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_cmap_digest(gpuCtx, t, C.size_t(nMax), nDev, splittersDev, C.size_t(m), hashOutDev, countOutDev))
}

// CMapSelect: the cells of t whose bucket has flagsDev[b] != 0 (m + 1 flags),
// in order and unchanged, into out (capacity nMax; nil: the count alone), their
// number into countDev: what a replica ships for the differing ranges.  The
// receiver's side is CMapMerge(dst, out) with countDev as nbDev.  Enqueued.
func CMapSelect(t *C.crdt_cmap, nMax int, nDev, splittersDev *C.uint64_t, m int, flagsDev *C.uint8_t,
	out *C.crdt_cmap, countDev *C.uint64_t) error {
	if t == nil || flagsDev == nil || countDev == nil || nMax < 0 || m < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_cmap_select(gpuCtx, t, C.size_t(nMax), nDev, splittersDev, C.size_t(m), flagsDev, out, countDev))
}

// CMapCombine: sorted cells with repeats -- in ascending by (key, rep) but not
// strictly -- into one cell per distinct (key, rep), p and n summed over the
// run mod 2^64 (capacity nMax; nil out: the count alone).  With idxDev (nMax
// uint32 values) cell i contributes in.p[idx[i]], in.n[idx[i]], columns of
// nSrc elements; an index out of range contributes 0 and raises
// CRDT_DEV_RANGE.  The per-key sum of the replay (main.go:87-96) over a sorted
// log.  Enqueued.
func CMapCombine(in *C.crdt_cmap, nMax int, nDev *C.uint64_t, idxDev *C.uint32_t, nSrc int, out *C.crdt_cmap,
	countDev *C.uint64_t) error {
	if in == nil || countDev == nil || nMax < 0 || nSrc < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_cmap_combine(gpuCtx, in, C.size_t(nMax), nDev, idxDev, C.size_t(nSrc), out, countDev))
}

// CMapAdd: the additive join of the state t and the batch d (both strictly
// ascending) -- the union of the cells, a cell of both with (p_t + p_d, n_t +
// n_d), a cell of d alone created with d's values -- into out (capacity ntMax +
// ndMax; nil: the count alone).  CMapApply for many replicas in one pass.  Not
// idempotent: each batch is delivered once.  Enqueued.
func CMapAdd(t *C.crdt_cmap, ntMax int, ntDev *C.uint64_t, d *C.crdt_cmap, ndMax int, ndDev *C.uint64_t,
	out *C.crdt_cmap, countDev *C.uint64_t) error {
	if t == nil || d == nil || countDev == nil || ntMax < 0 || ndMax < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_cmap_add(gpuCtx, t, C.size_t(ntMax), ntDev, d, C.size_t(ndMax), ndDev, out, countDev))
}

// CMapFromOps: m operations (opKey[i], opRep[i], +opDp[i], -opDn[i]) in any
// order, with repeats and any mix of replicas -- the log the replay walks
// (main.go:75-98) -- into the state whose cell (k, r) holds their sums (out of
// capacity m).  Synchronises once, for the device sort's plan.
func CMapFromOps(opKeyDev *C.uint64_t, opRepDev *C.uint32_t, opDpDev, opDnDev *C.uint64_t, m int, out *C.crdt_cmap,
	countDev *C.uint64_t) error {
	if out == nil || countDev == nil || m < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_cmap_from_ops(gpuCtx, opKeyDev, opRepDev, opDpDev, opDnDev, C.size_t(m), out, countDev))
}
