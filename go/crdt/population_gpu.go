//go:build cgo && rocm

// Device-level entry points for hosts whose replica state already lives in
// HBM (populations, sharded state), over the same C-ABI (include/crdt_amd.h).
// Uncompiled in the build image (no Go toolchain).
package crdt

/*
#include <stdlib.h>
#include "crdt_amd.h"
*/
import "C"

import (
	"bytes"
	"fmt"
	"log"
	"unsafe"
)

// GossipTick: one gossip tick for the replicas this process hosts
// (main.go:226-258).  Each binary pull is parked at ingest (validated on the
// host, its upload to HBM started); every ingested server merges in ONE
// batched device call.
func GossipTick(servers []*Server, bodies [][]byte) {
	hs := make([]*C.crdt_server, 0, len(servers))
	for i, s := range servers {
		if len(bodies[i]) == 0 {
			continue // a failed GET: no merge this round (main.go:234-239)
		}
		var out C.int
		C.crdt_server_ingest_binary(s.gpu, (*C.char)(unsafe.Pointer(&bodies[i][0])), C.size_t(len(bodies[i])), &out)
		if out == 0 {
			hs = append(hs, s.gpu)
		}
	}
	if len(hs) == 0 {
		return
	}
	if err := status(C.crdt_servers_merge(&hs[0], C.size_t(len(hs)))); err != nil {
		log.Printf("batched merge skipped, every server unchanged: %v", err) // (the next tick retries)
		return
	}
	for _, s := range servers {
		s.CurrentState = s.currentState()
	}
}

// GCounterJoin: a G-Counter population join on device pointers (crdt_dev_alloc).
func GCounterJoin(aDev, bDev, outDev unsafe.Pointer, rows, nodes int) error {
	return status(C.crdt_gcounter_join(gpuCtx, (*C.uint64_t)(aDev), (*C.uint64_t)(bDev), (*C.uint64_t)(outDev),
		C.size_t(rows), C.size_t(nodes)))
}

// UniqueID: rank 0 makes the RCCL id and ships it to the other ranks.
func UniqueID() ([]byte, error) {
	id := make([]byte, C.CRDT_SHARD_ID_BYTES)
	return id, status(C.crdt_shard_unique_id(unsafe.Pointer(&id[0]), C.size_t(len(id))))
}

// JoinPopulation: one process per GPU (the shape of bench.py --gpus N); each
// rank folds its row shard and one call all-reduces the folds over RCCL
// (ncclAllReduce(ncclUint64, ncclMax)): outDev = the global join.
func JoinPopulation(id []byte, nranks, rank int, shard unsafe.Pointer, rows, nodes int, outDev unsafe.Pointer) error {
	var comm *C.crdt_comm
	if err := status(C.crdt_shard_comm_init_rank(gpuCtx, unsafe.Pointer(&id[0]), C.int(nranks), C.int(rank), &comm)); err != nil {
		return err
	}
	defer C.crdt_shard_comm_destroy(comm)
	sh := []*C.uint64_t{(*C.uint64_t)(shard)}
	nr := []C.size_t{C.size_t(rows)}
	out := []*C.uint64_t{(*C.uint64_t)(outDev)}
	if err := status(C.crdt_shard_fold_max_u64(comm, &sh[0], &nr[0], C.size_t(nodes), &out[0])); err != nil {
		return err
	}
	return status(C.crdt_shard_sync(comm))
}

// MergeShardedBatch: merge() of one batch of replicas whose logs are split by
// ts range over the ranks -- the whole protocol (global max(L), local merge,
// accumulator all-reduces, finalize) on the communicator's stream.
func MergeShardedBatch(comm *C.crdt_comm, in *C.crdt_refmerge_in, out *C.crdt_refmerge_out) error {
	if err := status(C.crdt_shard_refmerge(comm, in, out)); err != nil {
		return err
	}
	return status(C.crdt_shard_sync(comm))
}

// GossipRound: the gossip loop of main.go:226-261 for all the replicas this
// rank hosts; every rank passes the same draw (friend ids, -1 = a dead
// friend, main.go:230, :234-239).  One call moves exactly the pulled Diffs
// over xGMI and merges.
func GossipRound(comm *C.crdt_comm, pop *C.crdt_population, draw []int64) error {
	pops := []*C.crdt_population{pop}
	return status(C.crdt_population_round_sharded(comm, &pops[0], (*C.int64_t)(unsafe.Pointer(&draw[0])),
		C.uint64_t(len(draw))))
}

func uploadBytes(b []byte) (unsafe.Pointer, error) {
	var dev unsafe.Pointer
	if err := status(C.crdt_dev_alloc(gpuCtx, C.size_t(len(b)), &dev)); err != nil || len(b) == 0 {
		return dev, err
	}
	if err := status(C.crdt_memcpy_h2d(gpuCtx, dev, unsafe.Pointer(&b[0]), C.size_t(len(b)))); err != nil {
		C.crdt_dev_free(gpuCtx, dev)
		return nil, err
	}
	return dev, nil
}

// GossipRoundWire: the same loop when the Diffs come over HTTP
// (main.go:231-256): bodies[i] is replica i's GET body (nil after a failed
// request), decoded and merged on the device; keys / vals are the context's
// string tables (vals seeded with the population's strings at their ids).
func GossipRoundWire(pop *C.crdt_population, keys, vals *C.crdt_strtab, bodies [][]byte) error {
	off := make([]uint64, len(bodies)+1)
	for i, b := range bodies {
		off[i+1] = off[i] + uint64(len(b))
	}
	dev, err := uploadBytes(bytes.Join(bodies, nil))
	if err != nil {
		return err
	}
	defer C.crdt_dev_free(gpuCtx, dev)
	st := make([]uint32, len(bodies))
	if rc := C.crdt_population_round_wire(pop, keys, vals, (*C.uint8_t)(dev), (*C.uint64_t)(unsafe.Pointer(&off[0])),
		(*C.uint32_t)(unsafe.Pointer(&st[0]))); rc != C.CRDT_OK {
		return fmt.Errorf("wire round refused (body status %v): %w", st, status(rc)) // decode those on the host
	}
	return nil
}

// MergeDistributedLWW: keyed sets of a distributed population -- this rank's
// own sorted LWW tuples (a, b); with gather every rank ends with the whole
// merged state in out.
func MergeDistributedLWW(comm *C.crdt_comm, a, b *C.crdt_tuples, na, nb int, out *C.crdt_tuples, capacity int) (int, error) {
	cna, cnb := []C.size_t{C.size_t(na)}, []C.size_t{C.size_t(nb)}
	n := []C.size_t{0}
	err := status(C.crdt_shard_lww_merge_local(comm, a, &cna[0], b, &cnb[0], out, C.size_t(capacity), &n[0], 1))
	return int(n[0]), err
}

// D2Merger: unsorted (D2) set state merged every round with no host
// synchronisation -- plan once per shape, then enqueue (also capturable in a
// HIP graph).  A call whose inputs leave the plan writes count = 2^64 - 1 and
// raises CRDT_DEV_PLAN: re-plan and run the unplanned call for that round.
type D2Merger struct {
	plan   C.crdt_set_plan
	na, nb C.size_t
}

func NewD2Merger(a, b *C.crdt_tuples, na, nb int) (*D2Merger, error) {
	m := &D2Merger{na: C.size_t(na), nb: C.size_t(nb)}
	// mode 0 = LWW; widen 1: field ranges padded by 1/256 of their span for drift
	err := status(C.crdt_set_merge_plan(gpuCtx, 0, a, m.na, b, m.nb, 1, &m.plan))
	return m, err
}

func (m *D2Merger) Enqueue(a, b, out *C.crdt_tuples, countDev *C.uint64_t) error {
	return status(C.crdt_lww_merge_unsorted_planned(gpuCtx, &m.plan, a, m.na, b, m.nb, out, countDev))
}

// SetElements: the live keys of a sorted set state already in HBM (what the
// reference serves as CurrentState on GET /data, main.go:129-139), ascending
// and each once into keysOutDev (capacity nMax keys), their number into
// countDev.  nDev (nil: nMax tuples) chains the read off a merge's device
// count with no read-back.  Enqueued: crdt_ctx_sync before reading.
func SetElements(lww bool, t *C.crdt_tuples, nMax int, nDev, keysOutDev, countDev *C.uint64_t) error {
	mode := C.int(C.CRDT_SET_ORSET)
	if lww {
		mode = C.int(C.CRDT_SET_LWW)
	}
	return status(C.crdt_set_elements(gpuCtx, mode, t, C.size_t(nMax), nDev, keysOutDev, countDev))
}

// SetCardinality: the number of live keys alone (one pass, no key output).
func SetCardinality(lww bool, t *C.crdt_tuples, nMax int, nDev, countDev *C.uint64_t) error {
	return SetElements(lww, t, nMax, nDev, nil, countDev)
}

// KeysContain: outDev[i] = 1 iff probesDev[i] is among the first *nDev (nil:
// nMax) of the ascending keys SetElements wrote.
func KeysContain(keysDev *C.uint64_t, nMax int, nDev, probesDev *C.uint64_t, m int, outDev *C.uint8_t) error {
	return status(C.crdt_u64_contains(gpuCtx, keysDev, C.size_t(nMax), nDev, probesDev, C.size_t(m), outDev))
}

// MapRead: the map a sorted set state holds beside a value column -- one row
// per member key (SetElements' keys, ascending): the key into keysOutDev (may
// be nil), the index in t of the first copy of the key's winner tag into
// winOutDev (LWW: the maximal tag; OR-Set: the greatest live tag) and the
// number of distinct live tags into nsibOutDev (may be nil; LWW: 1; > 1: the
// key is multi-valued), each of capacity nMax rows; their number into
// countDev.  winOutDev is SrcGather's a-side encoding: gather the value column
// by it with countDev as the device length.  Enqueued: crdt_ctx_sync before
// reading.
func MapRead(lww bool, t *C.crdt_tuples, nMax int, nDev, keysOutDev *C.uint64_t, winOutDev *C.int64_t,
	nsibOutDev *C.uint32_t, countDev *C.uint64_t) error {
	mode := C.int(C.CRDT_SET_ORSET)
	if lww {
		mode = C.int(C.CRDT_SET_LWW)
	}
	return status(C.crdt_map_read(gpuCtx, mode, t, C.size_t(nMax), nDev, keysOutDev, winOutDev, nsibOutDev, countDev))
}

// MapLookup: MapRead's row of each of the m probe keys in probesDev (any
// order, duplicates allowed): winOutDev[i] = the win of probesDev[i], or -1
// when the key is not a member; nsibOutDev (may be nil) its sibling count, 0
// for a non-member.  To SrcGather -1 is element 0 of the b side: a one-element
// b column is the default of the missing keys.  No probes (m == 0, the device
// pointers may then be nil) enqueue nothing.
func MapLookup(lww bool, t *C.crdt_tuples, nMax int, nDev, probesDev *C.uint64_t, m int, winOutDev *C.int64_t,
	nsibOutDev *C.uint32_t) error {
	if m == 0 {
		return nil
	}
	mode := C.int(C.CRDT_SET_ORSET)
	if lww {
		mode = C.int(C.CRDT_SET_LWW)
	}
	return status(C.crdt_map_lookup(gpuCtx, mode, t, C.size_t(nMax), nDev, probesDev, C.size_t(m), winOutDev, nsibOutDev))
}

// SetDelta: the tuples of the sorted set state src that dst lacks -- the
// smallest D with merge(dst, D) == merge(dst, src), dst the tie-winning side --
// in ascending order into out (capacity nsMax tuples), their number into
// countDev.  What a gossip pull needs to ship instead of the entire Diff
// (main.go:153-170, :245-256).  nsDev / ndDev (nil: all nMax tuples of the
// side) chain the call off device counts with no read-back.  An empty src
// (nsMax == 0) stores a count of 0 and touches neither side.  Enqueued:
// crdt_ctx_sync before reading.
func SetDelta(lww bool, src *C.crdt_tuples, nsMax int, nsDev *C.uint64_t, dst *C.crdt_tuples, ndMax int,
	ndDev *C.uint64_t, out *C.crdt_tuples, countDev *C.uint64_t) error {
	if src == nil || dst == nil || countDev == nil || nsMax < 0 || ndMax < 0 {
		return status(C.CRDT_E_INVAL)
	}
	mode := C.int(C.CRDT_SET_ORSET)
	if lww {
		mode = C.int(C.CRDT_SET_LWW)
	}
	return status(C.crdt_set_delta(gpuCtx, mode, src, C.size_t(nsMax), nsDev, dst, C.size_t(ndMax), ndDev, out, countDev))
}

// SetDeltaCount: the size of that delta alone (nothing stored but the count);
// 0 iff dst already holds all of src -- the in-sync test of an anti-entropy loop.
func SetDeltaCount(lww bool, src *C.crdt_tuples, nsMax int, nsDev *C.uint64_t, dst *C.crdt_tuples, ndMax int,
	ndDev, countDev *C.uint64_t) error {
	return SetDelta(lww, src, nsMax, nsDev, dst, ndMax, ndDev, nil, countDev)
}

// StableCut: the causal-stability cut of a [rows x nodes] uint64 vector-clock
// population in HBM -- outDev[c] = the minimum over the rows of column c, the
// number of node c's events every replica has seen.  What SetCompact takes as
// its cut.  rows == 0 is an error (the minimum over no replica is all-ones:
// every tombstone would be droppable).  Enqueued: crdt_ctx_sync before reading.
func StableCut(clocksDev *C.uint64_t, rows, nodes int, outDev *C.uint64_t) error {
	if rows <= 0 || nodes <= 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_vclock_stable_cut(gpuCtx, clocksDev, C.size_t(rows), C.size_t(nodes), outDev))
}

// SetCompact: the sorted set state t without its stable dead tuples --
// merge(t, {}) minus every OR-Set tag whose copies' tomb-OR is 1, and every
// LWW key whose winner is a tombstone, that is stable under the cut: rep <
// nCut and ts <= cutDev[rep].  The reference's Diff only grows; this is the
// pass that lets a long-running replica shed tombstones.  The caller vouches
// that the cut covers the remove as well as the add: every replica already
// holds the tombstone of every tag the cut makes stable.  The kept tuples go
// to out in ascending order (capacity nMax), their number to countDev;
// srcOutDev (nil: not wanted; capacity nMax) receives per output tuple the
// index in t of the tuple it is (the first copy of its tag), for GatherSrc
// with bColDev nil.  cutDev nil with nCut 0: no cut, the result is merge(t,
// {}).  nDev (nil: nMax tuples) chains the call off a merge's device count
// with no read-back.  Enqueued: crdt_ctx_sync before reading.
func SetCompact(lww bool, t *C.crdt_tuples, nMax int, nDev *C.uint64_t, cutDev *C.uint64_t, nCut int,
	out *C.crdt_tuples, srcOutDev *C.int64_t, countDev *C.uint64_t) error {
	if t == nil || countDev == nil || nMax < 0 || nCut < 0 {
		return status(C.CRDT_E_INVAL)
	}
	mode := C.int(C.CRDT_SET_ORSET)
	if lww {
		mode = C.int(C.CRDT_SET_LWW)
	}
	return status(C.crdt_set_compact(gpuCtx, mode, t, C.size_t(nMax), nDev, cutDev, C.size_t(nCut), out, srcOutDev, countDev))
}

// SetCompactCount: the size of that compaction alone (nothing stored but the
// count) -- how much a compaction under this cut would free.
func SetCompactCount(lww bool, t *C.crdt_tuples, nMax int, nDev *C.uint64_t, cutDev *C.uint64_t, nCut int,
	countDev *C.uint64_t) error {
	return SetCompact(lww, t, nMax, nDev, cutDev, nCut, nil, nil, countDev)
}

// OrsetMergeCausal: the merge of two tombstone-free OR-Set states, each a pair
// of sorted tuples and a causal context (ctxDev[r] = the events of replica r
// the state has seen).  A tag survives iff both sides hold it present (a copy,
// none tombstoned), or one side does and the other side's context does not
// cover it (rep < nCtx and ts <= ctxDev[rep]): a side whose context covers a
// tag it does not hold has seen and removed it.  No tombstone is kept and no
// population-wide cut is needed, where SetCompact needs StableCut over every
// replica's clock.  The surviving tags go to out in ascending order, tomb 0
// (capacity naMax + nbMax), their number to countDev; srcOutDev (nil: not
// wanted; same capacity) receives per output tuple the first copy of its tag
// on a side that holds it present, a before b, in OrsetMergeSrc's encoding,
// for GatherSrc; ctxOutDev (nil: not wanted; max(nCtxA, nCtxB) entries) the
// element-wise maximum of the contexts.  naDev / nbDev (nil: all nMax tuples of
// the side) chain the call off device counts with no read-back.  The caller
// vouches that each context covers its own state's present tags and is
// contiguous.  Enqueued: crdt_ctx_sync before reading.
func OrsetMergeCausal(a *C.crdt_tuples, naMax int, naDev, ctxADev *C.uint64_t, nCtxA int, b *C.crdt_tuples, nbMax int,
	nbDev, ctxBDev *C.uint64_t, nCtxB int, out *C.crdt_tuples, srcOutDev *C.int64_t, ctxOutDev, countDev *C.uint64_t) error {
	if a == nil || b == nil || countDev == nil || naMax < 0 || nbMax < 0 || nCtxA < 0 || nCtxB < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_orset_merge_causal(gpuCtx, a, C.size_t(naMax), naDev, ctxADev, C.size_t(nCtxA), b, C.size_t(nbMax),
		nbDev, ctxBDev, C.size_t(nCtxB), out, srcOutDev, ctxOutDev, countDev))
}

// OrsetMergeCausalCount: the size of that merge alone (nothing stored but the
// count) -- the live tags the two replicas hold between them.
func OrsetMergeCausalCount(a *C.crdt_tuples, naMax int, naDev, ctxADev *C.uint64_t, nCtxA int, b *C.crdt_tuples, nbMax int,
	nbDev, ctxBDev *C.uint64_t, nCtxB int, countDev *C.uint64_t) error {
	return OrsetMergeCausal(a, naMax, naDev, ctxADev, nCtxA, b, nbMax, nbDev, ctxBDev, nCtxB, nil, nil, nil, countDev)
}

// OrsetMergeCausalRanges: OrsetMergeCausal of the receiver's whole causal state
// a with what a peer shipped for the key ranges whose digests differ -- b is
// normally SetSelect(B, OR-Set, splittersDev, flagsDev), nbDev its countDev,
// ctxBDev the peer's whole context.  The causal merge is not monotone (a tag a
// holds and b's context covers is dropped unless b's copy is in the operand),
// so the buckets come along: SetDigest's, bucket(key) = the number of splitters
// <= key, m + 1 flags.  In a flagged bucket OrsetMergeCausal's rule applies
// unchanged; in an unflagged one b is taken to hold what a holds -- a tag
// survives iff a holds it present, b's copies there are ignored entirely and
// neither context is read.  Every flag set equals OrsetMergeCausal(a, b) bit
// for bit; no flag set gives a's present tags.  Not symmetric in a and b: run
// it in both directions and both replicas hold merge(A, B).  The caller
// vouches that the replicas' canonical tuples are equal in every unflagged
// bucket (what equal digests say).  Everything else as OrsetMergeCausal.
// Enqueued: crdt_ctx_sync before reading.
func OrsetMergeCausalRanges(a *C.crdt_tuples, naMax int, naDev, ctxADev *C.uint64_t, nCtxA int, b *C.crdt_tuples, nbMax int,
	nbDev, ctxBDev *C.uint64_t, nCtxB int, splittersDev *C.uint64_t, m int, flagsDev *C.uint8_t, out *C.crdt_tuples,
	srcOutDev *C.int64_t, ctxOutDev, countDev *C.uint64_t) error {
	if a == nil || b == nil || flagsDev == nil || countDev == nil || naMax < 0 || nbMax < 0 || nCtxA < 0 || nCtxB < 0 || m < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_orset_merge_causal_ranges(gpuCtx, a, C.size_t(naMax), naDev, ctxADev, C.size_t(nCtxA), b,
		C.size_t(nbMax), nbDev, ctxBDev, C.size_t(nCtxB), splittersDev, C.size_t(m), flagsDev, out, srcOutDev, ctxOutDev,
		countDev))
}

// OrsetMergeCausalRangesCount: the size of that merge alone (nothing stored
// but the count).
func OrsetMergeCausalRangesCount(a *C.crdt_tuples, naMax int, naDev, ctxADev *C.uint64_t, nCtxA int, b *C.crdt_tuples,
	nbMax int, nbDev, ctxBDev *C.uint64_t, nCtxB int, splittersDev *C.uint64_t, m int, flagsDev *C.uint8_t,
	countDev *C.uint64_t) error {
	return OrsetMergeCausalRanges(a, naMax, naDev, ctxADev, nCtxA, b, nbMax, nbDev, ctxBDev, nCtxB, splittersDev, m, flagsDev,
		nil, nil, nil, countDev)
}

// SetApply: a batch of local adds and removes applied to the sorted OR-Set
// state t of replica rep on the device -- the local write (AddCommand,
// main.go:173-207) for the OR-Set, in the tombstone form (causal false: a
// remove sets tomb = 1 on the key's tags) or the causal form (causal true: a
// remove deletes them, every output tomb 0).  clockDev is rep's clock row /
// causal context (nClock entries); opKeyDev (non-decreasing) and opKindDev (0 =
// add, else remove) hold the m operations.  Operation i is rep's event
// clock[rep] + 1 + i, add and remove alike; the result is the batch applied one
// operation at a time, each tag once in ascending order (capacity nMax + m),
// its length to countDev.  srcOutDev (nil: not wanted; same capacity) names per
// output tuple the tag's first copy in t (>= 0) or the add at batch index i as
// -(i + 1), for GatherSrc; clockOutDev (nil: not wanted; nClock entries) is the
// clock with [rep] advanced by m.  nDev (nil: all nMax tuples) chains the call
// off a device count.  The caller vouches that every tag of rep in t has ts <=
// clock[rep] and that the keys are sorted.  Enqueued: crdt_ctx_sync before
// reading.
func SetApply(causal bool, t *C.crdt_tuples, nMax int, nDev, clockDev *C.uint64_t, nClock int, rep uint32,
	opKeyDev *C.uint64_t, opKindDev *C.uint8_t, m int, out *C.crdt_tuples, srcOutDev *C.int64_t,
	clockOutDev, countDev *C.uint64_t) error {
	if t == nil || clockDev == nil || countDev == nil || nMax < 0 || nClock < 0 || m < 0 {
		return status(C.CRDT_E_INVAL)
	}
	form := C.int(C.CRDT_APPLY_TOMBSTONE)
	if causal {
		form = C.int(C.CRDT_APPLY_CAUSAL)
	}
	return status(C.crdt_set_apply(gpuCtx, form, t, C.size_t(nMax), nDev, clockDev, C.size_t(nClock), C.uint32_t(rep),
		opKeyDev, opKindDev, C.size_t(m), out, srcOutDev, clockOutDev, countDev))
}

// SetApplyCount: the size of that state alone (nothing stored but the count
// and, when asked, the advanced clock).
func SetApplyCount(causal bool, t *C.crdt_tuples, nMax int, nDev, clockDev *C.uint64_t, nClock int, rep uint32,
	opKeyDev *C.uint64_t, opKindDev *C.uint8_t, m int, clockOutDev, countDev *C.uint64_t) error {
	return SetApply(causal, t, nMax, nDev, clockDev, nClock, rep, opKeyDev, opKindDev, m, nil, nil, clockOutDev, countDev)
}

// SetDigest: one order-independent fingerprint per key range of the sorted set
// state t -- hashOutDev[b] = the wrapping sum of the tuple hash over the
// tuples of merge(t, {}) whose key falls into bucket b, countOutDev[b] their
// number, for the m + 1 buckets the ascending splittersDev cut the key space
// into (bucket(key) = the number of splitters <= key; m == 0 with a nil
// splittersDev: one bucket).  Two replicas exchange these 16 bytes a range
// instead of their state (the reference's pull ships the entire Diff,
// main.go:153-170, :245-256), SetDigestDiff flags the ranges that differ and
// SetSelect ships those alone.  The tuple hash is spelt out in crdt_amd.h so
// that a host in any language reproduces it.  nDev (nil: nMax tuples) chains
// the call off a merge's device count.  Enqueued: crdt_ctx_sync before reading.
func SetDigest(lww bool, t *C.crdt_tuples, nMax int, nDev *C.uint64_t, splittersDev *C.uint64_t, m int,
	hashOutDev, countOutDev *C.uint64_t) error {
	if t == nil || hashOutDev == nil || countOutDev == nil || nMax < 0 || m < 0 {
		return status(C.CRDT_E_INVAL)
	}
	mode := C.int(C.CRDT_SET_ORSET)
	if lww {
		mode = C.int(C.CRDT_SET_LWW)
	}
	return status(C.crdt_set_digest(gpuCtx, mode, t, C.size_t(nMax), nDev, splittersDev, C.size_t(m), hashOutDev, countOutDev))
}

// SetDigestDiff: flagsOutDev[b] = 1 iff the digests a and b differ in bucket b
// (hash or count; a poisoned digest, count ~0, flags every bucket), for
// nBuckets buckets; their number to nDiffDev.  Enqueued.
func SetDigestDiff(hashADev, countADev, hashBDev, countBDev *C.uint64_t, nBuckets int, flagsOutDev *C.uint8_t,
	nDiffDev *C.uint64_t) error {
	if nBuckets < 0 || nDiffDev == nil {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_set_digest_diff(gpuCtx, hashADev, countADev, hashBDev, countBDev, C.size_t(nBuckets), flagsOutDev,
		nDiffDev))
}

// SetSelect: the tuples of merge(t, {}) in the buckets with flagsDev[b] != 0
// (m + 1 flags over SetDigest's buckets), ascending, into out (capacity nMax),
// their number to countDev: what a replica ships for the differing ranges.
// srcOutDev (nil: not wanted) as in SetCompact, for GatherSrc with bColDev
// nil.  out nil (srcOutDev nil too): the count alone.  Enqueued.
func SetSelect(lww bool, t *C.crdt_tuples, nMax int, nDev *C.uint64_t, splittersDev *C.uint64_t, m int,
	flagsDev *C.uint8_t, out *C.crdt_tuples, srcOutDev *C.int64_t, countDev *C.uint64_t) error {
	if t == nil || flagsDev == nil || countDev == nil || nMax < 0 || m < 0 {
		return status(C.CRDT_E_INVAL)
	}
	mode := C.int(C.CRDT_SET_ORSET)
	if lww {
		mode = C.int(C.CRDT_SET_LWW)
	}
	return status(C.crdt_set_select(gpuCtx, mode, t, C.size_t(nMax), nDev, splittersDev, C.size_t(m), flagsDev, out, srcOutDev,
		countDev))
}

// LWWMergeSrc: crdt_lww_merge of two sorted set states in HBM that also names,
// for every output tuple, the input tuple it is -- srcOutDev[i] >= 0: a's tuple
// of that index; < 0: b's tuple j as -(j+1) -- the first element in merged
// order (a's copies of an equal tag before b's) carrying the key's maximal
// (ts, rep).  What a host that keeps a value beside each key needs (the
// reference Puts the value with its key, main.go:60-64 and :187): GatherSrc
// then moves the value columns.  out and srcOutDev hold na + nb entries; out
// and countDev are the plain merge's bit for bit.  Enqueued.
func LWWMergeSrc(a *C.crdt_tuples, na int, b *C.crdt_tuples, nb int, out *C.crdt_tuples, srcOutDev *C.int64_t,
	countDev *C.uint64_t) error {
	if na < 0 || nb < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_lww_merge_src(gpuCtx, a, C.size_t(na), b, C.size_t(nb), out, srcOutDev, countDev))
}

// ORSetMergeSrc: crdt_orset_merge likewise; the source of a tag's output is
// the tag's first element in merged order (its tomb stays the OR over all
// copies, so it may be 1 where the source's is 0).
func ORSetMergeSrc(a *C.crdt_tuples, na int, b *C.crdt_tuples, nb int, out *C.crdt_tuples, srcOutDev *C.int64_t,
	countDev *C.uint64_t) error {
	if na < 0 || nb < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_orset_merge_src(gpuCtx, a, C.size_t(na), b, C.size_t(nb), out, srcOutDev, countDev))
}

// GatherSrc: outColDev[i] = aColDev[src[i]] (src[i] >= 0) or bColDev[-(src[i]+1)]
// for the first *nDev (nil: nMax) source indices, elements of elemSize 1, 2,
// 4, 8 or 16 bytes: one payload column moved by a merge's source indices, one
// call per column.  Pass the merge's countDev as nDev: no read-back between
// the merge and the gather.  An index outside its side leaves its output
// element as it was and raises CRDT_DEV_RANGE, as does *nDev > nMax (nothing
// touched).  Enqueued: crdt_ctx_sync before reading.
func GatherSrc(srcDev *C.int64_t, nMax int, nDev *C.uint64_t, aColDev unsafe.Pointer, na int, bColDev unsafe.Pointer,
	nb int, outColDev unsafe.Pointer, elemSize int) error {
	if nMax < 0 || na < 0 || nb < 0 || elemSize < 0 {
		return status(C.CRDT_E_INVAL)
	}
	return status(C.crdt_src_gather(gpuCtx, srcDev, C.size_t(nMax), nDev, aColDev, C.size_t(na), bColDev, C.size_t(nb),
		outColDev, C.size_t(elemSize)))
}

// RCCLInfo: which RCCL the process runs (for the service's logs / metrics).
func RCCLInfo() (int, string) {
	var v C.int
	buf := make([]byte, 512)
	if status(C.crdt_rccl_info(&v, (*C.char)(unsafe.Pointer(&buf[0])), 512)) != nil {
		return 0, ""
	}
	return int(v), C.GoString((*C.char)(unsafe.Pointer(&buf[0])))
}
