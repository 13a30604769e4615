"""The table of tests/test_gpu_ws_fill.py as plain data: every row's id, the
kernel files whose scratch it exercises, and its shape.  Host only (nothing is
imported), so tests/test_ws_fill_table.py can hold the table against
crdt_amd/csrc without a GPU: a kernel file that carves the workspace and is
named by no row fails there.

Tile sizes (read from the code): kTile = 2048 tuples (settile.hpp: reads,
deltas, compaction, digests, causal, apply, map reads), LT = 4096 and
OT = 2048 merged items (sets.hip: LWW / OR-Set merges), MT = 4096 merge items
(refmerge.hip), 2048 items per look-back scan tile (scan.hpp).  A row's main
shape is three full tiles and a partial one of its kernel."""

T = 2048                      # kTile, OT, the scan tile
LT = 4096                     # LWW merge tile; MT of refmerge
N_SET = 3 * T + 17            # one state: 6161 tuples
N_DEV = 2 * T + 5             # a device count below the buffer: the last tile is never written
NA, NB = 7000, 3 * LT + 17 - 7000   # two sides, 12305 merged items: 3 LT tiles + 17 (6 OT tiles + 17)
N_SORT = 12_000

# (id, kernel files, shape)
ROWS = [
    # sorted merges
    ("lww_orset_merge", ("sets.hip", "settile.hpp"), f"na {NA} nb {NB}"),
    ("lww_orset_merge_one", ("sets.hip", "settile.hpp"), "na 0 nb 1, na 1 nb 0"),
    ("merge_src", ("sets.hip", "settile.hpp"), f"na {NA} nb {NB}"),
    ("merge_src_one", ("sets.hip", "settile.hpp"), "na 0 nb 1, na 1 nb 0"),
    ("map_merge", ("sets.hip", "settile.hpp"), f"na {NA} nb {NB}, gather off the device count"),
    ("tuples_merge", ("sets.hip",), f"na {NA} nb {NB}; na 0 nb 1"),
    # set reads, map reads, deltas, compaction: host length, then a device count below the buffer
    ("set_read", ("setread.hip", "settile.hpp"), f"n {N_SET}; n 1"),
    ("set_read_ndev", ("setread.hip", "settile.hpp"), f"buffer {N_SET}, device count {N_DEV}"),
    ("map_read", ("mapread.hip", "settile.hpp"), f"n {N_SET}; n 1"),
    ("map_read_ndev", ("mapread.hip", "settile.hpp"), f"buffer {N_SET}, device count {N_DEV}"),
    ("set_delta", ("setdelta.hip", "settile.hpp"), f"src {NA} dst {NB}; src 1 dst 0; src 0 dst 1"),
    ("set_delta_ndev", ("setdelta.hip", "settile.hpp"), f"buffers {NA} / {NB}, device counts {N_DEV} / {N_DEV - 100}"),
    ("set_compact", ("setcompact.hip", "settile.hpp"), f"n {N_SET}; n 1"),
    ("set_compact_ndev", ("setcompact.hip", "settile.hpp"), f"buffer {N_SET}, device count {N_DEV}"),
    # digests and selections
    ("set_digest", ("setdigest.hip", "settile.hpp"), f"n {N_SET}, 63 splitters; device count {N_DEV}; n 1"),
    ("digest_diff", ("setdigest.hip",), "1000 buckets"),
    ("set_select", ("setdigest.hip", "settile.hpp"), f"n {N_SET}, 63 splitters; device count {N_DEV}; n 1"),
    ("reconcile_round_lww", ("setdigest.hip", "setdelta.hip", "sets.hip", "settile.hpp"),
     "two 40000-tuple states, 63 splitters"),
    ("reconcile_round_orset", ("setdigest.hip", "setdelta.hip", "sets.hip", "settile.hpp"),
     "two 40000-tuple states, 63 splitters"),
    # causal OR-Set and mutators
    ("causal_merge", ("setcausal.hip", "settile.hpp"), f"na {NA} nb {NB}; na 0 nb 1"),
    ("causal_merge_ranges", ("setcausal.hip", "settile.hpp"), f"na {NA}, b buffer {NB} with n_b_dev {N_DEV}, 7 splitters"),
    ("set_apply", ("setapply.hip", "settile.hpp"), f"n {N_SET - 700} + 700 operations, both forms; device count {N_DEV}"),
    # sort and unsorted merges
    ("sort_tuples", ("sort.hip",), f"n {N_SORT}: one-, two- and three-word composites"),
    ("merge_unsorted", ("sort.hip",), f"na {N_SORT} nb {N_SORT - 1000}, both modes; na 0 nb 1"),
    ("merge_unsorted_planned", ("sort.hip",), f"na {N_SORT} nb {N_SORT - 1000}, a plan made before the fill"),
    # counters and clocks
    ("gcounter_fold", ("counters.hip",), "300 x 64 (5 partial blocks), 300 x 63 (300 partial blocks)"),
    ("vclock_stable_cut", ("stable.hip",), "300 x 64, 300 x 63"),
    ("counter_values", ("counters.hip",), "gcounter_value / pncounter_value: 300 x 64, 33 x 7"),
    # RefMerge
    ("refmerge_batch", ("refmerge.hip",), "3 replicas, L and R of about 6200 entries each (3 MT tiles + a partial per replica)"),
    ("refmerge_batch_kv", ("refmerge.hip",), "the same batch with the kv output"),
    ("refmerge_pull", ("refmerge.hip",), "12 replicas x 2000 entries a side, R read in place from a peer's L, slots re-based"),
    ("refmerge_delta", ("refmerge.hip",), "3 replicas, L and R of about 6200 entries each, after replay_state_init"),
    ("refmerge_small_plan", ("refmerge.hip",), "65536 replicas x 12 entries: the single-workgroup plan"),
    ("refmerge_large_plan", ("refmerge.hip",), "65537 replicas x 12 entries (the same batch and its last replica): the multi-kernel plan"),
    ("refmerge_lds_overflow", ("refmerge.hip",), "replicas of 2500 / 40 / 3000 distinct keys, 4000 entries each"),
    # gossip, codec, local apply
    ("seg_ops", ("gossip.hip", "scan.hpp"), f"counts_to_offsets n {N_SET}; seg_offsets / gather2 {N_SET} segments; copy2 700 segments"),
    ("local_apply", ("local.hip", "gossip.hip"), "9 replicas, 3 rounds of up to 24 commands each"),
    ("gossip_decode", ("codec.hip",), "11 bodies of up to 60 entries, 4-entry string tables that grow"),
    ("population_round", ("population.hip", "codec.hip", "refmerge.hip"), "9 replicas, 6 rounds, random and reference draws"),
    # sharded protocols, loopback(0, 3): every member's scratch and workspace filled before each call
    ("shard_set_merge_local", ("shard.hip", "sets.hip"), "sizes (0, 4000) (5000, 1) (2200, 0): gather, ranges, device counts"),
    ("shard_refmerge", ("shard.hip", "refmerge.hip"), "40 replicas x 2500 entries over 3 ts-range shards"),
]

# Files that only declare or implement the reservation itself.
NOT_KERNELS = {
    "capi.hip": "defines ws_reserve, crdt_ctx_reserve and the fill",
    "common.hpp": "declares ws_reserve",
}

# Part 3: (first family, the family run between its calls).  The second is
# chosen so that its carve (TileWs::reserve: [split] tcnt [rec] ic bits) lays
# other arrays over the first's: the merges and set_apply carve a split array
# and no rec, causal merge and delta both, reads / map reads / compaction a
# rec and no split, digests and selections neither, and the bitmap words per
# tile differ (1, 2 or 3 x the tile's words); sort, D2 and RefMerge lay
# min-max blocks, plans, histograms and tuple buffers over all of them.
SEQUENCES = [
    ("lww_orset_merge", "set_read"),
    ("merge_src", "map_read"),
    ("set_read", "lww_orset_merge"),
    ("map_read", "set_apply"),
    ("set_delta", "set_digest"),
    ("set_compact", "causal_merge"),
    ("set_digest", "set_apply"),
    ("set_select", "set_delta"),
    ("causal_merge", "map_read"),
    ("set_apply", "set_select"),
    ("sort_tuples", "lww_orset_merge"),
    ("merge_unsorted", "set_read"),
    ("refmerge_batch", "merge_unsorted"),
    ("lww_orset_merge", "refmerge_batch"),
]
