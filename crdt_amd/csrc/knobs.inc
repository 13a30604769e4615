// knobs.inc -- every kernel-shape knob: KNOB(variable, default, "name", valid(v)).
//
// The product library (libcrdt_amd.so) compiles each one as a constexpr at
// its default: the measured-slower variants behind non-default values fold
// away, crdt_set_option refuses every name, and no process-global mutable
// tuning state exists for two contexts to share.  The diagnostic build
// (libcrdt_amd_diag.so, -DCRDT_DIAG; tests and tools link it) makes them
// process-wide variables that crdt_set_option validates with valid(v).
// crdt_get_option reads the value in both builds.  DESIGN.md §5 records the
// measurement behind every default.
KNOB(g_join_unroll, 1, "join.unroll", v == 1 || v == 2 || v == 4 || v == 8)
KNOB(g_join_nontemporal, 1, "join.nontemporal", v == 0 || v == 1)
KNOB(g_join_blocks_per_cu, 2, "join.blocks_per_cu", v >= 1 && v <= 64)
KNOB(g_fold_unroll, 8, "fold.unroll", v == 1 || v == 2 || v == 4 || v == 8 || v == 16)
KNOB(g_fold_nontemporal, 1, "fold.nontemporal", v == 0 || v == 1)
KNOB(g_fold_blocks_per_cu, 1, "fold.blocks_per_cu", v >= 1 && v <= 64)
KNOB(g_vclock_pairs_per_wave, 32, "vclock.pairs_per_wave", v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32)
KNOB(g_vclock_blocks_per_cu, 1, "vclock.blocks_per_cu", v >= 1 && v <= 64)
KNOB(g_lww_chunk, 0, "sets.lww_chunk", v >= 0 && v <= 16384)
KNOB(g_or_chunk, 0, "sets.or_chunk", v >= 0 && v <= 16384)
KNOB(g_lww_parts, 4, "sets.lww_parts", v == 2 || v == 4 || v == 8 || v == 16)
KNOB(g_or_parts, 2, "sets.or_parts", v == 1 || v == 2 || v == 4)
KNOB(g_or_count_dma, 1, "sets.or_count_dma", v == 0 || v == 1)
KNOB(g_shard_exchange_always, 0, "shard.exchange_always", v == 0 || v == 1)
KNOB(g_shard_host_timing, 0, "shard.host_timing", v == 0 || v == 1)
KNOB(g_or_key_sort, 2, "sort.or_key_only", v >= 0 && v <= 2)
KNOB(g_sort_xcd, 1, "sort.xcd_tiles", v == 0 || v == 1)
KNOB(g_mm_bpc, 1, "sort.mm_blocks_per_cu", v >= 1 && v <= 16)
KNOB(g_rdd_diag, 0, "sort.rdd_diag", v >= 0 && v <= 8)
KNOB(g_lww_table, 1, "sort.lww_table", v == 0 || v == 1)
KNOB(g_or_table, 1, "sort.or_table", v == 0 || v == 1)
KNOB(g_sample_plan, 1, "sort.sample_plan", v == 0 || v == 1)
KNOB(g_lww_gather, 1, "sort.lww_gather", v == 0 || v == 1)
KNOB(g_or_bucket, 1, "sort.or_bucket", v == 0 || v == 1)
KNOB(g_or_place_batch, 1, "sort.or_place_batch", v == 0 || v == 1)
KNOB(g_up_threads, 512, "sort.up_threads", v == 256 || v == 512)
KNOB(g_group_tile, 4096, "sort.group_tile", v == 4096 || v == 8192)
KNOB(g_or_sub_hist, 1, "sort.or_sub_hist", v == 0 || v == 1)
KNOB(g_or_pair, 1, "sort.or_pair", v == 0 || v == 1)
KNOB(g_or_narrow, 1, "sort.or_narrow", v == 0 || v == 1)
KNOB(g_plan_cache, 2, "sort.plan_cache", v >= 0 && v <= 2)
KNOB(g_sample_min, 1 << 20, "sort.sample_min", v >= 0 && v <= 0x7FFFFFFF)
KNOB(g_or_lookback, 1, "sort.or_lookback", v == 0 || v == 1)
KNOB(g_sort_vec_up, 1, "sort.vec_up", v == 0 || v == 1)
KNOB(g_rm_affine, 1, "refmerge.affine_kv", v == 0 || v == 1)
KNOB(g_rm_count_dma, 1, "refmerge.count_dma", v == 0 || v == 1)
KNOB(g_rm_diag, 0, "refmerge.diag_fold", v >= 0 && v <= 5)
KNOB(g_short_tab, 3, "codec.short_tab", v >= 0 && v <= 4)
KNOB(g_dec_big_r, 4, "codec.big_r", v == 4 || v == 8)
KNOB(g_dec_small, 1, "codec.small", v >= 0 && v <= 3)
KNOB(g_pop_direct, 1, "pop.direct", v == 0 || v == 1)
KNOB(g_pop_wire_early, 1, "pop.wire_early", v == 0 || v == 1)
KNOB(g_read_poll, 1, "ctx.read_poll", v == 0 || v == 1)
KNOB(g_scan_items, 8, "scan.items", v == 4 || v == 8 || v == 16)
KNOB(g_tile_scan_round, 16384, "settile.scan_round", v == 1024 || v == 16384)
// Scratch fill (tests/test_gpu_ws_fill.py; DESIGN.md §5.22): a value >= 0 is the
// byte crdt_ctx_reserve writes over the whole workspace, and that a grown
// workspace or shard scratch starts from.  ctx.ws_filled_mb counts the MiB
// filled so far in the process (read it; setting it to 0 resets it).
KNOB(g_ws_fill, -1, "ctx.ws_fill", v >= -1 && v <= 255)
KNOB(g_ws_filled_mb, 0, "ctx.ws_filled_mb", v == 0)
