/*
 * mhx.h — C ABI of libmhx.so: MI355X-native SdBG construction (MEGAHIT's `count`,
 * `read2sdbg`, `seq2sdbg` hot path) as hand-written HIP kernels for gfx950.
 *
 * The reference (voutcn/megahit v1.2.9) has no FFI for this path; its seams are
 *   B1  the CLI  `megahit_core count|read2sdbg|seq2sdbg`  (src/main_sdbg_build.cpp:35-224),
 *   B2  the engine template method BaseSequenceSortingEngine::Run + six virtuals
 *       (src/sorting/base_engine.h:221-233,256),
 *   B3  the sort functor SelectSortingFunc (src/sorting/kmsort_selector.h:7).
 * Each entry point below names the reference interface it replaces.  The product CLI
 * (megahit_amd/csrc/host/mhx_core.cpp) sits on exactly these symbols and keeps B1's flags
 * and on-disk formats, so `megahit` (the Python orchestrator) and `megahit_core assemble`
 * consume the output unchanged.
 *
 * Conventions: plain C, opaque handle, int status (0 = ok, <0 = error, text via
 * mhx_last_error()), no exceptions cross the boundary, the caller owns every host buffer,
 * the library owns device memory.  One handle drives one GPU and one HIP stream; it is not
 * thread-safe (use one handle per thread).  All integers little-endian native.
 *
 * Packed sequences: uint32 words, base i of the concatenation of all sequences lives in word
 * i/16 at bits 31-2(i%16)..30-2(i%16) (A,C,G,T = 0..3), no padding between sequences — the
 * layout of SequencePackage (reference src/sequence/sequence_package.h:38-320).
 */
#ifndef MHX_H
#define MHX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHX_NUM_BUCKETS 65536 /* reference src/sorting/base_engine.h:21 */
#define MHX_MAX_MUL 65535     /* reference src/sdbg/sdbg_def.h:12 */
#define MHX_MAX_K 255         /* reference src/sdbg/sdbg_def.h:20 */

typedef struct mhx_ctx mhx_ctx;

/* ---- lifetime / errors ---- */
const char *mhx_last_error(void);
const char *mhx_version(void);
/* number of visible HIP devices, <0 on error */
int mhx_device_count(void);
/* device: HIP ordinal.  Fails (returns NULL, message in mhx_last_error) when no GPU / no
 * gfx950 code object is usable — there is no CPU fallback. */
mhx_ctx *mhx_create(int device);
void mhx_destroy(mhx_ctx *);
/* release cached device workspaces (they are otherwise kept between calls).  A bucket filter is switched off with its tables; the
   aggregated stage-2 items of the last stage 1 stay: the next stage 2 reads them. */
int mhx_trim(mhx_ctx *);
/* forget inputs, results, partition, filters and options, keep the device buffers: the next job starts as on a new
   handle without re-allocating (what `mhx_core --serve` does between two sub-programs) */
int mhx_reset(mhx_ctx *);
int mhx_synchronize(mhx_ctx *);
/* Tuning / diagnostic knobs of one handle (never needed for correct results).  A knob that was not set falls back to
 * the environment variable MHX_<NAME IN UPPER CASE>, then to its built-in default.  Known names:
 *   s1_seg (1)        0: stage 1 always sorts fully and reduces with the tile kernel (no segment group-by)
 *   s1_seg_bits (0)   force the prefix width of the partial stage-1 sort (0 = chosen from the item count)
 *   s1_seg_la (3)     look-ahead chunks of the segment group-by before a tile gives up (-> classic path)
 *   s1_seg_per (8)    records per thread and tile of the segment group-by (4 or 8)
 *   s1_stream (1)     0: never the bucket-streaming group-by (k_s1_stream).  Its sort prefix follows the job's density
 *                     (records per lv1 bucket where the group-by runs): s1_stream_max (40000) records per streamed
 *                     bucket at most — 16 prefix bits in two passes up to that, 2^s sub-rounds per bucket up to
 *                     2^s1_stream_sub_max (1) times that, 17..24 bits in three passes beyond (their
 *                     width aims at s1_stream_max3 = s1_stream_max / 2 records per bucket: a third pass costs the same at any width); s1_stream_bits (0) /
 *                     s1_stream_sub0 (-1) force the prefix width / the sub-rounds (tests; on several ranks the width is at
 *                     least 16 bits: the owners' slices are cut at lv1 bucket bounds); s1_stream_fill: keys a
 *                     round's table may end up with before the round is redone in two halves (7/8 of the table); s1_stream_probes (1024; the kernel looks at no more than 128 slots per insert)
 *   s1_filter_in_gen (1)  0: a bucket filter (memory plan) is applied to stage 1 by extraction batches + a keep/drop
 *                     split even where the generating first sort pass could leave the dropped buckets out itself
 *   s1_pos_bits (0)   width of the position word of compact stage-1 records (0 = 32); the position bits above it ride
 *                     as a tag in the key words (s1.hip s1_pos_tag).  Tests use narrow words to exercise the tags.
 *   s1_stream_direct (1)  0: k_s1_stream always reads a bucket twice (second time to mark); 1: when the marks are those of
 *                     the non-solid occurrences and m <= 2 they come from the table and the second read is skipped
 *   count_seg (1), count_seg_bits (0), count_seg_la (3)  the same for count (k_count_seg)
 *   count_extract_fixed (1)  0: count's items always come from the wave-per-read kernel (no fused digit histograms)
 *   dist_sparse_marks (0)  multi-GPU stage 1 emits MHX_ROUTE_S1_MARKS records instead of marking a bitmap of the
 *                     global read set (set by mhx_dist_setup)
 *   kmsort_emu_legacy (0)  1: read2sdbg --need_mercy replays kmsort with one thread per lv1 bucket on whole records
 *                     (round 1) instead of one wave per bucket on tags + indices (kmsort_emu.hip); same output
 *   sort_xcd_units (1)  0: the chained-scan scatter hands its units out from one ticket counter instead of one per
 *                     block-id class b % 8 (sort.hip); same output
 * Returns <0 for a NULL handle/name. */
int mhx_set_option(mhx_ctx *, const char *name, long long value);
/* The value a knob has for this handle: an explicit mhx_set_option, else the environment variable MHX_<NAME>, else the
 * installation's tuned default — a `name = value` line of mhx_tuning.conf beside libmhx.so (MHX_TUNING_FILE names another
 * file, MHX_NO_TUNING=1 ignores it; written by tools/ab_options.py --write-tuning from an A/B on the box; read once, at
 * mhx_create) — else `dflt`.  Knobs only ever choose between code paths with identical results.  (The library's own reads
 * take the default in parentheses below, declared once in megahit_amd/csrc/mhx_options.h.)  Round 3:
 *   sort_unit_runs (1)     0: the chained-scan pass ranks, stages and writes its unit tile by tile (k_radix_onesweep) instead of
 *                          unit-wide runs (k_radix_onesweep_u)
 *   sort_rank_uniform (1)  0: every loading pass ranks with the match-any ballots.  1: a pass whose plan declares the bits
 *                          sorted before it (the prefix plans of stage 1) ranks with one LDS atomic per record wherever all
 *                          records of a wavefront instruction agree on those bits — an order that cannot matter there — and
 *                          with the ballots elsewhere (sort_kernels.h RANK 2); correct on any hardware
 *   s1_gen_blocked (0)     1: the generating first sort pass of stage 1 gives every thread consecutive items and requests the
 *                          window words of a whole unit up front (S1GenBlocked) instead of one window load per item
 *   s1_digit_hist_preload (0) 1: the same in the digit-histogram pre-pass
 * (Round 6: s1_stream_half and s1_marks_list are gone with their code: slower on every box for two rounds.)
 * (Round 4: s1_stream_prefetch / s1_stream_next_bucket / s1_stream_used_list / s1_stream_read_first / s1_stream_unroll are gone:
 *  the bucket streaming always has its next trip's loads in flight, fetches the next bucket's bounds during the current bucket and
 *  walks its table once; setting them changes nothing.)
 * Round 5:
 *   s1_gen_roll (1)        0: the blocked generating pass forms every item's window and reverse complement anew (S1GenBlockedT) instead
 *                          of one 64-bit window + one reverse complement per run of a thread's eight items (S1GenRollT; k <= 23)
 *   s1_digit_hist_roll (1) the same for the digit-histogram pre-pass and the lv1 histogram taken from the packed reads
 *   s1_var_fast (1)        0: a library whose reads are not of one length never takes the generating pass (S1GenVarT / CountGenVarT:
 *                          item slots padded to the longest read's, unfilled slots declined); s1_var_min_fill (50): per cent of the
 *                          slots that have to be real records for that form to be taken
 *   s1_giant (1)           0: a bucket of the bucket streaming is always streamed by one workgroup alone; 1: buckets of at least
 *                          s1_giant_min (262144) records are cut into slices, reduced by many workgroups and finished from their
 *                          partial entries (S1Giant, s1.hip) — low-complexity reads
 *   count_stream (1)       0: `count` always extracts 16-byte items and reduces with the tile kernel (k_count_seg); 1: fixed- or
 *                          variable-length reads on one GPU, k <= 22, min count <= 2 take 12-byte records made by the first sort
 *                          pass and the bucket streaming (k_s1_stream<COUNT>)
 *   sdbg_fast (1)          0: the SdBG records of 8-byte items come from the generic tile kernel (k_tile_groups<SdbgOp>); 1: every run
 *                          head on its own (k_sdbg_fast) for aggregated and seq2sdbg items (short runs), the tile kernel for items per
 *                          occurrence (runs as long as the coverage); 2: the run-head form for every 8-byte item; sdbg_fast_keep (1): the counting launch keeps its findings (4 bytes per item,
 *                          up to sdbg_fast_keep_max_mb = 4096 MB) for the emitting launch; sdbg_fast_halo (128), sdbg_fast_tile (2048):
 *                          records staged either side of a tile / per tile (tests, tuning)
 *   edges_reserve_permille (1000)  room behind the edges mhx_load_edges uploads, for mercy edges (the CLI: 1250, or what
 *                          MEGAHIT_NUM_MERCY_FACTOR says: seq_to_sdbg.cpp:370-378)
 * Older knobs kept for A/Bs and tests (every one only chooses between code paths with identical results):
 *   s1_bucket_hist_fast (1)   0: the lv1 histogram of a memory plan extracts items instead of scanning the packed reads
 *   s1_digit_hist_blocked (1), s1_digit_hist_plain (1)   0: the digit-histogram pre-pass of the generating sort pass in its round-3 forms
 *   s1_gen_any_order (1)      0: the generating first sort pass ranks with ballots (a stable order) instead of LDS atomics
 *   s1_pack_fixed (1)         0: the byte map of the marks becomes the bitmap through the general kernel also for reads of one length
 *   sort_hybrid_margin_ps (6) picoseconds per record the prefix-passes + segment-finish plan has to win by in sort_whole_key's cost model
 * Round 6:
 *   count_stream (1)       now also: pass by pass under a bucket filter (memory plan; the filter sits inside the histogram pre-pass and the
 *                          generating sort pass), on several GPUs (pre-sorted exchange, the first_0_out / last_0_in events routed to the
 *                          read owners), min count 1..15 (3..15: per-char 4-bit counters that stop at m instead of seen-once / seen-twice
 *                          bits); count_stream_wide (1): k = 23..27 on the same design — a window per item (CountGenWideT), 64-bit table
 *                          keys, three-word edges from k = 24 —, reads of one length, read sets below 2^32 bases (no room for position tags)
 *   count_giant (1)        0: `count` streams a giant bucket (>= s1_giant_min records) with one workgroup; 1: slices + partial entries with
 *                          per-char counters + k_count_giant_look for the keys without an in- or out-edge
 *   count_event_share (4)  several GPUs: the event regions of k_s1_stream<COUNT> hold items / count_event_share events in all
 *   s1_stream_wide (1)     0: stage 1 at k = 23..29 takes the segment group-by (k_s1_seg); 1: the bucket streaming with 64-bit table keys
 *   s1_agg_wide (0)        1: stage 1 at k = 23..27 with a min count >= 2, no mercy, on the bucket streaming leaves stage 2's aggregated items
 *                          itself, as it does at k <= 22, in the compact form of stage 2 from a count — chars, flag | W, then the 60 - 2k
 *                          count bits that are left (14 at k = 23, 6 at k = 27); a larger multiplicity becomes several items, which the
 *                          emission sums — and stage 2 sorts them where they lie instead of counting the (k+1)-mers a second time; also
 *                          for reads of several lengths, under a bucket filter and on several GPUs (8-byte items in stage 2's exchange,
 *                          if every rank has them).  mhx_last_s1_plan then ends in "[aggregated stage-2 items, <cb> count bits]".  Any
 *                          way back from the bucket streaming (s1_stream_probes = 0, an output region that overflowed, k_s1_seg, the
 *                          classic kernel) leaves no items and stage 2 runs as with 0.  Same SdBG either way
 *   s2_agg_from_count (1)  0: stage 2 always makes its solid items per occurrence where stage 1 left no aggregated ones; 1: min count 1
 *                          (k <= 27) and min count >= 2 at k = 23..27 take them from a count of the (k+1)-mers (s2.hip s2_agg_from_count)
 *                          3: as 1, and a job the route gives up on fails mhx_read2sdbg_s2 ("... stage 2 from a count given up (why)", nothing
 *                          published) instead of running per occurrence — for a caller that left the memory plan to s2_count_pass_items
 *   s2_count_pass_items (0)  > 0: that count runs in passes of at most so many records over contiguous ranges of its own lv1 buckets (a
 *                          bucket above it: a pass of its own), every pass appends its aggregated items to one array, the '$' items are
 *                          added once, one sort, one emission — the 24.5 bytes per record of the count are what a large job cannot hold
 *                          at once.  More than 64 passes: the route declines.  0: one count over everything
 *   s2_count_budget_mb (0)   > 0: the route in passes checks its exact need (mhx_s2_from_count_bytes with the items counted so far, plus
 *                          a 16th) against so many MiB after every pass and gives up beyond them: the per-occurrence path runs
 *   s2_dummy_list (1)      the '$' items of aggregated stage 2 (csrc/s2.hip k_s2d_emit): 1: the run ends of a workgroup's bitmap words are
 *                          compacted into an LDS list and dealt one per lane, so that the gathers from the reads are in flight together;
 *                          0: every thread walks the run ends of its own words one after the other (same items, other order);
 *                          s2_dummy_list_cap (0 = the kernel's 4096): entries the list holds — a trip with more run ends is worked off in
 *                          pieces of that many (tests)
 *   s2_pre_hist (1)        1: the digit histograms of stage 2's sort are taken where its items are made — k_agg_compact at the end of stage 1,
 *                          k_s2d_emit (needs s2_dummy_list) — and the sort reads no histogram of its own (no radix_hist_all_8B launch);
 *                          0, or whenever the rows do not stand for exactly the items sorted: the sort takes them itself
 *   s2_bound_from_s1 (1)   1: the room for the '$' items of stage 2 comes from a count that stage 1's pack kernel (k_pack_solid_inv*) took of
 *                          the run ends in the words it wrote, valid while the bitmap is stage 1's own for this (k, m); 0, or a bitmap from
 *                          elsewhere (mercy edges, mhx_set_is_solid, several GPUs): k_s2d_bound reads the bitmap and the host waits for it;
 *                          2: both, and the call fails unless they agree (tests)
 *   sort_loaded_ut2 (0)    1: the 12-byte passes that load their records take units of two tiles (four workgroups per CU instead of three);
 *                          measured slower (profiles/r06_ab_loaded_ut2.jsonl): the passes are bound per scattered run, not by occupancy
 *   fetch_pinned (1)       0: mhx_fetch is one hipMemcpy into the caller's (pageable) memory; 1: results of >= 16 MB leave through two
 *                          pinned staging buffers, the copy off the device overlapped with the copy into the destination
 *   s1_skm (1)             stage 1 on super-k-mer records (csrc/s1_skm.hip): 0 never; 1 where the shape is served (one GPU, no mercy, no bucket
 *                          filter, 19 <= k <= 22, min count <= 2 (s1_skm_max_m: up to 4), fewer than 2^36 bases, reads of one length or at least s1_var_min_fill per cent
 *                          of the padded blocks filled) and the job has s1_skm_min_windows (2^22) windows; 2 whatever the size (tests);
 *                          3 as 1, but a job the path gives up on FAILS instead of taking the prefix plan (mhx_s1_self_planned).
 *                          s1_skm_cap_pct (36): records the arrays hold per 100 windows (0.284 per window in random sequence);
 *                          s1_skm_max_bin (65536): a bin of more records hands the job to the prefix plan (low-complexity reads);
 *                          s1_skm_pass_gb (48): both record arrays of a pass together — larger jobs run in passes over ranges of bins,
 *                          s1_skm_passes (0) forces their number; s1_skm_bin_bits (0 = by density: 16..20) the bins; s1_skm_tags (0) 1: the
 *                          kernel of read sets beyond 2^32 bases on any read set (tests); s1_skm_deal (2): how the group-by hands a
 *                          wavefront's windows to its lanes — 0: every lane expands its own record (measured 14 % slower than 2); 1: the
 *                          windows are dealt to the lanes, 64 at a time, and a window's record comes over with six shuffles, the records'
 *                          starts from a prefix sum of six more (8 % slower); 2: dealt, with three shuffles — the record's lane and the
 *                          window's index in it come from the bitmap of run heads, the reverse complement from the window itself
 *                          (csrc/skm_deal.h) — and the prefix sum and the trip's total from ballots, without the LDS (a value below 0 runs form
 *                          0, one above 2 form 2); s1_skm_hp (1) 0: the
 *                          windows of one base (poly-A, poly-G) stay in the records instead of being counted beside them (one GPU);
 *                          s1_skm_rep (0) 1: the windows of period 2, 3 and 4 — (AC)n, (AAG)n, (AGAT)n microsatellites — are counted
 *                          beside the records too, per entry of a table of 320 (the first four or three bases name the window), and
 *                          published as keys behind the group-by: reads of such repeats no longer fill one bin and cost the path
 *                          (stage 1 and count; looked at only where s1_skm_hp is on, on one GPU; the plan line says how many windows);
 *                          s1_skm_rep_slots (64 = all): slots of the LDS hash in which a workgroup of the make kernel tallies those
 *                          windows (48 in stage 1, 16 in count) — tests: few or 0, and the tallies go to the global table directly;
 *                          s1_skm_giant (0) 1: a bin of more than s1_skm_max_bin records — the non-periodic windows across the edges of
 *                          microsatellite stretches inside reads share the repeat's minimizer — no longer costs the job the path: the bin's
 *                          rounds are dealt to several workgroups, 2^d slices of it, each the rounds from (d, j) on (csrc/skm_giant.h);
 *                          stage 1 without mercy and count, one GPU (ignored on several); the plan line ends in "[G giant bins in S slices,
 *                          largest R records]".  s1_skm_giant_keys (4096): windows a slice should hold — the slices of a bin are its estimated
 *                          windows over this, up to a power of two, at most 1024; s1_skm_giant_work_pct (25): every slice reads its whole bin,
 *                          and all slices together may read this many per cent of the job's records once more — the costliest bin's slices
 *                          are halved until they do; not even with one slice each: the prefix plan; s1_skm_giant_max (2097152): a bin of
 *                          more records hands the job to the prefix plan, as do more than 1024 such bins (the plan line says which);
 *                          s1_skm_giant_slices (0 = as above): the slices of every giant bin, a power of two up to 1024, not halved to fit
 *                          the work budget (tests);
 *                          s1_skm_max_m (2): the largest min count that stage 1 and count serve on super-k-mer records on ONE GPU — 2, or
 *                          3 / 4 (a value below 2 means 2, one above 4 means 4; several GPUs keep min count <= 2).  Stage 1 at min count
 *                          3 and 4: a key of count 1 < c < m has c windows to mark and its slot keeps the position of one, so a round
 *                          that holds such a key expands its records a second time (the LOOK form of k_s1_skm); count: the tallies of
 *                          the bases either side climb to four (the four-level form of k_count_skm).  There s1_skm_deal, s1_skm_giant
 *                          and count_skm_group are NOT consulted: the windows are dealt with three shuffles, two chunks a round, and a
 *                          bin beyond s1_skm_max_bin gives the job up.  A key counted beside the records (a homopolymer; s1_skm_rep: of
 *                          period <= 4) keeps one position: with 1 < count < m windows it cannot be marked, and stage 1 takes the prefix
 *                          plan ("[super-k-mer records given up: a key beside the records has N windows, below the min count]"; an
 *                          error under s1_skm = 3); count's tallies are exact and it stays.  mhx_s1_self_planned and
 *                          mhx_count_self_planned follow the knob;
 *                          s1_skm_split (1): the make kernel puts every record into the range of its bin's low digit (256 ranges of the
 *                          array), so the sort starts at the second digit: one 16-byte pass fewer (bins of two digits or more; a range
 *                          that overflows — skewed bins — makes the records again, unsplit); 0: one cursor and all passes;
 *                          s1_skm_split_stage (2560): records of a workgroup's trip that are ordered by digit in LDS before they leave
 *                          (at most 2560; a trip that makes more writes them from the registers; tests shrink it);
 *                          s1_skm_make_grid (0 = 8 per CU): workgroups of the make kernel (tests: few workgroups, several trips each)
 *   count_skm (1)          `count` on super-k-mer records (k_skm_make<.., COUNT>, k_count_skm: a record carries one more base either side of its run,
 *                          the table the in / out characters): one GPU, 19 <= k <= 21, min count <= 2 (s1_skm_max_m: up to 4); jobs of more than s1_skm_pass_gb of
 *                          records in passes over ranges of bins (mhx_count_self_planned); 0: never; 3: fail instead of falling back;
 *                          count_skm_group (2): chunks of 64 windows per round of compare-and-swaps (4 spills registers: measured slower)
 *   dist_skm (1)           several GPUs: 0: stage 1 never exchanges super-k-mer records by bin (comm.hip dist_s1_skm; the pre-sorted exchange
 *                          of 12-byte records runs); 1: where every rank serves the shape (as s1_skm, at most 8 ranks, no memory plan)
 *   count_skm_dist (0)     several GPUs, opt-in: 1: `count` exchanges super-k-mer records by bin too (comm.hip dist_count_skm; needs count_skm,
 *                          s1_skm and dist_skm non-zero): 19 <= k <= 21, min count <= 2, at most 8 ranks, one pass (no memory plan); the bin
 *                          owners group the windows (k_count_skm<.., EVENTS>), solid edges cross to the owners of their lv1 buckets (8 bytes
 *                          each), homopolymer tallies are summed over the ranks; the ranks take it and give it up together, and the pre-sorted
 *                          exchange then runs.  Set it to the same value on every rank.  0: the pre-sorted exchange, as before.
 *                          count_skm_ev_cap (0 = sized by the driver): events a workgroup's region holds at a bin owner (tests: 1 forces
 *                          the overflow and the give-up)
 * The CLI's memory plan (host/mhx_core.cpp plan_ranges): MHX_PLAN_BY_TIME=0 plans by space only; MHX_ALLOC_S_PER_GB=<seconds> sets the
 * hipMalloc rate the time plan assumes (tests).
 * (mhx_tuning.conf of this tree: s1_gen_blocked = 1.) */
long long mhx_get_option(mhx_ctx *, const char *name, long long dflt);
/* What the last stage 1 of this handle ran as: "super-k-mers m13, 2^16 bins (366 M records for 1.29 G windows: 3.52 per record; …)" /
 * "stream p16 sub0 2 passes (20345 records per lv1 bucket)" / "seg p24 3 passes" /
 * "full sort 6 passes".  The string lives until the next stage 1 of the handle; "" before the first. */
const char *mhx_last_s1_plan(const mhx_ctx *);

/* ---- sequence store (replaces SeqPackage held by each engine:
 *      kmer_counter.h:76, read_to_sdbg.h:47-51, seq_to_sdbg.h:79) ---- */
/* Upload a packed sequence set.  start_pos has n_seqs+1 entries (base offsets; start_pos[0]=0)
 * or is NULL when every sequence has fixed_len bases.  For `count`/`read2sdbg` the reads must
 * already be REVERSED as the reference does at load time (binary_reader.h:41-45). */
int mhx_load_sequences(mhx_ctx *, const uint32_t *packed, uint64_t n_words, uint64_t n_seqs,
                       uint32_t fixed_len, const uint64_t *start_pos);
/* Same, but from the forward-orientation `.bin` record stream of a read library
 * (uint32 len + ceil(len/16) words per read, sequence_package.h:224-240): reversal and
 * concatenation happen on the GPU (replaces BinaryReader::Read + AppendReversedCompactSequence). */
int mhx_load_bin_records(mhx_ctx *, const uint32_t *records, uint64_t n_words, uint64_t n_seqs,
                         int reverse);
/* Append more sequences (and their multiplicities, may be NULL -> 0) behind the loaded set, as
 * SeqToSdbg::Initialize does for contigs after edges (seq_to_sdbg.cpp:449-503). */
int mhx_append_sequences(mhx_ctx *, const uint32_t *packed, uint64_t n_words, uint64_t n_seqs,
                         uint32_t fixed_len, const uint64_t *start_pos, const uint16_t *mult);
/* Load packed (k+1)-mer edges exactly as `.edges.<i>` files hold them (words_per_edge words per edge, the multiplicity in
 * the low 16 bits of the last word): sequences and multiplicities are unpacked on the GPU (replaces the per-edge
 * AppendCompactSequence loop of EdgeReader::ReadSorted/ReadUnsorted, edge_reader.h:24-52, seq_to_sdbg.cpp:388-420). */
int mhx_load_edges(mhx_ctx *, const uint32_t *edges, uint64_t n_edges, uint32_t k, uint32_t words_per_edge);
/* per-sequence multiplicities for seq2sdbg (seq_to_sdbg.h:80) */
int mhx_load_multiplicity(mhx_ctx *, const uint16_t *mult, uint64_t n_seqs);
uint64_t mhx_num_sequences(const mhx_ctx *);
/* common length of the loaded sequences, 0 when they differ (SequencePackage's fixed-length fast path,
 * sequence_package.h:131-137) */
uint32_t mhx_fixed_length(const mhx_ctx *);
uint64_t mhx_num_bases(const mhx_ctx *);

/* ---- result buffers (device resident until fetched) ---- */
enum mhx_buffer {
  MHX_BUF_EDGES = 1,        /* uint32[n_edges][words_per_edge], bucket order (edge_writer.h:69-80) */
  MHX_BUF_BUCKET_COUNT = 2, /* uint64[65536]: edges (count) or SdBG items (s2/seq2sdbg) per bucket */
  MHX_BUF_FIRST_0_OUT = 3,  /* uint32[n_reads]   (kmer_counter.h:78) */
  MHX_BUF_LAST_0_IN = 4,    /* uint32[n_reads]   (kmer_counter.h:79) */
  MHX_BUF_MUL_HIST = 5,     /* int64[65536]      (edge_counter.h:14-56) */
  MHX_BUF_IS_SOLID = 6,     /* uint64[ceil(n_bases/64)] (AtomicBitVector, kmbitvector.h:67-88) */
  MHX_BUF_MERCY_CAND = 7,   /* int64[n_mercy_cand], sorted ascending (read_to_sdbg_s1.cpp:466-551) */
  MHX_BUF_SDBG_BYTES = 8,   /* uint8[sdbg_bytes]: bucket byte streams, bucket-id order (sdbg_writer.cpp:38-57) */
  MHX_BUF_BUCKET_OFFSET = 9,/* uint64[65536] starting byte of each bucket in MHX_BUF_SDBG_BYTES */
  MHX_BUF_BUCKET_TIPS = 10, /* uint64[65536] */
  MHX_BUF_BUCKET_LARGE = 11,/* uint64[65536] */
  MHX_BUF_SORTED_ITEMS = 12,/* uint32[n_items][item_words]: the lv2 items of the last engine as its sort left them (tests): a view into the
                              sort workspace, overwritten by the next engine call.  Fully sorted on the tile paths; on the bucket-streaming
                              plans (stage 1 without mercy, `count` at k <= 22: mhx_count_result.item_words == 3) 12-byte records ordered
                              only by the plan's key prefix */
  MHX_BUF_W_COUNT = 13,     /* uint64[9] + ones_in_last: uint64[10] (sdbg_meta.h:41-48) */
  /* device-resident SdBG hand-over, filled by mhx_sdbg_build_index (below); layouts = the reference's in-memory ones */
  MHX_BUF_SDBG_W = 20,          /* uint64[ceil(n/16)]: 4 bits per item, item i at bits 4*(i%16) (sdbg_raw_content.h:22) */
  MHX_BUF_SDBG_LAST = 21,       /* uint64[ceil(n/64)]: bit i%64 of word i/64 */
  MHX_BUF_SDBG_TIP = 22,        /* same */
  MHX_BUF_SDBG_INVALID = 23,    /* tip | (W == 0): SDBG::invalid_ after LoadFromFile (sdbg.h:33-60) */
  MHX_BUF_SDBG_SMALL_MUL = 24,  /* uint8[n], 255 = look in MUL (sdbg_raw_content.cpp:72-83) */
  MHX_BUF_SDBG_MUL = 25,        /* uint16[n]: SDBG::EdgeMultiplicity */
  MHX_BUF_SDBG_TIP_LABELS = 26, /* uint32[n_tips][words_per_tip_label], chars reversed inside each word (:85-91) */
  MHX_BUF_SDBG_PREFIX_LKT = 27, /* int64[65536][2]: first / last item of every bucket (sdbg.h:38-49) */
  MHX_BUF_SDBG_RS_W_L2 = 28,    /* int64[9][num_l2_w]   kmlib::RankAndSelect<4,9> over W (kmrns.h:118-175) */
  MHX_BUF_SDBG_RS_W_L1 = 29,    /* uint16[9][num_l1_w] */
  MHX_BUF_SDBG_RS_W_SEL = 30,   /* uint32[]: select samples of character c at [w_sel_offset[c], w_sel_offset[c+1]) */
  MHX_BUF_SDBG_RS_LAST_L2 = 31, /* int64[num_l2_bits]   RankAndSelect<1,2> over last */
  MHX_BUF_SDBG_RS_LAST_L1 = 32, /* uint16[num_l1_bits] */
  MHX_BUF_SDBG_RS_LAST_SEL = 33,/* uint32[last_sel_count] */
  MHX_BUF_SDBG_RS_TIP_L2 = 34,  /* rank-only structure over tip */
  MHX_BUF_SDBG_RS_TIP_L1 = 35,
  MHX_BUF_LIB_RECORDS = 40,     /* uint32[]: read-library records (len + packed words per read) of mhx_fastx_to_records */
  /* the unitig graph of mhx_sdbg_unitigs (below), kept in HBM for the graph-cleaning steps (mhx_unitig_*, below) */
  MHX_BUF_UNITIG_VERTICES = 41, /* mhx_unitig_vertex[n_vertices], the reference's vertex order on one thread */
  MHX_BUF_UNITIG_SEQ = 42,      /* char[n_bases]: every vertex's contig text ('ACGT', before FoldPalindrome), back to back */
  MHX_BUF_UNITIG_OFFSET = 43,   /* uint64[n_vertices + 1]: where vertex v's text starts in MHX_BUF_UNITIG_SEQ */
  /* the --careful_bubble records of the last mhx_unitig_pop_bubbles call (below), in the order the reference writes them at -t 1 */
  MHX_BUF_UNITIG_BUBBLE_REC = 44, /* mhx_bubble_record[n_records] */
  MHX_BUF_UNITIG_BUBBLE_SEQ = 45, /* char[]: the records' text ('ACGT'), back to back */
  /* `local`, first half (mhx_local_map / mhx_local_collect, below) */
  MHX_BUF_LOCAL_REC = 46,     /* mhx_local_record[n_reads] */
  MHX_BUF_LOCAL_ITEMS = 47,   /* uint64[n_items]: the collector's encoded reads, grouped by contig, then end, ascending inside a group */
  MHX_BUF_LOCAL_OFFSETS = 48, /* uint64[2 * n_contigs + 1]: the items of (contig c, end e) are [offsets[2c + e], offsets[2c + e + 1]) */
  /* mhx_sdbg_mul_histogram (below) */
  MHX_BUF_SDBG_MUL_HIST = 49, /* uint64[65536]: bin v = valid edges (bit clear in MHX_BUF_SDBG_INVALID) with MHX_BUF_SDBG_MUL == v */
  /* mhx_bgzf_inflate (below) */
  MHX_BUF_FASTX_TEXT = 50     /* char[n_text]: the inflated text */
};
/* bytes currently held in a result buffer (0 if absent) */
uint64_t mhx_buffer_bytes(const mhx_ctx *, int which);
/* copy [offset, offset+bytes) of a result buffer to host memory */
int mhx_fetch(mhx_ctx *, int which, void *dst, uint64_t offset, uint64_t bytes);

/* ---- engines ---- */
typedef struct {
  uint64_t n_items;        /* items sorted = sum max(0, len-k) */
  uint64_t n_distinct;     /* distinct (k+1)-mers */
  uint64_t n_edges;        /* solid edges emitted */
  uint32_t words_per_edge; /* ceil((2(k+1)+16)/32), edge_writer.h:37-40 */
  uint32_t item_words;     /* stride of MHX_BUF_SORTED_ITEMS */
} mhx_count_result;
/* KmerCounter::Run (kmer_counter.cpp:60-414 under base_engine.cpp:143-211).
 * Fills EDGES, BUCKET_COUNT, FIRST_0_OUT, LAST_0_IN, MUL_HIST. */
int mhx_count(mhx_ctx *, uint32_t k, uint32_t min_count, mhx_count_result *out);

typedef struct {
  uint64_t n_items;      /* (k-1)-mer items sorted */
  uint64_t n_solid;      /* solid (k+1)-mer occurrences marked */
  uint64_t n_mercy_cand; /* 0 unless want_mercy */
  uint32_t item_words;
} mhx_s1_result;
/* Read2SdbgS1::Run (read_to_sdbg_s1.cpp:88-566).  Fills IS_SOLID, MUL_HIST and, when
 * want_mercy != 0, MERCY_CAND.  want_mercy: 0 = no candidates; 1 = candidates with the stable tie order
 * (a group's first item = first in read order); 2 = candidates with the reference's exact tie order
 * (kmlib::kmsort's unstable permutation replayed per lv1 bucket; slower) — see DESIGN.md "H1". */
int mhx_read2sdbg_s1(mhx_ctx *, uint32_t k, uint32_t min_count, int want_mercy, mhx_s1_result *out);
/* 1 when stage 1 of the loaded reads would run on super-k-mer records (csrc/s1_skm.hip: one GPU, no mercy, 19 <= k <= 22, min count <= 2,
 * no bucket filter) — a form that cuts a job too large for one working set into passes over ranges of its own bins BY ITSELF
 * (the lv1 bucket ranges of base_engine.cpp:54-141 would break its records apart).  A caller that plans bucket-range passes asks first:
 * on 1 it sets option s1_skm = 3 and calls mhx_read2sdbg_s1 once, without a filter — with 3 the call fails (instead of quietly taking the
 * prefix plan on the whole job) when the input turns out not to be served, low-complexity reads for one, and the caller plans as before
 * with s1_skm = 0.  host/mhx_core.cpp read2sdbg does exactly that. */
int mhx_s1_self_planned(mhx_ctx *, uint32_t k, uint32_t min_count, int want_mercy);
/* 1 while the handle holds the aggregated stage-2 items that the last mhx_read2sdbg_s1 left for (k, min_count) — always at k <= 22 with a
 * min count >= 2, at k = 23..27 where s1_agg_wide had the bucket streaming leave them — that is, until a stage 2 sorts them where they lie
 * or the reads or the bitmap change.  A caller that plans stage 2's memory asks this (about 0.5 items per base with them, 2.2 per
 * occurrence without); host/mhx_core.cpp does. */
int mhx_s1_left_items(mhx_ctx *, uint32_t k, uint32_t min_count);
/* The same question for mhx_count (count on super-k-mer records: one GPU, 19 <= k <= 21, min count <= 2): on 1 the caller sets option
 * count_skm = 3 and calls mhx_count once without a bucket filter; a job the path gives up on fails that call, and the caller plans lv1
 * bucket ranges as before with count_skm = 0. */
int mhx_count_self_planned(mhx_ctx *, uint32_t k, uint32_t min_count);

/* mercy block of Read2SdbgS2::Initialize (read_to_sdbg_s2.cpp:122-266): consumes MERCY_CAND,
 * sets extra IS_SOLID bits on the device copy; *num_mercy receives "Number mercy". */
int mhx_read2sdbg_add_mercy(mhx_ctx *, uint32_t k, uint64_t *num_mercy);
/* replace the device IS_SOLID bitmap (e.g. one produced elsewhere); n_words = ceil(n_bases/64) */
int mhx_set_is_solid(mhx_ctx *, const uint64_t *bits, uint64_t n_words);

typedef struct {
  uint64_t n_items;    /* lv2 items sorted */
  uint64_t n_sdbg;     /* SdBG records emitted */
  uint64_t n_tips;     /* $-tips */
  uint64_t n_large;    /* records with multiplicity > 254 */
  uint64_t sdbg_bytes; /* size of MHX_BUF_SDBG_BYTES */
  uint32_t words_per_tip_label;
  uint32_t item_words;
} mhx_sdbg_result;
/* Read2SdbgS2::Run minus the mercy block (read_to_sdbg_s2.cpp:271-630).  Uses IS_SOLID unless
 * min_count == 1 (for_sure_solid, read_to_sdbg_s2.cpp:295).  Fills SDBG_BYTES, BUCKET_*. */
int mhx_read2sdbg_s2(mhx_ctx *, uint32_t k, uint32_t min_count, mhx_sdbg_result *out);
/* SeqToSdbg::Run minus input parsing (seq_to_sdbg.cpp:530-807) on the loaded sequences +
 * multiplicities.  Fills SDBG_BYTES, BUCKET_*. */
int mhx_seq2sdbg(mhx_ctx *, uint32_t k, mhx_sdbg_result *out);

/* SeqToSdbg::GenMercyEdges (seq_to_sdbg.cpp:171-357): the loaded sequences must be the sorted
 * (k+1)-mer edges; cand = candidate reads (packed, start_pos as in mhx_load_sequences).  Appends
 * the mercy edges (multiplicity 1) to the loaded set; *n_mercy receives their number. */
int mhx_gen_mercy_edges(mhx_ctx *, uint32_t k, const uint32_t *cand_packed, uint64_t cand_words,
                        uint64_t n_cand, const uint64_t *cand_start, uint64_t *n_mercy);

/* ---- device-resident SdBG hand-over.  Builds, on the GPU and from the SdBG the handle holds
 * (MHX_BUF_SDBG_BYTES + MHX_BUF_BUCKET_* of the last stage-2 / seq2sdbg call, or a stream installed with
 * mhx_sdbg_load_bytes), everything SDBG::LoadFromFile builds on one CPU thread: the W / last / tip / multiplicity /
 * tip-label arrays of LoadSdbgRawContent (sdbg_raw_content.cpp:18-96) and the rank/select tables, prefix table, f and
 * rank_f of sdbg.h:26-61 over kmlib/kmrns.h:118-175 — in the reference's own layouts (MHX_BUF_SDBG_*), so a
 * downstream stage can adopt them without reading .sdbg files back. ---- */
typedef struct {
  uint64_t n_items, n_tips, n_large;
  uint32_t k, words_per_tip_label;
  int use_full_mul;          /* what the reference would choose: n_large >= 0.08 n (sdbg_raw_content.cpp:29-30) */
  uint64_t num_l1_w, num_l2_w;       /* table lengths per character of the W structure */
  uint64_t num_l1_bits, num_l2_bits; /* ... of the last / tip structures */
  uint64_t w_char_count[9];          /* kmrns char_count_ (character 0 includes the zero padding of the last word) */
  uint64_t w_sel_offset[10];
  uint64_t ones_in_last, ones_in_tip, last_sel_count;
  long long f[6], rank_f[6];         /* sdbg.h:482-483 */
} mhx_sdbg_index_info;
int mhx_sdbg_build_index(mhx_ctx *, uint32_t k, mhx_sdbg_index_info *out);
/* SdBG-level tip trimming on the device-resident graph — sdbg_pruning::RemoveTips
 * (assembly/sdbg_pruning.cpp:61-179: rounds of Trim with len = 2, 4, ... < max_tip_len, then max_tip_len) over the
 * succinct graph's Forward/Backward navigation (sdbg.h:106-121,240-330), one thread per edge, on the buffers that
 * mhx_sdbg_build_index left in HBM.  Updates MHX_BUF_SDBG_INVALID in place; *n_removed = tips removed (the number the
 * reference logs).  `assemble` calls it with max_tip_len = 2k by default (main_assemble.cpp:143-156). */
int mhx_sdbg_remove_tips(mhx_ctx *, const mhx_sdbg_index_info *info, int max_tip_len, uint64_t *n_removed);
/* The minimum depth `assemble` infers when none is given: sdbg_pruning::InferMinDepth (assembly/sdbg_pruning.cpp:36-59).
 *   mhx_sdbg_mul_histogram  the histogram of EdgeMultiplicity over the edges that are valid NOW into MHX_BUF_SDBG_MUL_HIST
 *       (uint64[65536]); *n_valid (may be NULL) = the sum of the bins.  It reads MHX_BUF_SDBG_MUL and the current bits of
 *       MHX_BUF_SDBG_INVALID, so it is valid whenever the index is — straight after mhx_sdbg_build_index (what the reference
 *       looks at: the graph as loaded), after mhx_sdbg_remove_tips, after cleaning calls; without an index of info->n_items
 *       items in the handle it is an error.  One kernel (csrc/sdbg_index.hip k_sdbg_mul_hist): values below 8192 are counted
 *       in LDS per workgroup, flushed after at most 2^30 items (knob sdbg_hist_flush_tiles: tiles of 16384 items between two
 *       flushes, 1..65536, for the tests), the others with one global atomic each.
 *   mhx_infer_min_depth  the fixed point of InferMinDepth on such a histogram, over the behaviour of Histgram<uint16_t>
 *       (utils/histgram.h).  Pure host code without a device call: works on a machine without a GPU.  Only non-zero bins exist
 *       and bin 0 is a value like any other.  cov = FirstLocalMinimum (the running minimum moves on `<=`, four larger bins in
 *       a row end the search, 0 when the minimum found is the largest value present); then at most 100 rounds of: TrimLow
 *       ((uint16_t)roundf((float)cov): cumulative), median = the first value whose running sum exceeds (size_t)(size * 0.5)
 *       (0: none), cov1 = sqrt(median); |cov - cov1| < 1e-2 returns cov (the OLD value) with *converged = 1.  After 100
 *       rounds *converged = 0 and *min_depth = 1 (the reference warns "Cannot detect min depth: unconverged").  converged may
 *       be NULL.  An all-zero histogram is the error "no valid edge" (the reference's behaviour is undefined there).
 *   mhx_sdbg_infer_min_depth  both: the histogram, its 512 KB fetched, the host function.
 * `mhx_core assemble` calls it after mhx_sdbg_build_index and before mhx_sdbg_remove_tips when the prune level is >= 1 and no
 * --min_depth > 0 was given, logs "min depth set to %.3f" and uses the full double.  Such a command line takes the GPU route
 * only at the second level of the route's opt-in variable (MHX_ASSEMBLE_PRUNE=2 / MHX_ASSEMBLE_BUBBLE=2, below). */
int mhx_sdbg_mul_histogram(mhx_ctx *, const mhx_sdbg_index_info *info, uint64_t *n_valid);
int mhx_infer_min_depth(const uint64_t hist[65536], double *min_depth, int *converged);
int mhx_sdbg_infer_min_depth(mhx_ctx *, const mhx_sdbg_index_info *info, double *min_depth, int *converged);
/* The unitig graph: UnitigGraph::UnitigGraph (assembly/unitig_graph.cpp:13-138) on the buffers mhx_sdbg_build_index
 * (+ mhx_sdbg_remove_tips) left in HBM, and the contig text OutputContigs writes (contig_output.cpp:62-119 over
 * VertexToDNAString, unitig_graph.cpp:357-394).  Vertices in the order the reference builds them on one thread (chains
 * ascending by min(tail, rc tail), then loops ascending by the smallest edge of the cycle pair), so vertex v is contig
 * k<k>_<v>.  The text of a vertex is on the strand ToUniqueFormat picks (the one beginning at min(b, rb)): GetLabel(begin)
 * + W of every edge, k + length characters; palindromes are not folded (FoldPalindrome stays with the writer).
 * Fails as the reference does when the vertices reach UnitigGraph::kMaxNumVertices (2^32 - 2). */
#define MHX_UNITIG_LOOP 1u        /* is_looped */
#define MHX_UNITIG_PALINDROME 2u  /* is_palindrome: b == rb */
#define MHX_UNITIG_STANDALONE 4u  /* a loop, or in-degree = out-degree = 0 (contig_output.cpp:83-117) */
#define MHX_UNITIG_CHANGED 8u     /* is_changed: the survivor of a merge in a Refresh that was asked to mark (unitig_graph.cpp:293,334) */
typedef struct {
  uint64_t b, e, rb, re;  /* begin / end edge of strand 0 and of its reverse complement (UnitigGraphVertex::strand_info) */
  uint64_t total_depth;   /* sum of EdgeMultiplicity over the unitig (a loop counts its end edge twice, unitig_graph.cpp:96-104) */
  uint32_t length;        /* edges */
  uint32_t flags;         /* MHX_UNITIG_* */
} mhx_unitig_vertex;
typedef struct {
  uint64_t n_vertices, n_loops;
  uint64_t n_palindromes; /* palindromic non-loop vertices: the reference's "Graph size without loops: N, palindrome: P" */
  uint64_t n_standalone;
  uint64_t n_bases;       /* size of MHX_BUF_UNITIG_SEQ */
} mhx_unitig_result;
int mhx_sdbg_unitigs(mhx_ctx *, const mhx_sdbg_index_info *info, mhx_unitig_result *out);
/* Graph cleaning on that unitig graph, in place on MHX_BUF_UNITIG_VERTICES and MHX_BUF_SDBG_INVALID: together they are
 * `assemble --bubble_level 0 --prune_level 0..2 --cleaning_rounds N` (main_assemble.cpp:182-301).  The result is the
 * reference's at -t 1 and does not depend on any thread count.  Valid only after mhx_sdbg_unitigs on the same index (any
 * other state returns an error); between these calls MHX_BUF_UNITIG_SEQ / _OFFSET and the vertices' STANDALONE flags are
 * stale until mhx_unitig_finish.  mhx_unitig_finish may be called in mid-run: it reads the vertex table and the SdBG and
 * rebuilds only the text, the offsets and the STANDALONE flags, so cleaning calls after a finish are valid and give what they
 * give without it; SEQ / OFFSET / STANDALONE are then stale again until the next finish (the non-final `assemble` writes
 * its contigs, prunes on, finishes again and writes the changed ones).
 *   mhx_unitig_disconnect_weak_links  DisconnectWeakLinks (assembly/weak_link_remover.cpp): at every vertex end with two or
 *       more out-neighbours, a neighbour whose average depth is <= ratio * the neighbours' total is flagged on the strand it
 *       is entered by; then UnitigGraph::Refresh (unitig_graph.cpp:140-355: flagged vertices lose their end edges, deleted
 *       ones all their edges, linear paths and cycles merge, survivors are compacted in index order).  *n_flagged = the
 *       (vertex, strand) flags set: the reference's "Number unitigs disconnected".
 *   mhx_unitig_remove_tips  RemoveTips on the unitig graph (assembly/tip_remover.cpp): thresholds 2, 4, 8, ... below
 *       max_tip_len, each followed by a Refresh; a vertex shorter than the threshold goes when it is a loop, has no
 *       neighbour, or has one neighbour in all whose average depth is > 8 times its own.  *n_removed = "Tips removed".
 *   mhx_unitig_remove_local_low_depth  RemoveLocalLowDepth (assembly/low_depth_remover.cpp:10-86), one pass: a vertex that is
 *       no loop, no longer than max_len, has a neighbour and (in-degree <= 1 and out-degree <= 1, or one of them 0) is
 *       deleted when its average depth is below min(min_depth, local_ratio * the mean depth of its neighbours, each
 *       counted over at most local_width edges); then a Refresh, only if something was deleted.  mark_changed != 0 is
 *       Refresh(true) (the reference's permanent_rm = false): survivors of merges get MHX_UNITIG_CHANGED, which every later
 *       call keeps.  *n_removed = vertices deleted; *is_changed = the reference's return value (some vertex deleted, or some
 *       qualifying vertex with min_depth < local_ratio * mean).  Plain IEEE double in the reference's order of operations.
 *   mhx_unitig_iterate_local_low_depth  IterateLocalLowDepth (low_depth_remover.cpp:88-102): passes with min_depth, 1.1 *
 *       min_depth, ... until one returns is_changed = 0 or min_depth reaches 65535.  *n_removed = the sum over the passes.
 *   mhx_unitig_finish  flags (MHX_UNITIG_STANDALONE from the degrees on the cleaned graph), MHX_BUF_UNITIG_SEQ and
 *       MHX_BUF_UNITIG_OFFSET for the vertex table as it is now.  total_depth is no longer a sum of multiplicities once a
 *       vertex was trimmed (lround(average * new length), unitig_graph.cpp:191-193).
 * The CLI (`mhx_core assemble`) runs the cleaning rounds only when MHX_ASSEMBLE_CLEAN=1 or MHX_ASSEMBLE_PRUNE=1 is in its
 * environment and only at --bubble_level 0; --prune_level 1 and 2 run here only with MHX_ASSEMBLE_PRUNE=1 (--min_depth > 0
 * given) or MHX_ASSEMBLE_PRUNE=2 (given, or inferred: mhx_sdbg_infer_min_depth above), which imply the cleaning rounds.
 * Otherwise such command lines are forwarded to MHX_REF_CORE.
 * MHX_ASSEMBLE_BUBBLE=1 (further below) implies both and adds the bubble levels 1 and 2 and prune level 3.
 * MHX_ASSEMBLE_REF=1 wins. */
int mhx_unitig_disconnect_weak_links(mhx_ctx *, const mhx_sdbg_index_info *info, double ratio, uint64_t *n_flagged);
int mhx_unitig_remove_tips(mhx_ctx *, const mhx_sdbg_index_info *info, uint32_t max_tip_len, uint64_t *n_removed);
int mhx_unitig_remove_local_low_depth(mhx_ctx *, const mhx_sdbg_index_info *info, double min_depth, uint32_t max_len, uint32_t local_width,
                                      double local_ratio, int mark_changed, uint64_t *n_removed, int *is_changed);
int mhx_unitig_iterate_local_low_depth(mhx_ctx *, const mhx_sdbg_index_info *info, double min_depth, uint32_t max_len, uint32_t local_width,
                                       double local_ratio, int mark_changed, uint64_t *n_removed);
int mhx_unitig_finish(mhx_ctx *, const mhx_sdbg_index_info *info, mhx_unitig_result *out);
/* Bubble popping and prune level 3 on the same unitig graph (same validity rules and stale-state errors as the calls above):
 * with them the cleaning calls cover `assemble --bubble_level 0..2 --prune_level 0..3` (main_assemble.cpp:182-301; its
 * InferMinDepth is mhx_sdbg_infer_min_depth above).  The result is the reference's at any -t: a search reads only what the pass never writes and sets only
 * to-delete flags, so the deleted set is a union and the count the number of distinct vertices in it.
 *   mhx_unitig_pop_bubbles  BaseBubbleRemover::PopBubbles (assembly/bubble_remover.cpp:58-152), one thread per (vertex, strand)
 *       node: a node with d >= 2 out-neighbours ("middles"), none longer than max_len, each with in-degree 1 and one
 *       out-neighbour, all the same node ("right") whose canonical id min(b, rb) is >= the left's and whose in-degree is d, is
 *       a bubble.  The middles are sorted by average depth (descending; ties: canonical id ascending) and all but the first
 *       are deleted.  similarity <= 0 is NaiveBubbleRemover (the caller passes max_len = k + 2).  similarity > 0 is
 *       ComplexBubbleRemover (the caller passes max_len = lround(merge_len * k / similarity)): every (middle[0], middle[j])
 *       must pass (len_j + k - 1) * similarity <= len_0 + k - 1, the same the other way round, and GetSimilarity >=
 *       similarity on the two vertices' own texts (mhx_unitig_similarity below), or the bubble stays; when max_len *
 *       (1 - similarity) < 1 the call returns 0 at once, as the reference does.  Then a Refresh, which marks the survivors of
 *       merges MHX_UNITIG_CHANGED when mark_changed != 0 (the reference's permanent_rm = false) — skipped when no flag was
 *       set, where it would change nothing.  *n_removed = vertices deleted.
 *       careful_threshold >= 0 (`--careful_bubble`: 0.2): a popped bubble leaves records — every deleted middle with average
 *       depth >= that of middle[0] * careful_threshold and, when there is one, the left and the right vertex — each the
 *       vertex's text (as in MHX_BUF_UNITIG_SEQ, taken before the Refresh) and average depth.  *n_records = their number;
 *       MHX_BUF_UNITIG_BUBBLE_REC / _SEQ hold them until the next call, ordered by left vertex, strand 0 then 1, middle.
 *       A bubble seen from both of its ends or from a palindromic left is counted once and recorded twice (as the reference).
 *       The text comes from mhx_unitig_finish, which the call runs by itself when a Refresh ran since the last one and it
 *       has a pair to compare or a record to write.
 *       Cap: in complex mode max_len + k <= MHX_SIM_MAX_LEN and (max_len + k) * (1 - similarity) < MHX_SIM_MAX_INDEL + 1,
 *       else an error.
 *   mhx_unitig_bubble_stats  of the last mhx_unitig_pop_bubbles: out[0] = complex candidates (bubbles that passed the
 *       structural and length tests), out[1] / out[2] = pairs whose similarity passed / failed, out[3] = mid-run finishes.
 *   mhx_unitig_remove_low_depth  RemoveLowDepth (low_depth_remover.cpp:104-117): every vertex with average depth < min_depth
 *       is deleted, then a Refresh (no marks).  Prune level 3.
 *   mhx_unitig_similarity  GetSimilarity (bubble_remover.cpp:10-54) of two host strings on the device, the kernel the complex
 *       mode uses: with max_indel = (int)(max(n, m) * (1 - similarity)), 0 when |n - m| > max_indel or max_indel < 1, else
 *       1 - d / max(n, m) for the edit distance d inside the band of 2 * max_indel + 1 diagonals with the reference's
 *       boundary conditions, in IEEE double.  Needs no graph.  Strings longer than MHX_SIM_MAX_LEN or a max_indel above
 *       MHX_SIM_MAX_INDEL are an error (two band rows of 4-byte cells are kept in 32 KB of LDS).
 * The CLI runs these only with MHX_ASSEMBLE_BUBBLE=1 in its environment (which implies MHX_ASSEMBLE_PRUNE and _CLEAN):
 * --bubble_level 0..2, --prune_level 0..3 (levels 1..3 with --min_depth > 0 given, or with MHX_ASSEMBLE_BUBBLE=2 inferred), --careful_bubble or not, and
 * --merge_len / --merge_similar within the cap at k = MHX_MAX_K.  Everything else is forwarded as before. */
#define MHX_SIM_MAX_LEN 16384
#define MHX_SIM_MAX_INDEL 2047
typedef struct {
  uint64_t offset;   /* where the text starts in MHX_BUF_UNITIG_BUBBLE_SEQ */
  uint32_t length;   /* characters: the vertex's length + k */
  uint32_t vertex;   /* index in the vertex table the pass ran on */
  double avg_depth;  /* total_depth / length: the record's multiplicity */
} mhx_bubble_record;
int mhx_unitig_pop_bubbles(mhx_ctx *, const mhx_sdbg_index_info *info, uint32_t max_len, double similarity, double careful_threshold,
                           int mark_changed, uint64_t *n_removed, uint64_t *n_records);
int mhx_unitig_bubble_stats(mhx_ctx *, uint64_t out[4]);
int mhx_unitig_remove_low_depth(mhx_ctx *, const mhx_sdbg_index_info *info, double min_depth, uint64_t *n_removed);
int mhx_unitig_similarity(mhx_ctx *, const char *a, uint32_t n, const char *b, uint32_t m, double similarity, double *out);
/* install an SdBG produced elsewhere (e.g. read back from .sdbg.* files: bucket byte ranges back to back) as the handle's
 * current SdBG; the four tables have 65536 entries (starting byte, items, tips, large multiplicities per bucket) */
int mhx_sdbg_load_bytes(mhx_ctx *, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *bucket_offset, const uint64_t *bucket_items,
                        const uint64_t *bucket_tips, const uint64_t *bucket_large);

/* ---- buildlib on the GPU.  FASTA / FASTQ text (already inflated) -> the record stream of a read
 * library (`<lib>.bin`: per read uint32 length + ceil(len/16) words, 2 bits per base MSB first, forward orientation;
 * sequence_package.h:224-240) in MHX_BUF_LIB_RECORDS, with the reference's N-trimming (fastx_reader.cpp:56-71) and
 * character mapping (sequence_package.h:78-83).  text2 != NULL: a paired library, records interleaved r1, r2, r1, ...
 * (paired_fastx_reader.cpp:7-43).  Replaces SequenceLibCollection::Build's parse + pack (sequence_lib.cpp:8-91).
 * out->status 1 = the text is not plain FASTA / four-line FASTQ (carriage returns, multi-line FASTQ, junk before the
 * first header, a FASTA text that ends in a '>' alone on its line, mates of different counts): nothing was produced, run a
 * sequential kseq-compatible parser instead. ---- */
typedef struct {
  uint64_t n_reads, n_bases, n_words; /* n_bases counts an all-N / empty read as 1 (it is stored as one 'A') */
  uint32_t max_len;
  int status;
} mhx_fastx_result;
int mhx_fastx_to_records(mhx_ctx *, const char *text1, uint64_t n1, const char *text2, uint64_t n2, mhx_fastx_result *out);

/* ---- BGZF read files (the blocked gzip of bgzip: a concatenation of gzip members of at most 64 KiB, each an independent DEFLATE
 * stream whose compressed size stands in its header and whose CRC32 and length stand in its trailer) inflated on the GPU, one block
 * per wavefront, and parsed where the text lies.  The host only walks the members (O(blocks), nothing inflated).
 * mhx_bgzf_inflate: gz[0 .. n) -> its text in MHX_BUF_FASTX_TEXT (mhx_fetch), every block checked against its CRC32 and ISIZE.
 * status 0: inflated.  status 2: the file is not BGZF throughout (reason: one of the scan's, bad_block: the member it is about) or a
 * block failed (reason: one of the decoder's, bad_block: the first such block); no text is left then.  An empty file and a file of
 * end-of-file blocks alone are BGZF with an empty text.
 * mhx_fastx_bgzf_to_records: mhx_fastx_to_records on the texts of one or two BGZF files (gz2 == NULL: unpaired).  status 0 / 1 as
 * there; status 2: a file was not inflated on the device (mhx_bgzf_inflate tells why) and nothing was produced: inflate on the host.
 * Device memory per file: the compressed bytes + the text + 64 + 32 bytes per block (+ 1.3 KB of tables), next to what
 * mhx_fastx_to_records takes for a text of that size less its own copy of the text. ---- */
enum mhx_bgzf_reason {
  MHX_BGZF_OK = 0,
  /* the scan: the file is not BGZF throughout */
  MHX_BGZF_NOT_GZIP = 1,     /* a member does not begin 1f 8b 08 */
  MHX_BGZF_FLG = 2,          /* FLG is not exactly 4 (plain gzip, or a name, a comment, a header CRC) */
  MHX_BGZF_NO_BC = 3,        /* no 'B','C' extra subfield of length 2 */
  MHX_BGZF_SHORT_BLOCK = 4,  /* a block shorter than 26 bytes, or than its own header, subfields and trailer */
  MHX_BGZF_PAST_EOF = 5,     /* a block that runs past the end of the file */
  MHX_BGZF_TRAILING = 6,     /* trailing bytes that are not a whole member (fewer than a member's fixed header) */
  MHX_BGZF_ISIZE = 7,        /* ISIZE above 65536 */
  /* the decoder: a block's DEFLATE stream or its trailer */
  MHX_BGZF_PAYLOAD_END = 8,     /* end of the payload before the final block's end-of-block symbol */
  MHX_BGZF_BTYPE = 9,           /* BTYPE 3 */
  MHX_BGZF_STORED_LEN = 10,     /* stored block: LEN != ~NLEN */
  MHX_BGZF_CODE_OVER = 11,      /* an over-subscribed code */
  MHX_BGZF_CODE_INCOMPLETE = 12, /* an incomplete code (beyond the single code of length 1 zlib accepts) */
  MHX_BGZF_BAD_SYMBOL = 13,     /* bits that are no code's, literal/length 286 / 287, distance 30 / 31, a repeat without a length before it
                                 * or past the counts, no end-of-block code, more than 286 / 30 codes */
  MHX_BGZF_DIST_FAR = 14,       /* a match that reaches before the block's start */
  MHX_BGZF_OUT_OVER = 15,       /* output past ISIZE */
  MHX_BGZF_OUT_SHORT = 16,      /* the stream ends with fewer bytes than ISIZE */
  MHX_BGZF_CRC = 17             /* the text's CRC32 is not the trailer's */
};
typedef struct {
  int status;
  uint32_t reason;   /* enum mhx_bgzf_reason */
  uint64_t bad_block;
  uint64_t n_blocks; /* members, empty ones included */
  uint64_t n_text;   /* bytes of text */
} mhx_bgzf_result;
int mhx_bgzf_inflate(mhx_ctx *, const void *gz, uint64_t n, mhx_bgzf_result *out);
int mhx_fastx_bgzf_to_records(mhx_ctx *, const void *gz1, uint64_t n1, const void *gz2, uint64_t n2, mhx_fastx_result *out);

/* ---- `iterate` — the (k+step+1)-mer edges that the loaded reads (FORWARD orientation:
 * mhx_load_bin_records(..., reverse = 0)) support next to the contigs of round k.  Replaces ContigFlankIndex +
 * KmerCollector (iterate/contig_flank_index.h:16-219, iterate/kmer_collector.h:49-69, main_iterate.cpp:117-145): flank
 * records sorted and searched, one thread per read, the k-mer set = sort + unique.  contigs: packed as
 * mhx_load_sequences takes them, forward, loop / standalone contigs already dropped by the caller
 * (async_sequence_reader.h:80).  Fills MHX_BUF_EDGES with n_edges records of words_per_edge words, multiplicity 0 as
 * the reference writes them, in sorted order (the reference's order is its hash set's). ---- */
typedef struct {
  uint64_t n_flanks, n_kmers, n_edges;
  uint32_t words_per_edge;
} mhx_iterate_result;
int mhx_iterate(mhx_ctx *, uint32_t k, uint32_t step, const uint32_t *contig_packed, uint64_t contig_words, uint64_t n_contigs,
                const uint64_t *contig_start, mhx_iterate_result *out);

/* ---- `local`, first half: reads mapped to contig ends for local assembly.  Replaces HashMapper (localasm/hash_mapper.cpp),
 * MappingResultCollector (localasm/mapping_result_collector.h) and EstimateInsertSize / LocalRange / MapToContigs
 * (localasm/local_assemble.cpp:83-223); AssembleAndOutput (the IDBA hash graph and contig graph, serial per contig end)
 * stays with the caller.  Every result equals the reference's at any thread count (its single-end loop at -t 1: the
 * `omp parallel` without `for` at :204 runs that loop once per thread).
 *   mhx_local_index   the seed index over the contigs: packed as mhx_load_sequences takes them, forward, contigs shorter
 *       than min_contig_len and loop contigs already dropped by the caller (ContigReader::SetMinLen / SetDiscardFlag); ids are
 *       the indices.  Every sparsity-th seed of seed_kmer (1..32) bases, keyed by its canonical form; a key seen twice is never
 *       used.  *index_size = distinct keys (the reference's "index size").  Contigs and table live in workspaces: mhx_trim and
 *       mhx_reset drop the index.  Fewer than 2^31 contigs, each shorter than 2^30 bases.
 *   mhx_local_map     HashMapper::TryMap of every loaded read (FORWARD orientation: mhx_load_bin_records(..., reverse = 0))
 *       into MHX_BUF_LOCAL_REC; *n_valid = records with valid != 0.  Without an index: the error "run mhx_local_index first".
 *       Read ids of 2^44 and more are an error.  Loading or appending sequences afterwards invalidates the records:
 *       mhx_local_collect then fails until mhx_local_map ran again.
 *   mhx_local_insert_size  EstimateInsertSize + LocalRange of one library [lib_begin, lib_end) on those records; read_len[i] =
 *       length of read i (indexed like rec).  Pure host code without a device call: works on a machine without a GPU.
 *       Unpaired: mean = sd = 0.  *local_range = min(650, paired && mean >= max_read_len ? (int32) min(2 mean, mean + 3 sd)
 *       : max_read_len - 1).
 *   mhx_local_collect MapToContigs' AddSingle / AddMate of n_libs libraries, each with its own range (at most 2^14: larger
 *       contig offsets do not fit the items and are an error; paired libraries hold an even number of reads), into
 *       MHX_BUF_LOCAL_ITEMS / _OFFSETS: what MappingResultCollector::GetMappingResults returns for every (contig, end), end 0 =
 *       the contig's start ("fwd"), values offset | is_mate:1 | min(mismatch, 15):4 | strand:1 | read id:44.  n_mapped[l] /
 *       n_added[l] = "aligned" / "added" of library l. ---- */
typedef struct {
  uint32_t contig_id;
  int32_t contig_from, contig_to; /* clipped to the contig, inclusive */
  int32_t query_from, query_to;
  uint32_t mismatch;
  uint32_t strand;
  uint32_t valid; /* 0: every other field is 0 */
} mhx_local_record;
int mhx_local_index(mhx_ctx *, const uint32_t *contig_packed, uint64_t contig_words, uint64_t n_contigs, const uint64_t *contig_start,
                    uint32_t seed_kmer, uint32_t sparsity, uint64_t *index_size);
int mhx_local_map(mhx_ctx *, int32_t min_mapping_len, double similarity, uint64_t *n_valid);
int mhx_local_insert_size(const mhx_local_record *rec, const uint32_t *read_len, uint64_t lib_begin, uint64_t lib_end, uint32_t max_read_len,
                          int paired, double *mean, double *sd, int32_t *local_range);
int mhx_local_collect(mhx_ctx *, uint32_t n_libs, const uint64_t *lib_begin, const uint64_t *lib_end, const int32_t *lib_paired,
                      const int32_t *lib_local_range, uint64_t *n_mapped, uint64_t *n_added);

/* B3: sort n fixed-width records in place on the GPU, ascending by the first key_words words
 * (lexicographic on uint32, as Substr::operator<, kmsort_selector.cpp:18-27); aux words ride
 * along.  Replaces SelectSortingFunc(key_words, aux_words) (kmsort_selector.cpp:61-63).  Stable. */
int mhx_sort_records(mhx_ctx *, uint32_t *host_items, uint64_t n, uint32_t key_words, uint32_t aux_words);

/* ---- multi-GPU: one handle per GPU/process.  The 65536 lv1 buckets are split into
 * contiguous owner ranges; every rank extracts the items of ITS reads, partitions them by owner
 * (one stable multisplit pass), the caller moves them with an all-to-all on its own communication
 * backend (or lets mhx_comm / mhx_dist_* below do it over RCCL), and every rank sorts + reduces the
 * buckets it owns — the reference's OffsetFiller::IsHandling bucket filter (base_engine.h:106-108)
 * turned into an exchange.  All three sub-programs are supported (BASELINE configs[2..4]). ---- */
int mhx_set_partition(mhx_ctx *, int my_part, int n_parts, const uint32_t *bucket_begin /* n_parts+1 */);
/* This rank's reads sit at base offset pos_base of a global read set of global_bases bases
 * (is_solid then spans the global set).  (0, 0) switches the global layout off. */
int mhx_set_global_layout(mhx_ctx *, uint64_t pos_base, uint64_t global_bases);
enum mhx_stage {
  MHX_STAGE_S1 = 1,        /* read2sdbg stage 1, no mercy: compact items */
  MHX_STAGE_S2 = 2,        /* read2sdbg stage 2 */
  MHX_STAGE_COUNT = 3,     /* count */
  MHX_STAGE_SEQ2SDBG = 4,  /* seq2sdbg */
  MHX_STAGE_S1_MERCY = 5   /* read2sdbg stage 1 with mercy candidates: full items (prev/next, 64-bit position) */
};
typedef struct {
  void *d_items;       /* device pointer: items grouped by owner, owners ascending */
  uint64_t n_items;
  uint32_t item_bytes;
} mhx_dist_items;
/* extract + partition; counts[p] = items destined to owner p (n_parts entries).  MHX_STAGE_S2 behind a stage 1 with a min count >= 2 at
 * k <= 22 yields the 8-byte aggregated items on every rank (a function of the arguments alone), else per-occurrence items: at k = 23..27
 * s1_agg_wide does NOT apply to a stage 1 run through these building blocks (mhx_dist_process_s1) — whether a rank's group-by leaves the
 * compact items follows its data, and only mhx_dist_read2sdbg makes the ranks agree on it before anything is exchanged */
int mhx_dist_extract(mhx_ctx *, int stage, uint32_t k, uint32_t min_count, mhx_dist_items *out, uint64_t *counts);
/* library-owned device buffer to receive n_items items into */
void *mhx_dist_recv_buffer(mhx_ctx *, uint64_t n_items, uint32_t item_bytes);
/* sort + reduce the received items: S1 sets bits of the GLOBAL bitmap MHX_BUF_IS_SOLID — by convention the bits of the
 * NON-solid (k+1)-mer occurrences of the owned buckets (fewer marks on typical inputs; summing over ranks still means
 * OR); mhx_adopt_is_solid_slice derives is_solid = "a (k+1)-mer starts here and it is not marked" for the local reads.
 * S2 emits the SdBG records of the owned buckets */
int mhx_dist_process_s1(mhx_ctx *, uint32_t k, uint32_t min_count, int want_mercy, uint64_t n_items, mhx_s1_result *out);
int mhx_dist_process_s2(mhx_ctx *, uint32_t k, uint64_t n_items, mhx_sdbg_result *out);
/* count: solid edges + bucket counts + histogram of the owned buckets; first_0_out / last_0_in of the LOCAL reads are
 * complete only after the read events have been routed (below).  seq2sdbg: SdBG records of the owned buckets (items
 * carry no positions, so the sequences may be spread over the ranks in any way; no mercy edges in this mode). */
int mhx_dist_process_count(mhx_ctx *, uint32_t k, uint32_t min_count, uint64_t n_items, mhx_count_result *out);
int mhx_dist_process_seq2sdbg(mhx_ctx *, uint32_t k, uint64_t n_items, mhx_sdbg_result *out);
/* Records keyed by a position in the GLOBAL read set, produced by the bucket owners and consumed by the rank that
 * holds the read (SURVEY §8e "secondary reductions"): the first_0_out/last_0_in updates of count
 * (kmer_counter.cpp:307-368) and the mercy candidates of read2sdbg stage 1 (read_to_sdbg_s1.cpp:466-551).
 * route: 8-byte records sorted by position + counts[p] = records for rank p, where rank p holds positions
 * [p*stride_bases, (p+1)*stride_bases); the caller moves them with an all-to-all into mhx_dist_recv_buffer;
 * apply: count -> finishes MHX_BUF_FIRST_0_OUT / MHX_BUF_LAST_0_IN; mercy -> installs the local candidate list used by
 * mhx_read2sdbg_add_mercy (which, with a global layout set, updates the adopted is_solid slice). */
enum mhx_route {
  MHX_ROUTE_COUNT_EVENTS = 1,
  MHX_ROUTE_MERCY_CAND = 2,
  /* stage 1 with the knob dist_sparse_marks set (mhx_dist_setup sets it): the global positions of the NON-solid
   * (k+1)-mer occurrences of the owned buckets; apply: the read owner derives its local is_solid from them — nothing of
   * the size of the global read set is allocated or reduced */
  MHX_ROUTE_S1_MARKS = 3
};
int mhx_dist_route_records(mhx_ctx *, int which, uint64_t stride_bases, mhx_dist_items *out, uint64_t *counts);
int mhx_dist_apply_routed(mhx_ctx *, int which, uint64_t n_records);
/* raw device pointer of a result buffer (for collectives on it); NULL if absent */
void *mhx_device_pointer(mhx_ctx *, int which);
/* after the bitmap reduction: install this rank's slice (device pointer, n_words uint64) as the
 * local is_solid used by stage 2 */
int mhx_adopt_is_solid_slice(mhx_ctx *, const void *d_words, uint64_t n_words);

/* ---- multi-GPU behind the C ABI: communicator + collective drivers (megahit_amd/csrc/comm.hip).  One rank per GPU;
 * ranks are threads of one process (mhx_core --gpus N) or separate processes (bench.py --gpus N).  The drivers are
 * COLLECTIVE: every rank calls them with the same arguments.  They replace, for N GPUs, what BaseSequenceSortingEngine::Run
 * does for N OpenMP threads (base_engine.cpp:143-211,318-363): lv1 buckets -> owners, one item all-to-all per stage
 * (RCCL ncclSend/ncclRecv over xGMI, <= 256 MiB per message), position-keyed records routed back to the read owners. ---- */
typedef struct mhx_comm mhx_comm;
#define MHX_COMM_ID_BYTES 128
/* RCCL transport: one rank creates the id and ships its 128 bytes to the others by any means (the launcher's store,
 * a file, a broadcast), then every rank calls mhx_comm_init_rank with the handle of ITS GPU.  n_ranks == 1 with
 * id == NULL gives a trivial communicator without RCCL.  Returns NULL on error. */
int mhx_comm_unique_id(void *id /* MHX_COMM_ID_BYTES */);
mhx_comm *mhx_comm_init_rank(mhx_ctx *, const void *id, int rank, int n_ranks);
/* A communicator whose bytes the CALLER moves, through host memory — e.g. torch.distributed over gloo when the ranks are
   processes without a shared RCCL world (several processes on one GPU; tests/test_gpu_multiprocess.py).  libmhx stages the
   per-peer segments in host memory and calls back; the callbacks return 0 on success.
     all_reduce_u64    in-place element-wise sum (is_max = 0) or max (is_max = 1) of n 64-bit values over all ranks; the max
                       may be computed on the values read as SIGNED 64-bit (libmhx only mixes values of one sign per element)
     all_to_all_bytes  send / recv: the segments for / from rank 0, 1, ... back to back, send_bytes[p] / recv_bytes[p] bytes
                       (0 for the caller's own rank) */
typedef struct mhx_host_transport {
  int (*all_reduce_u64)(void *user, uint64_t *values, uint64_t n, int is_max);
  int (*all_to_all_bytes)(void *user, const void *send, const uint64_t *send_bytes, void *recv, const uint64_t *recv_bytes);
  void *user;
} mhx_host_transport;
mhx_comm *mhx_comm_init_hosted(mhx_ctx *, int rank, int n_ranks, const mhx_host_transport *t);
/* in-process transport without RCCL: the n ranks are threads of this process and may share GPUs (tests); exchanges are
 * device-to-device copies between the ranks' buffers.  out receives n handles, out[r] bound to ctxs[r]. */
int mhx_comm_local_group(int n_ranks, mhx_ctx *const *ctxs, mhx_comm **out);
void mhx_comm_destroy(mhx_comm *);
int mhx_comm_rank(const mhx_comm *);
int mhx_comm_size(const mhx_comm *);
int mhx_comm_barrier(mhx_comm *);
/* payload bytes this rank has handed to OTHER ranks through the item / record exchanges since the last reset (what crosses xGMI) */
uint64_t mhx_comm_bytes_sent(mhx_comm *, int reset);
/* Device memory of the planned stages of this rank's mhx_dist_* calls so far, in call order; returns their number and, for
   0 <= i < that number, fills record i: the stage (enum mhx_stage), the bytes libmhx held in this process when the stage's plan
   was made, their peak until its last pass was done (mhx_alloc_peak: process-wide, so ranks that are threads of one process
   count together) and the free bytes the plan was made with.  clear != 0 forgets the records after reading.  Any pointer may be NULL. */
int mhx_dist_plan_memory(mhx_comm *, int i, int *stage, uint64_t *held_at_plan, uint64_t *peak, uint64_t *budget, int clear);
int mhx_comm_all_reduce_u64(mhx_comm *, uint64_t *values, uint64_t n, int is_max /* else sum */);
/* agree on the bucket partition (balance_stage = 0: equal ranges; else an enum mhx_stage whose all-reduced lv1 bucket
 * histogram balances the ranges) and on the global read layout (rank r's bases at r * stride); sets dist_sparse_marks */
int mhx_dist_setup(mhx_ctx *, mhx_comm *, int balance_stage, uint32_t k, uint32_t min_count);
/* read2sdbg over all ranks: afterwards every handle holds the SdBG records of ITS bucket range (MHX_BUF_SDBG_BYTES,
 * MHX_BUF_BUCKET_*: one file of the reference's multi-file .sdbg.<i> format) and MHX_BUF_MUL_HIST of its buckets.
 * need_mercy as want_mercy of mhx_read2sdbg_s1. */
int mhx_dist_read2sdbg(mhx_ctx *, mhx_comm *, uint32_t k, uint32_t min_count, int need_mercy, mhx_s1_result *out1,
                       mhx_sdbg_result *out2, uint64_t *num_mercy);
/* count: edges / bucket counts / histogram of the owned buckets, first_0_out / last_0_in of the local reads */
int mhx_dist_count(mhx_ctx *, mhx_comm *, uint32_t k, uint32_t min_count, mhx_count_result *out);
/* seq2sdbg: the loaded sequences (+ multiplicities) may be spread over the ranks in any way */
/* collective GenMercyEdges (seq_to_sdbg.cpp:171-357) for `seq2sdbg --need_mercy` on several GPUs: the (k+1)-mer edges are
   sharded over the ranks (mhx_load_edges of a contiguous slice each; a rank may hold none), EVERY rank passes ALL candidate
   reads; has_in / has_out are OR-ed over the ranks, each mercy edge is appended on exactly one rank.  *num_mercy = all. */
int mhx_dist_gen_mercy_edges(mhx_ctx *, mhx_comm *, uint32_t k, const uint32_t *cand_packed, uint64_t cand_words, uint64_t n_cand,
                             const uint64_t *cand_start, uint64_t *num_mercy);
int mhx_dist_seq2sdbg(mhx_ctx *, mhx_comm *, uint32_t k, mhx_sdbg_result *out);

/* ---- memory-bounded operation: the reference's lv1 passes (base_engine.cpp:54-141,213-281) ----
 * By default an engine call materialises all its items at once.  For inputs whose items exceed HBM, run the call
 * once per set of lv1 buckets: with a filter set, items are extracted over batches of reads (batch_bytes of staging,
 * 0 = 1 GiB) and only those of the kept buckets are stored, so the working set is 2 x expected_items x item size.
 * keep: 65536 flags (NULL switches the filter off); expected_items: an upper bound of the items in the kept buckets
 * (sum of mhx_bucket_histogram over them).  The outputs of a filtered call cover the kept buckets only (edges / SdBG
 * records and the per-bucket tables); with accumulate != 0 the state that spans buckets continues from the previous
 * call instead of being reset: is_solid marks, multiplicity histogram, mercy candidates and aggregated stage-2 items
 * of read2sdbg stage 1; first_0_out / last_0_in and the histogram of count.  Like the reference, every pass rescans
 * all reads.  Works with the single-GPU calls and with mhx_dist_extract. */
uint64_t mhx_device_free_bytes(mhx_ctx *);  /* free HBM on the handle's device right now (workspaces of this handle included in "used") */
int mhx_bucket_histogram(mhx_ctx *, int stage /* enum mhx_stage */, uint32_t k, uint32_t min_count, uint64_t *hist /* 65536 */);
/* Device bytes a bucket-range pass of `stage` over n_items kept items needs for its items (sort buffers, staging, status
 * words), the stage's fixed state aside — for the sequences loaded now (stage 1 on fixed-length reads makes its records in
 * the first sort pass and needs two 12-byte buffers; the general path three item buffers).  The lean routes count what they
 * hold besides: status words over all item slots, the giant buckets' tables, and the outputs of the kept buckets at their bound
 * (aggregated stage-2 items, solid edges); the answer for n_items = 0 is the part that does not grow with the items.  The
 * allocator's headroom (a 16th) is the caller's to add.  0 on error. */
uint64_t mhx_stage_pass_bytes(mhx_ctx *, int stage, uint32_t k, uint32_t min_count, uint64_t n_items);
/* Device bytes `stage` holds besides its fixed state when it runs ONCE over everything, no filter set, where that run has a leaner
 * route than a bucket-range pass (stage 2 from a count of the (k+1)-mers: the route is switched off under a filter, so this figure
 * decides only whether one run fits; the ranges of several passes are sized with mhx_stage_pass_bytes).  n_items: the caller's
 * estimate of the stage's per-occurrence items.  0: no such route, ask mhx_stage_pass_bytes. */
uint64_t mhx_stage_once_bytes(mhx_ctx *, int stage, uint32_t k, uint32_t min_count, uint64_t n_items);
/* Device bytes stage 2 from a count of the (k+1)-mers holds besides the stage's fixed state when its count runs in passes of at most
 * pass_records records over its own lv1 bucket ranges (option s2_count_pass_items; 0: everything at once): the count's lean figure for
 * one pass (that of mhx_stage_pass_bytes(MHX_STAGE_COUNT) without the solid-edge outputs), its per-read scratch and bitmap, and the
 * accumulated items at sort time, 25 bytes each (two 8-byte buffers, the first grown by a quarter with old and new held during the
 * copy; the emission's word per item; status words and records).  The items are not known before the count: the figure takes ONE
 * aggregated or '$' item per record of the count plus 4 per read, at most est_items (the caller's estimate of the per-occurrence items,
 * as for mhx_stage_once_bytes) — every second record a new edge; the metagenome shard has 0.45 per record.  A library of less
 * redundancy exceeds it: the route checks its exact need after every pass against s2_count_budget_mb and gives up beyond it.
 * The allocator's headroom (a 16th) is the caller's to add.  0: the route does not apply (or an error). */
uint64_t mhx_s2_from_count_bytes(mhx_ctx *, uint32_t k, uint32_t min_count, uint64_t est_items, uint64_t pass_records);
int mhx_set_bucket_filter(mhx_ctx *, const uint8_t *keep, uint64_t expected_items, uint64_t batch_bytes, int accumulate);

/* ---- measurement ---- */
typedef struct {
  char name[48];
  uint32_t launches;
  double total_ms;     /* HIP-event time on the engine's stream */
  double algo_bytes;   /* algorithmic bytes moved by those launches */
} mhx_kernel_stat;
/* host seconds this process spent in hipMalloc / hipFree for libmhx's device buffers, bytes and calls of hipMalloc
   (process-wide; any pointer may be NULL).  A process started right behind another GPU process waits there. */
void mhx_alloc_stats(double *malloc_s, double *free_s, uint64_t *bytes, uint64_t *calls);
/* device bytes libmhx's buffers of this process hold right now and their high-water mark (process-wide, every handle and
   rank thread together; any pointer may be NULL).  reset_peak != 0 sets the mark to the bytes held now, after reading it:
   what a memory plan is held to (mhx_core's "Device memory of <stage>" lines). */
void mhx_alloc_peak(uint64_t *held_now, uint64_t *peak, int reset_peak);
int mhx_profile_enable(mhx_ctx *, int on);
int mhx_profile_reset(mhx_ctx *);
/* returns number of distinct kernels; fills up to cap entries */
int mhx_profile_get(mhx_ctx *, mhx_kernel_stat *out, int cap);

#ifdef __cplusplus
}
#endif
#endif
