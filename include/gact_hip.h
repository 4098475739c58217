/*
 * gact_hip.h -- C-ABI of the MI355X-native GACT tiled-alignment engine.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch
 * types.  Each entry point names the reference interface it stands under
 * (file:line in Tongdongq/darwin-gpu); the C++ shim that keeps the
 * reference's own gact.h / align.h signatures on top of it is
 * darwin-gpu_amd/host/, and INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns 0 on success, a negative GACT_HIP_E* code on
 *     failure; gact_hip_last_error() returns the calling thread's message.
 *     (The reference has no return codes: cudaSafeCall prints and exit(-1)s,
 *     cuda_header.h:309-319; the shim reproduces that.)
 *   - `slot` is the feeder-thread index the reference passes around as a
 *     GPU_storage (gact.h:51-67, darwin.cpp:625): each slot owns a HIP stream
 *     and its buffers, so N host threads may call concurrently with N
 *     different slots.
 *   - caller owns every host buffer; the engine owns all device memory.
 *   - there is no CPU fallback: without a usable gfx950 device
 *     gact_hip_create fails.
 */
#ifndef GACT_HIP_H
#define GACT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GACT_HIP_OK          0
#define GACT_HIP_EINVAL     -1   /* bad argument / unsupported parameter   */
#define GACT_HIP_EDEVICE    -2   /* HIP runtime error                      */
#define GACT_HIP_ENOMEM     -3
#define GACT_HIP_ERANGE     -4   /* descriptor points outside a sequence   */

/* Largest tile_size: the reference's CPU AlignWithBT asserts ref_len, query_len < 2049 (align.h:19, align.cpp:66-67); its
 * CUDA kernel stops at 324 (cuda_header.h:45), and every caller in the reference passes tile_size = 320 (params.cfg:22).
 * Up to GACT_HIP_FAST_TILE the register-tiled kernels run (packed int16 where the scoring allows); beyond it, one wave
 * per tile with the pointer matrix in HBM (csrc/gact_big.hpp): the whole interface, at a fraction of the speed. */
#define GACT_HIP_FAST_TILE  512
#define GACT_HIP_MAX_TILE   2048

/* traceback states, align.h:23 */
#define GACT_STATE_Z 0
#define GACT_STATE_D 1   /* '-' in ref, consumes a query base (gact.cpp:126-130) */
#define GACT_STATE_I 2   /* '-' in query, consumes a ref base (gact.cpp:121-125) */
#define GACT_STATE_M 3

/* Ops of an alignment path (gact_hip_candidates_paths), BAM's CIGAR numbering and SAM's names, relative to the
 * reference -- the inverse of GACT's own state names:
 *   GACT_STATE_M, equal bases   -> '=' GACT_PATH_OP_EQ   (raw sets: raw byte equality, case matters, N == N: align.cpp:134)
 *   GACT_STATE_M, unequal bases -> 'X' GACT_PATH_OP_X
 *   GACT_STATE_D ('-' in ref)   -> 'I' GACT_PATH_OP_I    (consumes a query base)
 *   GACT_STATE_I ('-' in query) -> 'D' GACT_PATH_OP_D    (consumes a ref base)
 * An op word is len << 4 | op. */
#define GACT_PATH_OP_I   1
#define GACT_PATH_OP_D   2
#define GACT_PATH_OP_EQ  7
#define GACT_PATH_OP_X   8

/* which resident sequence set a descriptor addresses */
#define GACT_SET_REF       0   /* reference_seqs   (gact.cpp:40) */
#define GACT_SET_QUERY     1   /* reads_seqs       (gact.cpp:42) */
#define GACT_SET_QUERY_RC  2   /* rev_reads_seqs   (gact.cpp:43) */
#define GACT_NUM_SETS      3

typedef struct gact_hip_engine gact_hip_engine;

/*
 * Replaces the argument list of GPU_init (gact.h:85-87, cuda_host.cu:193-237)
 * plus the globals gact.cpp reads (gact.h:25-32): params.cfg values.
 * Scoring domain: mismatch <= 0, gap_open <= 0, gap_extend <= 0 (the
 * reference's traceback reads out of bounds otherwise, align.cpp:211-226).
 */
typedef struct {
    int32_t tile_size;                  /* params.cfg GACT_extend.tile_size   (<= GACT_HIP_MAX_TILE) */
    int32_t tile_overlap;               /* early_terminate = tile_size - tile_overlap, gact.cpp:94 */
    int32_t match, mismatch, gap_open, gap_extend;
    int32_t first_tile_score_threshold; /* gact.cpp:107 */
    int32_t device_id;                  /* reference hard-wires 0, cuda_host.cu:195 */
    int32_t n_slots;                    /* = num_threads of GPU_init */
    int32_t max_blocks;                 /* 0: every launch may fill the device (each slot then owns a traceback workspace for that
                                           many resident tiles, 1.3 GB at the reference's parameters); > 0: no launch of this
                                           engine uses more blocks, and the workspaces are sized for that -- an engine that only
                                           ever sees a handful of tiles or candidates per call (the shim's AlignWithBT / GACT) */
} gact_hip_params;

/* GPU_init: cuda_host.cu:193-237 */
int gact_hip_create(const gact_hip_params *params, gact_hip_engine **out);
/* GPU_close: cuda_host.cu:239-258 */
void gact_hip_destroy(gact_hip_engine *e);
const char *gact_hip_last_error(void);

/* device facts used by the measurement harness (rocminfo values) */
typedef struct {
    int32_t compute_units;
    int32_t clock_mhz;
    int32_t waves_per_cu;     /* resident waves per CU of the DP kernel */
    int32_t wave_size;
    int64_t hbm_bytes;
    char    arch[32];
} gact_hip_device_info;
int gact_hip_get_device_info(gact_hip_engine *e, gact_hip_device_info *info);

/*
 * Makes a read set resident in HBM (replaces the per-batch substr + interleave
 * + 2 H2D copies + gasal_pack_kernel of gact.cpp:400-407, cuda_host.cu:85-169
 * and cuda_header.h:47-90).  `concat` holds n_seqs sequences back to back,
 * sequence s = concat[offsets[s] .. offsets[s+1]).  Bytes may be ASCII
 * (CPU build) or the GPU build's 0..3 recode (A0 C1 T2 G3, darwin.cpp:320-332).
 * Bases are kept 2 bits each, 16 per uint32, when every byte is one of
 * A/C/G/T (or 0..3); a set holding anything else (N, lower case) is also kept
 * as raw bytes and aligned by raw byte equality like align.cpp:134.
 */
int gact_hip_upload_seqs(gact_hip_engine *e, int which_set,
                         const uint8_t *concat, const int64_t *offsets, int32_t n_seqs);

/*
 * GACT_SET_QUERY_RC := reverse complement of every sequence of GACT_SET_QUERY, made on the device
 * (stands where darwin.cpp:110-147 builds rev_reads_seqs on the host; saves the third upload).
 * Complement as darwin.cpp:122-142: a<->t, c<->g in either case, n and N stay; any other byte is an
 * error (the reference prints "Bad Nt char" and exits).
 */
int gact_hip_derive_revcomp(gact_hip_engine *e);

/* ---- per-tile batch: what Align_Batch_GPU does (cuda_host.cu:23-190) ---- */

/*
 * One tile = one AlignWithBT call (align.cpp:60-63).  The tile slices are
 * ref[ref_off, ref_off+ref_len) of sequence ref_id in GACT_SET_REF and
 * query[query_off, ...) of sequence query_id in `query_set`.
 * `reverse` and `first` have AlignWithBT's meaning (align.cpp:130: reverse
 * reads the slice back to front).  NOTE Align_Batch_GPU's reverses[] has the
 * opposite sense (cuda_host.cu:92-142 byte-reverses when reverses[t]==0);
 * the shim flips it.
 */
typedef struct {
    int32_t ref_id, query_id;
    int32_t ref_off, query_off;
    int32_t ref_len, query_len;      /* 0..tile_size; ref_len < 0 marks an idle slot (cuda_host.cu:70) */
    uint8_t reverse, first, query_set, pad;
} gact_tile;

/* out[0..4] of the reference's per-tile int block (cuda_header.h:254-302) */
typedef struct {
    int32_t score;        /* first ? max_score : pos_score  (align.cpp:190-199) */
    int32_t max_i, max_j; /* 1-based arg-max, first tiles only, else 0 */
    int32_t ref_steps;    /* i_steps of align.cpp:187 (ref bases consumed)   */
    int32_t query_steps;  /* j_steps (query bases consumed)                  */
    int32_t n_states;
} gact_tile_result;

/*
 * Aligns n tiles.  states receives, for tile t, n_states bytes (GACT_STATE_*)
 * at states + t*states_stride, in traceback order (the order AlignWithBT
 * pushes them).  states_stride must be >= 2*tile_size.
 */
int gact_hip_align_tiles(gact_hip_engine *e, int slot, int32_t n, const gact_tile *tiles,
                         gact_tile_result *results, uint8_t *states, int32_t states_stride);

/*
 * Same, with the tile slices passed inline like Align_Batch_GPU's
 * std::vector<std::string> arguments: tile t's ref bytes at
 * ref_bases + t*seq_stride (ref_lens[t] of them), likewise query.
 */
int gact_hip_align_tiles_inline(gact_hip_engine *e, int slot, int32_t n,
                                const uint8_t *ref_bases, const uint8_t *query_bases,
                                int32_t seq_stride,
                                const int32_t *ref_lens, const int32_t *query_lens,
                                const uint8_t *reverses, const uint8_t *firsts,
                                gact_tile_result *results, uint8_t *states, int32_t states_stride);

/* ---- per-candidate batch: what GACT / GACT_Batch do (gact.cpp:48-560) ---- */

/* the seed hit darwin.cpp:216-238 turns into a GACT_call */
typedef struct {
    int32_t ref_id, query_id, ref_pos, query_pos;
} gact_candidate;

/* one record per candidate, same order as the input */
typedef struct {
    int32_t ref_id, query_id;
    int32_t ab, ae, bb, be;     /* gact.cpp:219-222 */
    int32_t score;              /* total_score, gact.cpp:197-210 */
    int32_t comp;
    int32_t emitted;            /* 1 iff gact.cpp:213 would print the line */
    int32_t first_tile_score;
    int32_t n_tiles;            /* AlignWithBT-equivalents executed */
    int32_t reserved;
    int64_t cells;              /* sum of ref_len*query_len over those tiles */
} gact_overlap;

/*
 * Extends n candidates to overlaps on the device: the whole tile chain of
 * GACT (gact.cpp:82-195), the rescoring (gact.cpp:197-210) and the emit test
 * (gact.cpp:213) run inside one persistent kernel; no host round trip per
 * tile.  complement selects GACT_SET_QUERY_RC as darwin.cpp:279 does.
 */
int gact_hip_extend_candidates(gact_hip_engine *e, int slot, int32_t n,
                               const gact_candidate *cands, int complement, int same_file,
                               gact_overlap *out);

/* the same in three steps so a harness can time the device part alone with
 * the inputs already resident in HBM */
int gact_hip_candidates_upload(gact_hip_engine *e, int slot, int32_t n, const gact_candidate *cands);
int gact_hip_candidates_run(gact_hip_engine *e, int slot, int32_t n, int complement, int same_file);
/* fetch: records [0, n) into the caller's buffer (through the engine's own pinned staging area unless `out` lies
 * inside a buffer registered with gact_hip_register_output). */
int gact_hip_candidates_fetch(gact_hip_engine *e, int slot, int32_t n, gact_overlap *out);
/* Opt-in for a caller that fetches into one long-lived buffer again and again (a feeder thread's result array; the
 * reference's counterpart is the malloc'd outs_b of cuda_host.cu:67,183-189): page-locks [buf, buf + bytes) so that
 * fetches into it are one DMA with no staging copy.  One registered buffer per slot; it must stay allocated until
 * gact_hip_unregister_output (or gact_hip_destroy).  The engine never page-locks caller memory on its own. */
int gact_hip_register_output(gact_hip_engine *e, int slot, void *buf, int64_t bytes);
int gact_hip_unregister_output(gact_hip_engine *e, int slot);
/* runs on candidates [first, first+n) of the uploaded array (multi-GPU shards) */
int gact_hip_candidates_run_range(gact_hip_engine *e, int slot, int32_t first, int32_t n,
                                  int complement, int same_file);

/* one launch over both strands: uploaded candidates with index >= rc_from are
 * the reverse-complement ones (GACT_calls_rev of darwin.cpp:266-277), the rest
 * forward (GACT_calls_for, :227-238) */
int gact_hip_candidates_run_mixed(gact_hip_engine *e, int slot, int32_t first, int32_t n,
                                  int32_t rc_from, int same_file);

/* ---- alignment paths: the edit path of every selected candidate, as CIGAR ops ----
 * The reference builds each candidate's aligned strings (gact.cpp:60-61,111-131,172-192), rescores them (:197-210) and throws
 * them away; the run entries above fold the rescoring into the traceback and keep coordinates and a score only.  This entry is
 * an opt-in SECOND pass for the candidates a caller chooses (typically the emitted ones): the int32 chain kernel runs their
 * chains once more and its walker writes every alignment column, then a compaction kernel turns the columns into ops.
 *
 * Candidates sel[0..n_sel) of the slot's candidate array (uploaded, or made by the device filter); sel == NULL: [0, n_sel).
 * n_sel == 0 returns 0 at once, also on a slot without candidates.
 * Index >= rc_from: reverse-complement strand, as in gact_hip_candidates_run_mixed.  Synchronous on the slot's stream, never
 * merged with other slots' runs; the slot's record array and run statistics stay as its last run left them.
 *   records[k]  the chain's record, equal to what every run path writes for that candidate
 *   paths[k]    op_offset: where its ops start in `ops`; n_ops; n_columns: alignment columns (= the sum of the op lengths)
 *   ops         len << 4 | GACT_PATH_OP_*, left to right along the reference, ending at (ae, be) and starting at (ab, bb) --
 *               except where the left extension aligned nothing (its first tile under the threshold, or a hit at position
 *               0): there the right extension's first tile moved the start to its arg-max (gact.cpp:162-166) while ab / bb
 *               stay where the left one stopped (:136-137).  For comp == 1 the query coordinates and ops refer to the
 *               reverse-complemented read, as bb / be do.  A chain with no tile over the threshold has no columns.
 * ops_cap too small (or ops == NULL): returns GACT_HIP_EINVAL with records, paths and *ops_needed filled -- call again with
 * room for *ops_needed ops, as gact_hip_comm_gather_lines does.  The selection runs in chunks whose column buffers (ref_len +
 * query_len bytes per candidate) fit GACT_HIP_PATH_BUDGET_MB; the buffers are allocated on the first call.  Refused
 * (GACT_HIP_EINVAL): tile_size > GACT_HIP_FAST_TILE, a slot without candidates, an index outside the slot's array. */
typedef struct {
    int64_t op_offset;
    int32_t n_ops;
    int32_t n_columns;
} gact_path;
int gact_hip_candidates_paths(gact_hip_engine *e, int slot, int32_t n_sel, const int32_t *sel, int32_t rc_from,
                              int same_file, gact_overlap *records, gact_path *paths,
                              uint32_t *ops, int64_t ops_cap, int64_t *ops_needed);
/* What the slot's last gact_hip_candidates_paths call that got as far as the device did: HIP events on the slot's stream
 * around the whole call (its kernels, copies, and the host's scan between them), chunks it ran, the most column bytes one
 * chunk took, alignment columns and ops of the selection.  The slot's gact_hip_run_stats are the normal run's. */
typedef struct {
    float device_ms;
    int32_t chunks;
    int64_t column_bytes;
    int64_t columns;
    int64_t ops;
} gact_paths_stats;
int gact_hip_last_paths_stats(gact_hip_engine *e, int slot, gact_paths_stats *stats);

/* ---- alignment summaries: what identity, NM or a PAF line need of every selected candidate's alignment, without the ops ----
 * A second opt-in pass like the one above, for the caller that does not want the alignment itself: the int32 chain kernel runs
 * the selected chains once more and its walker COUNTS the columns instead of storing them (csrc/gact_summary.hpp).
 *   sums[k]  exactly what reducing candidate k's ops of gact_hip_candidates_paths gives: columns per kind and ops (runs) per
 *            kind over the whole alignment, the left part followed by the right part -- a run that goes on from one tile into
 *            the next, or across the junction of the two parts, is one run.  eq_runs + x_runs + ins_runs + del_runs = n_ops,
 *            n_eq + n_x + ins_bases + del_bases = n_columns.  A chain with no tile over the threshold: all eight fields 0.
 * Selection (sel, sel == NULL, rc_from, same_file, n_sel == 0), records[k] and the refusals are those of
 * gact_hip_candidates_paths.  Synchronous on the slot's stream, never merged with other slots' runs; the slot's record array,
 * run statistics and paths statistics stay as they were.  One chain-kernel launch for any selection, whatever
 * GACT_HIP_PATH_BUDGET_MB says, and no device memory but the selection's candidates, records and summaries. */
typedef struct {
    int32_t n_eq, n_x;             /* '=' columns, 'X' columns */
    int32_t ins_bases, del_bases;  /* 'I' columns (query base against a gap), 'D' columns (ref base against a gap) */
    int32_t eq_runs, x_runs, ins_runs, del_runs;   /* ops of each kind in the candidate's CIGAR */
} gact_path_summary;               /* 32 bytes */
int gact_hip_candidates_summaries(gact_hip_engine *e, int slot, int32_t n_sel, const int32_t *sel, int32_t rc_from,
                                  int same_file, gact_overlap *records, gact_path_summary *sums);
/* What the slot's last gact_hip_candidates_summaries call that got as far as the device did: HIP events on the slot's stream
 * around the whole call, chain-kernel launches (1), and the device memory the call holds for itself (candidates, records,
 * summaries and one counter: proportional to n_sel, nothing sized by read length). */
typedef struct { float device_ms; int32_t launches; int64_t scratch_bytes; } gact_summaries_stats;
int gact_hip_last_summaries_stats(gact_hip_engine *e, int slot, gact_summaries_stats *stats);

/* ---- selection: every overlap once, chosen on the device ahead of the fetch and of the second passes above ----
 * D-SOFT emits one candidate per diagonal bin over the threshold and a long overlap drifts over several bins, so a read pair is
 * extended more than once and the chains converge on the same or nearly the same overlap; the reference leaves the repeats to
 * `cat darwin.*.out | sort | uniq` (README:25).  This entry returns the indices of the records to keep (csrc/gact_select.hpp):
 *   GACT_SELECT_EXACT  class: emitted records that agree in ref_id, query_id, comp, ab, ae, bb, be and score -- the fields a line
 *                      is printed from (gact.cpp:214-224), what `sort | uniq` compares.  Kept: the lowest index of each class.
 *   GACT_SELECT_PAIR   class: emitted records that agree in (ref_id, query_id, comp).  Kept: the best record of each class
 *                      under the total order 1. higher score, 2. larger (ae - ab) + (be - bb), 3. lower index.
 * Records with emitted == 0 are never selected and belong to no class.
 *   records == NULL  records [0, n) of the slot's device-resident array as its last run left them; the call waits for that run
 *                    on the slot's stream, as gact_hip_comm_gather_lines does
 *   records != NULL  the caller's n host records, copied to the device first (rank 0 of a sharded job over the records it
 *                    gathered; records that come from no alignment)
 *   sel, *n_sel      the selected indices, ascending, the same list on every call; sel can be passed unchanged as `sel` to
 *                    gact_hip_candidates_paths and gact_hip_candidates_summaries
 * Synchronous on the slot's stream; the slot's record array, run statistics, paths statistics and summaries statistics stay as
 * they were.  Device memory of its own (the table, 4 bytes per slot, and about 8 bytes per record; 56 more per host record),
 * allocated on the first call and grown on demand.  n == 0 returns 0 with *n_sel = 0.  sel_cap < *n_sel (or sel == NULL):
 * returns GACT_HIP_EINVAL with *n_sel filled -- call again with room for it, as with gact_hip_candidates_paths.  Refused
 * (GACT_HIP_EINVAL, *n_sel = 0): an unknown mode, n < 0 or n > 2^30, records == NULL on a slot without records or with n beyond
 * them. */
#define GACT_SELECT_EXACT 0
#define GACT_SELECT_PAIR  1
int gact_hip_select_overlaps(gact_hip_engine *e, int slot, int32_t n, const gact_overlap *records,
                             int32_t mode, int32_t *sel, int32_t sel_cap, int32_t *n_sel);
/* What the slot's last gact_hip_select_overlaps call that got as far as the device did: HIP events on the slot's stream around
 * the whole call (copies and kernels), emitted records among the n, records selected, slots of the table (a power of two
 * >= 2 n), and the device memory the call holds for itself. */
typedef struct { float device_ms; int32_t emitted, selected; int64_t table_slots, scratch_bytes; } gact_select_stats;
int gact_hip_last_select_stats(gact_hip_engine *e, int slot, gact_select_stats *stats);

/* ---- per-read coverage: how deep every read is covered by an overlap set, and where it is covered min_depth deep ----
 * What a consumer of the overlaps (miniasm, racon) computes first: the depth along every read, and the stretch of it that is
 * covered at least min_depth deep -- the rest is adapter or chimera and gets clipped; for reads against contigs, the depth the
 * reads give each contig.  A read-level statistic: containment and transitive reduction are gact_hip_overlap_graph's, below,
 * which takes span_begin / span_end of this table as its clip.  The records
 * are on the device when a run ends, and so are the indices of gact_hip_select_overlaps and the summaries of
 * gact_hip_candidates_summaries; this entry sweeps them there (csrc/gact_cover.hpp).
 *   records          as in gact_hip_select_overlaps: NULL = records [0, n) of the slot's device-resident array as its last run
 *                    left them (the call waits for that run on the slot's stream); else the caller's n host records, copied over
 *   sel, n_sel       which records count: sel == NULL, every record of [0, n) (n_sel is ignored); else sel[0..n_sel), the list of
 *                    gact_hip_select_overlaps unchanged.  A record with emitted == 0 never counts, named by sel or not
 *   sides            GACT_COVER_REF: a counted record puts [ab, ae) on read ref_id.  GACT_COVER_QUERY: it puts [bb, be) of its
 *                    strand on read query_id -- [bb, be) for comp == 0, [len - be, len - bb) for comp == 1, len =
 *                    read_lens[query_id].  GACT_COVER_BOTH: both; ref and query ids name the same reads (self-overlap).  No
 *                    special rule for ref_id == query_id (the run paths emit no such record with same_file, gact.cpp:213)
 *   sums             NULL, or sums[k] = the summary of the k-th chosen record (sel[k]; record k when sel == NULL).  The begins
 *                    are then ae - (n_eq + n_x + del_bases) and be - (n_eq + n_x + ins_bases): the spans gact_hip_format_paf
 *                    prints, so the result agrees with the PAF lines also where the left extension aligned nothing and ab / bb
 *                    stayed at the hit.  A summary without columns gives empty intervals
 *   read_lens        the n_reads lengths; every interval is clipped to [0, len) of its read, and an interval that is empty then
 *                    is dropped and not counted
 *   cover[i]         read i: intervals counted, the highest depth, positions with depth >= 1, positions with depth >= min_depth,
 *                    the longest run of such positions [span_begin, span_end) -- of several longest the leftmost, 0, 0 when there
 *                    is none -- and the sum of the depth over the read.  The depth of a position is the number of counted
 *                    intervals that contain it; intervals are half-open: [a, b) and [b, c) make no dip and no spike at b
 *   depth            NULL, or room for sum(read_lens) values: the depth of every position, read after read, no padding
 * Synchronous on the slot's stream; the slot's records and its run, paths, summaries and select statistics stay as they were.
 * All results are integers, the same on every call and every slot.  A read of length 0 gets all zeros; n_reads == 0 returns 0;
 * n == 0 returns 0 with every cover[i] (and depth) zero.
 * Refused with GACT_HIP_EINVAL: min_depth < 1, sides not 1, 2 or 3, n < 0 or n > 2^30, n_reads < 0, a negative length (or one
 * above 2^31 - 65), records == NULL on a slot without records or with n beyond them, n_sel < 0 with sel, an index in sel outside
 * [0, n).  Refused with GACT_HIP_ERANGE: a counted record whose read id for a requested side is outside [0, n_reads).  On a
 * refusal cover and depth are untouched.
 * Device memory of its own, one allocation per slot made on the first call, grown on demand and released with the engine:
 * 4 (sum(len) + n_reads) bytes of depth differences and 40 bytes per read, 4 sum(len) more when depth is asked for, 56 per
 * host record, 4 per sel entry, 32 per summary -- 1.7 GB for 418 Mb of reads (3.3 GB with depth).  An allocation that fails
 * returns GACT_HIP_ENOMEM.  One wave sweeps one read: right for reads, correct and slow for a chromosome-length sequence. */
#define GACT_COVER_REF   1   /* the interval a record puts on its ref_id   */
#define GACT_COVER_QUERY 2   /* the interval a record puts on its query_id */
#define GACT_COVER_BOTH  3   /* both; ref and query ids name the same read set (self-overlap) */
typedef struct {
    int32_t n_intervals;          /* intervals counted on this read (after clipping, empty ones dropped) */
    int32_t max_depth;
    int32_t covered;              /* positions with depth >= 1 */
    int32_t well_covered;         /* positions with depth >= min_depth */
    int32_t span_begin, span_end; /* the longest run of positions with depth >= min_depth, [begin, end);
                                     of several longest runs the leftmost; 0, 0 when there is none */
    int64_t depth_sum;            /* sum of depth over the read's positions */
} gact_read_cover;                /* 32 bytes */
int gact_hip_read_coverage(gact_hip_engine *e, int slot, int32_t n, const gact_overlap *records,
                           int32_t n_sel, const int32_t *sel, const gact_path_summary *sums,
                           int32_t sides, int32_t min_depth,
                           int32_t n_reads, const int32_t *read_lens,
                           gact_read_cover *cover, int32_t *depth);
/* What the slot's last gact_hip_read_coverage call that got as far as the device did: HIP events on the slot's stream around
 * the whole call (copies and kernels), the reads, the intervals counted on them, their positions (sum(read_lens)), and the
 * device memory the call holds for itself. */
typedef struct { float device_ms; int32_t reads; int64_t intervals, positions, scratch_bytes; } gact_cover_stats;
int gact_hip_last_cover_stats(gact_hip_engine *e, int slot, gact_cover_stats *stats);

/* ---- filter: the overlap set by identity, by span and by each read's own best record, decided on the device ----
 * Under +1/-1/-1/-1 two unrelated sequences align with a positive score, so a false seed hit becomes an emitted record, and
 * every pass behind a run takes what the run emitted.  The summaries of gact_hip_candidates_summaries carry n_eq, and identity
 * parts the two kinds; where no absolute threshold does (reads against contigs and a diverged copy of them), the distance to
 * the best record of the same read does.  This entry sits between the summaries and every pass that takes `sel` and `sums`
 * (csrc/gact_filter.hpp).  The rule, all integers (64-bit where a product is formed), the same on every call and slot:
 *
 *   chosen   records sel[0..n_sel) of the n records; sel == NULL: all of [0, n).  k is a record's position in that list, r =
 *            records[sel[k]] and s = sums[k]; sums is REQUIRED here.
 *   figures  cols = n_eq + n_x + ins_bases + del_bases, t_span = n_eq + n_x + del_bases, q_span = n_eq + n_x + ins_bases,
 *            ident = cols ? floor(1000 * n_eq / cols) : 0.
 *   why[k]   the first test that fails, in this order:
 *            1 GACT_FILTER_NOT_EMITTED  r.emitted == 0
 *            2 GACT_FILTER_EMPTY        cols == 0
 *            3 GACT_FILTER_IDENTITY     ident < min_identity_permille
 *            4 GACT_FILTER_SPAN         min(t_span, q_span) < min_span
 *            5 GACT_FILTER_RELATIVE     only when max_drop_permille < 1000: for some read x that the record names on a requested
 *                                       side, best[x] - ident > max_drop_permille, where best[x] is the largest ident among the
 *                                       records that passed tests 1 to 4 and name x on a requested side.  One pass, not iterated:
 *                                       a record that this test drops still counts towards best
 *            0 GACT_FILTER_KEPT         otherwise
 *   counted  a chosen record that is emitted and has cols > 0
 *   sides    GACT_COVER_REF: a record names read ref_id.  GACT_COVER_QUERY: read query_id.  GACT_COVER_BOTH: both, ref and query
 *            ids naming the same reads.  No special rule for ref_id == query_id: such a record counts once per side, as in
 *            gact_hip_read_coverage
 *   window   the per-read table covers reads [read_first, read_first + n_reads), as gact_hip_place_reads takes them.
 *            n_reads == 0: no table and no per-read work, allowed only with max_drop_permille == 1000
 *   reads[i] read read_first + i: n_records = the counted records that name it on a requested side, n_passed = those that
 *            passed tests 1 to 4, n_kept = those kept, best_permille = best[x] (0 when none passed), eq_sum and col_sum = the
 *            sums of n_eq and cols over the passed records: eq_sum / col_sum is the read's own identity estimate
 *
 * Outputs, each of which may be NULL: why[0..n_chosen); kept_at[0..*n_kept), the ascending positions k of the kept records;
 * kept_sel[0..*n_kept), the kept record indices (sel[k], or k when sel == NULL); reads[0..n_reads); *n_kept.  kept_sel goes on
 * as `sel`, and sums[kept_at[.]] as `sums`, to every pass that takes those.  cap is the room of kept_at and kept_sel; with
 * cap < *n_kept and a list given the call returns GACT_HIP_EINVAL with *n_kept filled in and the lists untouched (why and reads
 * are written) -- call again with room, as with gact_hip_select_overlaps.
 * The defaults: 650 lies between the false records of the simulator's truth block B (identity at most 557) and its true ones
 * (at least 758) at the simulator's 15 % error; it is a parameter for the data, not a calibrated constant.  The span and the
 * relative test are off by default.
 * Refused with GACT_HIP_EINVAL, outputs untouched (*n_kept = 0): sums == NULL, min_identity_permille or max_drop_permille
 * outside [0, 1000], min_span < 0, sides not 1, 2 or 3, n < 0 or n > 2^30, n_sel < 0 or n_sel > 2^30 with sel, cap < 0, an index in sel outside
 * [0, n), n_reads < 0, max_drop_permille < 1000 with n_reads == 0, records == NULL on a slot without records or with n beyond
 * them.  Refused with GACT_HIP_ERANGE: a counted record whose read id on a requested side lies outside the window, when
 * n_reads > 0; the check is made on the device before the id is used as an index.  n == 0, or an empty selection, returns 0
 * with *n_kept = 0 and a zeroed table.
 * Synchronous on the slot's stream; the slot's records and every other pass's statistics stay as they were.  Device memory of
 * its own, one allocation per slot, grown on demand: about 16 bytes per chosen record and 32 per read, 56 per host record, 4 per
 * sel entry, 32 per summary. */
#define GACT_FILTER_KEPT        0
#define GACT_FILTER_NOT_EMITTED 1
#define GACT_FILTER_EMPTY       2
#define GACT_FILTER_IDENTITY    3
#define GACT_FILTER_SPAN        4
#define GACT_FILTER_RELATIVE    5
#define GACT_FILTER_DEFAULT_MIN_IDENTITY_PERMILLE 650
#define GACT_FILTER_DEFAULT_MIN_SPAN              0
#define GACT_FILTER_DEFAULT_MAX_DROP_PERMILLE     1000
typedef struct { int32_t min_identity_permille, min_span, max_drop_permille; } gact_filter_params;     /* 12 bytes */
typedef struct { int32_t n_records, n_passed, n_kept, best_permille; int64_t eq_sum, col_sum; } gact_read_filter;   /* 32 bytes */
int gact_hip_filter_overlaps(gact_hip_engine *e, int slot, int32_t n, const gact_overlap *records,
                             int32_t n_sel, const int32_t *sel, const gact_path_summary *sums,
                             int32_t sides, int32_t read_first, int32_t n_reads,
                             const gact_filter_params *params /* NULL: defaults */,
                             int32_t *why, int32_t *kept_at, int32_t *kept_sel, int32_t cap, int32_t *n_kept,
                             gact_read_filter *reads);
/* What the slot's last gact_hip_filter_overlaps call that got as far as the device and was not refused there did: HIP events on
 * the slot's stream around the whole call (copies and kernels), the reads of the window, the chosen records, the counted ones,
 * the kept ones, the dropped ones per reason, and the device memory the call holds for itself.  A call that is refused -- on the
 * host, or by the device's check of sel and of the window -- leaves the figures of the call before it; a call that lacks room
 * for its lists is not such a refusal and leaves its own. */
typedef struct { float device_ms; int32_t reads; int64_t chosen, counted, kept, not_emitted, empty, identity, span, relative,
                 scratch_bytes; } gact_filter_stats;
int gact_hip_last_filter_stats(gact_hip_engine *e, int slot, gact_filter_stats *stats);

/* ---- placement: where every read goes -- primary, supplementary and secondary records, and a MAPQ ----
 * What a user who maps reads against a reference or against contigs asks first: where does this read go, how sure is that, is
 * the read split between two places.  GACT_SELECT_PAIR answers per (ref, query, strand) only; this entry orders ALL records of
 * a read, across references and strands, and says of each what a mapper says of it (csrc/gact_place.hpp).  The records of a
 * query read sit together on the slot that ran its batch (gact_hip_dsoft_query(first_query, n_queries)), so a feeder places its
 * reads behind its run, before anything is fetched.  The rule, all integers, the same on every call and slot:
 *
 *   chosen   records sel[0..n_sel) of the n records; sel == NULL: all of [0, n) (n_sel is not read then, but for its sign).  k is
 *            a record's position in that list; an index that sel repeats is a chosen record of its own; sums[k], when given,
 *            belongs to chosen record k, as in gact_hip_read_coverage.
 *   counted  a chosen record is counted iff it is emitted and its query interval is not empty: the interval GACT_COVER_QUERY
 *            puts on the ORIGINAL read -- [bb', be) for comp == 0, [len - be, len - bb') for comp == 1, bb' = be - (n_eq + n_x +
 *            ins_bases) when sums is given, else bb -- clipped to [0, len).  A record that is not counted gets kind
 *            GACT_PLACE_NONE, mapq 0, parent -1 and rank -1.
 *   order    the counted records of one query_id, by 1. higher score, 2. larger (ae - ab) + (be - bb), 3. lower k.  rank is a
 *            record's position in that order, from 0.
 *   walk     through the read's records in rank order, with a list of PARENTS in the order they were made.  The current record
 *            t is tested against every parent p in that order: ov = min(e_t, e_p) - max(b_t, b_p), and p MASKS t iff ov > 0 and
 *            1000 * ov >= mask_permille * min(e_t - b_t, e_p - b_p) (64-bit; abutting intervals never mask).  If some parent
 *            masks t: t is GACT_PLACE_SECONDARY and its parent is the k of the first parent that masks it.  Else, with fewer
 *            than GACT_PLACE_MAX_PARENTS parents, t becomes a parent: GACT_PLACE_PRIMARY if it is the read's first one, else
 *            GACT_PLACE_SUPPLEMENTARY; its parent is its own k.  Else t is GACT_PLACE_EXTRA: parent its own k, not a parent,
 *            and nothing is tested against it.
 *   mapq     of a parent: s1 = its own score, s2 = the highest score among its secondaries (0 without any), clamped to
 *            [0, s1] (to 0 when s1 < 0); mapq = s1 <= 0 ? 0 : mapq_cap * (s1 - s2) / s1, floored, in 64 bits.  Secondaries,
 *            extras and NONE get 0.  A STATED RULE WITH TWO PARAMETERS, NOT A CALIBRATED MODEL: mapq says how far the best
 *            competing record of the same stretch falls short in score, nothing about an error probability.  The defaults follow
 *            minimap2's conventions (mask at half the shorter interval, MAPQ up to 60); they are parameters, not measurements.
 *
 *   records, sel, n_sel, sums   as in gact_hip_read_coverage; records == NULL: the slot's device array behind its last run
 *   window   reads [read_first, read_first + n_reads) of the query set; read_lens[i] is the length of read read_first + i
 *   place    NULL, or one gact_placement per chosen record
 *   reads    NULL, or one gact_read_place per read of the window: n_records = its counted records, primary = the chosen index k
 *            of its primary or -1, the counts per kind, score / second / mapq = the primary's s1, s2 and mapq.  A read without
 *            counted records is all zero with primary = -1.
 * Refused with GACT_HIP_EINVAL: mask_permille outside [0, 1000], mapq_cap outside [0, 255], negative n (or n > 2^30), n_sel,
 * n_reads or read_first, NULL read_lens with n_reads > 0, a negative length, records == NULL on a slot without records or with
 * n beyond them, an index in sel outside [0, n).  Refused with GACT_HIP_ERANGE: an emitted chosen record whose query_id lies
 * outside the window (its interval cannot be made without its read's length); the check is made on the device before the id
 * is used as an index.  On a refusal place and reads are untouched.  n_reads == 0 returns 0 and writes nothing; no chosen
 * record (n_sel == 0, or n == 0 without sel) returns 0 with every reads[i] empty.
 * Synchronous on the slot's stream; the slot's records and its run, paths, summaries, select, cover and graph statistics stay
 * as they were.  Device memory of its own, one allocation per slot, grown on demand: 80 bytes per chosen record and 44 per
 * read, 56 per host record, 4 per sel entry, 32 per summary.  One wave places one read, and ranks its m records in about
 * m * m / 64 steps: right for reads against a reference (tens of records), correct and slow for a read with many thousands. */
#define GACT_PLACE_NONE          0
#define GACT_PLACE_PRIMARY       1
#define GACT_PLACE_SUPPLEMENTARY 2
#define GACT_PLACE_SECONDARY     3
#define GACT_PLACE_EXTRA         4
#define GACT_PLACE_MAX_PARENTS   64
#define GACT_PLACE_DEFAULT_MASK_PERMILLE 500
#define GACT_PLACE_DEFAULT_MAPQ_CAP      60
typedef struct { int32_t mask_permille, mapq_cap; } gact_place_params;
typedef struct { int32_t kind, mapq, parent, rank; } gact_placement;                 /* 16 bytes, one per chosen record */
typedef struct { int32_t n_records, primary, n_supplementary, n_secondary, n_extra,
                 score, second, mapq; } gact_read_place;                             /* 32 bytes, one per read of the window */
int gact_hip_place_reads(gact_hip_engine *e, int slot, int32_t n, const gact_overlap *records,
                         int32_t n_sel, const int32_t *sel, const gact_path_summary *sums,
                         int32_t read_first, int32_t n_reads, const int32_t *read_lens,
                         const gact_place_params *params /* NULL: defaults */,
                         gact_placement *place, gact_read_place *reads);
/* What the slot's last gact_hip_place_reads call that got as far as the device did: HIP events on the slot's stream around the
 * whole call (copies and kernels), the reads of the window, the most counted records on one read, the counted records, the
 * parents (primaries and supplementaries), secondaries and extras among them, and the device memory the call holds for itself. */
typedef struct { float device_ms; int32_t reads, max_records, reserved; int64_t counted, parents, secondaries, extras, scratch_bytes; } gact_place_stats;
int gact_hip_last_place_stats(gact_hip_engine *e, int slot, gact_place_stats *stats);

/* ---- overlap graph: containment, bidirected dovetail arcs and their transitive flags, made on the device ----
 * The step between an all-vs-all overlap set and an assembler's layout stage (miniasm's): every overlap is classified against the
 * clipped reads, contained reads are marked, every dovetail overlap between two reads that are not contained becomes an arc and
 * its complement, and the arcs a triangle explains are flagged (csrc/gact_graph.hpp).  All integer, order-free.
 * Inputs.
 *   records, n, sel, n_sel, sums   exactly as gact_hip_read_coverage takes them: records == NULL is the slot's device array; a
 *                    record counts when it is emitted and named by sel (sel == NULL: every record of [0, n)); with sums the
 *                    begins are ab' = ae - (n_eq + n_x + del_bases), bb' = be - (n_eq + n_x + ins_bases), else ab' = ab, bb' = bb.
 *                    Ref and query ids name the same read set
 *   read_lens        the n_reads lengths
 *   clip             NULL: every read whole; else clip[2 i], clip[2 i + 1] = [cb, ce) of read i, 0 <= cb <= ce <= len: the caller
 *                    passes cover[i].span_begin / span_end of gact_hip_read_coverage
 *   params           NULL: GACT_GRAPH_DEFAULT_*.  max_hang, int_permille, min_ovlp, fuzz, all >= 0, int_permille <= 1000.  The
 *                    defaults are parameters chosen after miniasm's usual values, not measurements
 * Vertices.  2 i is read i as stored, 2 i + 1 its reverse complement.  The complement of vertex x is x ^ 1, the complement of arc
 * u -> v is v^1 -> u^1.
 * Class of a counted record (t = ref_id, q = query_id, rev = comp != 0); the first rule that applies wins; 64-bit arithmetic:
 *   1 GACT_GRAPH_SELF     t == q
 *   2 clip.  The query's clip is taken in the frame of its strand: (cbq, ceq) becomes (len_q - ceq, len_q - cbq) when rev.  Then
 *     cut5 = max(cb_t - ab', cbq - bb', 0), cut3 = max(ae - ce_t, be - ceq, 0) and ts = ab' + cut5, qs = bb' + cut5,
 *     te = ae - cut3, qe = be - cut3: both reads' ends move together, by what the deeper clip cuts, so that (ts, qs) and (te, qe)
 *     stay points of the alignment (to within its indels) and len below is the distance between the clipped reads' heads.  (Each
 *     end clamped on its own leaves len short by the entered read's cb.)  GACT_GRAPH_DROPPED when te <= ts or qe <= qs (so every
 *     record of a read whose clip is empty).  Then all four are rebased to the clips' begins; tl, ql are the clipped lengths
 *   3 ext5 = min(qs, ts), ext3 = min(ql - qe, tl - te), sq = qe - qs, st = te - ts.  GACT_GRAPH_INTERNAL when ext5 > max_hang or
 *     ext3 > max_hang or 1000 sq < int_permille (sq + ext5 + ext3)
 *   4 q_in = qs <= ts && ql - qe <= tl - te; t_in = qs >= ts && ql - qe >= tl - te.  GACT_GRAPH_QUERY_CONTAINED /
 *     GACT_GRAPH_TARGET_CONTAINED; both true: the contained read is the one with the shorter clipped length, on a tie the one with
 *     the higher read id
 *   5 GACT_GRAPH_SHORT    sq + ext5 + ext3 < min_ovlp or st + ext5 + ext3 < min_ovlp
 *   6 GACT_GRAPH_DOVETAIL the record proposes two arcs, with ov_q = sq + ext5 + ext3 and ov_t = st + ext5 + ext3:
 *       qs > ts     (2 q + rev) -> (2 t), len = qs - ts, ov_u = ov_q, ov_v = ov_t, and its complement
 *                   (2 t + 1) -> (2 q + 1 - rev), len = (tl - te) - (ql - qe), ov_u = ov_t, ov_v = ov_q
 *       otherwise   (2 t) -> (2 q + rev), len = ts - qs, ov_u = ov_t, ov_v = ov_q, and its complement
 *                   (2 q + 1 - rev) -> (2 t + 1), len = (ql - qe) - (tl - te), ov_u = ov_q, ov_v = ov_t
 *     Every len is >= 1 by construction (a record with qs == ts, or with equal 3' rests, is a containment).
 * A chosen record that is not counted has class GACT_GRAPH_NONE.
 * Contained reads.  Read i is contained iff some counted record's class names it as the contained read; contained_by is the
 * lowest such record index, else -1.  Two records that disagree -- (a, b) says a is inside b, (b, a) says the reverse -- remove
 * both reads: known, and not repaired.
 * Arcs.  The proposals of the DOVETAIL records whose two reads are both not contained.  One arc per (u, v): among the proposals
 * for a key the one of the record with the higher score wins, then the lower record index (then the earlier place in sel, which
 * matters only when sel names a record twice).  A record proposes an arc and its complement together, and two records that share
 * one key share the other, so the same record wins both keys: the set is closed under complement, with the same `record`.
 * Output ascending by (u, len, v).
 * Transitive flags.  Bit 0 of an arc u -> x: some w exists with arcs u -> w and w -> x in the set and len(u->w) + len(w->x) <=
 * len(u->x) + fuzz.  Bit 1: bit 0 of the complement arc x^1 -> u^1.  An arc is kept iff flags == 0.  A statement about
 * triangles, independent of any processing order: not Myers' in-play walk, and no promise of connectivity.
 * Result.
 *   reads[i]    n_hits: the counted records that name the read on either side, SELF and DROPPED ones left out; n_internal: those
 *               of class INTERNAL; n_contains: the records in which this read is the container; contained_by; deg[s] / kept[s]:
 *               the arcs out of vertex 2 i + s, all of them and those with flags == 0
 *   classes     NULL, or one byte per chosen record (sel[k]; record k when sel == NULL)
 *   arcs, *n_arcs   arcs_cap too small (or arcs == NULL): GACT_HIP_EINVAL with reads, classes and *n_arcs filled -- call again
 *               with room for *n_arcs, as with gact_hip_select_overlaps; twice the chosen count always suffices
 * Synchronous on the slot's stream; the slot's records and every other statistic stay as they were.  Every output is the same on
 * every call and every slot.  n == 0 (or no chosen record) returns 0 with zeros, contained_by = -1 and *n_arcs = 0; n_reads == 0
 * returns 0 with *n_arcs = 0.
 * Refused with GACT_HIP_EINVAL: n < 0 or n > 2^28, n_reads < 0 or > 2^30, n_sel < 0 with sel, NULL read_lens, reads or n_arcs, a
 * negative length, a clip outside 0 <= cb <= ce <= len, a parameter < 0 or int_permille > 1000, records == NULL on a slot without
 * records or with n beyond them, an index in sel outside [0, n).  Refused with GACT_HIP_ERANGE: a counted record whose ref_id or
 * query_id is outside [0, n_reads).  On a refusal reads, classes and arcs are untouched.
 * Device memory of its own, one allocation per slot, grown on demand and released with the engine: about 140 bytes per chosen
 * record, 4 bytes per slot of the arc table (a power of two >= four times the chosen count), 64 bytes per read (8 more with a clip); 56 per host
 * record, 4 per sel entry, 32 per summary.  Known limit: a vertex of out-degree d costs about d^2 look-ups, made by one wave --
 * right for reads after containment, slow for a repeat hub. */
#define GACT_GRAPH_NONE             0   /* not counted: not emitted */
#define GACT_GRAPH_SELF             1
#define GACT_GRAPH_DROPPED          2
#define GACT_GRAPH_INTERNAL         3
#define GACT_GRAPH_QUERY_CONTAINED  4
#define GACT_GRAPH_TARGET_CONTAINED 5
#define GACT_GRAPH_SHORT            6
#define GACT_GRAPH_DOVETAIL         7
#define GACT_GRAPH_DEFAULT_MAX_HANG     1000
#define GACT_GRAPH_DEFAULT_INT_PERMILLE 800
#define GACT_GRAPH_DEFAULT_MIN_OVLP     1000
#define GACT_GRAPH_DEFAULT_FUZZ         1000
typedef struct { int32_t max_hang, int_permille, min_ovlp, fuzz; } gact_graph_params;
typedef struct { int32_t u, v, len, ov_u, ov_v, record, score, flags; } gact_graph_arc;      /* 32 bytes */
typedef struct { int32_t n_hits, n_internal, n_contains, contained_by, deg[2], kept[2]; } gact_graph_read;  /* 32 bytes */
int gact_hip_overlap_graph(gact_hip_engine *e, int slot, int32_t n, const gact_overlap *records,
                           int32_t n_sel, const int32_t *sel, const gact_path_summary *sums,
                           int32_t n_reads, const int32_t *read_lens, const int32_t *clip,
                           const gact_graph_params *params /* NULL: the defaults */,
                           gact_graph_read *reads, uint8_t *classes /* NULL or one per chosen record */,
                           gact_graph_arc *arcs, int64_t arcs_cap, int64_t *n_arcs);
/* What the slot's last gact_hip_overlap_graph call that got as far as the device did: HIP events on the slot's stream around the
 * whole call (copies and kernels), the reads and how many of them are contained, the chosen records per class, the arcs
 * proposed, the arcs of the set, those with flags != 0 and with flags == 0, the slots of the arc table, and the device memory
 * the call holds for itself. */
typedef struct { float device_ms; int32_t reads, contained; int64_t by_class[8], proposed, arcs, transitive, kept,
                 table_slots, scratch_bytes; } gact_graph_stats;
int gact_hip_last_graph_stats(gact_hip_engine *e, int slot, gact_graph_stats *stats);

/* ---- unitigs: tip cut, unambiguous paths, their layouts and their bases, made on the device ----
 * The last step of a layout stage, on what gact_hip_overlap_graph returned: the short dead ends are cut, every unambiguous path of
 * kept arcs becomes a unitig, and one sequence is spelled per unitig (csrc/gact_unitig.hpp).  All integer, lengths and offsets
 * in 64 bits, order-free: every output is the same on every call and every slot.
 * Inputs.
 *   read_lens, clip  the ones passed to gact_hip_overlap_graph (clip NULL: every read whole)
 *   reads, arcs      what that call returned, host arrays; of reads only contained_by is read; arcs ascending by (u, len, v)
 *   params           NULL: tip_reads = GACT_UNITIG_DEFAULT_TIP_READS, after miniasm's "fewer than 4 reads": a parameter, not a
 *                    measurement.  tip_reads >= 0; 0 cuts nothing
 * The rule.
 *   1 Vertices as in the graph.  Read i is live iff contained_by < 0 and its clipped length cl(i) = ce - cb (len without a clip) is
 *     positive; the others get state GACT_UNITIG_CONTAINED or GACT_UNITIG_EMPTY, CONTAINED first
 *   2 E0 = the arcs with flags == 0.  out(x) = the arcs of the current set out of x, in(x) = out(x^1).  An arc u -> v is a join iff
 *     out(u) == 1 and in(v) == 1; joins are closed under complement.  A chain is a maximal path of joins, a vertex without joins a
 *     chain of one; it is linear, with head h and tail t, or a cycle.  No arc joins the two vertices of one read, so no chain
 *     holds both x and x^1, and the complement of a chain is another chain, with head t^1
 *   3 Tip cut, one simultaneous round on E0: a linear chain of c reads is a tip iff c <= tip_reads and (in(h) == 0 or
 *     out(t) == 0) -- so an isolated short chain and a live read without arcs are cut; a cycle never is.  Every read of a tip
 *     gets state GACT_UNITIG_TIP.  E1 = E0 without the arcs that touch a TIP read.  Two tips at one junction are both cut, and
 *     when every branch at a junction is short, all of them are: known, not repaired
 *   4 Unitigs are the chains of E1 over the live reads that are not cut, one per complement pair: of a linear chain the
 *     orientation with the smaller head vertex (a chain of one read is its even vertex); of a cycle the orientation that holds
 *     the lowest vertex id m of the cycle and its complement (m is even), opened in front of m: first = m, last = the vertex
 *     joined to m, circular = 1.  Numbered ascending by first
 *   5 Layout.  Entry layout_at + r is the vertex of rank r; take = len of the join to the next entry, the clipped length for the
 *     last entry of a linear unitig, len of the closing arc last -> first for the last entry of a circular one; start = the sum
 *     of the takes before it; length = the sum of the takes; seq_at = the sum of the lengths of the lower-numbered unitigs.
 *     places[i] = (unitig, rank, orient = the low bit of the read's vertex in the emitted orientation, GACT_UNITIG_PLACED), or
 *     (-1, -1, 0, state) for a read that is not placed
 *   6 Bases (seq != NULL): an entry with vertex 2 i + s and take T gives the first T bases of the clipped read in that
 *     orientation -- s == 0: bytes [cb, cb + T) of read i of GACT_SET_REF; s == 1: the complements of bytes ce - 1, ce - 2, ...
 *     (ACGTNacgtn to TGCANtgcan; any other byte gives N, and is not refused) -- at seq[seq_at + start ...].  seq_cap < *seq_len:
 *     GACT_HIP_EINVAL with everything else filled and *seq_len set; call again with room, as with arcs_cap.  seq == NULL: no
 *     bases, *seq_len (where given) is still the total length
 *   7 Links are not an output: every arc of E1 that is not a join inside a unitig runs from the tail of an oriented unitig to
 *     the head of one, the closing arc of a circular unitig (and its complement) among them; the orientation is + when the
 *     vertex's low bit is places[].orient.  The driver and the model derive them
 * Refused with GACT_HIP_EINVAL, outputs untouched: a NULL among read_lens, reads, n_unitigs, places, unitigs, layout; n_reads < 0
 * or > 2^30; n_arcs < 0 or > 2^29; tip_reads < 0; a negative length; a clip outside 0 <= cb <= ce <= len; an arc with u or v
 * outside [0, 2 n_reads), with u>>1 == v>>1 or with len < 1; arcs not (strictly) ascending by (u, len, v); an arc with flags == 0
 * that names a read that is not live, or whose complement v^1 -> u^1 is not an arc with flags == 0; with seq: seq_len NULL,
 * GACT_SET_REF not uploaded, of another number of sequences or of other lengths than read_lens, or an arc with flags == 0 longer
 * than the clipped length of the read it leaves (the bases of its take would lie outside the clip; the graph call makes none).
 * The arc checks run on the device.  n_reads == 0 returns 0 with *n_unitigs = 0 and *seq_len = 0.
 * Synchronous on the slot's stream; the slot's records and every other statistic stay as they were.  Device memory of its own, one
 * allocation per slot, grown on demand: 32 bytes per arc, about 300 per read (8 more with a clip), and with seq the reads'
 * clipped lengths.  Out of scope: sharded jobs, and taking the arcs from the graph call's scratch.  Bubble popping is
 * gact_hip_pop_bubbles', below; repeated rounds of cleaning and the pruning of short overlaps are gact_hip_clean_graph's and
 * gact_hip_prune_overlaps', below that. */
#define GACT_UNITIG_DEFAULT_TIP_READS 3
#define GACT_UNITIG_PLACED    0
#define GACT_UNITIG_CONTAINED 1
#define GACT_UNITIG_EMPTY     2   /* clipped length 0 */
#define GACT_UNITIG_TIP       3
typedef struct { int32_t tip_reads; } gact_unitig_params;
typedef struct { int32_t first, last, n_reads, circular; int64_t layout_at, seq_at, length; } gact_unitig;   /* 40 bytes */
typedef struct { int32_t vertex, take; int64_t start; } gact_unitig_entry;                                    /* 16 bytes */
typedef struct { int32_t unitig, rank, orient, state; } gact_unitig_place;                                    /* 16 bytes */
int gact_hip_unitigs(gact_hip_engine *e, int slot, int32_t n_reads, const int32_t *read_lens, const int32_t *clip,
                     const gact_graph_read *reads, int64_t n_arcs, const gact_graph_arc *arcs,
                     const gact_unitig_params *params /* NULL: the defaults */,
                     gact_unitig *unitigs /* room for n_reads */, int32_t *n_unitigs,
                     gact_unitig_entry *layout /* room for n_reads */, gact_unitig_place *places /* n_reads */,
                     uint8_t *seq /* NULL: no bases */, int64_t seq_cap, int64_t *seq_len);
/* What the slot's last gact_hip_unitigs call that got as far as the device did: HIP events on the slot's stream around the whole
 * call (copies and kernels), the reads, those placed in a unitig, cut as tips and contained, the unitigs, the circular ones, the
 * longest unitig in reads and in bases, the launches of the ranking kernel (three sweeps of ceil(log2(2 n_reads)) rounds), the
 * arcs of E0 and of E1, the joins of E1 (a cycle's closing join among them), the links (rule 7), and the device memory the call
 * holds for itself. */
typedef struct { float device_ms; int32_t reads, placed, cut, contained, unitigs, circular, longest_reads, rank_launches;
                 int64_t longest_bases, e0_arcs, e1_arcs, joins, links, scratch_bytes; } gact_unitig_stats;
int gact_hip_last_unitig_stats(gact_hip_engine *e, int slot, gact_unitig_stats *stats);

/* ---- bubbles: the short alternative paths of the overlap graph, found and popped on the device ----
 * The cleaning step of a layout stage that belongs between two rounds of tip cutting (miniasm's order): a bubble is two or more
 * paths that leave one vertex and meet again a few reads later -- reads with errors, lost overlaps, arcs the triangle rule did
 * not flag -- and gact_hip_unitigs breaks the layout at every one.  This call finds them, keeps one path of each and marks the
 * rest as removed (csrc/gact_bubble.hpp).  All integer, path lengths in 64 bits, order-free across sources: every output is the
 * same on every call and every slot.  The graph is not changed: the caller writes arc_flags into the arcs' flags for a
 * following gact_hip_unitigs.
 * Inputs.  read_lens, clip, reads, arcs: the ones gact_hip_unitigs takes, with the same meaning and the same refusals (no bases
 * are asked for, so an arc may be longer than the read it leaves).
 *   skip    NULL, or one byte per read: != 0 takes the read's arcs out of the working set.  A caller who wants the tips out of
 *           the way first passes skip[i] = places[i].state == GACT_UNITIG_TIP of an earlier gact_hip_unitigs call
 *   params  NULL: max_dist = GACT_BUBBLE_DEFAULT_MAX_DIST (miniasm's usual value: a parameter, not a measurement), max_vertices =
 *           GACT_BUBBLE_MAX_VERTICES
 * The rule.
 *   1 The working set W = the arcs with flags == 0 whose two reads are not named by skip.  out(x) = the W arcs out of x, in
 *     array order; in(x) = |out(x^1)|
 *   2 One search per source s with |out(s)| >= 2.  Every seen vertex x has a record (r, d, c, pd, pred): the in-arcs not yet
 *     crossed, the least distance from s, the arc count of the best path from s, that path's length (64 bits), its last arc.
 *     s is seen with (0, 0, 0, 0, -1) and alone on a LIFO stack; pending = 0.  Repeat: pop v; out(v) empty fails with `dead`;
 *     for each arc k: v -> w of out(v) in array order:
 *       w == s, w == s^1 or w^1 seen fails with `twice`;  d' = d[v] + len > max_dist fails with `dist`;
 *       w not seen: max_vertices vertices seen already fails with `many`, else w is seen with (in(w), d', c[v] + 1, pd[v] + len,
 *       k) and pending += 1;  w seen: d[w] = min(d[w], d'), and (c, pd, pred) becomes (c[v] + 1, pd[v] + len, k) when that c is
 *       larger, or equal with a smaller pd, or both equal with a lower k;
 *       then r[w] -= 1, and at 0 w is pushed and pending -= 1.
 *     Behind the arcs of v: exactly one vertex on the stack and pending == 0: it is the sink t, the search succeeds; the stack
 *     empty fails with `open` (some seen vertex has an in-arc from outside).  A vertex is expanded only after all its in-arcs
 *     are crossed, so its record is final when it is read; at success no arc of W enters the seen set from outside and none
 *     leaves it but out of t
 *   3 A found bubble: n_vertices = the seen vertices, s and t among them; its interior = the seen vertices without s and t, never
 *     empty; its kept path = the walk back from t along pred -- the path of the most arcs, then the fewest bases; n_path = the
 *     interior vertices on it, n_removed the others; path_len = pd[t]
 *   4 owner[read] = the lowest source among the found bubbles whose interior holds a vertex of the read.  A bubble is
 *     GACT_BUBBLE_POPPED iff it owns every read of its interior, else GACT_BUBBLE_LOST.  The same bubble found from its other
 *     side (source t^1) has the same interior reads, so one of the two loses; of two nested bubbles the one that owns the
 *     contested reads pops, and the other waits for a round this call does not make
 *   5 A popped bubble removes (a) its interior reads that are not on the kept path: every W arc that touches one gets the bit
 *     GACT_GRAPH_ARC_BUBBLE and read_bubble[i] = the bubble's index; (b) every W arc x -> y with x seen, x != t, x and y both on
 *     the kept path (s and t included) that is not an arc of the path: it gets the bit and so does its complement y^1 -> x^1
 * Result.  arc_flags[k] = arcs[k].flags | (removed ? GACT_GRAPH_ARC_BUBBLE : 0); read_bubble[i] = -1 for a read nothing removed;
 * bubbles = every found bubble, POPPED and LOST, ascending by source.  bubbles_cap too small (or bubbles == NULL): GACT_HIP_EINVAL
 * with *n_bubbles, read_bubble and arc_flags filled -- call again with room for *n_bubbles, as with arcs_cap in the graph call.
 * What follows.  The arcs left (flags == 0, no bit set) are closed under complement.  After the pops out(s) == 1 for a popped
 * bubble's source, and every arc of its kept path is a join in gact_hip_unitigs' sense.  A removed read keeps no arc: a
 * following gact_hip_unitigs with tip_reads >= 1 gives it the state GACT_UNITIG_TIP, and with tip_reads == 0 makes it a unitig
 * of one read: known, and not repaired, because the unitig call does not change.
 * Refused with GACT_HIP_EINVAL, outputs untouched: what gact_hip_unitigs refuses of read_lens, clip, reads and arcs (the arc
 * checks run on the device); max_dist < 1 or > 2^30; max_vertices < 3 or > GACT_BUBBLE_MAX_VERTICES; NULL n_bubbles, read_bubble
 * or arc_flags; bubbles_cap < 0.  n_reads == 0 returns 0 with *n_bubbles = 0.
 * Synchronous on the slot's stream; the slot's records and every other statistic stay as they were.  Device memory of its own,
 * one allocation per slot, grown on demand: 36 bytes per arc and about 150 per read (8 more with a clip, 4 more with skip).
 * Out of scope: bubbles of more than 64 vertices, sharded jobs.  Repeated rounds are gact_hip_clean_graph's and the pruning of
 * short overlaps is gact_hip_prune_overlaps', both below. */
#define GACT_GRAPH_ARC_BUBBLE 4            /* bit 2 of gact_graph_arc.flags: removed by gact_hip_pop_bubbles */
#define GACT_BUBBLE_DEFAULT_MAX_DIST 50000 /* after miniasm: a parameter, not a measurement */
#define GACT_BUBBLE_MAX_VERTICES 64        /* one wave: one seen vertex per lane */
#define GACT_BUBBLE_POPPED 0
#define GACT_BUBBLE_LOST   1               /* found, but some interior read belongs to a bubble with a lower source */
typedef struct { int32_t max_dist, max_vertices; } gact_bubble_params;
typedef struct { int32_t source, sink, n_vertices, n_path, n_removed, state; int64_t path_len; } gact_bubble;  /* 32 bytes */
int gact_hip_pop_bubbles(gact_hip_engine *e, int slot, int32_t n_reads, const int32_t *read_lens, const int32_t *clip,
                         const gact_graph_read *reads, int64_t n_arcs, const gact_graph_arc *arcs,
                         const uint8_t *skip /* NULL, or n_reads bytes: != 0 takes the read's arcs out of the working set */,
                         const gact_bubble_params *params /* NULL: the defaults */,
                         gact_bubble *bubbles, int64_t bubbles_cap, int64_t *n_bubbles,
                         int32_t *read_bubble /* n_reads */, int32_t *arc_flags /* n_arcs */);
/* What the slot's last gact_hip_pop_bubbles call that got as far as the device did: HIP events on the slot's stream around the
 * whole call (copies and kernels), the reads, the sources searched from, the bubbles found, popped and lost, the reads removed,
 * the arcs of the working set and those removed, the searches that failed by their first failure (open, dead, twice, dist,
 * many, in that order), and the device memory the call holds for itself. */
typedef struct { float device_ms; int32_t reads, sources, found, popped, lost, reads_removed;
                 int64_t working_arcs, arcs_removed, by_fail[5], scratch_bytes; } gact_bubble_stats;
int gact_hip_last_bubble_stats(gact_hip_engine *e, int slot, gact_bubble_stats *stats);

/* ---- weak arcs: the overlaps that are much shorter than the best one of their vertex, marked on the device ----
 * The third cleaning step of a layout stage (miniasm's asg_arc_del_short), the one that copes with repeats: a repeat shorter than
 * the reads puts an arc between two unrelated places; that arc is not transitive, no tip and no bubble, and gact_hip_unitigs
 * breaks the layout there.  Its overlap is short beside the true ones of the same read end, and that is what this call looks
 * for (csrc/gact_clean.hpp).  All integer, the products in 64 bits, order-free: every output is the same on every call and every
 * slot.  The graph is not changed: the caller writes arc_flags into the arcs' flags for a following call.
 * Inputs.  read_lens, clip, reads, arcs, skip: the ones gact_hip_pop_bubbles takes, with the same meaning and the same refusals.
 *   params  NULL: ratio_permille = GACT_PRUNE_DEFAULT_RATIO_PERMILLE (after miniasm: a parameter, not a measurement)
 * The rule.
 *   1 The working set W = the arcs with flags == 0 whose two reads are not named by skip.  out(x) = the W arcs out of x
 *   2 A vertex with |out(x)| >= 2 is examined; best(x) = the largest ov_u over out(x).  vertex_best[x] = best(x), and 0 for a
 *     vertex that is not examined
 *   3 An arc k: x -> w of an examined vertex is weak iff 1000 * ov_u(k) < ratio_permille * best(x), the products in 64 bits.
 *     Equality is not weak; an arc of a vertex with one W arc is never weak at that vertex
 *   4 An arc is removed iff it is weak or its complement w^1 -> x^1 (found in W as the arc checks find it) is weak: the removed
 *     set is closed under complement, and an arc can go although it is the best one of its own vertex
 *   5 arc_flags[k] = arcs[k].flags | (removed ? GACT_GRAPH_ARC_SHORT : 0)
 * Refused with GACT_HIP_EINVAL, outputs untouched: what gact_hip_pop_bubbles refuses of read_lens, clip, reads and arcs (the arc
 * checks run on the device); ratio_permille outside [0, 1000]; a NULL arc_flags.  n_reads == 0 returns 0.
 * Synchronous on the slot's stream; the slot's records and every other statistic stay as they were.  Device memory of its own,
 * one allocation per slot, grown on demand: 36 bytes per arc and about 60 per read (8 more with a clip, 4 more with skip).
 * Out of scope: a cut-off on the absolute overlap length (the graph call's min_ovlp is that), sharded jobs. */
#define GACT_GRAPH_ARC_TIP    8   /* bit 3: the arc touched a read cut as a tip by gact_hip_clean_graph */
#define GACT_GRAPH_ARC_SHORT 16   /* bit 4: removed as a weak arc */
#define GACT_PRUNE_DEFAULT_RATIO_PERMILLE 500   /* after miniasm: a parameter, not a measurement */
typedef struct { int32_t ratio_permille; } gact_prune_params;
int gact_hip_prune_overlaps(gact_hip_engine *e, int slot, int32_t n_reads, const int32_t *read_lens, const int32_t *clip,
                            const gact_graph_read *reads, int64_t n_arcs, const gact_graph_arc *arcs,
                            const uint8_t *skip /* NULL, or n_reads bytes */, const gact_prune_params *params /* NULL: the default */,
                            int32_t *arc_flags /* n_arcs */, int32_t *vertex_best /* NULL, or 2 n_reads */);
/* What the slot's last gact_hip_prune_overlaps call that got as far as the device did: HIP events on the slot's stream around the
 * whole call (copies and kernels), the reads, the vertices examined, the vertices with an arc in W and none behind the call
 * (bared), the arcs of W, the weak ones (rule 3), the removed ones (rule 4), and the device memory the call holds for itself. */
typedef struct { float device_ms; int32_t reads, examined, bared; int64_t working_arcs, weak, arcs_removed, scratch_bytes; } gact_prune_stats;
int gact_hip_last_prune_stats(gact_hip_engine *e, int slot, gact_prune_stats *stats);

/* ---- cleaning in rounds: tips, bubbles and weak arcs until nothing goes, on the device ----
 * The loop of a layout stage around the three steps above (miniasm's order): cut the tips and pop the bubbles until a pass
 * removes nothing, then drop the weak arcs at a rising ratio and settle again after every drop.  The arcs are uploaded once and
 * stay on the device; every step runs the kernels of its own entry on them and ORs its bits into their flags there; the host
 * reads one small block of counts per step to decide whether to go on (csrc/gact_clean.hpp).
 * The rule runs over a flags array F, which starts as arcs[].flags.
 *   T (tips)     rules 1 - 3 of gact_hip_unitigs on the arcs with F, with tip_reads.  Every read with the state TIP is removed,
 *                and every arc with F == 0 that touches one gets GACT_GRAPH_ARC_TIP.  A read that an earlier step removed has no
 *                arc left and is a tip again; it keeps the state and the step of its first removal and is not counted again
 *   B (bubbles)  the rule of gact_hip_pop_bubbles on the arcs with F, skip NULL, with max_dist and max_vertices.  Its
 *                GACT_GRAPH_ARC_BUBBLE bits go into F, the reads it removes get the state GACT_CLEAN_BUBBLE
 *   pass         T then B.  settle: passes until one removes no arc, or until max_passes passes have been made
 *   P(r)         the rule of gact_hip_prune_overlaps on the arcs with F, skip NULL, ratio_permille = r
 *   the call     settle; then for j = 0 .. n_ratios - 1: r_j = lo + (hi - lo) * j / (n_ratios - 1) in integer division (lo when
 *                n_ratios == 1); P(r_j); if it removed an arc, settle again.  n_ratios == 0 prunes nothing
 * The log.  One gact_clean_step per T, B and P, in the order made: kind, param = tip_reads, max_dist or r_j, the reads and arcs
 * the step removed, examined = the linear chains of the tip rule (one per head vertex, so a chain and its complement count
 * twice), the sources searched from, or the vertices examined, and arcs_left = the arcs with F == 0 behind the step.
 * read_state[i] = (state, step): GACT_CLEAN_KEPT, GACT_UNITIG_CONTAINED, GACT_UNITIG_EMPTY, GACT_UNITIG_TIP or GACT_CLEAN_BUBBLE,
 * and the index of the log step that removed the read, -1 for KEPT, CONTAINED and EMPTY.  A read that lost all its arcs to a
 * prune step is KEPT until a T step cuts it.  arc_flags = F behind the last step: written into the arcs it is what a following
 * gact_hip_unitigs takes.  The arcs left are closed under complement after every step.
 * steps_cap too small (or steps == NULL): GACT_HIP_EINVAL with *n_steps, arc_flags and read_state filled -- call again with room
 * for *n_steps, as with bubbles_cap.  (n_ratios + 1) * (2 * max_passes + 1) always suffices.
 * Refused with GACT_HIP_EINVAL, outputs untouched: what gact_hip_pop_bubbles refuses of read_lens, clip, reads and arcs (the arc
 * checks run on the device); tip_reads < 1 (with 0 the removed reads would come back as unitigs of one read); max_dist and
 * max_vertices as the bubble call; a ratio outside [0, 1000] or lo > hi; n_ratios outside [0, 16]; max_passes outside [1, 16];
 * NULL arc_flags, read_state or n_steps; steps_cap < 0.  n_reads == 0 returns 0 with *n_steps = 0.
 * Synchronous on the slot's stream; the slot's records and every other statistic stay as they were.  Device memory of its own,
 * one allocation per slot, grown on demand: 36 bytes per arc and about 230 per read (8 more with a clip).
 * Out of scope: bubbles of more than 64 vertices, sharded jobs, taking the arcs from the graph call's scratch. */
#define GACT_CLEAN_TIPS    0
#define GACT_CLEAN_BUBBLES 1
#define GACT_CLEAN_PRUNE   2
#define GACT_CLEAN_KEPT    0      /* read states 1..3 are GACT_UNITIG_CONTAINED / _EMPTY / _TIP */
#define GACT_CLEAN_BUBBLE  4
#define GACT_CLEAN_MAX_RATIOS 16
#define GACT_CLEAN_MAX_PASSES 16
typedef struct { int32_t tip_reads, max_dist, max_vertices, ratio_lo_permille, ratio_hi_permille, n_ratios, max_passes; } gact_clean_params;
typedef struct { int32_t kind, param, reads_removed, examined; int64_t arcs_removed, arcs_left; } gact_clean_step;   /* 32 bytes */
typedef struct { int32_t state, step; } gact_clean_read;                                                              /* 8 bytes */
int gact_hip_clean_graph(gact_hip_engine *e, int slot, int32_t n_reads, const int32_t *read_lens, const int32_t *clip,
                         const gact_graph_read *reads, int64_t n_arcs, const gact_graph_arc *arcs,
                         const gact_clean_params *params /* NULL: 3, 50000, 64, 500, 700, 3, 4 */,
                         int32_t *arc_flags /* n_arcs */, gact_clean_read *read_state /* n_reads */,
                         gact_clean_step *steps, int64_t steps_cap, int64_t *n_steps);
/* What the slot's last gact_hip_clean_graph call that got as far as the device did: HIP events on the slot's stream around the
 * whole call (copies, kernels and the waits between the steps), the reads, the steps of the log, the passes made, the reads
 * removed as tips and by bubbles, the arcs removed by kind (GACT_CLEAN_TIPS, _BUBBLES, _PRUNE), the arcs left, and the device
 * memory the call holds for itself. */
typedef struct { float device_ms; int32_t reads, steps, passes, reads_tip, reads_bubble;
                 int64_t arcs_removed[3], arcs_left, scratch_bytes; } gact_clean_stats;
int gact_hip_last_clean_stats(gact_hip_engine *e, int slot, gact_clean_stats *stats);

/* Per-base pileup and consensus of the reads of GACT_SET_REF from the overlaps' alignments, counted on the device: every chosen
 * candidate's alignment (the one gact_hip_candidates_paths returns as a CIGAR) is stacked on its target read, every position
 * counts what the other reads say there, and the majority is the consensus.  The pileup belongs to the engine, not to a slot:
 * a read's pileup needs the candidates of every batch of queries, so it accumulates over calls and over slots.
 *   gact_hip_pileup_begin   opens a window, reads [read_first, read_first + n_reads) of GACT_SET_REF, and zeroes its counts (32
 *                           bytes per position, one allocation of the engine's, grown on demand, released with the engine); a
 *                           second begin starts over, and a begin that is refused leaves no window open, an earlier one's
 *                           neither.  n_reads == 0 is allowed.  GACT_HIP_EINVAL: GACT_SET_REF not uploaded, a
 *                           window outside it, tile_size > GACT_HIP_FAST_TILE (as gact_hip_candidates_paths, for its reason);
 *                           GACT_HIP_ENOMEM: the allocation failed
 *   gact_hip_pileup_add     sel, n_sel, rc_from, same_file: the selection of gact_hip_candidates_paths, with its conventions and
 *                           refusals (sel == NULL: candidates [0, n_sel); n_sel == 0: nothing to do, also on a slot without
 *                           candidates).  Candidates whose ref_id lies outside the window are dropped on the host; the rest run
 *                           through the path run's chunks on the slot's stream (column buffers within GACT_HIP_PATH_BUDGET_MB),
 *                           and in each chunk the pileup kernel consumes the columns behind the chain kernel.  No ops are made
 *                           and nothing but 48 bytes of error state and counters comes back.  Synchronous on the slot's stream;
 *                           any number of calls, also from several threads on different slots at once: the counts are integer
 *                           atomic adds, so the result does not depend on order or interleaving.  A candidate whose record has
 *                           emitted == 0, or that has no columns, adds nothing.  Without an open window, or after GACT_SET_REF
 *                           was uploaded again: GACT_HIP_EINVAL.  GACT_HIP_ERANGE (none is expected: every index is checked on
 *                           the device before it is used): an alignment of this add, or of an add running beside it on
 *                           another slot, lay outside the window or outside its two reads; that alignment was left out, the
 *                           add's other alignments are counted and the add is in the statistics, and the condition is reported
 *                           once -- later adds answer for themselves.  A failure of the device or of an allocation part of the
 *                           way leaves the earlier chunks' alignments counted: begin again.  The slot's records and its run, paths, summaries, select and
 *                           cover statistics stay as they were
 *   gact_hip_pileup_finish  makes the consensus and the per-read table for min_depth (>= 1) and copies back whichever of counts
 *                           (the window's positions, read after read, no padding), consensus (one byte per position, same
 *                           layout) and reads[n_reads] are not NULL.  The counts stay: finish may be called again (another
 *                           min_depth) and be followed by more adds.  Not to be called while an add is running
 * Column rules.  Every coordinate is in the record's strand, as ab .. be are: for comp == 1 the query bytes are
 * GACT_SET_QUERY_RC's and nothing is complemented.  The alignment starts at target position ae - (ref-consuming columns) and
 * query position be - (query-consuming columns): the spans gact_hip_format_paf prints, not ab / bb.  With target cursor r and
 * query cursor q:
 *   '=' / 'X'   n[kind of query byte q] += 1 (case folded; anything but acgtACGT is OTHER), n[DEPTH] += 1 at r; r++, q++
 *   'D'         n[DEL] += 1, n[DEPTH] += 1 at r; r++
 *   'I'         q++; the FIRST column of a run of 'I' adds 1 to n[INS] at min(r, len - 1): a run counts once whatever its length
 *               (also across a tile boundary or the junction of the left and the right extension).  The inserted bases are kept
 *               by a window opened with gact_hip_pileup_begin_ins (below), and by that one only
 * Consensus byte of a position: its depth < min_depth: the read's own raw byte, unchanged.  Else the largest of A, C, G, T, DEL
 * (OTHER never wins); ties go to the read's own base (case folded) if it is among the tied kinds, else in the order A, C, G, T,
 * DEL; the byte is 'A' 'C' 'G' 'T' or '-'.  All five zero (every aligned query byte was OTHER): the read's own byte, which does
 * not count as changed. */
#define GACT_PILEUP_A 0      /* query base aligned here ('=' or 'X' column), case folded: a/A ... */
#define GACT_PILEUP_C 1
#define GACT_PILEUP_G 2
#define GACT_PILEUP_T 3
#define GACT_PILEUP_OTHER 4  /* ... any other query byte (N, ...) */
#define GACT_PILEUP_DEL 5    /* a 'D' column: the alignment spans the position, no query base */
#define GACT_PILEUP_INS 6    /* 'I' RUNS directly in front of this position */
#define GACT_PILEUP_DEPTH 7  /* alignments whose columns consume this position = sum of 0..5 */
typedef struct { uint32_t n[8]; } gact_pileup_col;          /* 32 bytes per position */
typedef struct {
    int32_t n_alignments;   /* alignments with at least one column, counted on this read */
    int32_t max_depth;
    int32_t called;         /* positions with depth >= min_depth */
    int32_t changed;        /* called positions whose consensus byte is a base other than the read's own (case folded) */
    int32_t deleted;        /* called positions whose consensus is '-' */
    int32_t ins_flagged;    /* called positions with 2 * n[INS] > n[DEPTH] */
    int32_t reserved[2];
} gact_read_pileup;         /* 32 bytes */
int gact_hip_pileup_begin (gact_hip_engine *e, int32_t read_first, int32_t n_reads);
int gact_hip_pileup_add   (gact_hip_engine *e, int slot, int32_t n_sel, const int32_t *sel, int32_t rc_from, int same_file);
int gact_hip_pileup_finish(gact_hip_engine *e, int32_t min_depth, gact_pileup_col *counts, uint8_t *consensus,
                           gact_read_pileup *reads);
/* The pileup since the last gact_hip_pileup_begin: HIP-event time of its adds and finishes together (each on its own stream,
 * copies and kernels), the adds, the path-run chunks they made, the alignments counted (inside the window, emitted, with at
 * least one column), their columns, the window's positions, and the device memory the window holds. */
typedef struct { float device_ms; int32_t adds, chunks; int64_t alignments, columns, positions, scratch_bytes; } gact_pileup_stats;
int gact_hip_last_pileup_stats(gact_hip_engine *e, gact_pileup_stats *stats);

/* The inserted bases, and the corrected reads spelled on the device.  A base the target read lacks shows in the pileup as a run
 * of 'I' in front of a position; a window opened with ins_slots = K keeps the first K bases of every such run, so that the
 * consensus can put them back.
 *   gact_hip_pileup_begin_ins   gact_hip_pileup_begin with 0 <= ins_slots <= GACT_PILEUP_MAX_INS_SLOTS slots in front of every
 *                               position: one gact_pileup_ins (16 bytes) per (position, slot), laid out [positions][K] behind the
 *                               counts in the window's allocation and zeroed here, so a position takes 32 + 16 K bytes.
 *                               gact_hip_pileup_begin is ins_slots = 0: no table, and its adds run the kernel they always ran.
 *                               ins_slots outside [0, 4]: GACT_HIP_EINVAL, and no window is open
 *   gact_hip_pileup_add         counts as above, and for an 'I' column that is the j-th of its run (j from 0; a run goes on across
 *                               tile boundaries and the junction of the two extensions, as for n[INS]), with the target cursor
 *                               at r: if j < K, r < len and the query byte is one of acgtACGT, ins[r][j].n[kind] += 1.  A run
 *                               behind the read's last base (r == len) and bytes of kind OTHER add nothing to the slots; n[INS]
 *                               is counted as ever.  A run longer than K is counted once in runs_truncated
 *   gact_hip_pileup_corrected   the consensus for min_depth (>= 1) as gact_hip_pileup_finish makes it, then the slot call, then
 *                               the corrected reads.  Slot j of position p is EMITTED iff p is called (n[DEPTH] >= min_depth),
 *                               every slot below j at p is emitted, and 2 * (the slot's nA + nC + nG + nT) > n[DEPTH] of p; its
 *                               byte is 'A' 'C' 'G' 'T' by the largest of the four counts, the first of equal ones in that
 *                               order.  A corrected read is, for every position in order, its emitted slots' bytes, then its
 *                               consensus byte unless that is '-' (an uncalled position gives the read's own raw byte).  With
 *                               K = 0 that is the consensus with every '-' left out.
 *                               Outputs, any of which may be NULL: ins, the table, positions * K records; read_at[n_reads + 1],
 *                               the reads lie back to back in seq and read_at[n_reads] == *seq_len; seq, the bytes; reads
 *                               [n_reads].  seq_cap < *seq_len (with seq not NULL): GACT_HIP_EINVAL with everything else filled
 *                               in, call again with room for *seq_len; positions * (K + 1) always suffices.  Synchronous on
 *                               slot 0's stream, as finish is, and as little to be called while an add is running; the counts
 *                               stay.  All integer: the same bytes on every call, whichever slots added in whichever order.
 *                               GACT_HIP_EINVAL: no open window, GACT_SET_REF uploaded again since, min_depth < 1, seq_cap < 0,
 *                               ins not NULL on a window without slots.  The spelled bytes lie in a second allocation of the
 *                               engine's, *seq_len bytes, grown on demand. */
#define GACT_PILEUP_MAX_INS_SLOTS 4
typedef struct { uint32_t n[4]; } gact_pileup_ins;          /* A C G T (GACT_PILEUP_A ..): 16 bytes per position and slot */
typedef struct {
    int32_t length;         /* bases of the corrected read = the read's length + inserted - deleted */
    int32_t inserted;       /* emitted slots: bases put in */
    int32_t ins_sites;      /* positions with at least one emitted slot */
    int32_t deleted;        /* positions whose consensus byte is '-': left out */
    int32_t changed;        /* as gact_read_pileup's */
    int32_t reserved[3];
} gact_read_corrected;      /* 32 bytes */
int gact_hip_pileup_begin_ins(gact_hip_engine *e, int32_t read_first, int32_t n_reads, int32_t ins_slots);
int gact_hip_pileup_corrected(gact_hip_engine *e, int32_t min_depth, gact_pileup_ins *ins, gact_read_corrected *reads,
                              int64_t *read_at, uint8_t *seq, int64_t seq_cap, int64_t *seq_len);
/* The slots since the last begin: HIP-event time of the gact_hip_pileup_corrected calls (copies and kernels), the window's
 * ins_slots, the adds to slots and the runs longer than ins_slots its gact_hip_pileup_add calls made, the bases the last
 * gact_hip_pileup_corrected put in (emitted slots), and the table's bytes. */
typedef struct { float device_ms; int32_t ins_slots; int64_t slot_adds, runs_truncated, emitted, table_bytes; } gact_pileup_ins_stats;
int gact_hip_last_pileup_ins_stats(gact_hip_engine *e, gact_pileup_ins_stats *stats);

/* Variants of the open window, called from its counts on the device (csrc/gact_variants.hpp).  What a user who maps reads
 * against a reference asks of the pileup: where does the sample differ from this sequence, and in all of its reads or in part
 * of them.  The consensus cannot say: a site where 40 % of the reads differ leaves it unchanged.  The rule, all integers, the
 * same on every call, whichever slots added in whichever order:
 *
 *   params     min_depth, min_alt, min_permille, hom_permille; NULL: GACT_VARIANT_DEFAULT_* (8, 4, 250, 750).  PARAMETERS OF A
 *              STATED RULE, NOT A CALIBRATED ERROR MODEL: thresholds on counts, no likelihoods, no QUAL, no strand counts.
 *   qualifies  (a, d) iff a >= min_alt and 1000 * a >= min_permille * d (64-bit)
 *   gt         (a, d) = 2 (all reads: 1/1) if 1000 * a >= hom_permille * d, else 1 (part of them: 0/1)
 *   examined   position x of sequence i of the window, with the counts n[] (gact_pileup_col), d = n[GACT_PILEUP_DEPTH] and `own`
 *              the sequence's raw byte at x, is examined iff d >= min_depth.  A position that is not examined makes no record
 *              and breaks a deletion run.
 *   INS        only on a window opened with ins_slots = K >= 1.  s_j = slot j's four counts at x together.  The record exists
 *              iff qualifies(s_0, d); len = the number of leading slots j with qualifies(s_j, d); bases = each such slot's
 *              largest count's letter, the first of equal ones in the order A C G T, slot j's in bits [8 j, 8 j + 8) (as the
 *              slot call of gact_hip_pileup_corrected packs them); alt = s_0; GACT_VARIANT_TRUNCATED is set when len == K (the
 *              window kept no more of the run).  The inserted bases lie IN FRONT OF x.
 *   DEL        x is a deleted position iff it is examined and qualifies(n[GACT_PILEUP_DEL], d).  A maximal run of consecutive
 *              deleted positions inside one sequence is one record: pos the run's first position, len its length, alt, depth
 *              and gt those of the first position.  Runs never cross a sequence boundary.
 *   SNV        only where own is one of acgtACGT: one record per base b other than own (case folded) with qualifies(n[b], d),
 *              in the order A C G T; len = 1, alt = n[b], bases = b's upper-case letter.  An SNV inside a called deletion is
 *              reported on its own.
 *   order      by seq, then pos, then kind (INS, DEL, SNV), then the SNV's base: VCF lines made in this order have
 *              non-decreasing POS.
 *
 *   variants   NULL, or room for cap records; n_variants: NULL, or where the number of records goes; seqs: NULL, or one
 *              gact_seq_variants per sequence of the window: its examined positions, its records per kind, and `first`, the
 *              index of its first record (of the next sequence's where it has none).
 * cap < *n_variants with variants not NULL: GACT_HIP_EINVAL with *n_variants and seqs filled in, call again with room (the
 * protocol of gact_hip_pileup_corrected).  GACT_HIP_EINVAL, with every output untouched: no open window, GACT_SET_REF uploaded
 * again since, cap < 0, min_depth < 1, min_alt < 1, anything but 0 <= min_permille <= hom_permille <= 1000.  A window without
 * slots makes no INS records; an empty window makes none at all.  Synchronous on slot 0's stream, as gact_hip_pileup_finish is,
 * and as little to be called while an add is running; the counts stay: it may be called again with other parameters, and more
 * adds may follow.  One wave takes GACT_VARIANT_CHUNK consecutive positions of the window, whichever sequences they belong to,
 * so a window of a few long sequences fills the device as one of many short ones does.  Device memory of its own, one
 * allocation of the engine's, grown on demand: 1 byte per position, 8 per chunk, 32 per sequence and 32 per record. */
#define GACT_VARIANT_INS 0
#define GACT_VARIANT_DEL 1
#define GACT_VARIANT_SNV 2
#define GACT_VARIANT_TRUNCATED 4        /* bit 2 of flags */
#define GACT_VARIANT_CHUNK 4096         /* positions a wave takes: a multiple of 64 */
#define GACT_VARIANT_DEFAULT_MIN_DEPTH    8
#define GACT_VARIANT_DEFAULT_MIN_ALT      4
#define GACT_VARIANT_DEFAULT_MIN_PERMILLE 250
#define GACT_VARIANT_DEFAULT_HOM_PERMILLE 750
typedef struct { int32_t min_depth, min_alt, min_permille, hom_permille; } gact_variant_params;
typedef struct {
    int32_t seq;            /* the sequence's id in GACT_SET_REF */
    int32_t pos;            /* 0-based, on that sequence */
    int32_t kind;           /* GACT_VARIANT_* */
    int32_t len;
    uint32_t bases;         /* SNV: the alt's letter in the low byte; INS: slot j's letter in bits [8 j, 8 j + 8); DEL: 0 */
    uint32_t alt, depth;
    int32_t flags;          /* gt (1 or 2) in bits 0-1, GACT_VARIANT_TRUNCATED */
} gact_variant;             /* 32 bytes */
typedef struct { int32_t examined, n_ins, n_del, n_snv, first, reserved[3]; } gact_seq_variants;      /* 32 bytes */
int gact_hip_pileup_variants(gact_hip_engine *e, const gact_variant_params *params /* NULL: defaults */, gact_variant *variants,
                             int64_t cap, int64_t *n_variants, gact_seq_variants *seqs);
/* The last gact_hip_pileup_variants call that got as far as the device: HIP events on slot 0's stream around the whole call
 * (copies and kernels), the chunks, the records per kind, the examined positions, the device memory the pass holds. */
typedef struct { float device_ms; int32_t chunks; int64_t n_ins, n_del, n_snv, examined, scratch_bytes; } gact_variant_stats;
int gact_hip_last_variant_stats(gact_hip_engine *e, gact_variant_stats *stats);

/* ------------------------------------------------------------------------
 * D-SOFT seed filter on the device (the stage in front of the path; optional:
 * the reference's host filter keeps working against the calls above).
 *
 * gact_hip_dsoft_build stands where darwin.cpp:532-560 builds the padded
 * reference string and `new SeedPosTable(...)` (seed_pos_table.cpp:46-98): the
 * index is built over GACT_SET_REF as uploaded (ASCII bases; anything but
 * acgtACGT counts as A, ntcoding.cpp:59-71).
 * gact_hip_dsoft_query stands where AlignReads calls sa->DSOFT for every read
 * and its reverse complement and decodes the hits (darwin.cpp:209-224,252-263):
 * queries [first_query, first_query + n_queries) of GACT_SET_QUERY / _RC are
 * filtered and the slot's candidate array is filled ON THE DEVICE, all forward
 * candidates first (query order, then emission order, as the reference's
 * GACT_calls_for), then the reverse-complement ones; run them with
 * gact_hip_candidates_run_mixed(e, slot, 0, *n_forward + *n_reverse, *n_forward, same_file).
 */
typedef struct {
    int32_t seed_size;                 /* params.cfg DSOFT_params.seed_size, 4..15 */
    int32_t bin_size;
    int32_t window_size;               /* < seed_size */
    int32_t threshold;
    int32_t num_seeds;
    int32_t seed_occurence_multiple;
    int32_t max_candidates;            /* per query strand: the first max_candidates threshold crossings are kept */
} gact_dsoft_params;

typedef struct {
    int64_t ref_length;                /* padded concatenation, darwin.cpp:544 */
    int64_t n_minimizers;
    int64_t table_bytes, pos_bytes;
    int32_t max_occurrence;            /* kmer_max_occurence_, seed_pos_table.cpp:59 */
    int32_t n_bins;
    float build_ms;                    /* HIP events, all build kernels */
} gact_dsoft_info;

int gact_hip_dsoft_build(gact_hip_engine *e, const gact_dsoft_params *p, gact_dsoft_info *info);
int gact_hip_dsoft_query(gact_hip_engine *e, int slot, int32_t first_query, int32_t n_queries,
                         int32_t *n_forward, int32_t *n_reverse, float *query_ms);
/* copies candidates [0, n) of the slot's device array to the host */
int gact_hip_candidates_download(gact_hip_engine *e, int slot, int32_t n, gact_candidate *out);

int gact_hip_sync(gact_hip_engine *e, int slot);
/* HIP-event time of the last kernel launched on this slot's stream, in ms */
int gact_hip_last_kernel_ms(gact_hip_engine *e, int slot, float *ms);
/* How the last candidates_run* on this slot was executed.  With the default
 * scoring the chain runs as two launches: a seed launch (first tile of every
 * candidate, arg-max + full pointer matrix) and the main launch (packed-int16
 * kernel, every later tile). */
typedef struct {
    float total_ms, seed_ms, main_ms;   /* HIP events on the slot's stream; read once per run, so every reading of a run gives
                                           the same three values */
    int32_t packed16;                   /* 0: one int32 launch; 1: seed + packed-int16 main launch, uniform
                                           column layout; 2: the same, split (two-region) layout; 3: wide layout
                                           (32 lanes per tile pair, chosen when there are few chains) */
    int32_t handed_off;                 /* candidates the main launch continued */
    int32_t seed_packed16;              /* 1: the seed launch ran the packed-int16 arg-max kernel, 0: the int32 one */
    int32_t tagged_pointers;            /* 1: the split layout ran its pointer phase on tagged scores */
    int32_t linear_gap;                 /* which drifted pass the main launch ran: 1 the linear-gap pass (open == extend ==
                                           mismatch, gact_lin.hpp), 2 the drifted affine pass (gact_aff.hpp), 0 neither;
                                           3 the linear-gap pass of the split layout in its row-drifted frame, which a scoring
                                           with match - 2 extend > 63 takes (gact_lin.hpp 12.) */
    int64_t seed_cells;                 /* DP cells executed by the seed launch */
    int32_t raw_candidates;             /* candidates the run aligned from raw bytes because one of their two reads holds a byte
                                           other than A/C/G/T (align.cpp:134), while the rest ran on the 2-bit image; 0 when no
                                           set holds such a byte, or when the whole run compared raw bytes */
    int32_t band_redos;                 /* linear-gap main launch: tiles run a second time with their whole pointer window stored,
                                           because the traceback left the band around the diagonal the first run had stored
                                           (exact either way; some tenths of a percent of the tiles at 15 % read error) */
    int32_t merged_callers;             /* how many callers' runs the launch carried: > 1 when the engine merged this run with runs
                                           other threads submitted on other slots at about the same time (feeder threads,
                                           darwin.cpp:619-629) into one seed + main launch; the times above are that launch's */
    int32_t overlapped_seeding;         /* 1: the candidates were seeded in order of chain length, most of them beside the main
                                           launch (large runs on an otherwise idle engine); seed_ms is then the first seed launch
                                           alone and main_ms holds the rest */
    int32_t critical_lane;              /* 1: beside the split main launch a wide one ran on a third of the blocks and took the
                                           longest chains (runs of 1-4 chains per tile slot on an otherwise idle engine) */
    int32_t role_waves;                 /* how the split linear-gap main launch walked its tracebacks: 0 every wave its own eight tiles
                                           behind their pass; 1 DP waves + walker waves (gact_roles.hpp); 2 two banks of tiles per wave,
                                           walks of the whole block batched on whichever wave needs a result first (gact_coop.hpp) */
} gact_hip_run_stats;
int gact_hip_last_run_stats(gact_hip_engine *e, int slot, gact_hip_run_stats *stats);

/* Optional, once, after the read sets are resident and before the first job: device arrays for jobs of up to
 * expected_candidates candidates (0: none), the second stream of every slot, and one empty launch of the chain kernels on
 * every stream -- what the first run would otherwise do inside the time its caller measures (allocations, stream
 * creation, code and scratch set-up: ~10 ms on a 65,766-candidate job).  The shim's GPU_init calls it; the reference's
 * caller makes exactly two GACT_Batch calls per feeder thread and per process (darwin.cpp:429-433). */
int gact_hip_prepare(gact_hip_engine *e, int32_t expected_candidates);

/* Scheduling switches of a live engine (none of them changes a record); unknown names are refused.
 *   "overlap_seed"       1 (default): a large run on an idle engine seeds its candidates in order of chain length, most of them
 *                        beside the main launch (gact_hip_run_stats.overlapped_seeding); 0: seed launch, then one main launch
 *   "combine"            1 (default when n_slots > 1): runs that different threads submit on different slots at about the same
 *                        time are merged into one launch (gact_hip_run_stats.merged_callers); 0: every run its own launches
 *   "combine_window_us"  how long the first of such runs waits for the others at most (default 1000)
 *   "runs_in_flight"     1: the caller keeps several runs in flight on this engine (a pipeline of steps, one slot each): every
 *                        launch takes the layout with the better throughput.  0 (default): the engine looks at the other slots'
 *                        events when a run is launched, which the first launches of a pipeline answer differently from run to run
 *   "coop"               the split linear-gap main launch with two banks of tiles per wave and cooperative, batched traceback
 *                        walks (gact_hip_run_stats.role_waves == 2): 1 always, 0 never, 2 (default) where throughput bounds the
 *                        launch -- it shares the machine and has 1.5 chains and more per resident tile slot, or has six and more
 *   "lone_lane"          a run of half as many to as many chains as there are resident tile slots, alone on the machine, runs as ONE
 *                        block per CU of two kinds: value wide blocks (e.g. 48) for its longest chains, split blocks with the
 *                        look-ahead walker on the other CUs (value < 0: without it); 0 (default): all wide, two blocks per CU, which
 *                        is faster.  (gact_hip_run_stats with the mix: layout split, critical_lane 1)
 *   "shared_twelfths"    a linear-gap main launch that shares the machine and has more chains than two thirds of the resident tile slots
 *                        hold takes value / 12 of the resident blocks (default 6)
 *   "overlap_big"        1: ordered, overlapped seeding also for runs of more than four chains per resident tile slot (seed launch A
 *                        takes the longest eighth of the list, B the rest beside main launch 1); 0 (default): seed launch, then one
 *                        main launch
 *   "roles"              1: the split linear-gap main launch runs as DP waves + walker waves (gact_hip_run_stats.role_waves);
 *                        0 (default): one wave does everything for its tiles.  Same records; measured no faster
 * Every other switch of the library is read once, in gact_hip_create, from an environment variable; set_option names the
 * variable when asked for one of those.  The whole table: gact_hip_options_describe, INTEGRATION.md 7. */
int gact_hip_set_option(gact_hip_engine *e, const char *name, int32_t value);
/* The table of every switch the library reads, one line per switch: `name | environment variable | when it is read |
 * class | what it does`.  Writes at most cap bytes (NUL-terminated) into buf, returns the size the whole table needs.
 * No engine, no device. */
int64_t gact_hip_options_describe(char *buf, int64_t cap);
/* GACT_HIP_POISON_SCRATCH=<seed> (a test switch, read in gact_hip_create): how many times since then the engine has filled
 * a pass's whole scratch allocation, a path buffer, a newly opened pileup window or the corrected reads' bytes with seeded
 * garbage in front of the call's first write, and how many bytes those fills covered.  Both 0 with the switch unset: no
 * launch is added then. */
int gact_hip_scratch_fills(gact_hip_engine *e, int64_t *fills, int64_t *bytes);
/* The launch plan -- sequence, kernels, grids -- that an engine of parameters p makes for one pass over `count` candidates on a
 * device of compute_units CUs (kernels at their nominal occupancy), as one JSON object.  flags: bit 0 = the read sets hold
 * bytes other than A/C/G/T, bit 1 = the launch shares the machine (other runs in flight), bit 2 = role launch on, bit 3 =
 * cooperative launch always, bit 4 = never (neither: where the policy takes it), bit 5 = "overlap_big" 1, bit 6 = "lone_lane" 48
 * (the two optional sequences of gact_hip_set_option).
 * The policy is a pure function (csrc/gact_policy.hpp); this entry exists so that it can be swept and tested without a
 * device.  Same buffer convention as gact_hip_options_describe. */
int64_t gact_hip_plan_describe(const gact_hip_params *p, int32_t compute_units, int32_t count, int32_t flags, char *buf, int64_t cap);

/* device address of the slot's gact_overlap array (for an RCCL gather) */
void *gact_hip_device_overlaps(gact_hip_engine *e, int slot);
/* the slot's hipStream_t as an opaque pointer */
void *gact_hip_stream(gact_hip_engine *e, int slot);

/* ---- multi-GPU: the one collective of a sharded job, for C / C++ callers ----
 * One process per GPU, every process with its own engine and its share of the candidates (they shard with no exchange on the
 * data path); what is left to do is bring the records together.  The reference is single-device (cuda_host.cu:195) and joins
 * the output files of separate processes with `cat darwin.*.out | sort | uniq` (README:25); here rank 0 receives every
 * rank's records with RCCL, out of the engines' device-resident record arrays, narrowed on the device to the 32 bytes a
 * line is printed from (gact.cpp:214-224).  bench.py makes the same gather through torch.distributed (gact_amd/dist.py).
 * RCCL is looked up when the first communicator is made (librccl.so.1; GACT_HIP_RCCL_LIB names another file): a
 * single-GPU caller needs none. */
typedef struct {
    int32_t ref_id, query_id;
    int32_t ab, ae, bb, be, score;
    int32_t comp_emitted;       /* bit 0: comp, bit 1: emitted (gact_overlap) */
} gact_line;
typedef struct gact_hip_comm gact_hip_comm;
/* Rank `rank` of `world` (collective: returns when every rank has called it).  The ranks find each other through id_path, a
 * file name all of them can reach and that does not exist yet: rank 0 puts RCCL's unique id there, the others wait for it
 * (timeout_s seconds, 0: 120), rank 0 removes it again.  The communicator works on the engine's device. */
int gact_hip_comm_create(gact_hip_engine *e, int32_t rank, int32_t world, const char *id_path, int32_t timeout_s,
                         gact_hip_comm **out);
/* Collective.  The first n records of `slot` (its last run's; the call waits for that run on the device) travel to rank 0.
 * counts[world] (every rank, may be NULL): records per rank.  lines (rank 0): all of them, rank after rank, each rank's in
 * candidate order; lines_cap = room in `lines`, in records.  Other ranks pass NULL, 0.
 * Too little room on rank 0 (or lines == NULL) does not break the collective: the records are received all the same, the other
 * ranks return 0, rank 0 returns GACT_HIP_EINVAL with counts[] filled in -- call again with room for their sum. */
int gact_hip_comm_gather_lines(gact_hip_comm *c, int slot, int32_t n, int64_t *counts, gact_line *lines, int64_t lines_cap);
int gact_hip_comm_destroy(gact_hip_comm *c);

/* measurement aid: sustained lane-ops/s of this device on the packed-int16 instructions the kernels are made of
 * (independent v_pk_add_i16 / v_pk_max_i16 streams, eight waves per SIMD, no memory) */
int gact_hip_measure_valu_rate(gact_hip_engine *e, double *lane_ops_per_s);

/* formats the exact bytes of gact.cpp:214-224 */
int gact_hip_format_overlap(const gact_overlap *o, const char *ref_name, const char *query_name,
                            char *buf, int32_t cap);

/* One PAF line for a record and its summary (no engine, no device), returning its length as gact_hip_format_overlap does:
 *   qname qlen qstart qend strand tname tlen tstart tend nmatch blocklen 255 AS:i:<score> NM:i:<n_x + ins_bases + del_bases>
 *   de:f:<1 - n_eq / (n_eq + n_x + ins_runs + del_runs), four decimals>
 * nmatch = n_eq, blocklen = the four column counts together.  Coordinates are 0-based, half-open, and the span the alignment
 * really covers: target [ae - (n_eq + n_x + del_bases), ae), query [be - (n_eq + n_x + ins_bases), be) on the record's strand --
 * not ab / bb, which stay where the left extension stopped when it aligned nothing (see gact_hip_candidates_paths).  For
 * comp == 1 the query span is mapped to the original read (qstart = qlen - end, qend = qlen - start) and the strand is '-'.
 * The line ends in '\n'; a caller that appends a cg:Z: tag overwrites it.  GACT_HIP_EINVAL for a summary without columns. */
int gact_hip_format_paf(const gact_overlap *o, const gact_path_summary *s, const char *query_name, int64_t query_len,
                        const char *ref_name, int64_t ref_len, char *buf, int32_t cap);

/* One SAM line for a record, its ops (gact_hip_candidates_paths: n_ops words len << 4 | GACT_PATH_OP_*, left to right) and its
 * placement (gact_hip_place_reads); no engine, no device.  Returns the line's length as snprintf does: with cap too small
 * (cap <= length) nothing useful is in buf, and the caller asks again with room for length + 1.
 *   QNAME FLAG RNAME POS MAPQ CIGAR * 0 0 SEQ * AS:i:<score> NM:i:<X + I + D columns>\n
 *   FLAG   16 for comp == 1, + 256 for GACT_PLACE_SECONDARY and GACT_PLACE_EXTRA, + 2048 for GACT_PLACE_SUPPLEMENTARY
 *   POS    ae - (the ref-consuming columns of ops: =, X, D) + 1; MAPQ is p->mapq
 *   CIGAR  the ops as =, X, I, D (the engine's I consumes the query, as SAM's does), a clip of be - (the query-consuming columns:
 *          =, X, I) in front -- where the alignment begins on the record's strand -- and a clip of query_len - be behind; clips of
 *          length 0 are omitted; S for a primary, H for the others
 *   SEQ    primary: the whole read, reverse-complemented for comp == 1 (case kept; the complement of anything outside acgtACGT
 *          is N).  Supplementary: the aligned stretch of that only.  Secondary and extra: *
 * query_seq is the ORIGINAL read (query_len bytes), whatever comp says; it is not read for a secondary or an extra.
 * GACT_HIP_EINVAL: n_ops <= 0, kind GACT_PLACE_NONE (or none of the kinds), an op that is none of the four, an alignment that
 * begins in front of the read or ends behind it.
 * gact_hip_format_sam_unmapped writes the line of a read without a placement: QNAME 4 * 0 0 * * 0 0 SEQ *\n. */
int64_t gact_hip_format_sam(const gact_overlap *o, const uint32_t *ops, int32_t n_ops, const gact_placement *p,
                            const char *query_name, const uint8_t *query_seq /* the ORIGINAL read */, int64_t query_len,
                            const char *ref_name, char *buf, int64_t cap);
int64_t gact_hip_format_sam_unmapped(const char *query_name, const uint8_t *query_seq, int64_t query_len, char *buf, int64_t cap);

/* One VCF 4.2 line for a record of gact_hip_pileup_variants and the sequence it lies on (seq_len raw bytes); no engine, no
 * device.  Returns the line's length as gact_hip_format_sam does: with cap too small (cap <= length) nothing useful is in buf.
 *   name POS . REF ALT . . DP=<depth>;AD=<alt> GT <0/1 for gt 1, 1/1 for gt 2>\n
 * Reference bytes are upper-cased, and anything that is not A C G T prints as N.  No QUAL: the rule has thresholds, not
 * likelihoods.
 *   SNV              POS = pos + 1, REF = seq[pos], ALT = the base
 *   DEL, pos > 0     POS = pos, REF = seq[pos - 1 .. pos + len), ALT = seq[pos - 1]
 *   INS, pos > 0     POS = pos, REF = seq[pos - 1], ALT = seq[pos - 1] + the bases
 *   DEL, pos == 0    (VCF's rule for the first base) POS = 1, REF = seq[0 .. len], ALT = seq[len]; a deletion of the whole
 *                    sequence has no line: 0 is returned
 *   INS, pos == 0    POS = 1, REF = seq[0], ALT = the bases + seq[0]
 * GACT_HIP_EINVAL: a NULL argument, a kind that is none of the three, a gt that is neither 1 nor 2, a record that does not lie
 * inside the sequence, an INS with len outside [1, 4] or a base that is none of A C G T. */
int gact_hip_format_vcf(const gact_variant *v, const char *seq_name, const uint8_t *seq, int64_t seq_len, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GACT_HIP_H */
