/* sweepga_gpu.h -- C ABI of the MI355X plane-sweep / scaffold filter.
 *
 * Drop-in boundary for sweepga's filter path (`sweepga <paf> --output-file ...`).  The
 * reference has no FFI layer; the seam this library replaces is
 *
 *     PafFilter::apply_filters(&self, Vec<RecordMeta>) -> Result<HashMap<usize, RecordMeta>>
 *                                                         (src/paf_filter.rs:379-382)
 *
 * called from PafFilter::filter_paf (src/paf_filter.rs:283), unified_filter::filter_file
 * (src/unified_filter.rs:316) and examples/compare_filter_outcomes.rs:62-63.  The host keeps
 * CLI parsing, PAF/.1aln I/O and name -> id interning; everything between "records parsed" and
 * "per-record status + chain id" runs in hand-written gfx950 kernels.
 *
 * Conventions
 *   - plain C types only; the caller owns every buffer it passes; the library owns device
 *     memory, streams and staging inside swg_ctx;
 *   - every call returns SWG_OK (0) or a negative SWG_ERR_* code; swg_last_error() gives text;
 *   - no exceptions, aborts or allocations cross the boundary;
 *   - one swg_ctx is used by one host thread at a time; contexts are independent (one per GPU);
 *   - there is NO CPU fallback: without a usable HIP device every compute call fails with
 *     SWG_ERR_NO_DEVICE.
 */
#ifndef SWEEPGA_GPU_H
#define SWEEPGA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWG_ABI_VERSION 1

/* error codes */
#define SWG_OK 0
#define SWG_ERR_INVALID (-1)     /* bad argument */
#define SWG_ERR_NO_DEVICE (-2)   /* no HIP device / device init failed */
#define SWG_ERR_HIP (-3)         /* a HIP runtime call or kernel failed */
#define SWG_ERR_OOM (-4)         /* device or host allocation failed */
#define SWG_ERR_RANGE (-5)       /* mapped stretch of a sequence >= 2^32 bases, or composite sort key wider than 64 bits */
#define SWG_ERR_UNSUPPORTED (-6) /* valid in the reference, not implemented here (documented) */

/* ScoringFunction, src/filter_types.rs:8-14 */
#define SWG_SCORE_IDENTITY 0
#define SWG_SCORE_LENGTH 1
#define SWG_SCORE_LENGTH_IDENTITY 2
#define SWG_SCORE_LOG_LENGTH_IDENTITY 3
#define SWG_SCORE_MATCHES 4

/* FilterMode, src/filter_types.rs:18-22 */
#define SWG_MODE_ONE_TO_ONE 0
#define SWG_MODE_ONE_TO_MANY 1
#define SWG_MODE_MANY_TO_MANY 2

/* per-record result, ChainStatus of src/mapping.rs:82-86 plus "dropped" */
#define SWG_ST_DROPPED 0
#define SWG_ST_SCAFFOLD 1   /* st:Z:scaffold   */
#define SWG_ST_RESCUED 2    /* st:Z:rescued    */
#define SWG_ST_UNASSIGNED 3 /* st:Z:unassigned */

/* usize::MAX of the reference ("keep all") for the k arguments of the sweep entry points */
#define SWG_K_INF UINT64_MAX

typedef struct swg_ctx swg_ctx;

/* The fields of FilterConfig (src/paf_filter.rs:20-49) that the filter reads, plus the two
 * PafFilter builder switches (src/paf_filter.rs:267-275).  Limits: 0 means None. */
typedef struct swg_config {
  uint64_t min_block_length;         /* --min-aln-length        */
  int32_t mapping_filter_mode;       /* --num-mappings (mode)   */
  uint64_t mapping_max_per_query;    /*   per-query limit, 0 = None  */
  uint64_t mapping_max_per_target;   /*   per-target limit, 0 = None */
  int32_t scaffold_filter_mode;      /* --scaffold-filter       */
  uint64_t scaffold_max_per_query;
  uint64_t scaffold_max_per_target;
  double overlap_threshold;          /* --overlap               */
  uint64_t scaffold_gap;             /* --scaffold-jump; 0 disables scaffolding */
  uint64_t min_scaffold_length;      /* --scaffold-mass         */
  double scaffold_overlap_threshold; /* --scaffold-overlap      */
  uint64_t scaffold_max_deviation;   /* --scaffold-dist         */
  int32_t scoring_function;          /* --scoring               */
  double min_identity;               /* --min-aln-identity      */
  double min_scaffold_identity;      /* --min-scaffold-identity */
  int32_t keep_self;                 /* --self                  */
  int32_t scaffolds_only;            /* --scaffolds-only        */
} swg_config;

/* Column (SoA) form of Vec<RecordMeta> (src/paf_filter.rs:54-71), one entry per parsed PAF /
 * .1aln record in input (rank) order.  Sequence names are interned by the host into one id
 * space shared by queries and targets (the reference's SequenceIndex, src/sequence_index.rs:7-31);
 * the two per-sequence tables give each sequence its genome under the two prefix rules the
 * reference uses.  Pointers are host pointers for swg_filter and device pointers for
 * swg_filter_device. */
typedef struct swg_records {
  uint64_t n;                /* number of records */
  const uint32_t* q_id;      /* [n] sequence id of the query name  */
  const uint32_t* t_id;      /* [n] sequence id of the target name */
  const uint32_t* q_start;   /* [n] */
  const uint32_t* q_end;     /* [n] */
  const uint32_t* t_start;   /* [n] */
  const uint32_t* t_end;     /* [n] */
  const double* identity;    /* [n] RecordMeta.identity; may be NULL = matches / max(block_len, 1) for every record, which
                                is what extract_metadata computes when no dv:f: tag overrides it (src/paf_filter.rs:322):
                                evaluated on the device (one IEEE division, same bits), 8 of 47 bytes per record less over PCIe */
  const uint32_t* matches;   /* [n] RecordMeta.matches */
  const uint32_t* block_len; /* [n] RecordMeta.block_length */
  const uint8_t* strand;     /* [n] 0 = '+', 1 = '-' */
  uint32_t n_seq;            /* number of sequence ids */
  const uint32_t* seq_genome_last; /* [n_seq] genome id, prefix = up to the LAST '#'
                                      (src/paf_filter.rs:1022-1030) */
  uint32_t n_genome_last;
  const uint32_t* seq_genome_two;  /* [n_seq] genome id, prefix = first two '#' parts
                                      (src/plane_sweep_scaffold.rs:13-22) */
  uint32_t n_genome_two;
} swg_records;

/* Per-call timing/statistics (optional, may be NULL). */
typedef struct swg_stats {
  uint64_t n_in;          /* records in */
  uint64_t n_retained;    /* after the step-1 retain (src/paf_filter.rs:384-388) */
  uint64_t n_swept;       /* after the mapping plane sweep */
  uint64_t n_chains;      /* chains built */
  uint64_t n_chains_kept; /* chains after span/identity filter and scaffold sweep */
  uint64_t n_out;         /* records kept */
  double device_ms;       /* GPU time of the call measured with HIP events on the ctx stream */
  double h2d_ms, d2h_ms;  /* copies (swg_filter only) */
} swg_stats;

/* ---- context ------------------------------------------------------------------------- */
int swg_abi_version(void);
/* device: HIP device ordinal.  On failure *out is NULL and the code says why. */
int swg_create(int device, swg_ctx** out);
void swg_destroy(swg_ctx* ctx);
/* Text of the last error on this context (or of the last failed swg_create if ctx is NULL). */
const char* swg_last_error(const swg_ctx* ctx);
/* The HIP stream (hipStream_t) all work of this context is enqueued on. */
void* swg_stream(swg_ctx* ctx);
int swg_synchronize(swg_ctx* ctx);

/* ---- the filter: PafFilter::apply_filters (src/paf_filter.rs:379-747) ----------------- */
/* status_out[n]: SWG_ST_*; chain_out[n]: N of "ch:Z:chain_N", 0 = no ch:Z: tag.
 * Host buffers in, host buffers out (copies included).  When the records are grouped by query genome (an aligner writes its
 * PAF query by query) and there are millions of them, the call is streamed: ranges of whole query genomes -- closed under
 * genome pairs, the filter's independent units -- are uploaded while their predecessors are filtered, and each range's
 * results are copied back as soon as it is done (SWG_STREAM=0 switches that off; results are identical either way). */
int swg_filter(swg_ctx* ctx, const swg_records* rec, const swg_config* cfg, uint8_t* status_out,
               uint32_t* chain_out, swg_stats* stats);
/* Ranged filter (swg_filter, swg_filter64, swg_filter_device, swg_filter_device64, swg_filter_multi, swg_filter_multi64): any n,
 * including n >= 2^31.  A record set of 2^31 records or more, or one whose one-piece footprint does not fit the memory limit
 * (swg_set_memory_limit; no limit: the device's free memory), is cut into ranges of whole genome pairs (first two '#' parts)
 * that each fit; results and chain numbers are those of one call.  Limits that stay: one genome pair of 2^31 records or more
 * (SWG_ERR_RANGE); a kept-chain number of 2^32 or more (SWG_ERR_RANGE); a genome pair that alone does not fit the memory
 * limit (SWG_ERR_OOM, the message names its size); more than 2^23 distinct genome pairs on the device path
 * (SWG_ERR_UNSUPPORTED); the two genome-prefix rules partitioning the sequences differently (SWG_ERR_UNSUPPORTED).  Only when
 * ranging is required.  Without a limit and below 2^31 records, swg_filter tries the streamed path first as before, and a call
 * that fits the device in one piece runs exactly as before. */
/* The ranges such a call would use (host code, no GPU): bounds_out[0 .. *n_chunks] are record indices, ranges of at least
 * target_records records cut where the query genome changes.  *n_chunks = 0: the records are not grouped by query genome
 * (or the reference's two genome-prefix rules partition the sequences differently) -- the call runs in one piece. */
int swg_stream_plan(const swg_records* rec, uint64_t target_records, uint64_t* bounds_out, uint64_t bounds_capacity,
                    uint64_t* n_chunks);
/* Same with every pointer of `rec`, status_out and chain_out in device memory of ctx's GPU (any n, see above).
 * Asynchronous on swg_stream(ctx) except for the small read-backs the pipeline needs. */
int swg_filter_device(swg_ctx* ctx, const swg_records* rec, const swg_config* cfg,
                      uint8_t* status_out, uint32_t* chain_out, swg_stats* stats);

/* Vec<RecordMeta> with the reference's own field widths (query_start .. block_length are u64, src/paf_filter.rs:58-62).
 * The device layout stays 32-bit: every coordinate is rebased to the smallest coordinate its sequence has anywhere in the
 * record set (query and target appearances alike).  apply_filters only ever uses differences, orders and midpoints of
 * positions on one sequence, so the results are those of the unrebased records; what has to fit 32 bits is the stretch of
 * each sequence that mappings touch (and every matches / block_length value).  A sequence touched over 2^32 bases or more is
 * rebased per sweep segment instead -- query coordinates to the smallest one of their (query sequence, genome of the target)
 * segment, target coordinates likewise (src/paf_filter.rs:1037-1100: no step of apply_filters compares coordinates across
 * those segments) -- so that only the stretch touched by the mappings against ONE genome has to fit; beyond that
 * SWG_ERR_RANGE.  start <= end is assumed, as in any PAF; any n (ranged as swg_filter).  swg_filter64: host pointers, rebased by host threads, then swg_filter (no extra PCIe bytes);
 * swg_filter_device64: device pointers, rebased by two kernels, then the same pipeline as swg_filter_device. */
typedef struct swg_records64 {
  uint64_t n;
  const uint32_t* q_id;
  const uint32_t* t_id;
  const uint64_t* q_start;
  const uint64_t* q_end;
  const uint64_t* t_start;
  const uint64_t* t_end;
  const double* identity;
  const uint64_t* matches;
  const uint64_t* block_len;
  const uint8_t* strand;
  uint32_t n_seq;
  const uint32_t* seq_genome_last;
  uint32_t n_genome_last;
  const uint32_t* seq_genome_two;
  uint32_t n_genome_two;
} swg_records64;
int swg_filter64(swg_ctx* ctx, const swg_records64* rec, const swg_config* cfg, uint8_t* status_out, uint32_t* chain_out,
                 swg_stats* stats);
int swg_filter_device64(swg_ctx* ctx, const swg_records64* rec, const swg_config* cfg, uint8_t* status_out,
                        uint32_t* chain_out, swg_stats* stats);

/* ---- lower public seams of the reference, exercised by its tests ---------------------- */
/* These lower seams keep the bound of fewer than 2^31 mappings / records per call, as does the ANI pre-pass below.
 * plane_sweep_query / plane_sweep_target / plane_sweep_both (src/plane_sweep_exact.rs:268,
 * 355, 436) on ONE segment of n mappings given as host arrays.  axis: 0 query, 1 target,
 * 2 both.  keep_out[i] = 1 iff index i is in the returned Vec<usize>.  u64 coordinates as in
 * PlaneSweepMapping: values >= 2^32 are handled by shrinking the stretches no interval covers (exact for a
 * sweep; the reference's u64::MAX test runs this way); SWG_ERR_RANGE only if the covered span of an axis
 * itself does not fit 32 bits.  The same holds for swg_plane_sweep_scaffolds. */
int swg_plane_sweep(swg_ctx* ctx, int axis, uint64_t n, const uint64_t* q_start,
                    const uint64_t* q_end, const uint64_t* t_start, const uint64_t* t_end,
                    const double* identity, uint64_t k_query, uint64_t k_target,
                    double overlap_threshold, int scoring, uint8_t* keep_out);

/* plane_sweep_scaffolds (src/plane_sweep_scaffold.rs:47-94) on n chains; q_id/t_id are
 * sequence ids, seq_genome_two as in swg_records.  order_out receives the kept indices in the
 * reference's output order, *n_kept their number. */
int swg_plane_sweep_scaffolds(swg_ctx* ctx, uint64_t n, const uint32_t* q_id, const uint32_t* t_id,
                              uint32_t n_seq, const uint32_t* seq_genome_two, uint32_t n_genome_two,
                              const uint64_t* q_start, const uint64_t* q_end,
                              const uint64_t* t_start, const uint64_t* t_end, const double* identity,
                              int mode, uint64_t max_per_query, uint64_t max_per_target,
                              double overlap_threshold, int scoring, uint64_t* order_out,
                              uint64_t* n_kept);

/* merge_mappings_into_chains (src/paf_filter.rs:750-933) on n records (no retain, no sweep).
 * chain_of[i] = index of record i's chain in the reference's all_chains order; per-chain
 * outputs hold *n_chains entries (buffers sized n). */
int swg_merge_chains(swg_ctx* ctx, const swg_records* rec, uint64_t max_gap, uint32_t* chain_of,
                     uint32_t* c_q_start, uint32_t* c_q_end, uint32_t* c_t_start,
                     uint32_t* c_t_end, double* c_weighted_identity, uint64_t* n_chains);

/* UnionFind::get_sets (src/union_find.rs:52-63) after union(xs[e], ys[e]) for e = 0..m-1:
 * set_of[i] = position of i's set in get_sets() order (ascending smallest... see DESIGN.md). */
int swg_union_find_sets(swg_ctx* ctx, uint64_t n, uint64_t m, const uint32_t* xs,
                        const uint32_t* ys, uint32_t* set_of, uint64_t* n_sets);

/* f64::ln as the reference evaluates it (glibc log) for n host doubles, computed on the GPU: any double,
 * glibc's branches for arguments near 1, zero, negatives, subnormals, inf and NaN included. */
int swg_log(swg_ctx* ctx, uint64_t n, const double* x, double* y);
/* ln(first + i * stride) for i in [0, n), compared on the device against nothing: returns the
 * values so a test can compare them with the host libm. */
int swg_log_range(swg_ctx* ctx, uint64_t first, uint64_t stride, uint64_t n, double* y);

/* ---- per-kernel timing (HIP events on swg_stream) ---------------------------------------- */
/* When enabled, every kernel launch of later calls is bracketed by HIP events on the context's
 * stream and its elapsed time accumulated per kernel name.  Costs two event records per launch. */
int swg_profile_enable(swg_ctx* ctx, int on);
/* Restricts the bracketing to the launches of ONE kernel (its name as swg_profile_get reports it; NULL or "" = every
 * launch again): a timed region can then carry HIP events around the kernel it wants the duration of -- two event records
 * per launch of that kernel -- without the ~200 event records per call that bracketing every launch costs (about 1 ms per
 * call on a pipeline of ~100 launches). */
int swg_profile_select(swg_ctx* ctx, const char* kernel_name);
int swg_profile_reset(swg_ctx* ctx);
/* Number of distinct kernel names seen since the last reset. */
int swg_profile_count(swg_ctx* ctx);
/* Entry i: name (owned by ctx, valid until the next reset), launches, summed milliseconds. */
int swg_profile_get(swg_ctx* ctx, int i, const char** name, uint64_t* launches, double* total_ms);
/* Elements worked on, summed over entry i's launches, for kernels that run on sub-problems of the call (the radix sort
 * passes: pairs sorted); 0 for kernels that always run over the call's whole record set. */
int swg_profile_units(swg_ctx* ctx, int i, uint64_t* units);

/* Device scratch of this context: capacity of the arena (kept between calls, grown on demand) and the high-water
 * mark of the last call.  A call whose scratch does not fit grows the arena and runs once more, so a host that
 * knows its sizes can avoid that by one warm-up call or by swg_reserve(). */
int swg_memory_info(const swg_ctx* ctx, uint64_t* arena_capacity, uint64_t* arena_peak_last_call);
int swg_reserve(swg_ctx* ctx, uint64_t arena_bytes);
/* Device memory one filter call of this context may hold: scratch arena plus staged columns (not the caller's own device
 * buffers).  0 (the default) = no limit beyond what the device has free.  Blocks the context holds beyond a new limit are
 * released; the arena never grows past it.  The limit is a resource cap, not a path switch: a call whose one-piece footprint
 * (from the per-record budgets) does not fit it -- or, without a limit, does not fit the device's free memory -- and every call
 * of 2^31 records or more is filtered in ranges of whole genome pairs; every other call runs in one piece as before. */
int swg_set_memory_limit(swg_ctx* ctx, uint64_t bytes);
int swg_get_memory_limit(const swg_ctx* ctx, uint64_t* bytes);
/* What a context's first swg_filter call would otherwise pay for inside the call (the reference has no counterpart: it has
 * no device): scratch and staging memory for about n_records_hint records (0 = none) and the library's code objects on the
 * device (one small built-in filter call).  Meant to run on its own host thread while the input is read and parsed. */
int swg_warmup(swg_ctx* ctx, uint64_t n_records_hint, uint32_t n_seq_hint, int with_scaffold);

/* ---- several devices of one node ---------------------------------------------------------------
 * swg_filter over n_ctx contexts (one per device, created by the caller).  Records grouped by query genome: ranges of whole
 * query genomes are dealt to the contexts by size (longest first), every context streams its ranges as swg_filter does --
 * slices of the caller's columns in, slices of the caller's result arrays out, no host-side copy of the record set.
 * Otherwise: records are partitioned by genome pair (first-two-'#'-parts prefix) on host threads, pairs are bin-packed
 * onto the contexts by mapping count, every context filters its part on its own host thread.  Either way chain numbers are
 * made global again on the host (the reference numbers kept chains genome pair by genome pair in first-appearance
 * order, src/paf_filter.rs:517-521).  No collective.  Falls
 * back to ctxs[0] alone when the two genome-prefix rules of the reference partition the sequences differently.
 * Results are identical to swg_filter(ctxs[0], ...).  Errors are reported on ctxs[0].  2^31 records or more, or more than a
 * context's memory limit holds in one piece: ranges of whole genome pairs, dealt round-robin over the contexts. */
int swg_filter_multi(swg_ctx* const* ctxs, int n_ctx, const swg_records* records, const swg_config* cfg, uint8_t* status_out,
                     uint32_t* chain_out, swg_stats* stats);
int swg_filter_multi64(swg_ctx* const* ctxs, int n_ctx, const swg_records64* records, const swg_config* cfg, uint8_t* status_out,
                       uint32_t* chain_out, swg_stats* stats); /* swg_filter64's rebasing, then the same */

/* ---- PAF ingest / egress (host side; no GPU needed for open/write) ----------------------------------------
 * The reference reads the PAF twice (extract_metadata, then write_filtered_output re-reads it).  A swg_paf
 * handle keeps the mapped text, the SoA columns swg_filter() takes and each record's (offset,length), so the
 * writer does not parse again.  `threads` <= 0 means "all host cores".  Errors: negative code, message from
 * swg_paf_last_error() (thread-local).
 */
typedef struct swg_paf swg_paf;
/* open_paf_input (src/paf.rs:10-30: .gz/.bgz -> BGZF, blocks inflated in parallel; "-" = stdin) +
 * PafFilter::extract_metadata (src/paf_filter.rs:292-376) + SequenceIndex (src/sequence_index.rs:7-31). */
int swg_paf_open(const char* path, int threads, swg_paf** out);
/* same, over PAF text already in memory (copied) */
int swg_paf_open_buffer(const char* text, uint64_t len, int threads, swg_paf** out);
void swg_paf_close(swg_paf* p);
/* records in input order; pointers are owned by the handle.  A file with a coordinate, matches or block length >= 2^32
 * is parsed once more into 64-bit columns and rebased per sequence as swg_filter64 does: the coordinate columns are
 * then relative to swg_paf_seq_offsets()[sequence id] (NULL for a file that needed no rebasing -- and for one with a sequence
 * touched over 2^32 bases or more, whose columns are relative to one constant per sweep segment, see swg_records64). */
const swg_records* swg_paf_records(const swg_paf* p);
/* 1 when every record's identity is matches / max(block_len, 1) -- no dv:f: tag had the last word on any line: a caller may
 * then pass identity = NULL in the records it hands to the filter and save the column's trip over PCIe. */
int swg_paf_identity_is_derived(const swg_paf* p);
const uint64_t* swg_paf_seq_offsets(const swg_paf* p);
/* ... a file with a sequence touched over 2^32 bases or more: [n] what was taken off every RECORD's query (axis 0) or target
 * (axis 1) coordinates (one constant per sweep segment, see swg_records64); NULL otherwise. */
const uint64_t* swg_paf_record_offsets(const swg_paf* p, int axis);
/* physical line count (incl. skipped lines) and each record's rank = 0-based line index (src/paf_filter.rs:298) */
uint64_t swg_paf_num_lines(const swg_paf* p);
const uint64_t* swg_paf_ranks(const swg_paf* p);
uint32_t swg_paf_num_sequences(const swg_paf* p);
const char* swg_paf_sequence_name(const swg_paf* p, uint32_t id);
void swg_paf_timing(const swg_paf* p, double* load_ms, double* parse_ms);
int swg_paf_text(const swg_paf* p, const char** text, uint64_t* len);
/* PafFilter::write_filtered_output (src/paf_filter.rs:1689-1726): records with status != 0, input order,
 * original bytes + "\tch:Z:chain_<N>" (chain != 0) + "\tst:Z:<status>".  out_path "-" = stdout. */
int swg_paf_write(const swg_paf* p, const char* out_path, const uint8_t* status, const uint32_t* chain, int threads,
                  uint64_t* n_written);
/* PafFilter::filter_paf (src/paf_filter.rs:278-289): open -> swg_filter -> write.
 * timing_ms (optional) = {load, parse, filter (incl. PCIe), write}. */
int swg_filter_paf(swg_ctx* ctx, const char* in_path, const char* out_path, const swg_config* cfg, int threads,
                   swg_stats* stats, double timing_ms[4]);
const char* swg_paf_last_error(void);

/* ---- .1aln front end: record derivation (src/unified_filter.rs:21-154) ----------------------------------------
 * The reference reads .1aln through fastga-rs (AlnReader::open / get_all_seq_names / read_alignment, call sites
 * src/unified_filter.rs:27-36, 67), an un-vendored dependency (fastga-rs 0.1.2 @5216a15, onecode 0.1.0 @5fa1e93,
 * Cargo.lock:617-619, 1192-1194): the DECODER stays in the Rust host.  What crosses the boundary is the decoded
 * alignment as that reader returns it; the library derives the RecordMeta columns exactly as extract_1aln_metadata does:
 *   names cut at the first white space after skipping leading white space, the whole header when it has no word
 *     (split_whitespace().next().unwrap_or(full), :83-92; white space = Unicode White_Space)
 *   block_length = (query_end - query_start) + (target_end - target_start)   (:107-112, wrapping u64)
 *   identity = matches / query_span as f64, 0.0 when the span is 0           (:119-123)
 *   rank = position of the alignment in the file                              (:63, :142)
 * and interns the names like the PAF path.  swg_filter() over swg_aln_records() is filter_file's .1aln branch
 * (src/unified_filter.rs:310-317); the host writes the passing alignments itself (write_1aln_filtered, :158-190: the
 * ranks with status != 0).  Values >= 2^32: coordinates are rebased per sequence as in swg_filter64 (offsets from
 * swg_aln_seq_offsets, NULL when nothing was rebased); SWG_ERR_RANGE if a sequence's mapped stretch, a block length or a
 * match count still does not fit 32 bits (same limit as the PAF path). */
typedef struct swg_aln_input {
  uint64_t n;
  const char* const* query_name;   /* [n] NUL-terminated: id_to_name[aln.query_name], or the raw field (:71-82) */
  const char* const* target_name;  /* [n] */
  const uint64_t* query_start;     /* [n] aln.query_start as u64 ... */
  const uint64_t* query_end;
  const uint64_t* target_start;
  const uint64_t* target_end;
  const uint64_t* matches;         /* [n] aln.matches as u64 (:115) */
  const char* strand;              /* [n] aln.strand: '+', anything else counts as '-' */
} swg_aln_input;
typedef struct swg_aln swg_aln;
int swg_aln_open(const swg_aln_input* in, swg_aln** out);
void swg_aln_close(swg_aln* a);
/* records in file order (rank k = record k); pointers are owned by the handle */
const swg_records* swg_aln_records(const swg_aln* a);
const uint64_t* swg_aln_seq_offsets(const swg_aln* a);
const uint64_t* swg_aln_record_offsets(const swg_aln* a, int axis);  /* (as swg_paf_record_offsets) */
uint32_t swg_aln_num_sequences(const swg_aln* a);
const char* swg_aln_sequence_name(const swg_aln* a, uint32_t id); /* the name after the first-word cut */

/* ---- tree sparsification of the PAF before the filter (--sparsify tree:<near>[:<far>[:<random>]] / knn:...) ---------
 * tree_filter::apply_tree_filter_to_paf (src/tree_filter.rs:205-285), which the reference runs on the input before
 * PafFilter::filter_paf (src/main.rs:3640-3688): per unordered pair of genomes (first two '#' parts) identity =
 * sum(matches) / sum(block length); every genome keeps its k_nearest best and k_farthest worst neighbours, plus every pair
 * whose DefaultHasher (SipHash-1-3) value is <= random_fraction * 2^64; the lines of the kept pairs survive (input order,
 * "\n" ends).  Identity ties fall to the neighbour's prefix in ascending order (the reference's order is arbitrary
 * there).  Host code.  *out_text is allocated by the library: release it with swg_free(). */
int swg_paf_tree_filter(const char* text, uint64_t len, uint64_t k_nearest, uint64_t k_farthest, double random_fraction,
                        char** out_text, uint64_t* out_len);
void swg_free(void* p);

/* ---- tree sparsification on RECORDS: a keep flag per record from the device, and the filter on the kept subset -------------
 * The same selection as swg_paf_tree_filter (one implementation serves both) over record columns instead of text, for callers
 * whose records are columns already: an open handle, device-resident records, a .1aln handle (which keeps no text).
 *
 * swg_tree_select_pairs: steps 2-3 alone, host code, no GPU.  n_pairs unordered pairs of DIFFERENT genomes (pair_a[k], pair_b[k]:
 * genome ids in either order, every pair listed once) with their sums; genome_prefix[n_genome] are distinct NUL-terminated
 * strings (they decide the canonical order of a pair, the tie order and the hash).  selected[k] = 1 when pair k survives.
 * A sum of 2^53 or more: SWG_ERR_RANGE (the reference accumulates in f64; below 2^53 integer sums are the same numbers). */
int swg_tree_select_pairs(uint32_t n_genome, const char* const* genome_prefix, uint64_t n_pairs, const uint32_t* pair_a,
                          const uint32_t* pair_b, const uint64_t* sum_matches, const uint64_t* sum_block_len, uint64_t k_nearest,
                          uint64_t k_farthest, double random_fraction, uint8_t* selected);
/* keep[i] = 1 when record i survives the sparsification, 0 otherwise (a record whose two genomes are equal never survives,
 * src/tree_filter.rs:183-186); *n_kept (optional) their number.  Read: q_id, t_id, matches, block_len of rec, and
 * seq_genome[rec->n_seq] (genome ids < n_genome; the reference's rule is the two-part prefix, i.e. rec->seq_genome_two of a
 * handle, but any partition works).  The per-pair sums are integer reductions on the device (kernels in csrc/swg_sparsify.hip),
 * the selection runs on the host over (pair sums, genome_prefix), the mask is written by the device.  Host pointers for the four
 * columns, seq_genome and keep (staged: 17 bytes per record); genome_prefix are host strings in both entries -- the device never
 * sees a string.  n >= 2^31: SWG_ERR_RANGE.  A pair's sum >= 2^53: SWG_ERR_RANGE.  An id out of range: SWG_ERR_INVALID.  Scratch
 * (the pair table: 24 bytes per genome pair when n_genome^2 <= 2^20, else up to 128 bytes per record) comes from the context's
 * arena: SWG_ERR_OOM when the memory limit does not hold it. */
int swg_tree_select_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                            const char* const* genome_prefix, uint64_t k_nearest, uint64_t k_farthest, double random_fraction,
                            uint8_t* keep, uint64_t* n_kept);
/* The same with the four columns, seq_genome and keep in device memory of ctx's GPU; no record column is copied to the host. */
int swg_tree_select_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                   const char* const* genome_prefix, uint64_t k_nearest, uint64_t k_farthest, double random_fraction,
                                   uint8_t* keep, uint64_t* n_kept);
/* swg_filter_device on the records with keep[i] != 0, answered in the caller's record indices: the columns that are non-NULL in rec
 * are compacted in input order on the device, the unchanged swg_filter_device runs on them, and the results are scattered back.
 * Contract: for kept records, status and chain number are exactly what swg_filter_device gives on the compacted columns; dropped
 * records get 0 / 0; every entry of status_out[n] and chain_out[n] is written.  keep == NULL is swg_filter_device.  Sequence ids
 * are NOT renumbered: the compacted columns keep the ids (and the two sequence -> genome tables) of the full input.  The
 * reference has no ids -- it keys by names and orders by record position -- and no answer here depends on the order of ids
 * (DESIGN.md section 12), so this equals filtering the sparsified text parsed afresh.  n >= 2^31: SWG_ERR_RANGE.  The compacted
 * columns live in a block of the context beside the arena; under a memory limit the filter call inside runs under what the limit
 * leaves beside them.  stats (optional): those of the inner call, n_in = rec->n. */
int swg_filter_subset_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* keep, const swg_config* cfg, uint8_t* status_out,
                             uint32_t* chain_out, swg_stats* stats);
/* Host pointers: compacted by host threads, then the unchanged swg_filter (streamed path included) / swg_filter_multi. */
int swg_filter_subset(swg_ctx* ctx, const swg_records* rec, const uint8_t* keep, const swg_config* cfg, uint8_t* status_out,
                      uint32_t* chain_out, swg_stats* stats);
int swg_filter_subset_multi(swg_ctx* const* ctxs, int n_ctx, const swg_records* rec, const uint8_t* keep, const swg_config* cfg,
                            uint8_t* status_out, uint32_t* chain_out, swg_stats* stats);
/* The two-part-prefix genome table of a handle (src/tree_filter.rs:15-24: the first two '#' parts + '#', the whole name without a
 * '#'): prefix of genome id g < swg_*_num_genomes_two() under records->seq_genome_two, owned by the handle. */
uint32_t swg_paf_num_genomes_two(const swg_paf* p);
const char* swg_paf_genome_two_prefix(const swg_paf* p, uint32_t g);
uint32_t swg_aln_num_genomes_two(const swg_aln* a);
const char* swg_aln_genome_two_prefix(const swg_aln* a, uint32_t g);
/* The mask of an open PAF: keep[n] on the host, what swg_paf_tree_filter keeps of the handle's text, record for record.
 * *route (optional) says how it was made: SWG_TREE_ROUTE_DEVICE from the handle's columns (swg_tree_select_records), or
 * SWG_TREE_ROUTE_TEXT by the text pass over the text the handle keeps -- same answer, slower -- for a handle whose columns are not
 * what that pass reads (swg_paf_tree_needs_text() == 1): a cg:Z: total replaced column 10 by another value; column 10 or 11 did
 * not parse; a '#'-led line with 11 fields (a record for the handle, a comment for the tree pass); a file with values >= 2^32 (64-bit
 * columns, rebased); and, found only when summing, a pair's sum >= 2^53.  ctx may be NULL for a handle without records or one
 * that takes the text route.  `threads` is reserved (both routes ignore it). */
#define SWG_TREE_ROUTE_DEVICE 0
#define SWG_TREE_ROUTE_TEXT 1
int swg_paf_tree_needs_text(const swg_paf* p);
int swg_paf_tree_select(swg_ctx* ctx, const swg_paf* p, uint64_t k_nearest, uint64_t k_farthest, double random_fraction, int threads,
                        uint8_t* keep, uint64_t* n_kept, int* route);
/* The twin for a .1aln record handle: apply_tree_filter_to_1aln (src/tree_filter.rs:286-…) sums aln.matches over
 * aln.query_end - aln.query_start (:314-317) -- not over the record's block length, which is query span + target span -- so that
 * is the length summed here.  No text, so no other route: a pair's sum >= 2^53 is SWG_ERR_RANGE. */
int swg_aln_tree_select(swg_ctx* ctx, const swg_aln* a, uint64_t k_nearest, uint64_t k_farthest, double random_fraction,
                        uint8_t* keep, uint64_t* n_kept);

/* ---- alnstats (src/bin/alnstats.rs): statistics of a PAF and the comparison of two ------------------------------------
 * parse_paf (:103-164) over host threads: lines with fewer than 11 fields are skipped; a line whose columns 2, 3, 4, 7,
 * 10 or 11 do not parse as u64 ends the run as in the reference (SWG_ERR_INVALID, "Invalid query length" ... in
 * swg_alnstats_last_error()).  mapping length = query_end - query_start; genome = name up to the last '#' (:94-100);
 * a genome's size = sum of the last-seen lengths of its sequences; coverage of (query genome, target genome) =
 * 100 * bases / size(query genome) over the inter-genome lines (:42-73).  The reference lists the pairs in HashMap
 * order; here they come in order of first appearance in the file (that fixes the summation order of avg_coverage and
 * the order of equal coverages in the detailed table).  swg_alnstats_report / _compare produce the exact text of
 * print_stats (:166-228) / compare_stats (:230-284); release it with swg_free().  Host code, no GPU. */
typedef struct swg_alnstats swg_alnstats;
typedef struct swg_alnstats_summary {
  uint64_t total_mappings, total_bases, total_matches, self_mappings, inter_chromosomal, inter_genome, chr_pair_count;
  uint64_t genome_pairs, above_95_pct;
  double avg_identity; /* total_matches / total_bases, 0 when there are no bases (:75-81) */
  double avg_coverage;
} swg_alnstats_summary;
int swg_alnstats_open(const char* path, int threads, swg_alnstats** out); /* plain / .gz / .bgz / "-" like swg_paf_open */
int swg_alnstats_open_buffer(const char* text, uint64_t len, int threads, swg_alnstats** out);
void swg_alnstats_close(swg_alnstats* s);
const swg_alnstats_summary* swg_alnstats_get(const swg_alnstats* s);
/* pair i < genome_pairs; the genome strings keep their trailing '#' and are owned by the handle */
int swg_alnstats_pair(const swg_alnstats* s, uint64_t i, const char** q_genome, const char** t_genome, double* coverage,
                      uint64_t* bases, uint64_t* matches);
int swg_alnstats_report(const swg_alnstats* s, const char* label, int detailed, char** out_text, uint64_t* out_len);
int swg_alnstats_compare(const swg_alnstats* a, const swg_alnstats* b, const char* file1, const char* file2,
                         char** out_text, uint64_t* out_len);
const char* swg_alnstats_last_error(void);

/* ---- alnstats on the device: the same statistics from record columns, "before" and "after" a filter call in one pass --------
 * The integer results of parse_paf (:103-161) over n records given as columns -- q_id, t_id, q_start, q_end and matches are
 * read, nothing else -- under a sequence -> genome map the caller supplies (alnstats' own rule is the prefix up to and
 * including the last '#', the whole name without one; any other partition of the sequences works).  status == NULL: one
 * result set, ALL records.  status != NULL: a second set, KEPT, over the records with status != 0 -- the rule of
 * swg_paf_write -- from the same launches.  Sums are u64 and wrap as the reference's release build does; mapping length =
 * q_end - q_start in 32 bits (start <= end is assumed, as everywhere in this library).  Integers only: coverage and the
 * averages are derived on the host, in the reference's operation order.  n >= 2^31 records or n_seq > 2^31 sequences:
 * SWG_ERR_RANGE.  A sequence or genome id out of range: SWG_ERR_INVALID.  Scratch (the distinct-pair hash set, 16 to 32 bytes
 * per record at most, the genome-pair table, and for host columns 21 bytes per record of staging) comes from the context's
 * arena: SWG_ERR_OOM when the memory limit does not hold it. */
typedef struct swg_alnstats_pair_counts {
  uint32_t q_genome, t_genome; /* ORDERED pair of genome ids (query genome, target genome) */
  uint64_t bases, matches;     /* sums over the pair's inter-genome records */
  uint64_t first_record;       /* smallest index of such a record: the pairs are listed in ascending order of it */
} swg_alnstats_pair_counts;
typedef struct swg_alnstats_counts {
  uint64_t total_mappings, total_bases, total_matches;
  uint64_t self_mappings;     /* q_id == t_id */
  uint64_t inter_chromosomal; /* different sequences of one genome */
  uint64_t inter_genome;      /* the genomes differ (tested after self, before inter-chromosomal, :140-152) */
  uint64_t chr_pair_count;    /* distinct (q_id, t_id) over every record of the set */
  uint64_t n_pairs;           /* out: genome pairs that occur; never more than min(n, n_genome * n_genome) */
  uint64_t pair_capacity;     /* in: entries `pairs` can hold */
  swg_alnstats_pair_counts* pairs; /* in: caller-owned [pair_capacity] or NULL; written only when n_pairs <= pair_capacity
                                      (otherwise the call still returns SWG_OK: compare the two and call again) */
  uint64_t* seq_last;         /* in: caller-owned [n_seq] or NULL.  Per sequence, the last line of the set that names it:
                                 2 * record + side, side 1 = as target (:132-133 insert the target after the query, so on
                                 one line the target's length has the last word); UINT64_MAX = no record of the set names it */
} swg_alnstats_counts;
/* rec: host pointers; seq_genome[rec->n_seq] and status[n] on the host.  all / kept: either may be NULL (kept is ignored
 * when status is NULL). */
int swg_alnstats_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                         const uint8_t* status, swg_alnstats_counts* all, swg_alnstats_counts* kept);
/* The same with the five columns of rec, seq_genome and status in device memory of ctx's GPU (status as swg_filter_device
 * leaves it); the counts structures and the arrays they point to stay on the host.  No record column is copied to the host. */
int swg_alnstats_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                const uint8_t* status, swg_alnstats_counts* all, swg_alnstats_counts* kept);
/* Statistics of the records of an open PAF, computed on the device.  status == NULL: every record (what swg_alnstats_open
 * gives for the same file).  status != NULL: *all_out as before and *kept_out over the records with status != 0 (what
 * swg_alnstats_open gives for the file swg_paf_write would write).  Either out may be NULL.  The handles are ordinary ones:
 * swg_alnstats_get, _pair, _report, _compare and _close work on them.  Sequence lengths are read from the text the handle
 * keeps -- column 2 or 7 of the one line per sequence the device names -- so no length column exists and nothing more crosses
 * PCIe than the five columns.  An unparsable length on one of THOSE lines is SWG_ERR_INVALID with the host tool's message; on a
 * line that no sequence's size depends on it goes unnoticed, where the host tool stops.  A file in which column 3, 4, 10 or 11
 * of some line does not parse, or whose cg:Z: tag overrode column 10, is rare: its six columns are checked and column 10 read
 * again line by line on the host first (same errors as swg_alnstats_open).  Errors: text in swg_alnstats_last_error().
 * A PAF with no records needs no device (ctx may be NULL then).  .1aln handles keep no text to read lengths from: the
 * swg_alnstats_records seam works on swg_aln_records, swg_paf_alnstats has no .1aln twin. */
int swg_paf_alnstats(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, swg_alnstats** all_out, swg_alnstats** kept_out);

/* ---- breadth: merged-interval coverage per ordered genome pair, on the device ---------------------
 * alnstats' coverage sums mapping lengths, so overlapping mappings count once each; breadth is the number of bases under AT
 * LEAST ONE mapping.  Over the records whose two genomes differ under the map the caller supplies (alnstats' inter-genome
 * rule: self and intra-genome records are ignored), per ordered pair (query genome, target genome):
 *   q_bases = sum(q_end - q_start), t_bases = sum(t_end - t_start);
 *   q_union = sum over the sequences s of the query genome of |union of [q_start, q_end)| over the pair's records with
 *             q_id == s; t_union likewise per sequence of the target genome over [t_start, t_end).
 * Intervals are half-open, zero-length ones add nothing, touching ones join without double counting, and the intervals of one
 * sequence against two genomes are never merged with each other.  start <= end is assumed.  q_id, t_id and the four
 * coordinate columns are read (32-bit layout).  status == NULL: one result set, ALL records; status != NULL: a second set,
 * KEPT, over the records with status != 0 -- the rule of swg_paf_write -- from the same launches.  The pairs are listed in
 * ascending first_record, one to one with swg_alnstats_pair_counts of the same input.  Every value is a sum of integers and
 * does not depend on the order of the records (first_record and the listing order aside).  Capacity protocol and errors as
 * the alnstats record seams: n_pairs > pair_capacity still returns SWG_OK and leaves `pairs` alone; n >= 2^31 records:
 * SWG_ERR_RANGE; a sequence or genome id out of range: SWG_ERR_INVALID; a NULL context: SWG_ERR_INVALID (there is no CPU
 * path).  Scratch comes from the context's arena, SWG_ERR_OOM when the memory limit does not hold it: 28 bytes per record
 * (two 8-byte key buffers, two 4-byte value buffers, one 4-byte buffer of ends; both axes use the same ones), plus the radix
 * sort's own histograms, plus the segment set and the genome-pair table (sized by what occurs).  swg_breadth_records stages
 * its host columns there too: 25 more bytes per record (six columns and the status byte). */
typedef struct swg_breadth_pair {
  uint32_t q_genome, t_genome; /* ORDERED pair of genome ids (query genome, target genome) */
  uint64_t q_bases, t_bases;   /* summed lengths on either side */
  uint64_t q_union, t_union;   /* bases under at least one mapping on either side */
  uint64_t first_record;       /* smallest index of a record of the pair */
} swg_breadth_pair;
typedef struct swg_breadth_counts {
  uint64_t n_pairs;        /* out: genome pairs that occur */
  uint64_t pair_capacity;  /* in: entries `pairs` can hold */
  swg_breadth_pair* pairs; /* in: caller-owned [pair_capacity] or NULL; written only when n_pairs <= pair_capacity */
} swg_breadth_counts;
/* rec: host pointers; seq_genome[rec->n_seq] and status[n] on the host.  all / kept: either may be NULL (kept is ignored when
 * status is NULL). */
int swg_breadth_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                        const uint8_t* status, swg_breadth_counts* all, swg_breadth_counts* kept);
/* The same with the six columns of rec, seq_genome and status in device memory of ctx's GPU; the counts structures and their
 * arrays stay on the host. */
int swg_breadth_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                               const uint8_t* status, swg_breadth_counts* all, swg_breadth_counts* kept);
/* The breadth report of an open PAF under its last-'#' genome map, as text (release it with swg_free): tab-separated, the
 * header line
 *   set query_genome target_genome q_bases q_union q_size q_breadth_pct q_depth t_bases t_union t_size t_breadth_pct t_depth
 * then per set -- `all`, and with status != NULL `kept` -- one row per genome pair in first_record order (only when
 * `detailed`) and a last row with `*` in both genome columns that holds the sums over the pairs (sizes summed per pair).
 * Genome names keep their trailing '#'; sizes are those swg_paf_alnstats derives for the set (last-seen lengths, read from the
 * handle's text); breadth_pct = 100.0 * union / size and depth = bases / union, computed in double and printed "%.4f", `-`
 * when the divisor is 0.  A PAF without records needs no device (ctx may be NULL then).  A handle whose columns are rebased
 * (the file has a value >= 2^32): SWG_ERR_UNSUPPORTED.  Errors: text in swg_alnstats_last_error().  .1aln handles keep no
 * text: the record seams above work on swg_aln_records. */
int swg_paf_breadth(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, int detailed, char** out_text, uint64_t* out_len);

/* ---- blocks: one row per scaffold chain that a filter call kept, on the device -----------------------
 * A pure function of the record columns plus status[n] and chain[n] as swg_filter* writes them (the MergedChain of
 * src/paf_filter.rs:139-155, which the reference drops after numbering).  A record takes part when status != 0 and chain != 0; a
 * block exists for every chain number that at least one such record carries.  All records of one chain share (q_id, t_id).  The
 * SWG_ST_SCAFFOLD records of a chain are its members; on a '+' chain they include the '-' records that inversion capture added,
 * so strand = '+' if any SCAFFOLD record of the chain is '+', else '-'.  core = the SCAFFOLD records on the block's strand,
 * inverted = the SCAFFOLD '-' records of a '+' block, rescued = the SWG_ST_RESCUED records.  (A record with any other non-zero
 * status and a chain number -- no filter writes one -- adds to the sums and covers only.)
 *   q_start .. t_end    minimum of the starts and maximum of the ends over the core records: MergedChain's span
 *   matches, block_len  sums over all records of the chain
 *   q_bases, t_bases    sum(end - start) over all records of the chain
 *   q_cover, t_cover    |union of [start, end)| over all records of the chain, per axis: half-open, zero-length intervals add
 *                       nothing, touching ones join (breadth's rules with the chain as the unit)
 *   first_record        smallest index of a core record
 * Rows come in ascending chain number; a number that no record carries gives no row.  Every value is an integer and does not
 * depend on the order of the records.  q_id, t_id, the four coordinates, strand, matches and block_len are read (32-bit
 * layout; start <= end is assumed).  Capacity protocol of swg_breadth_counts: n_blocks > block_capacity still returns SWG_OK
 * and leaves `blocks` alone.  Errors: a chain whose records name two (q_id, t_id) pairs, a chain without a SCAFFOLD record, a
 * sequence id >= n_seq, a NULL context (there is no CPU path): SWG_ERR_INVALID; n >= 2^31 records or a chain number of
 * 2^32 - 1: SWG_ERR_RANGE.  Scratch comes from the context's arena, SWG_ERR_OOM when the memory limit does not hold it: 28 bytes
 * per record (two 8-byte key buffers, two 4-byte value buffers, one 4-byte buffer of ends; both axes use the same ones) plus
 * the radix sort's histograms, 120 bytes per chain NUMBER (the table is dense in the chain number: its largest value sizes it)
 * and 104 bytes per block.  swg_blocks_records stages its host columns there too: 38 more bytes per record. */
typedef struct swg_block {
  uint32_t chain;        /* N of ch:Z:chain_N */
  uint32_t q_id, t_id;
  uint32_t strand;       /* 0 = '+', 1 = '-' */
  uint32_t q_start, q_end, t_start, t_end;
  uint32_t n_core, n_inverted, n_rescued;
  uint32_t reserved;     /* 0 */
  uint64_t matches, block_len;
  uint64_t q_bases, t_bases;
  uint64_t q_cover, t_cover;
  uint64_t first_record;
} swg_block;
typedef struct swg_block_table {
  uint64_t n_blocks;       /* out: chains that occur */
  uint64_t block_capacity; /* in: entries `blocks` can hold */
  swg_block* blocks;       /* in: caller-owned [block_capacity] or NULL; written only when n_blocks <= block_capacity */
} swg_block_table;
/* rec: host pointers; status[n] and chain[n] on the host. */
int swg_blocks_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const uint32_t* chain, swg_block_table* table);
/* The same with the nine columns of rec, status and chain in device memory of ctx's GPU (as swg_filter_device leaves them: no
 * copy in between); the table structure and its array stay on the host. */
int swg_blocks_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const uint32_t* chain, swg_block_table* table);
/* The blocks of an open PAF as PAF text (release it with swg_free), one line per block in chain order, tab-separated:
 *   qname qlen q_start q_end strand tname tlen t_start t_end matches block_len 255
 *   ch:Z:chain_N nc:i:<n_core> ni:i:<n_inverted> nr:i:<n_rescued> qc:i:<q_cover> tc:i:<t_cover> id:f:<identity>
 * qname, qlen, tname and tlen are copied as text from the line of the block's first_record; identity = matches /
 * max(block_len, 1) in double, printed "%.6f".  matches is the handle's column (RecordMeta.matches).  A PAF without records, or
 * a status and chain without a chain, gives empty text and needs no device (ctx may be NULL then).  A handle whose columns are
 * rebased (the file has a value >= 2^32): SWG_ERR_UNSUPPORTED.  Errors: text in swg_alnstats_last_error().  .1aln handles keep
 * no text: the record seams above work on swg_aln_records. */
int swg_paf_blocks(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const uint32_t* chain, char** out_text, uint64_t* out_len);

/* ---- components: which sequences belong together under the kept mappings, on the device ------------
 * A pure function of q_id, t_id and the four coordinates (32-bit layout; start <= end is assumed), status[n], seq_len[n_seq]
 * and two parameters; all integers, independent of record order and grid shape.
 *   nodes       every sequence id < n_seq
 *   links       a record takes part when status != 0 (the rule of swg_paf_write; status == NULL: every record) and
 *               q_id != t_id.  Every unordered pair {a, b}, a < b, that such a record names is a link: a_bases / b_bases =
 *               sum(end - start) on the axis where a / b lies, over the pair's records of BOTH orientations; n_records their
 *               number; first_record the smallest record index.  These are plain SUMS, not unions: overlapping mappings count
 *               once each (a pile of repeats over one locus adds up; breadth, section 17, is the union).
 *   joined      with need(s) = ceil(min_share_ppm * seq_len[s] / 10^6):  max(a_bases, b_bases) >= min_bases  and
 *               (a_bases >= need(a) or b_bases >= need(b)).  A contig that aligns mostly to a chromosome joins it, two
 *               chromosomes tied by a short translocation do not.  The defaults 0, 0 join every link: plain connected components.
 *   components  connected sets of sequences over the joined links, numbered 1..C in ascending order of their smallest member
 *               (first_seq); a sequence without a joined link is a component of its own.  length = sum of seq_len; n_links,
 *               n_records and bases = sum(a_bases + b_bases) run over the links whose two ends lie in the component, joined or
 *               not.  cross_links, cross_records, cross_bases: the same three sums over the links whose ends lie in different
 *               components.
 * `links` comes in ascending (a, b), `components` in ascending id; seq_component[s] is the id of s's component.  Capacity
 * protocol of swg_breadth_counts, per array: a count above its capacity still returns SWG_OK and leaves that array alone.
 * n == 0 gives n_seq singleton components and no links.  Errors: a NULL context (there is no CPU path), a sequence id >=
 * n_seq, min_share_ppm > 10^6, reserved != 0: SWG_ERR_INVALID; n >= 2^31 records: SWG_ERR_RANGE.  Scratch comes from the
 * context's arena, SWG_ERR_OOM when the memory limit does not hold it: nothing per record on the device seam (the host seam
 * stages its columns there: 25 bytes per record), 32 bytes per slot of the sequence-pair table (n_seq^2 slots while that is at
 * most 2^20, else 40 bytes per slot of an open-addressing table of at least twice the pairs that can occur -- the smaller of
 * n_seq (n_seq - 1) / 2 and the runs of one pair in input order), 40 bytes per link, 16 bytes per sequence (20 on the host
 * seam) and 40 per component. */
typedef struct swg_component_params {
  uint64_t min_bases;
  uint32_t min_share_ppm; /* <= 1000000 */
  uint32_t reserved;      /* 0 */
} swg_component_params;
typedef struct swg_link {
  uint32_t a, b; /* a < b */
  uint32_t n_records;
  uint32_t joined; /* 0 or 1 */
  uint64_t a_bases, b_bases;
  uint64_t first_record;
} swg_link; /* 40 bytes */
typedef struct swg_component {
  uint32_t id, first_seq, n_seq, n_links;
  uint64_t length, n_records, bases;
} swg_component; /* 40 bytes */
typedef struct swg_component_table {
  uint64_t n_components;       /* out */
  uint64_t component_capacity; /* in: entries `components` can hold */
  swg_component* components;   /* in: caller-owned [component_capacity] or NULL; written only when n_components <= component_capacity */
  uint64_t n_links;            /* out */
  uint64_t link_capacity;      /* in */
  swg_link* links;             /* in: caller-owned [link_capacity] or NULL; written only when n_links <= link_capacity */
  uint32_t* seq_component;     /* in: caller-owned [n_seq] or NULL */
  uint64_t cross_links, cross_records, cross_bases; /* out */
} swg_component_table;
/* rec: host pointers; seq_len[n_seq] and status[n] (or NULL) on the host; params NULL = the defaults 0, 0. */
int swg_components_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint8_t* status,
                           const swg_component_params* params, swg_component_table* table);
/* The same with the six columns of rec, seq_len and status in device memory of ctx's GPU (status as swg_filter_device leaves
 * it: no copy in between); params, the table structure and its three arrays stay on the host. */
int swg_components_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint8_t* status,
                                  const swg_component_params* params, swg_component_table* table);
/* The components of an open PAF as text (release it with swg_free), tab-separated, a header line
 *   sequence length component component_sequences component_length links records bases
 * and one row per sequence in sequence-id order: length = the sequence's last-seen length (the line that mentions it last has
 * the last word, its target column after its query column: the rule of swg_paf_alnstats' genome sizes, read from the handle's
 * text -- which is also seq_len of the call); links, records, bases = the sums n_links, n_records, a_bases + b_bases over the
 * sequence's own links.  With `detailed` a line `#links` follows and per link, in ascending (a, b), by name:
 *   a b records a_bases b_bases joined
 * A last line `#cross <links> <records> <bases>` closes the text.  A PAF without records gives the header and `#cross 0 0 0`
 * (and `#links`) and needs no device (ctx may be NULL then).  A handle whose columns are rebased (the file has a value >=
 * 2^32): SWG_ERR_UNSUPPORTED.  Errors: text in swg_alnstats_last_error().  .1aln handles keep no text: the record seams above
 * work on swg_aln_records. */
int swg_paf_components(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_component_params* params, int detailed,
                       char** out_text, uint64_t* out_len);

/* ---- intervals: WHERE the coverage lies, as merged intervals, on the device ---------------------------
 * Breadth (above) says how many bases of a sequence lie under at least one mapping; this says which.  Units and the counting
 * rule are breadth's: only records whose two genomes differ under the caller's seq_genome map count; on the query axis (0) the
 * unit is (query sequence, genome of the target) over [q_start, q_end), on the target axis (1) it is (target sequence, genome of
 * the query) over [t_start, t_end).  Intervals are half-open, zero-length records add nothing, touching intervals join, the
 * intervals of one sequence against two genomes are never merged with each other, start <= end is assumed.  Per unit:
 *   SWG_IV_ALL   the maximal intervals of the union over all counted records
 *   SWG_IV_KEPT  the same over the records with status != 0 (the rule of swg_paf_write)
 *   SWG_IV_LOST  the maximal intervals of ALL minus KEPT: covered by a mapping before the filter, by none after it.  Every KEPT
 *                interval lies inside one ALL interval, so LOST is, inside every ALL interval, the gaps its KEPT intervals leave.
 * A list is ordered by (seq, other_genome, start), ascending; that order and every value are independent of the order of the
 * records.  q_id, t_id and the four coordinate columns are read (32-bit layout).  `want` selects the lists: bit (set * 2 +
 * axis); a list whose bit is clear is left untouched, and the device passes only it would need are not launched (LOST needs the
 * rows of ALL and KEPT of its axis on the device, not on the host).  For every wanted list n and bases = sum(end - start) are
 * always written.  Capacity protocol of swg_breadth_counts, per list: n > capacity still returns SWG_OK and leaves `rows` alone
 * (call once with capacity 0, then with the n that came back).  Errors: a NULL context (there is no CPU path), reserved != 0,
 * want == 0 or a bit beyond the six, a KEPT or LOST bit with status == NULL, a sequence id >= n_seq or a genome id >=
 * n_genome: SWG_ERR_INVALID; n >= 2^31 records: SWG_ERR_RANGE.  Scratch comes from the context's arena, SWG_ERR_OOM when the
 * memory limit does not hold it: 28 bytes per record (two 8-byte key buffers, two 4-byte value buffers, one 4-byte buffer of
 * ends; both axes use the same ones) plus the radix sort's histograms and the segment set, and per axis, while it runs, 16
 * bytes per ALL / KEPT / LOST interval whose list is wanted or that LOST needs -- with LOST 16 more per ALL and KEPT interval
 * (its sort key, a flag, a link).  swg_intervals_records stages its host columns there too: 25 more bytes per record. */
typedef struct swg_interval {
  uint32_t seq;          /* the sequence of the axis */
  uint32_t other_genome; /* the genome on the other side */
  uint32_t start, end;   /* half-open */
} swg_interval; /* 16 bytes */
typedef struct swg_interval_list {
  uint64_t n;         /* out: intervals of this list */
  uint64_t bases;     /* out: sum(end - start) over them */
  uint64_t capacity;  /* in: entries `rows` can hold */
  swg_interval* rows; /* in: caller-owned [capacity] or NULL; written only when n <= capacity */
} swg_interval_list;
#define SWG_IV_ALL 0
#define SWG_IV_KEPT 1
#define SWG_IV_LOST 2
typedef struct swg_interval_request {
  uint32_t want;     /* bit (set * 2 + axis), axis 0 = query, 1 = target; a clear bit leaves that list untouched */
  uint32_t reserved; /* 0 */
  swg_interval_list list[3][2]; /* [set][axis] */
} swg_interval_request;
/* rec: host pointers; seq_genome[rec->n_seq] and status[n] (NULL: only ALL lists) on the host. */
int swg_intervals_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                          const uint8_t* status, swg_interval_request* req);
/* The same with the six columns of rec, seq_genome and status in device memory of ctx's GPU (status as swg_filter_device leaves
 * it: no copy in between); the request and its row arrays stay on the host. */
int swg_intervals_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                 const uint8_t* status, swg_interval_request* req);
/* One set of an open PAF under its last-'#' genome map (that of swg_paf_breadth) as BED-like text (release it with swg_free),
 * one line per interval, tab-separated:
 *   sequence_name start end other_genome_name q|t
 * the query-axis list first, then the target-axis list, each in list order.  Sequence names are the handle's, genome names keep
 * their trailing '#'.  set: SWG_IV_ALL, SWG_IV_KEPT or SWG_IV_LOST, anything else SWG_ERR_INVALID; KEPT or LOST with status ==
 * NULL: SWG_ERR_INVALID.  A PAF without records gives empty text and needs no device (ctx may be NULL then).  A handle whose
 * columns are rebased (the file has a value >= 2^32): SWG_ERR_UNSUPPORTED.  Errors: text in swg_alnstats_last_error().  .1aln
 * handles keep no names: the record seams above work on swg_aln_records. */
int swg_paf_intervals(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, int set, char** out_text, uint64_t* out_len);
/* Several sets from ONE device call: bit s of `sets` asks for set s (at least one, none beyond bit 2); out_text[s] and
 * out_len[s] of [3] arrays are written for those sets only, each text as swg_paf_intervals gives it and released with swg_free. */
int swg_paf_interval_texts(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t sets, char** out_text, uint64_t* out_len);

/* ---- sharing: how many genomes cover each base, on the device ----------------------------------------
 * Breadth and intervals (above) work per (sequence, other genome) unit; this counts ACROSS genomes.  The counting rule is
 * breadth's: only records whose two genomes differ under the caller's seq_genome map count, intervals are half-open, zero-length
 * records add nothing, start <= end is assumed, a record is KEPT when status != 0.  cover(s, g), g != genome(s), is the union of
 * [q_start, q_end) over the counted records with q_id == s and genome(t_id) == g AND of [t_start, t_end) over those with t_id ==
 * s and genome(q_id) == g: both axes in one union, so a base that a genome covers from both sides counts once.  depth(s, x) is
 * the number of genomes g with x in cover(s, g), 0 .. n_genome - 1.  Per set (0 = all counted records, 1 = the kept ones):
 *   runs      the maximal half-open intervals of a sequence with one depth >= 1, ordered by (seq, start); two touching stretches
 *             of equal depth are one run, also where one genome's cover ends exactly where another's begins; depth 0 is not
 *             listed.  bases = sum(end - start).
 *   spectrum  spectrum[g * n_genome + d] = bases of the sequences of genome g at depth d.  With seq_len, d = 0 is the sum of
 *             seq_len over the sequences of g minus the rest of the row (and then a genome id >= n_genome anywhere in seq_genome,
 *             or a counted record that ends beyond seq_len of its sequence, is SWG_ERR_INVALID); with seq_len == NULL column 0
 *             stays 0.
 * Order and values are independent of the order of the records.  `want`: bit 0 = runs of ALL, bit 1 = runs of KEPT, bit 2 =
 * spectrum of ALL, bit 3 = spectrum of KEPT; only the device passes the bits need are launched.  A runs bit writes n and bases of
 * its list and, under the capacity protocol of swg_breadth_counts, its rows (n > capacity still returns SWG_OK and leaves `rows`
 * alone); a spectrum bit writes all n_genome * n_genome entries of the caller's array and reads back no rows.  Errors: a NULL
 * context (there is no CPU path), reserved != 0, want == 0 or a bit beyond the four, a KEPT bit with status == NULL, a spectrum
 * bit with a NULL spectrum, a sequence id >= n_seq or a genome id >= n_genome: SWG_ERR_INVALID; n >= 2^30 records, or a spectrum
 * bit with n_genome > 4096: SWG_ERR_RANGE.  Scratch comes from the context's arena, SWG_ERR_OOM when the memory limit does not
 * hold it: 56 bytes per record (every record is sorted twice, once per axis) and, while a set's depth sweep runs, 66 bytes per
 * merged interval of the set, 17 per breakpoint, 20 per run and 8 * n_genome^2 for a spectrum (DESIGN.md section 21 has the
 * formula).  swg_sharing_records stages its host columns there too: 25 more bytes per record. */
typedef struct swg_depth_run {
  uint32_t seq;
  uint32_t start, end; /* half-open */
  uint32_t depth;      /* >= 1 */
} swg_depth_run; /* 16 bytes */
typedef struct swg_depth_list {
  uint64_t n;          /* out (runs bit): runs of this set */
  uint64_t bases;      /* out (runs bit): sum(end - start) over them */
  uint64_t capacity;   /* in: entries `rows` can hold */
  swg_depth_run* rows; /* in: caller-owned [capacity] or NULL; written only when n <= capacity */
  uint64_t* spectrum;  /* in (spectrum bit): caller-owned [n_genome * n_genome], fully written */
} swg_depth_list; /* 40 bytes */
#define SWG_SHARING_RUNS_ALL 1u
#define SWG_SHARING_RUNS_KEPT 2u
#define SWG_SHARING_SPECTRUM_ALL 4u
#define SWG_SHARING_SPECTRUM_KEPT 8u
typedef struct swg_sharing_request {
  uint32_t want;     /* the four bits above; a set neither of whose bits is given is left untouched */
  uint32_t reserved; /* 0 */
  swg_depth_list set[2]; /* 0 = ALL, 1 = KEPT */
} swg_sharing_request; /* 88 bytes */
/* rec: host pointers; seq_genome[rec->n_seq], seq_len[rec->n_seq] (or NULL) and status[n] (NULL: only the ALL bits) on the host. */
int swg_sharing_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint32_t* seq_len,
                        const uint8_t* status, swg_sharing_request* req);
/* The same with the six columns of rec, seq_genome, seq_len and status in device memory of ctx's GPU; the request and its arrays
 * stay on the host. */
int swg_sharing_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                               const uint32_t* seq_len, const uint8_t* status, swg_sharing_request* req);
/* Both texts of an open PAF under its last-'#' genome map from ONE device call: out_text[0] receives the table, out_text[1] the
 * BED (release each with swg_free).  The caller marks the texts it wants on entry: an entry whose out_text[k] is NULL on entry is
 * skipped (it stays NULL, out_len[k] = 0, and the device passes only it needs are not launched); any other value asks for text k
 * and is replaced by it (it is never dereferenced).  Tab-separated:
 *   table  header `genome length private_all shared_all core_all private_kept shared_kept core_kept`, one row per genome in
 *          genome-id order (names keep their trailing '#'; length = sum of the last-seen lengths of swg_paf_components; private
 *          = depth 0, core = depth n_genome - 1, shared = everything between; one genome: all private), then a `#total` row;
 *          with `detailed` a `#spectrum` line and `genome all|kept depth bases` for every non-zero entry in (genome, set, depth)
 *          order.
 *   BED    `sequence start end n_all n_kept`: the maximal stretches of constant (n_all, n_kept) with n_all >= 1, ordered by
 *          (sequence id, start), merged on the host from the two run lists.
 * status is needed (SWG_ERR_INVALID without).  A PAF without records gives the header-only table and an empty BED and needs no
 * device (ctx may be NULL then).  A handle whose columns are rebased: SWG_ERR_UNSUPPORTED.  Errors: swg_alnstats_last_error(). */
int swg_paf_sharing(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, int detailed, char* out_text[2], uint64_t out_len[2]);

/* ---- dot plot: the records before and after the filter, rasterised on the device ---------------------------
 * x is the target axis, y the query axis; each is a concatenation of sequences: x_off[s] / y_off[s] is where sequence s begins on
 * its axis, SWG_DOT_ABSENT = not on this axis; x_total / y_total are the axes' lengths.  px(a) = a * width / x_total, py(a) = a *
 * height / y_total (floor, 64-bit); 1 <= width, height <= 16384 and 1 <= total < 2^48 keep the product below 2^62.  A record is
 * DRAWN when q_end > q_start, t_end > t_start and both its sequences are on their axes (intra-genome and self records like any
 * other; start <= end is assumed); it is KEPT when status != 0.  Endpoints: x0 = px(x_off[t] + t_start), x1 = px(x_off[t] + t_end
 * - 1), ya = py(y_off[q] + q_start), yb = py(y_off[q] + q_end - 1); strand '+': (y0, y1) = (ya, yb), strand '-': (yb, ya), the
 * line falls.  dx = x1 - x0, dy = |y1 - y0|, L = max(dx, dy); the record's pixels are, for k = 0 .. L,
 *   x = x0 + (2 k dx + L) / (2 L),  y = y0 +- (2 k dy + L) / (2 L)      (floor; L = 0: the one pixel (x0, y0))
 * so a record touches a pixel at most once.  Four uint32 count planes of height * width entries, index y * width + x with y = 0
 * at the axis origin: plane 2 * set + strand, set 0 = all drawn records, set 1 = the kept ones, strand 0 = '+', 1 = '-'; a drawn
 * record adds 1 to each of its pixels in its ALL plane, a kept one also in its KEPT plane.  hits[p] = the sum of plane p;
 * drawn[set] = the drawn records of the set (drawn[1] = 0 without a status), always written.  Values do not depend on the order of
 * the records.  Only the planes named by `want` are allocated, cleared, summed and read back: an unwanted plane's pointer is never
 * touched, its hits stay as found.  q_id, t_id, the four coordinates and strand are read (32-bit layout).  Errors: a NULL context
 * (there is no CPU path), reserved != 0, want == 0 or a bit beyond the four, a KEPT bit with status == NULL, a wanted plane with
 * a NULL array, width, height or a total out of range, an id >= n_seq, a drawn record that ends beyond the total of an axis
 * (x_off[t] + t_end > x_total, likewise y): SWG_ERR_INVALID; n >= 2^31 records: SWG_ERR_RANGE.  Scratch comes from the context's
 * arena, SWG_ERR_OOM when the memory limit does not hold it: 4 bytes per record (the list of records longer than a pixel) and 4 *
 * width * height per wanted plane; swg_dotplot_records stages its host columns there too: 26 more bytes per record and 16 per
 * sequence. */
#define SWG_DOT_ABSENT UINT64_MAX
#define SWG_DOT_ALL_PLUS 1u   /* plane 0 */
#define SWG_DOT_ALL_MINUS 2u  /* plane 1 */
#define SWG_DOT_KEPT_PLUS 4u  /* plane 2 */
#define SWG_DOT_KEPT_MINUS 8u /* plane 3 */
typedef struct swg_dot_axes {
  uint32_t width, height;
  uint64_t x_total, y_total;
  const uint64_t* x_off; /* [n_seq] */
  const uint64_t* y_off; /* [n_seq] */
} swg_dot_axes; /* 40 bytes */
typedef struct swg_dot_request {
  uint32_t want;      /* the four bits above */
  uint32_t reserved;  /* 0 */
  uint32_t* plane[4]; /* in: caller-owned [height * width], fully written when wanted */
  uint64_t hits[4];   /* out, wanted planes only */
  uint64_t drawn[2];  /* out: drawn records, ALL and KEPT */
} swg_dot_request; /* 88 bytes */
/* rec: host pointers; x_off, y_off and status[n] (NULL: only the ALL planes) on the host. */
int swg_dotplot_records(swg_ctx* ctx, const swg_records* rec, const swg_dot_axes* axes, const uint8_t* status, swg_dot_request* req);
/* The same with the six columns and strand of rec, status, x_off and y_off in device memory of ctx's GPU; the request and its
 * planes stay on the host. */
int swg_dotplot_records_device(swg_ctx* ctx, const swg_records* rec, const swg_dot_axes* axes, const uint8_t* status, swg_dot_request* req);
/* The dot plot of an open PAF: out[0] receives the image, out[1] the layout table (release each with swg_free), under the marking
 * protocol of swg_paf_sharing: an entry that is NULL on entry is skipped, any other value asks for text k and is replaced by it.
 * The y axis holds the sequences that occur as the query of at least one record of the handle, whatever its status, and whose name
 * starts with query_prefix (NULL or "" = all), ordered by (genome id under the last-'#' map, sequence id); the x axis the same for
 * targets and target_prefix.  Lengths follow the last-seen rule of swg_paf_components, offsets are cumulative, the total is the
 * sum.  The axes are made on the host from the handle's id columns; the four planes come from one device call.
 *   image   binary PPM: `P6\n<W> <H>\n255\n` and 3 W H bytes; image row r is y = H - 1 - r (the origin is bottom-left).  The first
 *           rule that holds gives the colour: kept+ + kept- > 0 and kept- > kept+ (200,30,30); kept+ + kept- > 0 (0,0,0); all+ +
 *           all- > 0 and all- > all+ (245,190,190); all+ + all- > 0 (190,190,190); the pixel's column is px(off), or its row
 *           py(off), of the first sequence of a genome other than the axis' first (225,232,245); otherwise (255,255,255).
 *   layout  tab-separated, header `axis sequence genome offset length first_pixel last_pixel`, the rows of x, then of y, in axis
 *           order (genome names keep their trailing '#'; first_pixel = px(offset), last_pixel = px(offset + length - 1); a
 *           sequence of length 0: both px(min(offset, total - 1))).
 * status is needed (SWG_ERR_INVALID without); width or height outside 1 .. 16384: SWG_ERR_INVALID.  A PAF without records, or an
 * axis without a sequence or a base, gives an all-white image and the header-only table; that, and the layout alone, need no
 * device (ctx may be NULL then).  A handle whose columns are rebased: SWG_ERR_UNSUPPORTED.  Errors: swg_alnstats_last_error(). */
typedef struct swg_dot_view {
  uint32_t width, height;
  const char* query_prefix;  /* NULL or "" = all */
  const char* target_prefix; /* NULL or "" = all */
} swg_dot_view; /* 24 bytes */
int swg_paf_dotplot(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_dot_view* view, char* out[2], uint64_t out_len[2]);

/* ---- lift: caller-given regions projected through the mappings, on the device ----------------------------
 * A region is (seq, start, end), start <= end, half-open, on a sequence id of the record set; seq == UINT32_MAX is "a name the
 * input does not have" and has no hits.  Regions are numbered 0 .. m - 1 in the order given; they may overlap, repeat or be empty.
 * Record i is a HIT of region r on axis 0 (query) when q_id[i] == seq, q_end[i] > q_start[i] and max(start, q_start[i]) <
 * min(end, q_end[i]); on axis 1 (target) the same with t_id, t_start, t_end.  Self and intra-genome records count like any other
 * (no genome rule); a record with q_id == t_id can be a hit on both axes; start <= end of the records is assumed.  The set is
 * SWG_IV_ALL (every record) or SWG_IV_KEPT (status != 0, the rule of swg_paf_write).  For a hit, [s0, s1) is the record's side on
 * the axis (the source), [d0, d1) on dst_seq its other side, L = s1 - s0 > 0, D = d1 - d0; the clip is ca = max(start, s0), cb =
 * min(end, s1), o0 = ca - s0, o1 = cb - s0, f(o) = floor(o D / L), c(o) = ceil(o D / L) in unsigned 64 bits (exact: o D <=
 * (2^32 - 1)^2).  No CIGAR is on the device: the projection is linear interpolation, rounded outward,
 *   strand '+':  dst = [d0 + f(o0), d0 + c(o1))        strand '-':  dst = [d1 - c(o1), d1 - f(o0))
 * so a region that holds the whole source side gives exactly [d0, d1), dst lies inside [d0, d1], is non-empty whenever D > 0,
 * and growing the region never shrinks it.  Rows are ordered by (region, axis, s0, record), s0 the record's own start on the
 * axis; every value but `record` is independent of the order of the records, and the rows of a region do not depend on the other
 * regions.  summary[r].hits[set][axis] counts the hits of region r in both sets from the same pass (KEPT: 0 without a status; an
 * unwanted axis: 0): a region with hits in ALL and none in KEPT is one the filter left without a projection.  candidates[axis]
 * is the number of index entries the join looked at (section 23: the price of the prune, >= the hits of ALL on that axis; among
 * records with one start it depends on their order, the one figure here that does).
 * Capacity protocol of swg_breadth_counts: n > capacity still returns SWG_OK, leaves `rows` alone and has not run the write
 * pass.  m == 0 or n == 0 records needs no device work: n = 0 and zeroed summaries.  q_id, t_id, the four coordinates and strand
 * are read (32-bit layout).  Errors: a NULL context (there is no CPU path), reserved != 0 (request or region), axes == 0 or a bit
 * beyond bit 1, set > 1, KEPT without a status, a region with start > end or a seq that is neither < n_seq nor UINT32_MAX, a
 * record id >= n_seq: SWG_ERR_INVALID; 2^31 records or regions or more: SWG_ERR_RANGE (so a region has fewer than 2^31 hits per
 * set and axis, and the counters cannot overflow).  Scratch comes from the context's arena, SWG_ERR_OOM when the memory limit
 * does not hold it: per wanted axis 24 bytes per record (two 8-byte key buffers, two 4-byte value buffers; the running maximum
 * and the gathered ends live in the sort's spare pair), 12 bytes per region and 8 per tile of 1024 candidates; 16 bytes per region
 * for the summary, 16 more when both axes give rows, and 32 per row when the rows are written.  swg_lift_records stages its host
 * columns there too: 26 more bytes per record and 16 per region. */
typedef struct swg_lift_region {
  uint32_t seq, start, end;
  uint32_t reserved; /* 0 */
} swg_lift_region; /* 16 bytes */
typedef struct swg_lift_row {
  uint32_t region, record;     /* index into the regions; index into the records (what status[] indexes) */
  uint32_t src_start, src_end; /* ca, cb */
  uint32_t dst_seq;
  uint32_t dst_start, dst_end;
  uint32_t flags;              /* bit 0: strand (1 = '-'), bit 1: axis (1 = target); other bits 0 */
} swg_lift_row; /* 32 bytes */
typedef struct swg_lift_summary {
  uint32_t hits[2][2]; /* [set][axis] */
} swg_lift_summary; /* 16 bytes */
#define SWG_LIFT_AXIS_QUERY 1u
#define SWG_LIFT_AXIS_TARGET 2u
#define SWG_LIFT_MINUS 1u /* row flags */
#define SWG_LIFT_ON_TARGET 2u
typedef struct swg_lift_request {
  uint32_t set;              /* rows of SWG_IV_ALL (0) or SWG_IV_KEPT (1) */
  uint32_t axes;             /* bit 0 query, bit 1 target; at least one */
  uint64_t n;                /* out: rows */
  uint64_t candidates[2];    /* out: candidates per axis (0 for an unwanted axis) */
  uint64_t capacity;         /* in: entries `rows` can hold */
  swg_lift_row* rows;        /* in: caller-owned [capacity] or NULL; written only when n <= capacity */
  swg_lift_summary* summary; /* in: caller-owned [m] or NULL; written whenever non-NULL */
} swg_lift_request; /* 56 bytes */
/* rec: host pointers; status[n] (NULL: SWG_IV_ALL only) and regions[m] on the host. */
int swg_lift_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                     swg_lift_request* req);
/* The same with the six columns and strand of rec, status and regions in device memory of ctx's GPU; the request, its rows and
 * its summary stay on the host. */
int swg_lift_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                            swg_lift_request* req);
/* BED regions lifted through an open PAF: out_text[0] receives the rows, out_text[1] the summary (release each with swg_free),
 * under the marking protocol of swg_paf_sharing (an entry that is NULL on entry is skipped).  BED: tab-separated, columns 1-3
 * (name, start, end) required, column 4 an optional label (default `name:start-end`); empty lines and lines starting with `#`,
 * `track` or `browser` are skipped; a malformed line, start > end or a value >= 2^32 is SWG_ERR_INVALID with the line number in
 * swg_alnstats_last_error(); a name the handle does not know becomes seq = UINT32_MAX.  set: SWG_IV_ALL or SWG_IV_KEPT (the
 * rows' set; KEPT needs a status); axes as in the request.  Tab-separated texts:
 *   rows     one line per row in row order: dst_name dst_start dst_end label src_name src_start src_end strand(+|-) axis(q|t) record
 *   summary  header `label sequence start end all_q all_t kept_q kept_t state`, then one line per region in input order; state:
 *            `unknown` for an unknown name, `none` without hits in ALL on the wanted axes, `lost` with hits in ALL and none in
 *            KEPT, else `kept`.  Without a status the kept columns are `-` and state is `unknown`, `none` or `all`.
 * The BED is always parsed.  Empty BED text, or a PAF without records, gives the header-only summary and empty rows, and needs
 * no device (ctx may be NULL then).  A handle whose columns are rebased: SWG_ERR_UNSUPPORTED.  Errors: swg_alnstats_last_error(). */
int swg_paf_lift(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set, uint32_t axes,
                 char** out_text, uint64_t* out_len);

/* ---- base-exact lift: the rows of the lift refined through the records' CIGARs, on the device --------------
 * Hits, clips, sets, axes, row order, summary and candidates are the lift's, unchanged.  A CIGAR SET names k records (strictly
 * ascending) and gives each an ENTRY, a CIGAR text; only records that are hit need one (swg_lift_hit_records lists them).
 * The walk: an op is 1 to 10 decimal digits, value < 2^32 (0 allowed), and one letter of MIDNSHP=X.  With offsets x (query) and y
 * (target) from 0, in text order: M, = and X of length l make l aligned COLUMNS (x + i, y + i) and advance both; I advances x; D and
 * N advance y; S, H and P advance nothing.  A column's target coordinate is t_start + y, its query coordinate q_start + x on '+' and
 * q_end - 1 - x on '-' (PAF CIGARs run along the target's forward strand).
 * Entry state, a byte, 0 = usable:  1 syntax (a foreign byte, a letter without digits, more than 10 digits, trailing digits);
 * 2 an op value >= 2^32 (in at most 10 digits);  4 the query advances do not sum to q_end - q_start;  8 the target advances do not
 * sum to t_end - t_start (both sums in 64 bits, and looked at only when neither 1 nor 2 is set);  16 the entry is empty (a record
 * without CIGAR).  1 to 8 count as bad (cigar_bad), 16 does not.
 * Exact row: for a hit with clip [ca, cb) on the source side and destination side [d0, d1), A = the columns whose source coordinate
 * lies in [ca, cb); aligned = |A|, matches = the members of A from '=' ops.  A non-empty: dst = [min dst coordinate over A, max + 1).
 * A empty (the clip lies in bases without a partner): dst_start = dst_end = p, with B = the columns whose source coordinate is < ca:
 * on '+' p = max dst(B) + 1, or d0 when B is empty; on '-' p = min dst(B), or d1 when B is empty.  A row is exact when its record
 * has an entry of state 0: flag SWG_LIFT_EXACT is set.  Every other row keeps the lift's interpolated dst, aligned = matches = 0 and
 * the flag clear.  So dst lies inside [d0, d1], matches <= aligned <= min(cb - ca, dst_end - dst_start), a row with columns never
 * shrinks when its region grows, and a record whose CIGAR is the single op `L M` with equal sides gives the interpolated interval.
 * Capacity protocol and errors of swg_lift_records; besides: a set that is not strictly ascending, a record >= n, offset[0] != 0 or
 * a decreasing offset: SWG_ERR_INVALID; k >= 2^31, or 2^31 ops or more: SWG_ERR_RANGE.  k == 0 or cigars == NULL: every row is
 * interpolated (the first 32 bytes of each row are swg_lift_records' row).  ops, cigar_bad and state are written whenever the call
 * succeeds; exact_rows is 0 when the rows were not written.  n == 0 records with k > 0 is SWG_ERR_INVALID (a record >= n); m == 0
 * with k > 0 still parses the set.  Scratch from the arena on top of the lift's (SWG_ERR_OOM under a limit that does not hold it):
 * per text byte 1 byte staged (host seam only) and 0.25 of a rank per 16 bytes, plus 8 per tile of 4,096; per op 32 bytes (four
 * 64-bit prefix sums; the scans' own block sums are 1/4096 of that); per entry 5 bytes and, host seam only, the 12 of record[] and
 * offset[]; per row 40 bytes more when the rows are written. */
typedef struct swg_cigar_set {
  const uint32_t* record; /* [k] strictly ascending record indices, each < n */
  const uint64_t* offset; /* [k + 1], offset[0] = 0, non-decreasing: entry j is text[offset[j] .. offset[j + 1]) */
  const char* text;       /* the CIGARs end to end, no separators */
  uint64_t k;
} swg_cigar_set; /* 32 bytes */
typedef struct swg_lift_exact_row {
  uint32_t region, record;     /* the eight words of swg_lift_row */
  uint32_t src_start, src_end;
  uint32_t dst_seq;
  uint32_t dst_start, dst_end;
  uint32_t flags;              /* bits 0 and 1 as in swg_lift_row, bit 2: SWG_LIFT_EXACT */
  uint32_t aligned, matches;   /* columns inside the clip, and those of them from '=' ops; 0 on an interpolated row */
} swg_lift_exact_row; /* 40 bytes */
#define SWG_LIFT_EXACT 4u
#define SWG_CIGAR_SYNTAX 1u /* entry states */
#define SWG_CIGAR_VALUE 2u
#define SWG_CIGAR_QUERY_SUM 4u
#define SWG_CIGAR_TARGET_SUM 8u
#define SWG_CIGAR_EMPTY 16u
typedef struct swg_lift_exact_request {
  uint32_t set, axes;          /* as in swg_lift_request */
  uint64_t n;                  /* out: rows */
  uint64_t candidates[2];      /* out */
  uint64_t capacity;           /* in: entries `rows` can hold */
  swg_lift_exact_row* rows;    /* in: caller-owned [capacity] or NULL; written only when n <= capacity */
  swg_lift_summary* summary;   /* in: caller-owned [m] or NULL; written whenever non-NULL */
  uint8_t* state;              /* in: caller-owned [k] or NULL; written whenever non-NULL */
  uint64_t ops;                /* out: ops parsed over the whole set */
  uint64_t cigar_bad;          /* out: entries with a state bit of 1 .. 8 */
  uint64_t exact_rows;         /* out: rows with SWG_LIFT_EXACT; 0 when the rows were not written */
} swg_lift_exact_request; /* 88 bytes */
/* Everything on the host. */
int swg_lift_exact_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                           const swg_cigar_set* cigars, swg_lift_exact_request* req);
/* Columns, strand, status, regions and the three arrays of the set in device memory of ctx's GPU; the set structure itself, the
 * request, its rows, summary and state on the host. */
int swg_lift_exact_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                  const swg_cigar_set* cigars, swg_lift_exact_request* req);
/* The distinct records with at least one hit of `set` on the wanted axes, ascending: the records whose CIGARs an exact call needs.
 * *k receives their number; out (host, [capacity], may be NULL) is written only when *k <= capacity.  Checks and errors of
 * swg_lift_records; one byte per record of scratch on top of the lift's and its rows. */
int swg_lift_hit_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m, uint32_t set,
                         uint32_t axes, uint32_t* out, uint64_t capacity, uint64_t* k);
/* The same with the columns, strand, status and regions in device memory; out and k on the host. */
int swg_lift_hit_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                uint32_t set, uint32_t axes, uint32_t* out, uint64_t capacity, uint64_t* k);
/* swg_paf_lift through the CIGARs of the handle's own lines: contract, BED parser, marking protocol and refusals of swg_paf_lift.
 * The hit records come from the device (swg_lift_hit_records), the LAST cg:Z: tag of each one's line is its entry (the parser's
 * "last writer wins"; a line without the tag gives an empty entry), then one exact call.  Rows text: the ten columns of swg_paf_lift,
 * then `aligned matches mode`, mode = exact | interp.  The summary text is swg_paf_lift's. */
int swg_paf_lift_exact(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set, uint32_t axes,
                       char** out_text, uint64_t* out_len);
/* What the calling thread's last successful swg_paf_lift_exact met: records hit, entries of state 0, bad entries, records without
 * a tag. */
void swg_paf_lift_exact_counts(uint64_t out[4]);

/* ---- UCSC chain files: one chain per record from its CIGAR, built and formatted on the device --------------
 * The CIGAR set, the walk and the entry states 1 .. 16 are those of the base-exact lift above.  One more state bit, 32 = BEYOND:
 * q_end > seq_len[q_id] or t_end > seq_len[t_id].  An entry gives a chain when its state is 0 and its record is in `set`
 * (SWG_IV_ALL, or SWG_IV_KEPT: status != 0).
 * An op ADVANCES when it adds to x or y and is ALIGNED when it makes columns (M, =, X of non-zero length).  An aligned op is a BLOCK
 * START when the nearest earlier advancing op of its entry is not aligned, or there is none: zero-length ops and S, H, P neither
 * start nor separate blocks, runs of M, = and X merge, runs of I, D and N are one gap.  With the block starts s_0 < ... < s_{B-1},
 * e the entry's end and X, Y, A, E the exclusive prefix sums of x, y, columns and '=' columns over the ops:
 *   size_j = A[next] - A[s_j]  (next = s_{j+1}, or e for the last block);  for j < B - 1  dq_j = X[s_{j+1}] - X[s_j] - size_j and
 *   dt_j = Y[s_{j+1}] - Y[s_j] - size_j;  the last block has dt = dq = 0.  Leading and trailing gaps are cut off:
 *   x0 = X[s_0] - X[first], x1 = X[s_{B-1}] - X[first] + size_{B-1}, y0 and y1 alike on Y.
 * from = SWG_UCSC_FROM_TARGET (the PAF's target is the chain's reference sequence, as liftOver expects):
 *   ref = [t_start + y0, t_start + y1);  other = [q_start + x0, q_start + x1) on '+', and in UCSC's reverse-complement coordinates
 *   [seq_len[q] - q_end + x0, seq_len[q] - q_end + x1) on '-';  blocks in text order, (size, dt, dq).
 * from = SWG_UCSC_FROM_QUERY: on '+' the two sides and dt, dq change places; on '-' ref = [q_end - x1, q_end - x0), other =
 *   [seq_len[t] - t_start - y1, seq_len[t] - t_start - y0) on '-', and the blocks are reversed: block j' has size_{B-1-j'} and, for
 *   j' < B - 1, dt' = dq_{B-2-j'}, dq' = dt_{B-2-j'}.
 * score = the entry's '=' columns when it has any, else its aligned columns.  B == 0 (no aligned column): no chain (empty_chains).
 * Rows: one swg_ucsc_chain per ENTRY in set order (n_blocks == 0: no chain); its blocks are blocks[first_block .. + n_blocks), its
 * block lines text[text_first ..): `size\tdt\tdq\n` per block but the last, `size\n\n` for the last.  n_blocks, text_bytes and
 * first_block / text_first run over the emitted chains in set order.
 * Capacity protocol: chains is written when k <= chain_capacity, blocks when n_blocks <= block_capacity, text when text_bytes <=
 * text_capacity (each only when non-NULL); state whenever non-NULL; the counts whenever the call succeeds.  Refusals of the set as in
 * swg_lift_exact_records; a NULL seq_len, set or from out of range, SWG_IV_KEPT without status: SWG_ERR_INVALID; 2^32 text bytes
 * or more in one call, 2^31 blocks or more: SWG_ERR_RANGE.  k == 0 needs no device work.  Scratch from the arena (SWG_ERR_OOM under a
 * limit that does not hold it): the build's (see swg_lift_exact_records) plus, per op, 1 byte (flag) and 16 bytes per tile of 1,024;
 * per block 4 + 12 + 8 bytes and its text; per entry 48 bytes; the host seam stages 26 bytes per record and 4 per sequence. */
#define SWG_CIGAR_BEYOND 32u
#define SWG_UCSC_FROM_TARGET 0u
#define SWG_UCSC_FROM_QUERY 1u
#define SWG_UCSC_MINUS 1u /* swg_ucsc_chain.flags bit 0: the other side's strand is '-'; bits 8 .. 15: the entry's state */
typedef struct swg_ucsc_block {
  uint32_t size, dt, dq;
} swg_ucsc_block; /* 12 bytes */
typedef struct swg_ucsc_chain {
  uint32_t record, flags;
  uint32_t ref_start, ref_end; /* on the reference side, '+' */
  uint32_t oth_start, oth_end; /* on the other side, in that side's strand coordinates */
  uint32_t score, n_blocks;    /* n_blocks == 0: the entry gives no chain, every other field but record and flags is 0 */
  uint64_t first_block;        /* into blocks */
  uint64_t text_first;         /* into text */
} swg_ucsc_chain; /* 48 bytes */
typedef struct swg_ucsc_request {
  uint32_t set, from;          /* in */
  uint64_t chain_capacity;     /* in: entries `chains` can hold */
  swg_ucsc_chain* chains;      /* in: caller-owned or NULL; written only when k <= chain_capacity */
  uint64_t block_capacity;
  swg_ucsc_block* blocks;      /* written only when n_blocks <= block_capacity */
  uint64_t text_capacity;
  char* text;                  /* written only when text_bytes <= text_capacity */
  uint8_t* state;              /* in: caller-owned [k] or NULL; written whenever non-NULL */
  uint64_t n_chains;           /* out: entries that give a chain */
  uint64_t n_blocks;           /* out */
  uint64_t text_bytes;         /* out */
  uint64_t ops;                /* out: ops parsed over the whole set */
  uint64_t cigar_bad;          /* out: entries with a state bit of 1 .. 8 */
  uint64_t beyond;             /* out: entries with state bit 32 */
  uint64_t empty_chains;       /* out: entries of the set with state 0 and no aligned column */
} swg_ucsc_request; /* 120 bytes */
/* Everything on the host.  seq_len: [rec->n_seq]. */
int swg_ucsc_chain_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint8_t* status, const swg_cigar_set* cigars,
                           swg_ucsc_request* req);
/* Columns, strand, seq_len, status and the three arrays of the set in device memory of ctx's GPU; the set structure, the request
 * and its arrays on the host. */
int swg_ucsc_chain_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint8_t* status, const swg_cigar_set* cigars,
                                  swg_ucsc_request* req);
typedef struct swg_ucsc_counts {
  uint64_t records;  /* records of the set */
  uint64_t chains;   /* chains written */
  uint64_t bad;      /* entries with a state bit of 1 .. 8 */
  uint64_t beyond;   /* records that end beyond their sequence */
  uint64_t untagged; /* records without a cg:Z: tag */
  uint64_t empty;    /* entries without an aligned column */
  uint64_t blocks;
  uint64_t batches;  /* device calls */
} swg_ucsc_counts; /* 64 bytes */
/* The chain file of an open PAF: one chain per record of `set` whose line's LAST cg:Z: tag parses and fits (a line without the tag
 * is an empty entry), in record order, ids from 1.  Header `chain score tName tSize tStrand tStart tEnd qName qSize qStrand qStart
 * qEnd id` (names from the handle, sizes = the length on the line that mentions the sequence last), then the block lines.  The
 * records go to the device in batches of consecutive records whose CIGAR text stays within batch_bytes (0: a default from the
 * context's memory limit or the free device memory, below 2^32; a record larger than the batch is a batch of its own; one CIGAR of
 * 2^32 bytes or more is SWG_ERR_RANGE); the output is the same bytes for every batch_bytes.  counts may be NULL.  A PAF without
 * records of the set gives an empty file and needs no device (ctx may be NULL).  A handle whose columns are rebased:
 * SWG_ERR_UNSUPPORTED.  Errors: swg_alnstats_last_error(). */
int swg_paf_ucsc_chain_write(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t from, const char* out_path,
                             uint64_t batch_bytes, swg_ucsc_counts* counts);
/* The same as one malloc'd text (release with swg_free), for small inputs. */
int swg_paf_ucsc_chain_text(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t from, uint64_t batch_bytes,
                            swg_ucsc_counts* counts, char** text, uint64_t* len);

/* ---- lift slices: each lifted region as an alignment of its own, with its sliced CIGAR, on the device -------
 * Hit, clip [ca, cb), the walk offsets x and y, column, entry state and row order are those of the lift and of the base-exact lift
 * above.  Take an exact row (flag SWG_LIFT_EXACT) with aligned > 0, and let g0 < g1 be the column numbers of its record, in walk
 * order, so that A = columns g0 .. g1 - 1; x(g), y(g) are the walk offsets of column g.  The SLICE of the row is
 *   target  [t_start + y(g0), t_start + y(g1 - 1) + 1)
 *   query   [q_start + x(g0), q_start + x(g1 - 1) + 1) on '+',  [q_end - 1 - x(g1 - 1), q_end - x(g0)) on '-'
 * On the source axis this lies inside [ca, cb): the clip trimmed to its first and last aligned base; on the other axis it is the
 * row's dst exactly.  aligned and matches are the row's own; block = (x(g1 - 1) - x(g0) + 1) + (y(g1 - 1) - y(g0) + 1) - aligned in
 * 64 bits: columns plus inserted plus deleted bases inside the slice.
 * CIGAR text: with i0, i1 the ops that hold columns g0 and g1 - 1, A the exclusive prefix sum of the columns relative to the record's
 * first op, and pos[r] the byte of op r's letter in the entry's text: `<g1 - g0><letter i0>` when i0 == i1; otherwise
 * `<A[i0 + 1] - g0><letter i0>`, then the entry's bytes [pos[i0] + 1, pos[i1 - 1] + 1) verbatim (empty when i1 == i0 + 1; zero-length
 * ops and S, H, P in between are copied as they stand), then `<g1 - A[i1]><letter i1>`.  The text is never longer than the entry's
 * own, so text_len fits 32 bits; parsed as the entry of a record with the slice's four coordinates and strand it has state 0.
 * Flag bit 3 (SWG_SLICE_HAS_EQ): the whole entry has at least one '=' column (then `matches` is a count of matches, else it is 0
 * and only `aligned` says anything).
 * Rows without a slice are counted: a row without SWG_LIFT_EXACT as n_interp, an exact row with aligned == 0 as n_empty, an exact row
 * with 0 < aligned < min_aligned as n_short (min_aligned 0 is 1).  Slices are in the lift's row order; text_first runs over the slices
 * in that order, their texts end to end without separators.
 * Capacity protocol of swg_ucsc_chain_records: slices is written when n_slices <= slice_capacity, text when text_bytes <=
 * text_capacity (each only when non-NULL), state whenever non-NULL, the counts whenever the call succeeds.  Refusals of
 * swg_lift_exact_records; besides 2^32 rows or more, or 2^32 bytes of slice text or more, in one call: SWG_ERR_RANGE.  m == 0, or no
 * records, or no entries, needs no device work (every count 0 but for what the set alone gives).  Scratch from the arena on top of
 * the exact lift's: 4 bytes per op (pos), 81 bytes per row (the row's slice, its copy plan and a flag), 92 bytes per slice (slice,
 * copy plan, the scanned length, its row), the text itself, and nothing per tile: the text kernel cuts the output into tiles of
 * SWG_SLICE_TEXT_TILE bytes, one work-group each, which search their first slice themselves. */
#define SWG_SLICE_HAS_EQ 8u
#define SWG_SLICE_TEXT_TILE 4096u
typedef struct swg_lift_slice {
  uint32_t region, record;
  uint32_t q_start, q_end;
  uint32_t t_start, t_end;
  uint32_t flags;            /* bits 0 and 1 as in swg_lift_row: strand, axis; bit 3: SWG_SLICE_HAS_EQ */
  uint32_t aligned, matches;
  uint32_t text_len;
  uint64_t block;
  uint64_t text_first;       /* into text */
} swg_lift_slice; /* 56 bytes */
typedef struct swg_lift_slice_request {
  uint32_t set, axes;        /* as in swg_lift_request */
  uint32_t min_aligned;      /* slices with fewer aligned columns are counted, not written */
  uint32_t reserved;         /* 0 */
  uint64_t slice_capacity;   /* in: entries `slices` can hold */
  swg_lift_slice* slices;    /* in: caller-owned or NULL; written only when n_slices <= slice_capacity */
  uint64_t text_capacity;
  char* text;                /* written only when text_bytes <= text_capacity */
  uint8_t* state;            /* in: caller-owned [k] or NULL; written whenever non-NULL */
  uint64_t n_rows;           /* out: rows of the lift */
  uint64_t n_slices;         /* out */
  uint64_t n_interp;         /* out: rows without SWG_LIFT_EXACT */
  uint64_t n_empty;          /* out: exact rows without an aligned column */
  uint64_t n_short;          /* out: exact rows with 0 < aligned < min_aligned */
  uint64_t text_bytes;       /* out */
  uint64_t ops;              /* out: ops parsed over the whole set */
  uint64_t cigar_bad;        /* out: entries with a state bit of 1 .. 8 */
} swg_lift_slice_request; /* 120 bytes */
/* Everything on the host. */
int swg_lift_slice_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                           const swg_cigar_set* cigars, swg_lift_slice_request* req);
/* Columns, strand, status, regions and the three arrays of the set in device memory of ctx's GPU; the set structure, the request
 * and its arrays on the host. */
int swg_lift_slice_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                  const swg_cigar_set* cigars, swg_lift_slice_request* req);
/* SWG_SLICE_TEXT_TILE as the library was built with it. */
uint32_t swg_lift_slice_text_tile(void);
typedef struct swg_lift_paf_counts {
  uint64_t rows;     /* rows of the lift over all regions */
  uint64_t slices;   /* lines written */
  uint64_t interp;   /* rows whose record has no usable CIGAR */
  uint64_t empty;    /* exact rows without an aligned column */
  uint64_t too_short; /* exact rows below min_aligned */
  uint64_t hits;     /* entries uploaded, summed over the batches (a record hit from two batches counts twice) */
  uint64_t bad;      /* of those, entries with a state bit of 1 .. 8 */
  uint64_t batches;  /* slice calls */
} swg_lift_paf_counts; /* 64 bytes */
/* Each slice of BED regions lifted through an open PAF as one PAF line, in slice order: BED parser and refusals of swg_paf_lift,
 * the entries are the LAST cg:Z: tag of each hit record's line as in swg_paf_lift_exact.  Tab-separated:
 *   q_name q_len q_start q_end strand t_name t_len t_start t_end col10 block mapq cg:Z:<text> rn:Z:<label> ri:i:<record>
 * col10 = matches when bit 3 is set, else aligned; q_len, t_len and mapq are copied from the record's own line; names from the
 * handle.  One plain lift gives the hits per region; the BED is then cut into batches of consecutive regions whose cost, the sum
 * over their hits of (cg length + 24), stays within batch_bytes (0: the default of swg_paf_ucsc_chain_write; a region above the batch
 * is a batch of its own; one region of 2^32 or more is SWG_ERR_RANGE).  Each batch is one hit list and one slice call; a record hit
 * from two batches is uploaded twice.  The output is the same bytes for every batch_bytes.  counts may be NULL.  An empty BED or a
 * PAF without records gives an empty file and needs no device (ctx may be NULL).  Errors: swg_alnstats_last_error(). */
int swg_paf_lift_paf_write(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set, uint32_t axes,
                           uint32_t min_aligned, uint64_t batch_bytes, const char* out_path, swg_lift_paf_counts* counts);
/* The same as one malloc'd text (release with swg_free). */
int swg_paf_lift_paf_text(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set, uint32_t axes,
                          uint32_t min_aligned, uint64_t batch_bytes, swg_lift_paf_counts* counts, char** text, uint64_t* len);

/* ---- differences: every mismatch run, insertion and deletion of the CIGARs, on the device -------------------
 * The CIGAR set, the walk offsets x / y and the entry states 1 .. 16 are those of the base-exact lift above.  An entry is USABLE when
 * its state is 0 and its record is in `set` (SWG_IV_ALL, or SWG_IV_KEPT: status != 0).  Each op of a usable entry with letter c and
 * length l > 0 gives at most one ROW:
 *   X  SWG_DIFF_SNP   target [t_start + y, t_start + y + l), query length l
 *   I  SWG_DIFF_INS   target empty at t_start + y,           query length l
 *   D  SWG_DIFF_DEL   target [t_start + y, t_start + y + l), query length 0
 *   N  SWG_DIFF_SKIP  as D
 * =, M, S, H, P and ops of length 0 give no row; adjacent ops of one kind are NOT merged.  The query interval of query length L at
 * walk offset x is [q_start + x, q_start + x + L) on '+' and [q_end - x - L, q_end - x) on '-' (L == 0: the empty interval at that
 * point).  A row is written when its kind is in `kinds` and -- INS, DEL, SKIP only -- l >= min_indel.  left: the length of the op
 * directly in front of the row's op in the same entry when its letter is '=', else 0; right: the same for the op directly behind.
 * Rows come in (entry, op) order: record order, then text order (on '-' descending along the query).
 * Summary: per ordered genome pair (seq_genome[q_id], seq_genome[t_id]) over ALL ops of the usable entries, whatever kinds and
 * min_indel are; pairs ascend by (q_genome, t_genome); aligned = eq + snp_bases + m_columns.  Spectrum: [4][SWG_DIFF_BINS] over the
 * same ops, first index SNP, INS, DEL, SKIP, bin = the bit length of l (bin 0 stays 0).
 * Capacity protocol: rows is written when n_rows <= row_capacity, pairs when n_pairs <= pair_capacity (each only when non-NULL; rows
 * that nobody can take are counted and not built); spectrum and state whenever non-NULL; the counts whenever the call succeeds.
 * Refusals of the set as in swg_lift_exact_records; kinds == 0 or > 15, SWG_IV_KEPT without status, a NULL seq_genome, a record of the
 * set whose q_id / t_id is >= n_seq or whose sequence has a genome id >= n_genome: SWG_ERR_INVALID; 2^32 text bytes or more, 2^31
 * rows or more: SWG_ERR_RANGE.  k == 0 needs no device work.  Scratch from the arena (SWG_ERR_OOM under a limit that does not hold
 * it): the build's (see swg_lift_exact_records) plus, per op, 2 bytes (letter kind, row flag); per entry 8 bytes (its genome pair);
 * per row 4 + 32 bytes when the rows are built; the genome-pair table (96 bytes per slot, 120 per listed pair); the host seam stages
 * 26 bytes per record and 4 per sequence. */
#define SWG_DIFF_SNP 1u
#define SWG_DIFF_INS 2u
#define SWG_DIFF_DEL 4u
#define SWG_DIFF_SKIP 8u
#define SWG_DIFF_MINUS 256u /* swg_diff_row.kind_flags bit 8: the record is on the '-' strand; bits 0 .. 7: the kind */
#define SWG_DIFF_BINS 33
typedef struct swg_diff_row {
  uint32_t record, kind_flags;
  uint32_t t_start, t_end;
  uint32_t q_start, q_end;
  uint32_t left, right;
} swg_diff_row; /* 32 bytes */
typedef struct swg_diff_pair {
  uint32_t q_genome, t_genome;
  uint64_t entries, aligned, eq;
  uint64_t m_columns;            /* columns under M ops: mismatches there are unknowable */
  uint64_t snp_runs, snp_bases;
  uint64_t n_ins, ins_bases;
  uint64_t n_del, del_bases;
  uint64_t n_skip, skip_bases;
} swg_diff_pair; /* 104 bytes */
typedef struct swg_diff_request {
  uint32_t set, kinds;           /* in */
  uint32_t min_indel, reserved;  /* in; reserved must be 0 */
  uint64_t row_capacity;         /* in: entries `rows` can hold */
  swg_diff_row* rows;            /* in: caller-owned or NULL; written only when n_rows <= row_capacity */
  uint64_t pair_capacity;
  swg_diff_pair* pairs;          /* written only when n_pairs <= pair_capacity */
  uint64_t* spectrum;            /* in: caller-owned [4 * SWG_DIFF_BINS] or NULL; written whenever non-NULL */
  uint8_t* state;                /* in: caller-owned [k] or NULL; written whenever non-NULL */
  uint64_t n_rows;               /* out */
  uint64_t n_pairs;              /* out */
  uint64_t ops;                  /* out: ops parsed over the whole set */
  uint64_t cigar_bad;            /* out: entries with a state bit of 1 .. 8 */
  uint64_t usable;               /* out: usable entries */
} swg_diff_request; /* 104 bytes */
/* Everything on the host.  seq_genome: [rec->n_seq]. */
int swg_diff_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                     const swg_cigar_set* cigars, swg_diff_request* req);
/* Columns, strand, seq_genome, status and the three arrays of the set in device memory of ctx's GPU; the set structure, the request
 * and its arrays on the host. */
int swg_diff_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                            const swg_cigar_set* cigars, swg_diff_request* req);
typedef struct swg_diff_counts {
  uint64_t records;  /* records of the set */
  uint64_t usable;   /* usable entries */
  uint64_t bad;      /* entries with a state bit of 1 .. 8 */
  uint64_t untagged; /* records without a cg:Z: tag */
  uint64_t rows;
  uint64_t snp_runs, snp_bases; /* over all ops of the usable entries, as the summary */
  uint64_t n_ins, ins_bases;
  uint64_t n_del, del_bases;
  uint64_t n_skip, skip_bases;
  uint64_t m_columns;
  uint64_t batches;  /* device calls */
} swg_diff_counts; /* 120 bytes */
/* The differences of an open PAF into files: the records of `set` with the LAST cg:Z: tag of each one's line as its entry (a line
 * without the tag is an empty entry), in batches as swg_paf_ucsc_chain_write sends them; both texts are the same bytes for every
 * batch_bytes.  Genomes: the handle's seq_genome_two.  Either path may be NULL (not both); without rows_path the rows are counted
 * and not built.  Tab-separated texts, each with one header line when the set has a record:
 *   rows     t_name t_start t_end q_name q_start q_end strand(+|-) kind(SNP|INS|DEL|SKIP) len left right record
 *   summary  q_genome t_genome entries aligned eq m_columns snp_runs snp_bases ins ins_bases del del_bases skip skip_bases, one line
 *            per genome pair with an entry, ascending; then `#spectrum KIND lo hi count` per non-empty bin
 * A PAF without records of the set gives empty outputs (no header either) and needs no device (ctx may be NULL).  Every refusal comes before a file is
 * opened.  A handle whose columns are rebased: SWG_ERR_UNSUPPORTED.  counts may be NULL.  Errors: swg_alnstats_last_error(). */
int swg_paf_diffs_write(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t kinds, uint32_t min_indel,
                        uint64_t batch_bytes, const char* rows_path, const char* summary_path, swg_diff_counts* counts);
/* The same as malloc'd texts (release each with swg_free); rows_text or summary_text may be NULL (not both). */
int swg_paf_diffs_text(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t kinds, uint32_t min_indel,
                       uint64_t batch_bytes, swg_diff_counts* counts, char** rows_text, uint64_t* rows_len, char** summary_text,
                       uint64_t* summary_len);

/* ---- transitive lift: the closure of each region under the lift, hop by hop, on the device -----------------
 * Per region, independently of every other region (all sets are point sets per sequence, all arithmetic is in integers):
 *   hop 0      F_0 = V_0 = { [start, end) on seq } when seq is known and start < end, else both empty
 *   hop h >= 1 a piece (s, [x, y)) of F_{h-1} is WALKED when h == 1 or y - x >= min_len (the region itself always is).  A walked
 *              piece is lifted as the region (s, x, y) of the lift above: for every wanted axis and every record of the set that
 *              is a hit, dst by the outward-rounded rule, empty dst (D == 0) dropped.  P_h = the union of these intervals;
 *              F_h = the maximal intervals of P_h \ V_{h-1} (touching intervals are one, a gap of one base separates);
 *              V_h = V_{h-1} u P_h.  The walk stops after hop max_hops, or when no region has a piece left to walk from.
 * Rows: one per piece of every F_h, hop 0 included, ordered by (region, seq, start); the pieces of a region are disjoint; adjacent
 * pieces of different hops stay separate rows.  No strand is carried: a merged piece can come from both orientations.  Nothing
 * depends on the order of the records.  summary[r]: bases = the sum of the rows' lengths, pieces = the rows, sequences = the
 * distinct seq among them, hops = the largest hop of a row, flags bit 0 (SWG_CLOSURE_CUT) = a row of hop max_hops has length >=
 * max(min_len, 1): max_hops ended the walk, not the data.  An unknown or empty region has all fields 0.  min_len == 0 behaves as 1.
 * Out: n = rows; hops_run = the hops h >= 1 whose frontier F_{h-1} was not empty for every region (<= max_hops); projections =
 * the dst intervals made, summed over the hops (before the union); candidates[axis] as in the lift, summed over the hops.
 * Capacity protocol of the lift.  m == 0 gives n = 0.  A record set of n == 0 records still has the hop-0 rows of its known,
 * non-empty regions (pieces = 1, hops = 0): they are made on the host, without a kernel (the device seam copies the regions back).
 * Errors as in the lift (reserved != 0 of the request included), plus max_hops == 0 or > 65,535: SWG_ERR_INVALID; 2^30 intervals
 * or more in one hop's union: SWG_ERR_RANGE.  Scratch comes from the context's arena, SWG_ERR_OOM when the memory limit does not
 * hold it: per wanted axis the index of the lift, 24 bytes per record, built ONCE and joined by every hop; 45 bytes per region;
 * per hop 12 bytes per frontier slot and wanted axis and 32 per interval of the union (P_h + |V_{h-1}|: the slots of the new
 * frontier and of the new visited set) -- these stay until the call ends -- and, given back after the hop, 16 per projection and
 * 124 per interval of the union (two events of 16 bytes, and per event 24 of sort buffers, 8 of depth, 4 of position, 2 flags
 * and 8 of edge lists); at the end 64 bytes per row, 24 more when the rows are fetched.  swg_lift_closure_records stages its
 * host columns there too: 26 more bytes per record, 16 per region. */
typedef struct swg_closure_row {
  uint32_t region, seq;
  uint32_t start, end;
  uint32_t hop;
  uint32_t reserved; /* 0 */
} swg_closure_row; /* 24 bytes */
typedef struct swg_closure_summary {
  uint64_t bases;
  uint32_t pieces, sequences, hops, flags;
} swg_closure_summary; /* 24 bytes */
#define SWG_CLOSURE_CUT 1u
typedef struct swg_closure_request {
  uint32_t set;                 /* SWG_IV_ALL (0) or SWG_IV_KEPT (1) */
  uint32_t axes;                /* bit 0 query, bit 1 target; at least one */
  uint32_t max_hops;            /* 1 .. 65,535 */
  uint32_t min_len;             /* a piece shorter than this is reported and not walked on */
  uint64_t capacity;            /* in: entries `rows` can hold */
  swg_closure_row* rows;        /* in: caller-owned [capacity] or NULL; written only when n <= capacity */
  swg_closure_summary* summary; /* in: caller-owned [m] or NULL; written whenever non-NULL */
  uint64_t n;                   /* out: rows */
  uint64_t projections;         /* out */
  uint64_t candidates[2];       /* out */
  uint32_t hops_run;            /* out */
  uint32_t reserved;            /* 0 */
} swg_closure_request; /* 80 bytes */
/* rec: host pointers; status[n] (NULL: SWG_IV_ALL only) and regions[m] on the host. */
int swg_lift_closure_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                             swg_closure_request* req);
/* The same with the six columns and strand of rec, status and regions in device memory of ctx's GPU. */
int swg_lift_closure_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                    swg_closure_request* req);
/* BED regions walked through an open PAF: the BED parser, the marking protocol and the refusals of swg_paf_lift.  Texts:
 *   rows     one line per row in row order: name start end label hop   (BED-like: the piece first; no strand, see above)
 *   summary  header `label sequence start end pieces sequences genomes bases hops state`, then one line per region in input order;
 *            genomes = the distinct genome prefixes (up to the last '#') of the rows' sequences; state: `unknown` for an unknown
 *            name, `none` when nothing lies beyond hop 0 (an empty region included), `cut` when SWG_CLOSURE_CUT is set, else `closed`.
 * Empty BED text gives the header-only summary and empty rows.  A PAF without records knows no name: every region is `unknown`
 * and there are no rows.  Neither needs a device (ctx may be NULL then). */
int swg_paf_lift_closure(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set, uint32_t axes,
                         uint32_t max_hops, uint32_t min_len, char** out_text, uint64_t* out_len);

/* ---- mosaic: the best mapping at every base (no reference counterpart) ---------------------------------
 * The reports above say how much is covered, where, and by how many genomes; this says BY WHICH MAPPING.  Every value is an
 * integer, every comparison exact.  On the query axis (0) record r lies on sequence q_id[r] over [q_start, q_end) and its other
 * sequence is t_id[r]; on the target axis (1) the roles swap.  The counting rule is breadth's: a record counts only when the
 * genomes of its two sequences differ under the caller's seq_genome, intervals are half-open, a zero-length record on the axis
 * adds nothing, start <= end is assumed.  set: SWG_IV_ALL = the counted records, SWG_IV_KEPT = those with status != 0.
 *   priority  P(r) = (uint64)weight[r] << 32 | (0xffffffff - r): the heavier record wins, among equal weights the lower index.
 *             weight == NULL: rec->matches.
 *   winner    at base x of sequence s: the record of the set on the axis with seq == s, start <= x < end and maximal P.
 *   rows      the maximal half-open intervals of a sequence with one winner, ordered by (seq, start); stretches without a
 *             winner are not listed.  One record can own several rows (a heavier record nested inside it cuts it in two).
 *             bases = sum(end - start) = the bases under at least one record of the set.
 *   share     share[g * n_genome + h] = bases of the sequences of genome g won by records whose other sequence is of genome h;
 *             the diagonal is 0.
 * Values and order depend neither on the launch shapes nor, with pairwise different weights, on the order of the records.
 * `want`: SWG_MOSAIC_ROWS writes n and bases and, under the capacity protocol of swg_breadth_counts, the rows (n > capacity
 * still returns SWG_OK and leaves `rows` alone); SWG_MOSAIC_SHARE writes all n_genome * n_genome entries of the caller's array
 * and reads back no rows.  Errors: a NULL context (there is no CPU path), reserved != 0, want == 0 or a bit beyond the two, axis
 * > 1, set > 1, SWG_IV_KEPT with status == NULL, the share bit with a NULL share, a sequence id >= n_seq or a genome id >=
 * n_genome, weight == NULL with rec->matches == NULL: SWG_ERR_INVALID; n >= 2^31 records, or the share bit with n_genome > 4096
 * (the rows stay available): SWG_ERR_RANGE.  q_id, t_id, the four coordinates and matches (weight == NULL) are read.  Scratch
 * comes from the context's arena, SWG_ERR_OOM when the memory limit does not hold it: 48 bytes per record for the sort of the
 * 2n boundary entries, then per DISTINCT boundary (B <= 2n + 1) 21 bytes and 8 * bits(B / T) / T for the tile table (T = 512), 5
 * per change of winner, 20 per row and 8 * n_genome^2 for a share (DESIGN.md section 25 has the formula).  swg_mosaic_records
 * stages its host columns there too: 29 more bytes per record. */
typedef struct swg_mosaic_row {
  uint32_t seq;
  uint32_t start, end; /* half-open */
  uint32_t record;     /* the winner */
} swg_mosaic_row; /* 16 bytes */
#define SWG_MOSAIC_ROWS 1u
#define SWG_MOSAIC_SHARE 2u
typedef struct swg_mosaic_request {
  uint32_t want;          /* the two bits above */
  uint32_t axis;          /* 0 = query, 1 = target */
  uint32_t set;           /* SWG_IV_ALL or SWG_IV_KEPT */
  uint32_t reserved;      /* 0 */
  const uint32_t* weight; /* [n] or NULL = rec->matches; host / device as the columns */
  uint64_t n, bases;      /* out (rows bit) */
  uint64_t capacity;      /* in: entries `rows` can hold */
  swg_mosaic_row* rows;   /* in: caller-owned [capacity] or NULL; written only when n <= capacity */
  uint64_t* share;        /* in (share bit): caller-owned [n_genome * n_genome], fully written */
} swg_mosaic_request; /* 64 bytes, no implicit padding */
/* rec: host pointers; seq_genome[rec->n_seq], status[n] (NULL: SWG_IV_ALL only) and req->weight on the host. */
int swg_mosaic_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                       swg_mosaic_request* req);
/* The same with the columns of rec, seq_genome, status and req->weight in device memory of ctx's GPU; the request and its
 * arrays stay on the host. */
int swg_mosaic_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                              swg_mosaic_request* req);
/* Both texts of an open PAF under its last-'#' genome map from ONE device call (release each with swg_free); a text is asked
 * for by a non-NULL out_text[k] on entry, as in swg_paf_sharing.  The weight is the matches column, with by_length != 0 the
 * record's end - start on the axis (computed on the device).  Tab-separated:
 *   text 0  BED-like, one line per row: sequence start end other_sequence strand(+|-) record weight other_start other_end --
 *           record is the 0-based record number, the other interval the whole record's; the file is a --lift-regions input.
 *   text 1  header `genome other_genome bases`, one line per non-zero share entry in (g, h) order (names keep their trailing
 *           '#'), then `#total <bases>`.
 * A PAF without records gives the header-only texts (text 0 is empty) and needs no device (ctx may be NULL then).  set ==
 * SWG_IV_KEPT with status == NULL: SWG_ERR_INVALID; a handle with rebased columns: SWG_ERR_UNSUPPORTED; more than 4096 genomes
 * with text 1: SWG_ERR_RANGE.  Errors: text in swg_alnstats_last_error(). */
int swg_paf_mosaic(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t axis, uint32_t set, int by_length, char** out_text,
                   uint64_t* out_len);

/* ---- gaps: the indel at every link of a kept chain, and every captured inversion (no reference counterpart)
 * A pure function of the record columns (q_id, t_id, the four coordinates and strand; 32-bit layout), status[n] and chain[n] as
 * swg_filter* writes them, seq_genome[n_seq] and min_size.  Every value is an integer, every comparison exact.
 *   takes part  a record with status == SWG_ST_SCAFFOLD and chain != 0 (rescued, unassigned and dropped records take no part).
 *   strand      of a chain: '+' if any record of it that takes part is '+', else '-'.  core = its records on that strand,
 *               inverted = the '-' records of a '+' chain (swg_block's rule).  All records of a chain share (q_id, t_id).
 *   order       inside a chain (q_start, record index) ascending: the reference's chaining order (src/paf_filter.rs:774-866), so
 *               the consecutive core records of a filter's own output are the links chaining made.
 *   link        for a core record b with an earlier core record in its chain, a = the nearest such (inverted records between
 *               the two are skipped): dq = q_start[b] - q_end[a]; dt = t_start[b] - t_end[a] on a '+' chain and t_start[a] -
 *               t_end[b] on a '-' chain; both signed 64-bit, negative = overlap; size = dq - dt.
 *   link row    when |size| >= min_size (min_size 0: every link): kind = SWG_GAP_INS for size > 0, SWG_GAP_DEL for size < 0,
 *               SWG_GAP_EVEN for size == 0; left = a, right = b; q_lo / q_hi = min / max of (q_end[a], q_start[b]); t_lo / t_hi
 *               = min / max of the two facing target ends ('+': t_end[a], t_start[b]; '-': t_start[a], t_end[b]); flags bit 0 =
 *               dq < 0, bit 1 = dt < 0.  dq, dt and size follow from the row (|dq| = q_hi - q_lo, its sign is the flag).
 *   inversion   every inverted record r with q_end - q_start >= min_size: kind = SWG_GAP_INV, left = right = r, its own query
 *               and target interval, flags 0.
 *   row order   (chain, q_start[right], right) ascending; link rows and inversion rows interleave.
 *   summary     per ORDERED genome pair (seq_genome[q_id], seq_genome[t_id]): links = all links whatever min_size; n_ins,
 *               ins_bases = sum(size); n_del, del_bases = sum(-size); n_inv, inv_bases = sum(q_end - q_start) -- the last six
 *               over the rows only.  A pair has an entry when links or n_inv is non-zero; ascending (q_genome, t_genome).
 *   spectrum    [2][33], row 0 INS and row 1 DEL, over the rows: bin = bit length of |size| (bin k: 2^(k-1) <= |size| < 2^k),
 *               the last bin taking everything from 2^31 (|size| reaches 2^33 - 2).  Bin 0 is empty; SWG_GAP_EVEN is not counted.
 * Nothing depends on the order of the records beyond the index tie-break, nor on a launch shape.  `want`: SWG_GAPS_ROWS writes
 * n_rows and, under the capacity protocol of swg_breadth_counts, the rows (n_rows > capacity still returns SWG_OK and leaves
 * `rows` alone); SWG_GAPS_SUMMARY writes n_pairs, the pairs under the same protocol, and all 66 entries of a non-NULL spectrum.
 * Errors: a NULL context (there is no CPU path), reserved != 0, want == 0 or a bit beyond the two, a NULL column, a chain whose
 * records that take part name two (q_id, t_id) pairs (the message names the chain), a sequence id >= n_seq or a genome id >=
 * n_genome: SWG_ERR_INVALID; n >= 2^31 records or a chain number of 2^32 - 1: SWG_ERR_RANGE.  Scratch comes from the context's
 * arena, SWG_ERR_OOM when the memory limit does not hold it: 24 bytes per record for the sort (two 8-byte key and two 4-byte value
 * buffers) plus the radix sort's histograms, 6 bytes per record that takes part (class, row flag, predecessor), 4 bytes per chain
 * NUMBER (the strand table is dense in the chain number: its largest value sizes it), 36 bytes per row, and the genome-pair
 * table (sized by what occurs).  swg_gaps_records stages its host columns there too: 30 more bytes per record. */
#define SWG_GAP_EVEN 0u
#define SWG_GAP_INS 1u
#define SWG_GAP_DEL 2u
#define SWG_GAP_INV 3u
typedef struct swg_gap_row {
  uint32_t chain;       /* N of ch:Z:chain_N */
  uint32_t left, right; /* record numbers: a and b of a link, the record itself for an inversion */
  uint32_t q_lo, q_hi;
  uint32_t t_lo, t_hi;
  uint8_t kind;         /* SWG_GAP_* */
  uint8_t flags;        /* bit 0: dq < 0, bit 1: dt < 0 */
  uint16_t reserved;    /* 0 */
} swg_gap_row; /* 32 bytes, no implicit padding */
typedef struct swg_gap_pair {
  uint32_t q_genome, t_genome; /* ORDERED pair of genome ids (query genome, target genome) */
  uint64_t links;              /* all links of the pair, whatever min_size */
  uint64_t n_ins, ins_bases;
  uint64_t n_del, del_bases;
  uint64_t n_inv, inv_bases;
} swg_gap_pair; /* 64 bytes */
#define SWG_GAPS_ROWS 1u
#define SWG_GAPS_SUMMARY 2u
#define SWG_GAPS_BINS 33
typedef struct swg_gaps_request {
  uint32_t want;          /* the two bits above */
  uint32_t min_size;
  uint64_t n_rows;        /* out (rows bit) */
  uint64_t capacity;      /* in: entries `rows` can hold */
  swg_gap_row* rows;      /* in: caller-owned [capacity] or NULL; written only when n_rows <= capacity */
  uint64_t n_pairs;       /* out (summary bit) */
  uint64_t pair_capacity; /* in: entries `pairs` can hold */
  swg_gap_pair* pairs;    /* in: caller-owned [pair_capacity] or NULL; written only when n_pairs <= pair_capacity */
  uint64_t* spectrum;     /* in (summary bit): caller-owned [2 * SWG_GAPS_BINS] or NULL; fully written */
  uint64_t reserved;      /* 0 */
} swg_gaps_request; /* 72 bytes, no implicit padding */
/* rec: host pointers; status[n], chain[n] and seq_genome[rec->n_seq] on the host. */
int swg_gaps_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const uint32_t* chain, const uint32_t* seq_genome,
                     uint32_t n_genome, swg_gaps_request* req);
/* The same with the seven columns of rec, status, chain and seq_genome in device memory of ctx's GPU (as swg_filter_device
 * leaves them: no copy in between); the request and its arrays stay on the host. */
int swg_gaps_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const uint32_t* chain, const uint32_t* seq_genome,
                            uint32_t n_genome, swg_gaps_request* req);
/* Both texts of an open PAF under its last-'#' genome map from ONE device call (release each with swg_free); a text is asked
 * for by a non-NULL rows_text / summary_text (its length pointer must then be non-NULL too).  Tab-separated:
 *   rows     header `#query q_start q_end target t_start t_end kind size chain dq dt left right`, then one line per row:
 *            names from the handle, q_lo q_hi, t_lo t_hi, kind INS | DEL | INV | EVEN, size dq dt as signed decimals (INV: size =
 *            the query length, dq = dt = 0), left and right as 0-based record numbers.
 *   summary  header `#query_genome target_genome links ins ins_bases del del_bases inv inv_bases`, one line per genome pair
 *            (names keep their trailing '#'), then one line `#spectrum KIND lo hi count` per non-empty bin (lo and hi inclusive).
 * A PAF without records, or a status and chain without a chain that takes part, gives the header-only texts and needs no
 * device (ctx may be NULL then).  A handle with rebased columns: SWG_ERR_UNSUPPORTED.  Errors: swg_alnstats_last_error(). */
int swg_paf_gaps(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const uint32_t* chain, uint32_t min_size, char** rows_text,
                 uint64_t* rows_len, char** summary_text, uint64_t* summary_len);

/* ---- place: every sequence ordered and oriented along its best partner (no reference counterpart) -------
 * Which sequence of the other genome does this one belong to, in which orientation, and where along it?  A pure function of the
 * record columns (q_id, t_id, the four coordinates and strand; 32-bit layout), seq_len[n_seq], seq_genome[n_seq], status[n] (for
 * the KEPT set), the axis, the set and min_bases.  Every value is an integer, every comparison exact.
 *   axis        on axis 0 (query) record r places sequence s = q_id[r] on partner p = t_id[r] with weight w = q_end - q_start; on
 *               axis 1 (target) the roles and the columns swap (s = t_id, p = q_id, w = t_end - t_start).
 *   anchor      off = the partner coordinate that base 0 of s extrapolates to.  Axis 0: '+' record off = t_start - q_start, '-'
 *               record off = t_end + q_start; axis 1: q_start - t_start and q_end + t_start.  Signed 64-bit, within
 *               -(2^32 - 1) .. 2 * (2^32 - 1).
 *   takes part  a record of the set with seq_genome[s] != seq_genome[p] (breadth's and mosaic's counting rule).  SWG_IV_ALL:
 *               every such record; SWG_IV_KEPT: those with status != 0.  A zero-length record takes part with weight 0.
 *   candidate   (s, p): fwd, rev = sum of w over its '+' / '-' records that take part, n_records = their number, bases = fwd + rev.
 *   winner      of (s, g), g = seq_genome[p]: the candidate with the largest bases, among equals the smaller p.  total_bases = sum
 *               of bases over all candidates of (s, g); runner_bases = the bases of the second candidate under the same order, 0
 *               when there is none.
 *   orientation '+' (0) when fwd >= rev and the winner has a '+' record, else '-' (1).  (The second condition matters only for a
 *               winner of weight 0 without '+' records: it is '-', so that the deciding records are never none.)  The deciding
 *               records are the winner's records on that strand.
 *   offset      the weighted median of off over the deciding records: ordered by (off, record index), W = sum of their weights,
 *               half = max(1, ceil(W / 2)), offset = the off of the first record whose inclusive prefix sum of weights is >= half;
 *               W == 0: the first record's off.  The VALUE does not depend on how equal off are ordered.
 *   span        q_lo, q_hi = min of the starts / max of the ends of the deciding records on the placed axis, t_lo, t_hi on the
 *               partner axis; start = offset for '+', offset - seq_len[s] for '-' (signed; seq_len is taken as given).
 *   rows        one per (s, g) whose winner has bases >= min_bases, in layout order (seq_genome[s], g, p, start, s) ascending;
 *               rank = the 0-based position of the row among the rows with its (seq_genome[s], p).
 *   summary     one entry per ordered genome pair (seq_genome[s], g) that has a row, ascending: rows, reversed (the '-' rows),
 *               length = sum of seq_len[s], bases = sum of the winners' bases, total_bases = sum of the rows' total_bases.
 * Nothing depends on the order of the records or on a launch shape.  `want`: SWG_PLACE_ROWS writes n_rows and, under the capacity
 * protocol of swg_breadth_counts, the rows (n_rows > capacity still returns SWG_OK and leaves `rows` alone); SWG_PLACE_SUMMARY
 * writes n_pairs and the pairs under the same protocol, each array on its own.  Errors: a NULL context (there is no CPU path),
 * reserved != 0, want == 0 or a bit beyond the two, axis > 1, set > 1, SWG_IV_KEPT with status == NULL, a NULL column, a
 * sequence id >= n_seq or a genome id >= n_genome (found on the device before any gather trusts it): SWG_ERR_INVALID; n >= 2^31
 * records, n_seq > 2^31 (sequence, partner and strand share one 64-bit sort key) or 2^30 rows or more (the median's sort key
 * holds the row above the 34-bit anchor): SWG_ERR_RANGE.  Scratch comes from the context's arena, SWG_ERR_OOM when the memory
 * limit does not hold it: 24 bytes per record for the sort plus the radix sort's histograms, 9 per record that takes part, 5 per
 * (s, p, strand) run, 73 per candidate, 25 per (s, g), 32 per deciding record, 218 per row and 52 per genome pair (DESIGN.md
 * section 28 has the formula).  swg_place_records stages its host columns there too: 26 more bytes per record and 8 per sequence. */
typedef struct swg_placement {
  uint32_t seq, partner;           /* s and p */
  uint32_t genome, partner_genome; /* seq_genome[s] and g */
  int64_t offset;                  /* the weighted median of the anchors */
  int64_t start;                   /* where base 0 ('+') or the last base's far side ('-') of s falls: the layout coordinate */
  uint64_t bases, fwd, rev;        /* of the winner; bases = fwd + rev */
  uint64_t total_bases;            /* over all candidates of (s, g) */
  uint64_t runner_bases;           /* of the second candidate, 0 = none */
  uint64_t n_records;              /* of the winner, both strands */
  uint32_t q_lo, q_hi;             /* span of the deciding records on s */
  uint32_t t_lo, t_hi;             /* ... and on p */
  uint32_t rank;                   /* among the rows of (genome, partner) */
  uint8_t orient;                  /* 0 = '+', 1 = '-' */
  uint8_t reserved[3];             /* 0 */
} swg_placement; /* 104 bytes, no implicit padding */
typedef struct swg_place_pair {
  uint32_t genome, partner_genome; /* ORDERED pair: the genome of the placed sequences, the genome they are placed on */
  uint64_t rows, reversed;
  uint64_t length;                 /* sum of seq_len over the placed sequences */
  uint64_t bases, total_bases;
} swg_place_pair; /* 48 bytes, no implicit padding */
#define SWG_PLACE_ROWS 1u
#define SWG_PLACE_SUMMARY 2u
typedef struct swg_place_request {
  uint32_t want;           /* the two bits above */
  uint32_t axis;           /* 0 = query, 1 = target */
  uint32_t set;            /* SWG_IV_ALL or SWG_IV_KEPT */
  uint32_t reserved;       /* 0 */
  uint64_t min_bases;      /* a row needs a winner with at least this many bases */
  uint64_t n_rows;         /* out (rows bit) */
  uint64_t capacity;       /* in: entries `rows` can hold */
  swg_placement* rows;     /* in: caller-owned [capacity] or NULL; written only when n_rows <= capacity */
  uint64_t n_pairs;        /* out (summary bit) */
  uint64_t pair_capacity;  /* in: entries `pairs` can hold */
  swg_place_pair* pairs;   /* in: caller-owned [pair_capacity] or NULL; written only when n_pairs <= pair_capacity */
} swg_place_request; /* 72 bytes, no implicit padding */
/* rec: host pointers; seq_len[rec->n_seq], seq_genome[rec->n_seq] and status[n] (NULL: SWG_IV_ALL only) on the host. */
int swg_place_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                      const uint8_t* status, swg_place_request* req);
/* The same with the seven columns of rec, seq_len, seq_genome and status in device memory of ctx's GPU (as swg_filter_device
 * leaves them: no copy in between); the request and its arrays stay on the host. */
int swg_place_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                             const uint8_t* status, swg_place_request* req);
/* Both texts of an open PAF from ONE device call (release each with swg_free) under its last-'#' genome map and the last-seen
 * lengths of swg_paf_components; a text is asked for by a non-NULL out_text[k] on entry, as in swg_paf_mosaic.  Tab-separated:
 *   text 0  header `#sequence length partner partner_length orient start end rank bases fwd rev total runner records q_lo q_hi
 *           t_lo t_hi`, then one line per row: names and lengths from the handle, orient + | -, end = start + length, start and
 *           end as signed decimals.
 *   text 1  header `#genome partner_genome sequences reversed length bases total_bases`, one line per summary entry (names keep
 *           their trailing '#').
 * A PAF without records gives the header-only texts and needs no device (ctx may be NULL then).  axis > 1, set > 1, SWG_IV_KEPT
 * with status == NULL: SWG_ERR_INVALID; a handle with rebased columns: SWG_ERR_UNSUPPORTED.  Errors: swg_alnstats_last_error(). */
int swg_paf_place(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t axis, uint32_t set, uint64_t min_bases, char** out_text,
                  uint64_t* out_len);

/* ---- windows: depth, cover and identity per fixed window (no reference counterpart) -----------------------
 * The track along a sequence: per window of W bases how deep the pile of mappings is, how much of the window is covered at all
 * and how well it matches, for ALL records and for the records a filter call KEPT, from one device call.  A pure function of the
 * record columns (q_id, t_id, the two coordinates of the axis, matches or `weight`; 32-bit layout), seq_len[n_seq],
 * seq_genome[n_seq], status[n], the axis, W and other_genome.  Every value is an integer, every comparison exact.
 *   axis        on axis 0 (query) record r lies on s = q_id[r] over [a, b) = [q_start, q_end) and its other sequence is
 *               o = t_id[r]; on axis 1 (target) the roles and the columns swap.  m = weight[r]; weight == NULL: rec->matches[r].
 *   takes part  (set ALL) seq_genome[s] != seq_genome[o] (breadth's counting rule), a < b (a zero-length or reversed record adds
 *               nothing and lists nothing), and other_genome == SWG_WINDOWS_ANY or seq_genome[o] == other_genome.
 *   set KEPT    the records of ALL with status != 0.  status == NULL: there is no KEPT set and every [1] entry below is 0.
 *   windows     sequence s has K_s = ceil(seq_len[s] / W) windows, window k = [k W, min((k + 1) W, seq_len[s])).  A record that
 *               takes part with b > seq_len[s] is an error (found on the device before any write trusts it; the message names the
 *               record with the smallest index).  A sequence is LISTED when at least one record of ALL lies on it.
 *   per window and set, with ov(r, k) = the length of [a, b) in window k:
 *               n = the records with ov > 0; depth = sum of ov; covered = the bases of the window under at least one record (the
 *               union); matches = sum of floor(ov * m / (b - a)) (the product is below 2^64; a record inside one window gives
 *               exactly m, an interior window of a long record floor(W * m / (b - a))).  Mean depth is depth / (end - start),
 *               identity matches / depth, breadth covered / (end - start): the caller divides.
 *   rows        one per window of every listed sequence, empty windows included, (seq, index) ascending; sequences that are not
 *               listed have none.
 *   summary     one entry per listed sequence, ascending: windows = K_s; empty[set] = its windows with covered == 0 (status ==
 *               NULL: empty[1] = 0 like every [1] entry); covered, depth and matches summed over its windows; records[set] = the
 *               records that take part on it (one that spans five windows counts once).
 * Nothing depends on the order of the records or on a launch shape: all updates are integer additions.  `want`:
 * SWG_WINDOWS_ROWS writes n_rows and, under the capacity protocol of swg_breadth_counts, the rows (n_rows > capacity still returns
 * SWG_OK and leaves `rows` alone); SWG_WINDOWS_SUMMARY writes n_seqs and the entries under the same protocol, each array on its
 * own.  On an error found after the arguments were accepted the counts are 0.  Errors: a NULL context (there is no CPU path),
 * reserved != 0, want == 0 or a bit beyond the two, axis > 1, window == 0, other_genome >= n_genome and not SWG_WINDOWS_ANY, a
 * NULL column (seq_len and seq_genome included), weight == NULL with rec->matches == NULL, a sequence id >= n_seq or a genome id
 * >= n_genome, a record that takes part and ends beyond its sequence: SWG_ERR_INVALID; n >= 2^31 records, n_seq > 2^31 or 2^31
 * windows or more in the listed sequences (refused before anything of that size is allocated): SWG_ERR_RANGE.  Scratch comes
 * from the context's arena, SWG_ERR_OOM when the memory limit does not hold it: 28 bytes per record (the union's sort: two 8-byte
 * key and two 4-byte value buffers, and the ends in sorted order) plus the radix sort's histograms and 16 bytes per tile of 1,024
 * records; 9 bytes per sequence (listed flag, window prefix) and 4 per listed one; 120 bytes per window (per set five 8-byte
 * count / difference arrays, two 8-byte and one 4-byte edge accumulators) plus 64 for its row, and 80 per listed sequence with
 * the summary.  swg_windows_records stages its host columns there too: 21 more bytes per record (the two ids, the
 * axis' two coordinates, the weight, the status) and 8 per sequence. */
#define SWG_WINDOWS_ANY 0xffffffffu
typedef struct swg_window_row {
  uint32_t seq, index;  /* s and k */
  uint32_t start, end;  /* the window, half-open, clipped to seq_len */
  uint32_t n[2];        /* [0] = ALL, [1] = KEPT */
  uint32_t covered[2];
  uint64_t depth[2];
  uint64_t matches[2];
} swg_window_row; /* 64 bytes, no implicit padding */
typedef struct swg_window_seq {
  uint32_t seq, windows;
  uint32_t empty[2];
  uint64_t covered[2], depth[2], matches[2], records[2];
} swg_window_seq; /* 80 bytes, no implicit padding */
#define SWG_WINDOWS_ROWS 1u
#define SWG_WINDOWS_SUMMARY 2u
typedef struct swg_windows_request {
  uint32_t want;          /* the two bits above */
  uint32_t axis;          /* 0 = query, 1 = target */
  uint32_t window;        /* W >= 1 */
  uint32_t other_genome;  /* a genome id or SWG_WINDOWS_ANY */
  const uint32_t* weight; /* [n] or NULL = rec->matches; host / device as the columns */
  uint64_t n_rows;        /* out (rows bit) */
  uint64_t capacity;      /* in: entries `rows` can hold */
  swg_window_row* rows;   /* in: caller-owned [capacity] or NULL; written only when n_rows <= capacity */
  uint64_t n_seqs;        /* out (summary bit) */
  uint64_t seq_capacity;  /* in: entries `seqs` can hold */
  swg_window_seq* seqs;   /* in: caller-owned [seq_capacity] or NULL; written only when n_seqs <= seq_capacity */
  uint64_t reserved;      /* 0 */
} swg_windows_request; /* 80 bytes, no implicit padding */
/* rec: host pointers; seq_len[rec->n_seq], seq_genome[rec->n_seq], status[n] (or NULL) and req->weight on the host. */
int swg_windows_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                        const uint8_t* status, swg_windows_request* req);
/* The same with the columns of rec, seq_len, seq_genome, status and req->weight in device memory of ctx's GPU (as
 * swg_filter_device leaves them: no copy in between); the request and its arrays stay on the host. */
int swg_windows_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                               const uint8_t* status, swg_windows_request* req);
/* Both texts of an open PAF from ONE device call (release each with swg_free) under its last-'#' genome map and the last-seen
 * lengths of swg_paf_components, m = column 10; a text is asked for by a non-NULL out_text[k] on entry, as in swg_paf_place.
 * Tab-separated, integers only:
 *   text 0  header `#sequence start end n_all depth_all covered_all matches_all n_kept depth_kept covered_kept matches_kept`, then
 *           one line per row (the first three columns make it a BED / bedGraph source).
 *   text 1  header `#sequence length windows empty_all empty_kept covered_all covered_kept depth_all depth_kept matches_all
 *           matches_kept records_all records_kept`, one line per listed sequence.
 * other_genome: a genome name as the other reports print it, with or without its trailing '#'; NULL = any.  An unknown name is
 * SWG_ERR_INVALID with the name in the message.  A PAF without records gives the header-only texts and needs no device (ctx may
 * be NULL then).  axis > 1, window == 0: SWG_ERR_INVALID; a handle with rebased columns: SWG_ERR_UNSUPPORTED.  Errors:
 * swg_alnstats_last_error(). */
int swg_paf_windows(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t axis, uint32_t window, const char* other_genome,
                    char** out_text, uint64_t* out_len);

/* ---- divergence: exact matches, mismatches and indels per fixed window, from the CIGARs (no reference counterpart; DESIGN.md
 * section 33) ----
 * The windows, the axis and who takes part are those of the windows above; the CIGAR set, the walk offsets x / y, the entry states
 * and USABLE (state 0, record in `set`: SWG_IV_ALL, or SWG_IV_KEPT: status != 0) are those of the differences.  One set per call.
 *   takes part  a record of the set with seq_genome[s] != seq_genome[o], a < b and other_genome == SWG_WINDOWS_ANY or
 *               seq_genome[o] == other_genome.  One that ends beyond its sequence is an error that names the smallest such record.
 *   listed      a sequence that carries a record that takes part, WHETHER OR NOT the record has an entry in the CIGAR set: the
 *               window table does not depend on which records a call's CIGAR set carries.
 *   coordinate  of an aligned column or of a base facing a gap: t_start + y on axis 1; on axis 0 q_start + x on '+' and
 *               q_end - 1 - x on '-'.
 * Per window, over the usable entries whose records take part (ov = the overlap of [a, b) with the window):
 *   n              the entries with ov > 0
 *   aligned        the columns of =, X and M ops whose axis coordinate is in the window
 *   matches        those of = ops;  mismatches  those of X ops;  m_columns  those of M ops (aligned is the sum of the three)
 *   unaligned      axis bases in the window that the entry consumes against a gap (D / N on axis 1, I on axis 0); aligned +
 *                  unaligned = the sum of ov
 *   inserted       bases of the OTHER sequence inserted at a point p of this axis (I on axis 1, D / N on axis 0): p = t_start + y
 *                  on axis 1, q_start + x on axis 0 '+', q_end - x on axis 0 '-'; the op belongs with all its bases to the window
 *                  of base min(p, b - 1)
 *   mismatch_runs  X ops of length > 0 whose lowest axis base is in the window
 *   indels         I, D and N ops of length > 0: one with axis extent in the window of its lowest axis base, one without in the
 *                  window of `inserted`
 * S, H, P and ops of length 0 add nothing.  Column identity is matches / aligned, gap-compressed identity matches / (aligned +
 * indels), BLAST identity matches / (aligned + unaligned + inserted): the caller divides.
 * Rows: one per window of every listed sequence, (seq, window) ascending, empty windows included.  Summary: one entry per listed
 * sequence, ascending: windows, records (of the set that take part on it), entries (the usable ones among them) and the eight sums
 * over its windows.  Nothing depends on the order of the records or on a launch shape.
 * `want` and the capacity protocol are those of swg_windows_records; state whenever non-NULL; ops, cigar_bad and usable (usable
 * entries whose records take part) whenever the call succeeds.  Refusals: those of swg_windows_records (window == 0, axis > 1, a bad
 * other_genome, want, reserved, NULL columns, bad ids, the record beyond its sequence) and of the set as in swg_lift_exact_records,
 * set > 1, SWG_IV_KEPT without status: SWG_ERR_INVALID; n, k or ops >= 2^31, 2^32 text bytes, 2^31 windows or more (refused before
 * anything of that size is allocated): SWG_ERR_RANGE.  n == 0 needs no device work.  Scratch from the arena (SWG_ERR_OOM under a
 * limit that does not hold it): the build's (see swg_lift_exact_records) plus 1 byte per op, 16 per entry, 17 per sequence, 104 per
 * window plus 80 for its row, 88 per listed sequence; the host seam stages 26 bytes per record and 8 per sequence. */
typedef struct swg_divergence_row {
  uint32_t seq, start, end; /* the window, half-open, clipped to seq_len */
  uint32_t n;
  uint64_t aligned, matches, mismatches, m_columns, unaligned, inserted, mismatch_runs, indels;
} swg_divergence_row; /* 80 bytes, no implicit padding */
typedef struct swg_divergence_seq {
  uint32_t seq, windows;
  uint64_t records, entries;
  uint64_t aligned, matches, mismatches, m_columns, unaligned, inserted, mismatch_runs, indels;
} swg_divergence_seq; /* 88 bytes, no implicit padding */
#define SWG_DIVERGENCE_ROWS 1u
#define SWG_DIVERGENCE_SUMMARY 2u
typedef struct swg_divergence_request {
  uint32_t set;             /* in: SWG_IV_ALL or SWG_IV_KEPT */
  uint32_t axis;            /* 0 = query, 1 = target */
  uint32_t window;          /* W >= 1 */
  uint32_t other_genome;    /* a genome id or SWG_WINDOWS_ANY */
  uint32_t want;            /* the two bits above */
  uint32_t reserved;        /* 0 */
  uint64_t capacity;        /* in: entries `rows` can hold */
  swg_divergence_row* rows; /* in: caller-owned [capacity] or NULL; written only when n_rows <= capacity */
  uint64_t seq_capacity;
  swg_divergence_seq* seqs; /* written only when n_seqs <= seq_capacity */
  uint8_t* state;           /* in: caller-owned [k] or NULL; written whenever non-NULL */
  uint64_t n_rows;          /* out (rows bit) */
  uint64_t n_seqs;          /* out (summary bit) */
  uint64_t ops;             /* out: ops parsed over the whole set */
  uint64_t cigar_bad;       /* out: entries with a state bit of 1 .. 8 */
  uint64_t usable;          /* out: usable entries whose records take part */
} swg_divergence_request; /* 104 bytes, no implicit padding */
/* Everything on the host.  seq_len, seq_genome: [rec->n_seq]. */
int swg_divergence_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                           const uint8_t* status, const swg_cigar_set* cigars, swg_divergence_request* req);
/* Columns, strand, seq_len, seq_genome, status and the three arrays of the set in device memory of ctx's GPU; the set structure, the
 * request and its arrays on the host. */
int swg_divergence_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                                  const uint8_t* status, const swg_cigar_set* cigars, swg_divergence_request* req);
typedef struct swg_divergence_counts {
  uint64_t records;  /* records of the set */
  uint64_t usable;   /* usable entries whose records take part */
  uint64_t bad;      /* entries with a state bit of 1 .. 8 */
  uint64_t untagged; /* records of the set without a cg:Z: tag */
  uint64_t windows;  /* rows */
  uint64_t seqs;     /* listed sequences */
  uint64_t batches;  /* device calls */
} swg_divergence_counts; /* 56 bytes */
/* Both texts of an open PAF (release each with swg_free; a text is asked for by a non-NULL out_text[k] on entry, as in
 * swg_paf_windows): the records of `set` with the LAST cg:Z: tag of each one's line as its entry, in batches as
 * swg_paf_ucsc_chain_write cuts them, one device call per batch over ALL records and that batch's CIGAR set, the rows and summaries
 * added up across the batches; both texts are the same bytes for every batch_bytes.  Genome map, names and lengths as in
 * swg_paf_windows.  Tab-separated, integers only:
 *   text 0  header `#sequence start end n aligned matches mismatches m_columns unaligned inserted mismatch_runs indels`, one line
 *           per row (the first three columns are a BED source)
 *   text 1  header `#sequence length windows records entries aligned matches mismatches m_columns unaligned inserted mismatch_runs
 *           indels`, one line per listed sequence
 * A PAF without records of the set gives the header-only texts and needs no device (ctx may be NULL then).  set > 1, SWG_IV_KEPT
 * without status, axis > 1, window == 0, an unknown genome name: SWG_ERR_INVALID; a handle with rebased columns:
 * SWG_ERR_UNSUPPORTED.  counts may be NULL.  Errors: swg_alnstats_last_error(). */
int swg_paf_divergence(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t axis, uint32_t window,
                       const char* other_genome, uint64_t batch_bytes, char** out_text, uint64_t* out_len, swg_divergence_counts* counts);

/* ---- variants: SNVs, insertions and deletions with their bases, from the CIGARs and the sequences (no reference counterpart;
 * DESIGN.md section 34) ----
 * The CIGAR set, the walk offsets x / y and the entry states are those of the base-exact lift; kinds and the query interval on '-'
 * are those of the differences.  Integers and bytes only.
 * SEQUENCES: n_seq (= rec->n_seq), offset[n_seq + 1] and bases (as read).  Sequence s is PRESENT when offset[s + 1] > offset[s]; the
 * difference is its length.  norm(b): A, C, G, T for those letters in either case, N for every other byte; comp swaps A/T and C/G
 * and keeps N.
 * An entry is USABLE when its state is 0, its record is in `set`, the target's genome is t_genome or t_genome is SWG_VARIANTS_ANY
 * (likewise q_genome), both sequences are present, and t_end <= len(t), q_end <= len(q).  One that fails the presence test (and no
 * earlier one) counts as no_sequence, one that fails the bounds test (and no earlier one) as out_of_sequence.
 * QUERY COLUMN at walk offset x: norm(Q[q_start + x]) on '+', comp(norm(Q[q_end - 1 - x])) on '-'.
 * Per op of a usable entry with length l > 0, p = t_start + y:
 *   X, M  column by column, b in 0 .. l - 1: r = norm(T[p + b]), a = the query column at x + b.  r or a is N: n_columns.  r == a:
 *         `same` under X, m_equal under M.  Else an SNV: pos = p + b, REF r, ALT a, q_pos = the column's forward-strand query
 *         coordinate, sub[r][a] + 1.  Runs are split per base: there are no MNPs.
 *   I     ins = the l query columns from x on (text order: reverse-complemented on '-').  p > 0: pos = p - 1, REF T[p - 1], ALT
 *         T[p - 1] + ins.  p == 0: pos = 0, REF T[0], ALT ins + T[0] (the VCF rule at a contig's first base).
 *   D     p > 0: pos = p - 1, REF T[p - 1 .. p + l), ALT T[p - 1].  p == 0 and l < len(t): pos = 0, REF T[0 .. l] (l + 1 bases), ALT
 *         T[l].  p == 0 and l == len(t): UNANCHORED, counted, no variant.
 *   An I or D that is not unanchored with l > max_indel (max_indel != 0) counts as long_indels and gives no variant.  Allele bytes go
 *   through norm; N may stand in an indel allele.  N, =, S, H, P and ops of length 0 give nothing.
 * A VARIANT is 32 bytes; q_pos of an indel is the start of the op's query interval; its ref_len + alt_len allele bytes lie in the
 * POOL at allele_offset, REF first.  Variants come in (entry, op, column) order; the pool offsets are the exclusive sum of ref_len +
 * alt_len in that order.
 * SUMMARY per ordered genome pair over the usable entries; only long_indels depends on max_indel.  compared = snvs + same + m_equal
 * + n_columns (the columns under X and M), snvs = the sum of sub; n_ins .. del_bases count every I / D of length > 0.  Pairs ascend
 * by (q_genome, t_genome).
 * Capacity protocol: variants AND pool are written only when n_variants <= variant_capacity, pool_bytes <= pool_capacity and both
 * arrays are non-NULL (else they are counted and not built); pairs when n_pairs <= pair_capacity; the counts whenever the call
 * succeeds.  Refusals: those of swg_diff_records (the set, SWG_IV_KEPT without status, a NULL seq_genome or column, bad ids,
 * reserved != 0); a NULL seqs, offset or bases, or seqs->n_seq != rec->n_seq, with k > 0; offsets that descend; t_genome or q_genome
 * >= n_genome and not SWG_VARIANTS_ANY: SWG_ERR_INVALID.  2^32 text bytes, 2^32 candidates (the columns under X and M plus one per
 * indel with a variant: no range loop is built), 2^31 variants or 2^32 pool bytes or more: SWG_ERR_RANGE.  k == 0 needs no device.
 * Scratch from the arena: the build's plus, per op, 1 + 16 bytes (kind, candidates and their scan); per entry 8; per candidate 1
 * (its flag); per variant 4 + 8, and 32 plus its allele bytes when variants and pool are built; the genome-pair table (176 bytes
 * per slot, 184 per listed pair); the host seam stages 26 bytes per record, 12 per sequence and every base. */
#define SWG_VARIANTS_ANY 0xffffffffu
#define SWG_VARIANT_SNP 1u
#define SWG_VARIANT_INS 2u
#define SWG_VARIANT_DEL 4u
#define SWG_VARIANT_MINUS 256u /* swg_variant.kind_flags bit 8: the record is on the '-' strand; bits 0 .. 7: the kind */
typedef struct swg_seq_set {
  const uint64_t* offset; /* [n_seq + 1], non-decreasing: sequence s is bases[offset[s] .. offset[s + 1]) */
  const uint8_t* bases;   /* offset[n_seq] bytes, as read */
  uint32_t n_seq;         /* = rec->n_seq */
  uint32_t reserved;      /* 0 */
} swg_seq_set; /* 24 bytes */
typedef struct swg_variant {
  uint32_t record, kind_flags;
  uint32_t pos;              /* 0-based on the target */
  uint32_t ref_len, alt_len;
  uint32_t q_pos;            /* 0-based on the query's forward strand */
  uint64_t allele_offset;    /* into the pool: ref_len bytes of REF, then alt_len of ALT */
} swg_variant; /* 32 bytes, no implicit padding */
typedef struct swg_variant_pair {
  uint32_t q_genome, t_genome;
  uint64_t entries, compared, snvs;
  uint64_t sub[12];          /* REF>ALT: A>C A>G A>T C>A C>G C>T G>A G>C G>T T>A T>C T>G */
  uint64_t same, m_equal, n_columns;
  uint64_t n_ins, ins_bases, n_del, del_bases;
  uint64_t long_indels, unanchored;
} swg_variant_pair; /* 200 bytes, no implicit padding */
typedef struct swg_variant_request {
  uint32_t set;                /* in: SWG_IV_ALL or SWG_IV_KEPT */
  uint32_t t_genome, q_genome; /* in: a genome id or SWG_VARIANTS_ANY */
  uint32_t max_indel;          /* in: 0 = no limit */
  uint64_t reserved;           /* in: 0 */
  uint64_t variant_capacity;   /* in: entries `variants` can hold */
  swg_variant* variants;       /* in: caller-owned or NULL */
  uint64_t pool_capacity;      /* in: bytes `pool` can hold */
  uint8_t* pool;               /* in: caller-owned or NULL */
  uint64_t pair_capacity;
  swg_variant_pair* pairs;     /* written only when n_pairs <= pair_capacity */
  uint64_t n_variants;         /* out */
  uint64_t pool_bytes;         /* out */
  uint64_t n_pairs;            /* out */
  uint64_t ops;                /* out: ops parsed over the whole set */
  uint64_t cigar_bad;          /* out: entries with a state bit of 1 .. 8 */
  uint64_t usable;             /* out: usable entries */
  uint64_t no_sequence;        /* out */
  uint64_t out_of_sequence;    /* out */
  uint64_t columns;            /* out: columns compared (the sum of `compared`) */
} swg_variant_request; /* 144 bytes, no implicit padding */
/* Everything on the host.  seq_genome: [rec->n_seq]. */
int swg_variant_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                        const swg_cigar_set* cigars, const swg_seq_set* seqs, swg_variant_request* req);
/* Columns, strand, seq_genome, status, the three arrays of the set, seqs->offset and seqs->bases in device memory of ctx's GPU; the
 * two set structures, the request and its arrays on the host. */
int swg_variant_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                               const swg_cigar_set* cigars, const swg_seq_set* seqs, swg_variant_request* req);

/* ---- ANI pre-pass for "aniN" identity thresholds (src/main.rs:296-688, src/cli.rs:76-130) -------------------
 * calculate_ani_stats: median over genome pairs (last-'#' prefixes, unordered) of Σmatches / Σblock_len, over
 *   SWG_ANI_ALL         every inter-genome line                                   main.rs:339-342, 392-498
 *   SWG_ANI_ORTHOGONAL  the survivors of a fixed 1:1 / >= 1 kb / matches-scored filter   main.rs:343-382
 *   SWG_ANI_NPERCENTILE lines taken in descending length / identity / identity*max(ln len,1) order (stable)
 *                       until their block lengths cover `percentile` % of the total sequence size   main.rs:500-688
 * Host threads parse the ANI view of each line (f64 matches/block length, first valid dv:f:, sequence lengths);
 * the GPU does the key sort, the prefix cut and the per-pair sums (each pair summed in reference order, so the
 * f64 sums are bit-identical); the 1:1 filter of ORTHOGONAL is swg_filter.  The reference panics on NaN keys
 * (partial_cmp().unwrap()); here that is SWG_ERR_INVALID.  Non-integral block lengths: SWG_ERR_UNSUPPORTED. */
enum { SWG_ANI_ALL = 0, SWG_ANI_ORTHOGONAL = 1, SWG_ANI_NPERCENTILE = 2 };
enum { SWG_NSORT_LENGTH = 0, SWG_NSORT_IDENTITY = 1, SWG_NSORT_SCORE = 2 };
typedef struct swg_ani_input {
  uint64_t n;               /* records of the swg_paf handle */
  const uint8_t* eligible;  /* [n] line takes part (not '#'-led, genomes differ)         main.rs:406-432 */
  const uint32_t* pair;     /* [n] unordered genome-pair id < n_pairs */
  uint64_t n_pairs;
  const double* matches;    /* [n] final_matches: column 10, or (1-dv)*block_len          main.rs:435-446 */
  const double* block_len;  /* [n] column 11 as f64 (default 1.0) */
  double total_genome_size; /* Σ first-seen length of every sequence on an eligible line  main.rs:560-572, 626 */
} swg_ani_input;
/* parse_ani_method (main.rs:296-330): returns 1 and fills the outputs, 0 for None */
int swg_parse_ani_method(const char* s, int* kind, double* percentile, int* sort);
/* parse_identity_value (cli.rs:76-130): ani_percentile < 0 means None.  Returns SWG_OK or SWG_ERR_INVALID. */
int swg_parse_identity_value(const char* s, double ani_percentile, double* out);
/* host side: the ANI view of the records (arrays owned by the handle, valid until swg_paf_close) */
int swg_paf_ani_input(swg_paf* p, int threads, swg_ani_input* out);
/* device side: median per-pair ANI.  `select` (optional, [n]) further restricts the lines (ORTHOGONAL survivors);
 * kind ALL/ORTHOGONAL = file order, no cut.  0.0 when no line takes part (main.rs:448-451, 604-607). */
int swg_ani_median(swg_ctx* ctx, const swg_ani_input* in, const uint8_t* select, int kind, double percentile, int sort,
                   double* ani50);
/* calculate_ani_stats over an open PAF (runs the ORTHOGONAL filter itself) */
int swg_paf_ani_stats(swg_ctx* ctx, swg_paf* p, int kind, double percentile, int sort, int threads, double* ani50);

/* ---- --joblist: haplotype pairs to align, chosen from MinHash sketches (src/mash.rs, src/knn_graph.rs, src/pansn.rs,
 * src/joblist.rs, src/main.rs:791-990, 2711-2745) --------------------------------------------------------------------
 * FASTA (host): records of every file in order; name = first whitespace token after '>'; sequence = its lines trimmed and
 *   concatenated; lines before a file's first header are prepended to that file's first record (main.rs:963-990).
 *   .gz / .bgz through the BGZF reader.  Errors: text in swg_fasta_last_error(). */
typedef struct swg_fasta swg_fasta;
int swg_fasta_open(const char* const* paths, int n_paths, int threads, swg_fasta** out);
void swg_fasta_close(swg_fasta* f);
uint64_t swg_fasta_num_records(const swg_fasta* f);
const char* swg_fasta_name(const swg_fasta* f, uint64_t i);   /* owned by the handle */
int swg_fasta_file_index(const swg_fasta* f, uint64_t i);      /* which of the paths record i came from */
const uint64_t* swg_fasta_offsets(const swg_fasta* f);         /* [n + 1]: record i = bases[offsets[i], offsets[i + 1]) */
const uint8_t* swg_fasta_bases(const swg_fasta* f);            /* every record's bytes, as read (case kept) */
const char* swg_fasta_last_error(void);

/* ---- --vcf: the variant calls of an open PAF against FASTA records, as VCF 4.2 ----
 * The handle's sequence names are matched to swg_fasta_name by exact name (of two FASTA records with one name the first); a PAF
 * sequence without a FASTA record is absent, and so is one whose PAF length (on the line that mentions it last) differs from the
 * FASTA record's: that one counts as length_mismatch, once per sequence.  The records of `set` with the LAST cg:Z: tag of each
 * one's line as its entry go through swg_variant_records' definitions in batches as swg_paf_ucsc_chain_write cuts them; the bases
 * of the sequences the set names are sent to the device once per call.  Genomes: the handle's seq_genome_two; ref_genome /
 * query_genome: a two-part genome prefix with or without its trailing '#', or NULL = any.
 *   VCF      ##fileformat=VCFv4.2, ##source=sweepga-gpu (no date line), one ##contig=<ID=,length=> per sequence that is the target
 *            of a usable entry, in sequence-id order, the INFO lines, then CHROM POS(= pos + 1) . REF ALT . . QNAME=;QSTART=;
 *            QSTRAND=+|-;REC= per variant; ';', '=', ',', '%' and bytes <= 0x20 of QNAME are percent-encoded.  With a query_genome
 *            also ##FORMAT=<ID=GT,...>, one sample column named as that genome, and GT 1 on every line.  The lines are ordered by
 *            (target sequence id, pos) with one stable device sort, ties in (record, op, column) order: sorted per contig, and the
 *            same bytes for every batch_bytes.
 *   summary  a header, then per genome pair, (query genome, target genome) ascending, the sums of swg_variant_pair and ts, tv
 * A PAF without records of the set gives empty outputs and needs no device (ctx may be NULL).  Every refusal comes before a file
 * is opened: set > 1, SWG_IV_KEPT without status, reserved != 0, a NULL fasta or opts, an unknown genome name: SWG_ERR_INVALID; a
 * handle whose columns are rebased: SWG_ERR_UNSUPPORTED.  counts may be NULL.  Errors: swg_alnstats_last_error(). */
typedef struct swg_vcf_options {
  uint32_t set;             /* SWG_IV_ALL or SWG_IV_KEPT */
  uint32_t max_indel;       /* 0 = no limit */
  const char* ref_genome;   /* the target's genome, or NULL = any */
  const char* query_genome; /* the query's genome, or NULL = any */
  uint64_t batch_bytes;     /* CIGAR text per device call; 0 = a default from the device's memory */
  uint64_t reserved;        /* 0 */
} swg_vcf_options; /* 40 bytes */
typedef struct swg_vcf_counts {
  uint64_t records;  /* records of the set */
  uint64_t usable;   /* usable entries */
  uint64_t bad;      /* entries with a state bit of 1 .. 8 */
  uint64_t untagged; /* records without a cg:Z: tag */
  uint64_t variants;
  uint64_t snvs, n_ins, n_del; /* over the usable entries, as the summary */
  uint64_t same, n_columns, m_equal;
  uint64_t long_indels, unanchored;
  uint64_t no_sequence, out_of_sequence; /* entries */
  uint64_t length_mismatch;              /* sequences */
  uint64_t batches;                      /* device calls */
} swg_vcf_counts; /* 136 bytes */
/* Either path may be NULL (not both); without vcf_path the variants are counted and not built. */
int swg_paf_vcf_write(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_vcf_options* opts,
                      const char* vcf_path, const char* summary_path, swg_vcf_counts* counts);
/* The same as malloc'd texts (release each with swg_free); vcf_text or summary_text may be NULL (not both). */
int swg_paf_vcf_text(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_vcf_options* opts,
                     swg_vcf_counts* counts, char** vcf_text, uint64_t* vcf_len, char** summary_text, uint64_t* summary_len);

/* ---- resolved CIGARs: every entry rewritten in canonical =/X form against the sequences (no reference counterpart; DESIGN.md
 * section 36) ----
 * The CIGAR set, the walk offsets x / y and the entry states are those of the base-exact lift; norm, comp, the query column at walk
 * offset x, sequence presence and the bounds test are those of the variants above.  Integers and bytes only.
 * An entry is USABLE when its state is 0, its record is in `set`, both sequences are present, and t_end <= len(t), q_end <= len(q).
 * The first failing test counts: cigar_bad (a state bit of 1 .. 8), empty (state 16), no_sequence, out_of_sequence; an entry
 * outside the set counts nowhere.  There are no genome filters.
 * A COLUMN OP is an M, = or X op.  A COLUMN RUN is a maximal sequence of consecutive column ops in the entry's text; column ops of
 * length 0 belong to it, any other op ends it, one of length 0 included.
 * A column at target index p = t_start + y and walk offset x, r = norm(T[p]), a = the query column: eq = (r == a and r != N).  A
 * column with an N on either side is never equal.
 * OUTPUT TEXT of a usable entry, in text order: a column run of L > 0 columns becomes its maximal stretches of constant eq, each
 * written `<length>=` or `<length>X` in decimal without leading zeros; a run with L = 0 becomes nothing; every other op is copied
 * byte for byte, digits and letter (leading zeros and zero lengths stay).  The output, taken as an entry of the same record, has
 * state 0 and the same advances; it holds no M, and inside a run no two neighbouring ops carry the same letter.
 * One swg_eqx_entry per entry of the set, in set order (no compaction); an entry that is not usable has only `record` set.  The
 * texts of the usable entries lie end to end, without separators, in set order; text_first runs over them.
 * Capacity protocol of swg_ucsc_chain_records: entries is written when k <= entry_capacity, text when text_bytes <= text_capacity
 * (each only when non-NULL; without a text pointer the text is counted and not built); the counts whenever the call succeeds.
 * Refusals: those of swg_variant_records for the set, the columns, the sequences and the offsets (SWG_ERR_INVALID); 2^32 bytes of
 * CIGAR text, 2^32 columns, 2^32 output ops or 2^32 output bytes or more in one call: SWG_ERR_RANGE (no range loop is built).
 * k == 0 needs no device.  Scratch from the arena: the build's plus, per op, 1 + 4 + 1 + 16 bytes (kind, letter position, class,
 * the scans of columns and verbatim ops); per entry 1 + 64; per column 1 (boundary flag and letter); per output op 4 + 8 + 8 (its
 * column, the item, the scanned length); the text; the host seam stages 26 bytes per record, 8 per sequence and every base. */
#define SWG_EQX_USABLE 1u  /* swg_eqx_entry.flags bit 0 */
#define SWG_EQX_CHANGED 2u /* bit 1: the output bytes differ from the input bytes */
#define SWG_EQX_COLUMN_TILE 4096u /* columns per work-group of the column pass */
#define SWG_EQX_TEXT_TILE 4096u   /* output bytes per work-group of the text kernel */
typedef struct swg_eqx_entry {
  uint32_t record, flags;
  uint32_t text_len, out_ops;
  uint32_t matches, mismatches; /* columns with eq, the other columns */
  uint32_t n_columns;           /* columns with an N: a subset of mismatches */
  uint32_t eq_wrong, x_wrong;   /* columns under = with eq false, under X with eq true */
  uint32_t m_columns;           /* columns under M */
  uint32_t inserted, deleted;   /* bases under I, under D (N ops count in neither) */
  uint64_t block;               /* matches + mismatches + inserted + deleted */
  uint64_t text_first;          /* into text */
} swg_eqx_entry; /* 64 bytes, no implicit padding */
typedef struct swg_eqx_request {
  uint32_t set;            /* in: SWG_IV_ALL or SWG_IV_KEPT */
  uint32_t reserved;       /* in: 0 */
  uint64_t entry_capacity; /* in: entries `entries` can hold */
  swg_eqx_entry* entries;  /* in: caller-owned or NULL; written only when k <= entry_capacity */
  uint64_t text_capacity;
  char* text;              /* written only when text_bytes <= text_capacity */
  uint64_t ops;            /* out: ops parsed over the whole set */
  uint64_t cigar_bad;      /* out: entries with a state bit of 1 .. 8 */
  uint64_t empty;          /* out: entries of state 16 */
  uint64_t usable, no_sequence, out_of_sequence;
  uint64_t columns;        /* out: matches + mismatches */
  uint64_t out_ops, text_bytes;
  uint64_t changed;        /* out: usable entries with SWG_EQX_CHANGED */
  uint64_t matches, mismatches, n_columns, eq_wrong, x_wrong, m_columns; /* out: over the usable entries */
} swg_eqx_request; /* 168 bytes, no implicit padding */
/* Everything on the host. */
int swg_eqx_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                    swg_eqx_request* req);
/* Columns, strand, status, the three arrays of the set, seqs->offset and seqs->bases in device memory of ctx's GPU; the two set
 * structures, the request and its arrays on the host. */
int swg_eqx_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                           swg_eqx_request* req);
/* --eqx: the records of `set` of an open PAF, in record order, each usable one's line byte for byte but for column 10 (= matches),
 * column 11 (= block) and the value of its LAST cg:Z: tag (= the output text).  Other tags (NM:i, de:f, gi:f, ...) are copied and
 * may be stale.  A record that is not usable (no tag, a bad or empty entry, a sequence that is missing or of another length, out of
 * bounds) is copied unchanged under SWG_EQX_KEEP and left out under SWG_EQX_DROP.  Sequence names are matched to the FASTA records
 * as swg_paf_vcf_write does it (length_mismatch included); the bases go to the device once per call; batches come from
 * swg_paf_ucsc_chain_write's planner over the cost text length + min(q_end - q_start, t_end - t_start), which bounds an entry's
 * columns and, at 2 bytes per column plus the input text, its output: one device pass per batch with that bound as the text
 * capacity.  The file is the same bytes for every batch_bytes.  A set without records gives an empty file and needs no device (ctx
 * may be NULL).  Refusals, all before a file is opened: set > 1, unresolved > 1, reserved != 0, SWG_IV_KEPT without status, a NULL
 * fasta or opts: SWG_ERR_INVALID; a handle whose columns are rebased: SWG_ERR_UNSUPPORTED.  counts may be NULL.  Errors:
 * swg_alnstats_last_error(). */
#define SWG_EQX_KEEP 0u
#define SWG_EQX_DROP 1u
typedef struct swg_eqx_options {
  uint32_t set;         /* SWG_IV_ALL or SWG_IV_KEPT */
  uint32_t unresolved;  /* SWG_EQX_KEEP or SWG_EQX_DROP */
  uint64_t batch_bytes; /* cost per device call; 0 = a default from the device's memory */
  uint64_t reserved;    /* 0 */
} swg_eqx_options; /* 24 bytes */
typedef struct swg_eqx_counts {
  uint64_t records;  /* records of the set */
  uint64_t usable;   /* lines rewritten */
  uint64_t bad;      /* entries with a state bit of 1 .. 8 */
  uint64_t untagged; /* records without a cg:Z: tag */
  uint64_t no_sequence, out_of_sequence; /* entries */
  uint64_t length_mismatch;              /* sequences */
  uint64_t changed;  /* usable entries whose text changed */
  uint64_t lines;    /* lines written */
  uint64_t columns, matches, mismatches, eq_wrong, x_wrong, m_columns;
  uint64_t batches;  /* device calls */
} swg_eqx_counts; /* 128 bytes */
int swg_paf_eqx_write(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_eqx_options* opts,
                      const char* out_path, swg_eqx_counts* counts);
/* The same as one malloc'd text (release with swg_free). */
int swg_paf_eqx_text(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_eqx_options* opts,
                     swg_eqx_counts* counts, char** text, uint64_t* len);

/* ---- alignment blocks with their gapped bases: the two rows of every block, as MAF reads them (no reference counterpart;
 * DESIGN.md section 37) ----
 * The CIGAR set, the walk offsets x / y and the entry states are those of the base-exact lift; sequence presence and the bounds
 * test are those of the variants; USABLE is that of the resolved CIGARs above, and the first failing test counts as there:
 * cigar_bad, empty, no_sequence, out_of_sequence.  Integers and bytes only.
 * ALIGNMENT COLUMNS: an op of length l gives l columns under M, =, X, I, D or N and none under S, H, P.  The target row of a column
 * holds the target byte under M = X D N and '-' under I; the query row holds the query byte under M = X I and '-' under D and N.
 * BYTES are copied as read (case and IUPAC codes kept, no norm): the target byte is T[t_start + y]; the query byte at walk offset x
 * is Q[q_start + x] on '+' and comp_raw(Q[q_end - 1 - x]) on '-'.  comp_raw swaps A-T, C-G, R-Y, K-M, B-V, D-H, maps U to A, the
 * same in lower case, and leaves every other byte (S, W, N, '-', '*', ...) unchanged: the table SWG_MAF_COMP_RAW below.
 * BREAKERS AND BLOCKS: with split_gap = g > 0 an I, D or N op with l >= g is a BREAKER; with g = 0 there is none.  The breakers
 * taken out of a usable entry, every maximal run of the remaining consecutive ops is a CANDIDATE; one with an aligned column (an M,
 * = or X op of length > 0) is a BLOCK, the others count as gap_only.  Zero-length ops, S, H and P belong to the run they stand in
 * and give no columns.  A block keeps its leading and trailing gap columns (no trimming).  Bases under breakers appear in no block
 * and are summed in skipped_t / skipped_q.  The bases of a gap_only candidate (an I op shorter than g between two breakers, as in
 * 3D1I3D with g = 3) appear in no block and in NEITHER skipped sum: per entry, the blocks' bases plus skipped_* equal the record's
 * lengths only when gap_only counts none of its candidates.
 * BLOCK FIELDS, with x0, y0 the walk offsets at the block's first op, q_bases / t_bases its advances, aligned its aligned columns:
 * columns = q_bases + t_bases - aligned; the target interval is [t_start + y0, + t_bases); the query interval on the forward strand
 * is [q_start + x0, + q_bases) on '+' and [q_end - x0 - q_bases, + q_bases) on '-'.  op_first / op_end count from the entry's first
 * op.  One swg_maf_block per block, in (entry, op) order.
 * TEXT: per block the target row (columns bytes), then the query row (columns bytes); the blocks lie end to end in block order,
 * without separators; text_first runs over them in 64 bits.
 * Capacity protocol of swg_eqx_records: blocks is written when n_blocks <= block_capacity, text when text_bytes <= text_capacity
 * (each only when non-NULL; without a text pointer the text kernel does not run); the counts whenever the call succeeds.
 * Refusals: those of swg_eqx_records for the set, the columns, the sequences and the offsets (SWG_ERR_INVALID); 2^32 bytes of CIGAR
 * text or 2^32 alignment columns (of all candidates) or more in one call: SWG_ERR_RANGE (no range loop is built).  k == 0 needs no
 * device.  Scratch from the arena: the build's plus, per op, 8 + 8 + 1 bytes (the scans of columns and breakers, the start flag);
 * per entry 1; per candidate 4 + 64 + 40 + 1; per block 4 + 64 + 40 + 8; the text; the host seam stages as swg_eqx_records. */
#define SWG_MAF_MINUS 1u       /* swg_maf_block.flags bit 0: the record's strand is '-' */
#define SWG_MAF_TEXT_TILE 4096u /* output bytes per work-group of the text kernel */
#define SWG_MAF_COMP_RAW                                                                                                            \
  {0,   1,   2,   3,   4,   5,   6,   7,   8,   9,   10,  11,  12,  13,  14,  15,  16,  17,  18,  19,  20,  21,  22,  23,  24,  25,   \
   26,  27,  28,  29,  30,  31,  32,  33,  34,  35,  36,  37,  38,  39,  40,  41,  42,  43,  44,  45,  46,  47,  48,  49,  50,  51,   \
   52,  53,  54,  55,  56,  57,  58,  59,  60,  61,  62,  63,  64,  'T', 'V', 'G', 'H', 69,  70,  'C', 'D', 73,  74,  'M', 76,  'K',  \
   78,  79,  80,  81,  'Y', 83,  'A', 'A', 'B', 87,  88,  'R', 90,  91,  92,  93,  94,  95,  96,  't', 'v', 'g', 'h', 101, 102, 'c',  \
   'd', 105, 106, 'm', 108, 'k', 110, 111, 112, 113, 'y', 115, 'a', 'a', 'b', 119, 120, 'r', 122, 123, 124, 125, 126, 127, 128, 129,  \
   130, 131, 132, 133, 134, 135, 136, 137, 138, 139, 140, 141, 142, 143, 144, 145, 146, 147, 148, 149, 150, 151, 152, 153, 154, 155,  \
   156, 157, 158, 159, 160, 161, 162, 163, 164, 165, 166, 167, 168, 169, 170, 171, 172, 173, 174, 175, 176, 177, 178, 179, 180, 181,  \
   182, 183, 184, 185, 186, 187, 188, 189, 190, 191, 192, 193, 194, 195, 196, 197, 198, 199, 200, 201, 202, 203, 204, 205, 206, 207,  \
   208, 209, 210, 211, 212, 213, 214, 215, 216, 217, 218, 219, 220, 221, 222, 223, 224, 225, 226, 227, 228, 229, 230, 231, 232, 233,  \
   234, 235, 236, 237, 238, 239, 240, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250, 251, 252, 253, 254, 255}
typedef struct swg_maf_block {
  uint32_t record, entry;     /* the record, and its entry's place in the set */
  uint32_t op_first, op_end;  /* the block's ops, counted from the entry's first op */
  uint32_t t_start, t_bases;
  uint32_t q_start, q_bases;  /* on the forward strand */
  uint32_t aligned, columns;
  uint32_t flags, walk_x;     /* SWG_MAF_MINUS; x0 */
  uint64_t text_first;        /* into text: the target row, then the query row */
  uint64_t reserved;          /* 0 */
} swg_maf_block; /* 64 bytes, no implicit padding */
typedef struct swg_maf_request {
  uint32_t set;            /* in: SWG_IV_ALL or SWG_IV_KEPT */
  uint32_t split_gap;      /* in: g; 0 = no breakers */
  uint64_t block_capacity; /* in: blocks `blocks` can hold */
  swg_maf_block* blocks;   /* in: caller-owned or NULL; written only when n_blocks <= block_capacity */
  uint64_t text_capacity;
  char* text;              /* written only when text_bytes <= text_capacity */
  uint64_t ops;            /* out: ops parsed over the whole set */
  uint64_t cigar_bad;      /* out: entries with a state bit of 1 .. 8 */
  uint64_t empty;          /* out: entries of state 16 */
  uint64_t usable, no_sequence, out_of_sequence;
  uint64_t n_blocks, gap_only; /* out: candidates with and without an aligned column */
  uint64_t breakers;           /* out: breaker ops of usable entries */
  uint64_t skipped_t, skipped_q; /* out: bases under them */
  uint64_t columns, aligned;   /* out: over the blocks */
  uint64_t text_bytes;         /* out: 2 * columns */
} swg_maf_request; /* 152 bytes, no implicit padding */
/* Everything on the host. */
int swg_maf_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                    swg_maf_request* req);
/* Columns, strand, status, the three arrays of the set, seqs->offset and seqs->bases in device memory of ctx's GPU; the two set
 * structures, the request and its arrays on the host. */
int swg_maf_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                           swg_maf_request* req);
/* --maf: the blocks of the records of `set` of an open PAF as MAF.  `##maf version=1\n`, then per block, in (record, block) order,
 *   a score=<aligned>
 *   s <tname> <t_start> <t_bases> + <tlen> <target row>
 *   s <qname> <qs> <q_bases> <+|-> <qlen> <query row>
 *   <empty line>
 * with single spaces; qs = q_start on '+' and qlen - q_start - q_bases on '-' (MAF's reverse-strand coordinate); the names are the
 * handle's, the lengths columns 2 and 7 of the record's own line.  score is the block's aligned columns: no bases are compared.  A
 * record of the set that is not usable writes nothing and is counted.  Sequence names are matched to the FASTA records as
 * swg_paf_vcf_write does it (length_mismatch included); the bases go to the device once per call; the entry is the LAST cg:Z: of
 * the line; batches come from swg_paf_ucsc_chain_write's planner over the cost text length + (q_end - q_start) + (t_end - t_start),
 * which bounds a usable entry's alignment columns and, at 2 bytes per column, its output: one device pass per batch with that bound
 * as the text capacity.  The file is the same bytes for every batch_bytes.  A set without records gives the header line alone and
 * needs no device (ctx may be NULL).  Refusals, all before a file is opened: set > 1, reserved != 0, SWG_IV_KEPT without status, a
 * NULL fasta or opts: SWG_ERR_INVALID; a handle whose columns are rebased: SWG_ERR_UNSUPPORTED.  counts may be NULL.  Errors:
 * swg_alnstats_last_error(). */
typedef struct swg_maf_options {
  uint32_t set;         /* SWG_IV_ALL or SWG_IV_KEPT */
  uint32_t split_gap;   /* g; 0 = one block per record */
  uint64_t batch_bytes; /* cost per device call; 0 = a default from the device's memory */
  uint64_t reserved;    /* 0 */
} swg_maf_options; /* 24 bytes */
typedef struct swg_maf_counts {
  uint64_t records;  /* records of the set */
  uint64_t usable;   /* entries walked */
  uint64_t bad;      /* entries with a state bit of 1 .. 8 */
  uint64_t untagged; /* records without a cg:Z: tag */
  uint64_t no_sequence, out_of_sequence; /* entries */
  uint64_t length_mismatch;              /* sequences */
  uint64_t blocks, gap_only, breakers, skipped_t, skipped_q, columns, aligned;
  uint64_t file_bytes; /* bytes written */
  uint64_t batches;    /* device calls */
} swg_maf_counts; /* 128 bytes */
int swg_paf_maf_write(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_maf_options* opts,
                      const char* out_path, swg_maf_counts* counts);
/* The same as one malloc'd text (release with swg_free). */
int swg_paf_maf_text(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_maf_options* opts,
                     swg_maf_counts* counts, char** text, uint64_t* len);
/* Per contig, the bottom-s MULTISET of min(SipHash-1-3(le64(k) || window), SipHash-1-3(le64(k) || revcomp upper-cased))
 * over the windows of k bytes all in ACGTacgt, ascending (KmerSketch::from_sequence, mash.rs:78-131).  Contig i =
 * seq[offsets[i], offsets[i + 1]); counts_out[n_seq]; minimizers_out[n_seq * s], row i holds counts_out[i] values.  The
 * contigs stream through the device in fixed-size chunks (device memory does not grow with the input).  k in 1..64,
 * s in 1..65536, else SWG_ERR_UNSUPPORTED.  timing_ms (optional, [5]): wall, H2D, hash, select (ms, device events), k-mers. */
int swg_mash_sketch(swg_ctx* ctx, const uint8_t* seq, const uint64_t* offsets, uint64_t n_seq, int k, uint64_t s,
                    uint64_t* counts_out, uint64_t* minimizers_out, double* timing_ms);
/* merge_sketches (knn_graph.rs:568-582), host: the rows `members` of a [.. x stride] sketch table concatenated, sorted,
 * deduplicated and truncated to s -> out[<= s], *out_count */
int swg_mash_merge(const uint64_t* minimizers, const uint64_t* counts, uint64_t stride, const uint64_t* members,
                   uint64_t n_members, uint64_t s, uint64_t* out, uint64_t* out_count);
/* All-vs-all Mash distance (mash.rs:39-73) over n sketch rows (row i = sketches[i * stride ..], counts[i] ascending
 * values, taken as SETS): dist_out[n * n] (diagonal 0.0), intersection / union sizes in the optional [n * n] outputs.
 * ln is glibc's log, bit for bit.  n <= 65535. */
int swg_mash_distances(swg_ctx* ctx, const uint64_t* sketches, const uint64_t* counts, uint64_t stride, uint64_t n, int k,
                       double* dist_out, uint32_t* inter_out, uint32_t* union_out);
/* generate_random_pairs (knn_graph.rs:362-386) for rows [row_begin, row_end): mask_out[(row_end - row_begin) * ceil(n / 64)],
 * bit j of row i set when i < j and SipHash-1-3(le64(i) || le64(j)) <= (fraction * u64::MAX as f64) as u64. */
int swg_mash_random_pairs(swg_ctx* ctx, uint64_t n, double fraction, uint64_t row_begin, uint64_t row_end, uint64_t* mask_out);
/* Pair selection over n items (select_pairs_from_sketches, knn_graph.rs:498-560) for a --sparsify string; dist ([n * n])
 * is needed by auto, giant:/connectivity: and tree:/knn:.  *pairs_out = 2 * *n_pairs values (i < j), sorted, released
 * with swg_free().  ctx may be NULL when no random pairs are drawn (none, all, wfmash:). */
int swg_select_pairs(swg_ctx* ctx, const char* strategy, const double* dist, uint64_t n, uint64_t** pairs_out, uint64_t* n_pairs);
/* `sweepga --joblist` over PanSN FASTA (main.rs:848-960, 2711-2745; joblist.rs:124-145): one line per selected haplotype
 * pair plus every haplotype's self pair, "wfmash -t T [-l L] -T A -Q B a.fa [b.fa] > DIR/A_vs_B.paf" with '#' etc. as
 * '_' in the file name.  threads = T (the reference's default is 8); min_aln_length 0 omits -l; output_dir NULL = ".".
 * Input without PanSN structure: SWG_ERR_UNSUPPORTED (the reference's per-file sweepga fallback is not emitted).
 * *out_text is released with swg_free().  timing_ms (optional, [6]): read, sketch, merge, distances, select, total. */
int swg_joblist(swg_ctx* ctx, const char* const* paths, int n_paths, const char* strategy, int k, uint64_t s, uint64_t threads,
                uint64_t min_aln_length, const char* output_dir, int io_threads, char** out_text, uint64_t* out_len,
                double* timing_ms);

#ifdef __cplusplus
}
#endif
#endif /* SWEEPGA_GPU_H */
