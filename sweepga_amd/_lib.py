"""ctypes binding of include/sweepga_gpu.h.  There is no CPU fallback: if the HIP library is
missing or no GPU is usable, every compute call raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsweepga_gpu.so")

SWG_OK = 0
ERR_NAMES = {-1: "SWG_ERR_INVALID", -2: "SWG_ERR_NO_DEVICE", -3: "SWG_ERR_HIP", -4: "SWG_ERR_OOM",
             -5: "SWG_ERR_RANGE", -6: "SWG_ERR_UNSUPPORTED"}
K_INF = 2**64 - 1

# every symbol include/sweepga_gpu.h declares
SYMBOLS = ["swg_abi_version", "swg_create", "swg_destroy", "swg_last_error", "swg_stream", "swg_synchronize",
           "swg_set_memory_limit", "swg_get_memory_limit",
           "swg_filter", "swg_filter_device", "swg_filter64", "swg_filter_device64", "swg_plane_sweep", "swg_plane_sweep_scaffolds",
           "swg_merge_chains", "swg_union_find_sets", "swg_log", "swg_log_range", "swg_profile_enable",
           "swg_profile_reset", "swg_profile_count", "swg_profile_get", "swg_profile_units", "swg_profile_select",
           "swg_paf_open", "swg_paf_open_buffer", "swg_paf_close", "swg_paf_records", "swg_paf_num_lines",
           "swg_paf_ranks", "swg_paf_num_sequences", "swg_paf_sequence_name", "swg_paf_timing", "swg_paf_text",
           "swg_paf_write", "swg_filter_paf", "swg_paf_last_error",
           "swg_parse_ani_method", "swg_parse_identity_value", "swg_paf_ani_input", "swg_ani_median", "swg_paf_ani_stats",
           "swg_filter_multi", "swg_filter_multi64", "swg_memory_info", "swg_reserve", "swg_warmup",
           "swg_aln_open", "swg_aln_close", "swg_aln_records", "swg_aln_num_sequences", "swg_aln_sequence_name",
           "swg_paf_seq_offsets", "swg_aln_seq_offsets", "swg_paf_record_offsets", "swg_aln_record_offsets",
           "swg_paf_tree_filter", "swg_free", "swg_stream_plan", "swg_paf_identity_is_derived",
           "swg_alnstats_open", "swg_alnstats_open_buffer", "swg_alnstats_close", "swg_alnstats_get", "swg_alnstats_pair",
           "swg_alnstats_report", "swg_alnstats_compare", "swg_alnstats_last_error",
           "swg_alnstats_records", "swg_alnstats_records_device", "swg_paf_alnstats",
           "swg_fasta_open", "swg_fasta_close", "swg_fasta_num_records", "swg_fasta_name", "swg_fasta_file_index",
           "swg_fasta_offsets", "swg_fasta_bases", "swg_fasta_last_error", "swg_mash_sketch", "swg_mash_merge",
           "swg_mash_distances", "swg_mash_random_pairs", "swg_select_pairs", "swg_joblist",
           "swg_tree_select_pairs", "swg_tree_select_records", "swg_tree_select_records_device", "swg_filter_subset",
           "swg_filter_subset_device", "swg_filter_subset_multi", "swg_paf_tree_select", "swg_paf_tree_needs_text",
           "swg_aln_tree_select", "swg_paf_num_genomes_two", "swg_paf_genome_two_prefix", "swg_aln_num_genomes_two",
           "swg_aln_genome_two_prefix",
           "swg_breadth_records", "swg_breadth_records_device", "swg_paf_breadth",
           "swg_blocks_records", "swg_blocks_records_device", "swg_paf_blocks",
           "swg_components_records", "swg_components_records_device", "swg_paf_components",
           "swg_intervals_records", "swg_intervals_records_device", "swg_paf_intervals", "swg_paf_interval_texts",
           "swg_sharing_records", "swg_sharing_records_device", "swg_paf_sharing",
           "swg_dotplot_records", "swg_dotplot_records_device", "swg_paf_dotplot",
           "swg_lift_records", "swg_lift_records_device", "swg_paf_lift",
           "swg_lift_closure_records", "swg_lift_closure_records_device", "swg_paf_lift_closure",
           "swg_lift_exact_records", "swg_lift_exact_records_device", "swg_lift_hit_records", "swg_lift_hit_records_device",
           "swg_paf_lift_exact", "swg_paf_lift_exact_counts",
           "swg_lift_slice_records", "swg_lift_slice_records_device", "swg_lift_slice_text_tile", "swg_paf_lift_paf_write", "swg_paf_lift_paf_text",
           "swg_ucsc_chain_records", "swg_ucsc_chain_records_device", "swg_paf_ucsc_chain_write", "swg_paf_ucsc_chain_text",
           "swg_diff_records", "swg_diff_records_device", "swg_paf_diffs_write", "swg_paf_diffs_text",
           "swg_mosaic_records", "swg_mosaic_records_device", "swg_paf_mosaic",
           "swg_gaps_records", "swg_gaps_records_device", "swg_paf_gaps",
           "swg_place_records", "swg_place_records_device", "swg_paf_place",
           "swg_windows_records", "swg_windows_records_device", "swg_paf_windows",
           "swg_divergence_records", "swg_divergence_records_device", "swg_paf_divergence",
           "swg_variant_records", "swg_variant_records_device", "swg_paf_vcf_write", "swg_paf_vcf_text",
           "swg_eqx_records", "swg_eqx_records_device", "swg_paf_eqx_write", "swg_paf_eqx_text",
           "swg_maf_records", "swg_maf_records_device", "swg_paf_maf_write", "swg_paf_maf_text"]


class SwgError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {text}")
        self.code = code


class SwgConfig(C.Structure):
    _fields_ = [
        ("min_block_length", C.c_uint64),
        ("mapping_filter_mode", C.c_int32),
        ("mapping_max_per_query", C.c_uint64),
        ("mapping_max_per_target", C.c_uint64),
        ("scaffold_filter_mode", C.c_int32),
        ("scaffold_max_per_query", C.c_uint64),
        ("scaffold_max_per_target", C.c_uint64),
        ("overlap_threshold", C.c_double),
        ("scaffold_gap", C.c_uint64),
        ("min_scaffold_length", C.c_uint64),
        ("scaffold_overlap_threshold", C.c_double),
        ("scaffold_max_deviation", C.c_uint64),
        ("scoring_function", C.c_int32),
        ("min_identity", C.c_double),
        ("min_scaffold_identity", C.c_double),
        ("keep_self", C.c_int32),
        ("scaffolds_only", C.c_int32),
    ]


class SwgRecords(C.Structure):
    _fields_ = [
        ("n", C.c_uint64),
        ("q_id", C.c_void_p),
        ("t_id", C.c_void_p),
        ("q_start", C.c_void_p),
        ("q_end", C.c_void_p),
        ("t_start", C.c_void_p),
        ("t_end", C.c_void_p),
        ("identity", C.c_void_p),
        ("matches", C.c_void_p),
        ("block_len", C.c_void_p),
        ("strand", C.c_void_p),
        ("n_seq", C.c_uint32),
        ("seq_genome_last", C.c_void_p),
        ("n_genome_last", C.c_uint32),
        ("seq_genome_two", C.c_void_p),
        ("n_genome_two", C.c_uint32),
    ]


class SwgStats(C.Structure):
    _fields_ = [
        ("n_in", C.c_uint64),
        ("n_retained", C.c_uint64),
        ("n_swept", C.c_uint64),
        ("n_chains", C.c_uint64),
        ("n_chains_kept", C.c_uint64),
        ("n_out", C.c_uint64),
        ("device_ms", C.c_double),
        ("h2d_ms", C.c_double),
        ("d2h_ms", C.c_double),
    ]


class SwgAniInput(C.Structure):
    _fields_ = [
        ("n", C.c_uint64),
        ("eligible", C.c_void_p),
        ("pair", C.c_void_p),
        ("n_pairs", C.c_uint64),
        ("matches", C.c_void_p),
        ("block_len", C.c_void_p),
        ("total_genome_size", C.c_double),
    ]


class SwgAlnstatsPairCounts(C.Structure):
    _fields_ = [("q_genome", C.c_uint32), ("t_genome", C.c_uint32), ("bases", C.c_uint64), ("matches", C.c_uint64),
                ("first_record", C.c_uint64)]


class SwgAlnstatsCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("total_mappings", "total_bases", "total_matches", "self_mappings", "inter_chromosomal",
                                           "inter_genome", "chr_pair_count", "n_pairs", "pair_capacity")] + \
               [("pairs", C.POINTER(SwgAlnstatsPairCounts)), ("seq_last", C.POINTER(C.c_uint64))]


class SwgBreadthPair(C.Structure):
    _fields_ = [("q_genome", C.c_uint32), ("t_genome", C.c_uint32), ("q_bases", C.c_uint64), ("t_bases", C.c_uint64),
                ("q_union", C.c_uint64), ("t_union", C.c_uint64), ("first_record", C.c_uint64)]


class SwgBreadthCounts(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("pair_capacity", C.c_uint64), ("pairs", C.POINTER(SwgBreadthPair))]


class SwgBlock(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("chain", "q_id", "t_id", "strand", "q_start", "q_end", "t_start", "t_end", "n_core",
                                           "n_inverted", "n_rescued", "reserved")] + \
               [(k, C.c_uint64) for k in ("matches", "block_len", "q_bases", "t_bases", "q_cover", "t_cover", "first_record")]


class SwgBlockTable(C.Structure):
    _fields_ = [("n_blocks", C.c_uint64), ("block_capacity", C.c_uint64), ("blocks", C.POINTER(SwgBlock))]


class SwgComponentParams(C.Structure):
    _fields_ = [("min_bases", C.c_uint64), ("min_share_ppm", C.c_uint32), ("reserved", C.c_uint32)]


class SwgLink(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("a", "b", "n_records", "joined")] + \
               [(k, C.c_uint64) for k in ("a_bases", "b_bases", "first_record")]


class SwgComponent(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("id", "first_seq", "n_seq", "n_links")] + \
               [(k, C.c_uint64) for k in ("length", "n_records", "bases")]


class SwgComponentTable(C.Structure):
    _fields_ = [("n_components", C.c_uint64), ("component_capacity", C.c_uint64), ("components", C.POINTER(SwgComponent)),
                ("n_links", C.c_uint64), ("link_capacity", C.c_uint64), ("links", C.POINTER(SwgLink)),
                ("seq_component", C.POINTER(C.c_uint32)),
                ("cross_links", C.c_uint64), ("cross_records", C.c_uint64), ("cross_bases", C.c_uint64)]


class SwgInterval(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("seq", "other_genome", "start", "end")]


class SwgIntervalList(C.Structure):
    _fields_ = [("n", C.c_uint64), ("bases", C.c_uint64), ("capacity", C.c_uint64), ("rows", C.POINTER(SwgInterval))]


class SwgIntervalRequest(C.Structure):
    _fields_ = [("want", C.c_uint32), ("reserved", C.c_uint32), ("list", (SwgIntervalList * 2) * 3)]   # list[set][axis]


_lib = None


class SwgDepthRun(C.Structure):
    _fields_ = [("seq", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("depth", C.c_uint32)]


class SwgDepthList(C.Structure):
    _fields_ = [("n", C.c_uint64), ("bases", C.c_uint64), ("capacity", C.c_uint64), ("rows", C.POINTER(SwgDepthRun)),
                ("spectrum", C.POINTER(C.c_uint64))]


class SwgSharingRequest(C.Structure):
    _fields_ = [("want", C.c_uint32), ("reserved", C.c_uint32), ("set", SwgDepthList * 2)]   # set[ALL, KEPT]


class SwgGapRow(C.Structure):
    _fields_ = [("chain", C.c_uint32), ("left", C.c_uint32), ("right", C.c_uint32), ("q_lo", C.c_uint32), ("q_hi", C.c_uint32),
                ("t_lo", C.c_uint32), ("t_hi", C.c_uint32), ("kind", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint16)]


class SwgGapPair(C.Structure):
    _fields_ = [("q_genome", C.c_uint32), ("t_genome", C.c_uint32), ("links", C.c_uint64), ("n_ins", C.c_uint64), ("ins_bases", C.c_uint64),
                ("n_del", C.c_uint64), ("del_bases", C.c_uint64), ("n_inv", C.c_uint64), ("inv_bases", C.c_uint64)]


class SwgGapsRequest(C.Structure):
    _fields_ = [("want", C.c_uint32), ("min_size", C.c_uint32), ("n_rows", C.c_uint64), ("capacity", C.c_uint64), ("rows", C.POINTER(SwgGapRow)),
                ("n_pairs", C.c_uint64), ("pair_capacity", C.c_uint64), ("pairs", C.POINTER(SwgGapPair)), ("spectrum", C.POINTER(C.c_uint64)),
                ("reserved", C.c_uint64)]


class SwgPlacement(C.Structure):
    _fields_ = [("seq", C.c_uint32), ("partner", C.c_uint32), ("genome", C.c_uint32), ("partner_genome", C.c_uint32), ("offset", C.c_int64),
                ("start", C.c_int64), ("bases", C.c_uint64), ("fwd", C.c_uint64), ("rev", C.c_uint64), ("total_bases", C.c_uint64),
                ("runner_bases", C.c_uint64), ("n_records", C.c_uint64), ("q_lo", C.c_uint32), ("q_hi", C.c_uint32), ("t_lo", C.c_uint32),
                ("t_hi", C.c_uint32), ("rank", C.c_uint32), ("orient", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class SwgPlacePair(C.Structure):
    _fields_ = [("genome", C.c_uint32), ("partner_genome", C.c_uint32), ("rows", C.c_uint64), ("reversed", C.c_uint64), ("length", C.c_uint64),
                ("bases", C.c_uint64), ("total_bases", C.c_uint64)]


class SwgPlaceRequest(C.Structure):
    _fields_ = [("want", C.c_uint32), ("axis", C.c_uint32), ("set", C.c_uint32), ("reserved", C.c_uint32), ("min_bases", C.c_uint64),
                ("n_rows", C.c_uint64), ("capacity", C.c_uint64), ("rows", C.POINTER(SwgPlacement)), ("n_pairs", C.c_uint64),
                ("pair_capacity", C.c_uint64), ("pairs", C.POINTER(SwgPlacePair))]


class SwgWindowRow(C.Structure):
    _fields_ = [("seq", C.c_uint32), ("index", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("n", C.c_uint32 * 2),
                ("covered", C.c_uint32 * 2), ("depth", C.c_uint64 * 2), ("matches", C.c_uint64 * 2)]


class SwgWindowSeq(C.Structure):
    _fields_ = [("seq", C.c_uint32), ("windows", C.c_uint32), ("empty", C.c_uint32 * 2), ("covered", C.c_uint64 * 2), ("depth", C.c_uint64 * 2),
                ("matches", C.c_uint64 * 2), ("records", C.c_uint64 * 2)]


class SwgWindowsRequest(C.Structure):
    _fields_ = [("want", C.c_uint32), ("axis", C.c_uint32), ("window", C.c_uint32), ("other_genome", C.c_uint32), ("weight", C.c_void_p),
                ("n_rows", C.c_uint64), ("capacity", C.c_uint64), ("rows", C.POINTER(SwgWindowRow)), ("n_seqs", C.c_uint64),
                ("seq_capacity", C.c_uint64), ("seqs", C.POINTER(SwgWindowSeq)), ("reserved", C.c_uint64)]


class SwgMosaicRow(C.Structure):
    _fields_ = [("seq", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("record", C.c_uint32)]


class SwgMosaicRequest(C.Structure):
    _fields_ = [("want", C.c_uint32), ("axis", C.c_uint32), ("set", C.c_uint32), ("reserved", C.c_uint32), ("weight", C.c_void_p),
                ("n", C.c_uint64), ("bases", C.c_uint64), ("capacity", C.c_uint64), ("rows", C.POINTER(SwgMosaicRow)),
                ("share", C.POINTER(C.c_uint64))]


class SwgDotAxes(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("x_total", C.c_uint64), ("y_total", C.c_uint64),
                ("x_off", C.c_void_p), ("y_off", C.c_void_p)]


class SwgDotRequest(C.Structure):
    _fields_ = [("want", C.c_uint32), ("reserved", C.c_uint32), ("plane", C.c_void_p * 4), ("hits", C.c_uint64 * 4),
                ("drawn", C.c_uint64 * 2)]


class SwgDotView(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("query_prefix", C.c_char_p), ("target_prefix", C.c_char_p)]


class SwgLiftRegion(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("seq", "start", "end", "reserved")]


class SwgLiftRow(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("region", "record", "src_start", "src_end", "dst_seq", "dst_start", "dst_end", "flags")]


class SwgLiftSummary(C.Structure):
    _fields_ = [("hits", (C.c_uint32 * 2) * 2)]   # hits[set][axis]


class SwgLiftRequest(C.Structure):
    _fields_ = [("set", C.c_uint32), ("axes", C.c_uint32), ("n", C.c_uint64), ("candidates", C.c_uint64 * 2), ("capacity", C.c_uint64),
                ("rows", C.c_void_p), ("summary", C.c_void_p)]


class SwgCigarSet(C.Structure):
    _fields_ = [("record", C.c_void_p), ("offset", C.c_void_p), ("text", C.c_void_p), ("k", C.c_uint64)]


class SwgLiftExactRow(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("region", "record", "src_start", "src_end", "dst_seq", "dst_start", "dst_end", "flags", "aligned", "matches")]


class SwgLiftExactRequest(C.Structure):
    _fields_ = [("set", C.c_uint32), ("axes", C.c_uint32), ("n", C.c_uint64), ("candidates", C.c_uint64 * 2), ("capacity", C.c_uint64),
                ("rows", C.c_void_p), ("summary", C.c_void_p), ("state", C.c_void_p), ("ops", C.c_uint64), ("cigar_bad", C.c_uint64),
                ("exact_rows", C.c_uint64)]


class SwgLiftSlice(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("region", "record", "q_start", "q_end", "t_start", "t_end", "flags", "aligned", "matches", "text_len")]
    _fields_ += [("block", C.c_uint64), ("text_first", C.c_uint64)]


class SwgLiftSliceRequest(C.Structure):
    _fields_ = [("set", C.c_uint32), ("axes", C.c_uint32), ("min_aligned", C.c_uint32), ("reserved", C.c_uint32), ("slice_capacity", C.c_uint64),
                ("slices", C.c_void_p), ("text_capacity", C.c_uint64), ("text", C.c_void_p), ("state", C.c_void_p)]
    _fields_ += [(k, C.c_uint64) for k in ("n_rows", "n_slices", "n_interp", "n_empty", "n_short", "text_bytes", "ops", "cigar_bad")]


class SwgLiftPafCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("rows", "slices", "interp", "empty", "too_short", "hits", "bad", "batches")]


class SwgUcscBlock(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("size", "dt", "dq")]


class SwgUcscChain(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("record", "flags", "ref_start", "ref_end", "oth_start", "oth_end", "score", "n_blocks")]
    _fields_ += [("first_block", C.c_uint64), ("text_first", C.c_uint64)]


class SwgUcscRequest(C.Structure):
    _fields_ = [("set", C.c_uint32), ("from_", C.c_uint32), ("chain_capacity", C.c_uint64), ("chains", C.c_void_p), ("block_capacity", C.c_uint64),
                ("blocks", C.c_void_p), ("text_capacity", C.c_uint64), ("text", C.c_void_p), ("state", C.c_void_p)]
    _fields_ += [(k, C.c_uint64) for k in ("n_chains", "n_blocks", "text_bytes", "ops", "cigar_bad", "beyond", "empty_chains")]


class SwgUcscCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("records", "chains", "bad", "beyond", "untagged", "empty", "blocks", "batches")]


DIVERGENCE_SUMS = ("aligned", "matches", "mismatches", "m_columns", "unaligned", "inserted", "mismatch_runs", "indels")


class SwgDivergenceRow(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("seq", "start", "end", "n")] + [(k, C.c_uint64) for k in DIVERGENCE_SUMS]


class SwgDivergenceSeq(C.Structure):
    _fields_ = [("seq", C.c_uint32), ("windows", C.c_uint32), ("records", C.c_uint64), ("entries", C.c_uint64)] + [(k, C.c_uint64) for k in DIVERGENCE_SUMS]


class SwgDivergenceRequest(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("set", "axis", "window", "other_genome", "want", "reserved")]
    _fields_ += [("capacity", C.c_uint64), ("rows", C.c_void_p), ("seq_capacity", C.c_uint64), ("seqs", C.c_void_p), ("state", C.c_void_p)]
    _fields_ += [(k, C.c_uint64) for k in ("n_rows", "n_seqs", "ops", "cigar_bad", "usable")]


class SwgDivergenceCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("records", "usable", "bad", "untagged", "windows", "seqs", "batches")]


class SwgDiffRow(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("record", "kind_flags", "t_start", "t_end", "q_start", "q_end", "left", "right")]


DIFF_SUMS = ("entries", "aligned", "eq", "m_columns", "snp_runs", "snp_bases", "n_ins", "ins_bases", "n_del", "del_bases", "n_skip", "skip_bases")


class SwgDiffPair(C.Structure):
    _fields_ = [("q_genome", C.c_uint32), ("t_genome", C.c_uint32)] + [(k, C.c_uint64) for k in DIFF_SUMS]


class SwgDiffRequest(C.Structure):
    _fields_ = [("set", C.c_uint32), ("kinds", C.c_uint32), ("min_indel", C.c_uint32), ("reserved", C.c_uint32), ("row_capacity", C.c_uint64),
                ("rows", C.c_void_p), ("pair_capacity", C.c_uint64), ("pairs", C.c_void_p), ("spectrum", C.c_void_p), ("state", C.c_void_p)]
    _fields_ += [(k, C.c_uint64) for k in ("n_rows", "n_pairs", "ops", "cigar_bad", "usable")]


class SwgDiffCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("records", "usable", "bad", "untagged", "rows", "snp_runs", "snp_bases", "n_ins", "ins_bases", "n_del",
                                          "del_bases", "n_skip", "skip_bases", "m_columns", "batches")]


VARIANT_SUBS = tuple(f"{r}>{a}" for r in "ACGT" for a in "ACGT" if r != a)
VARIANT_SUMS = ("entries", "compared", "snvs") + VARIANT_SUBS + ("same", "m_equal", "n_columns", "n_ins", "ins_bases", "n_del", "del_bases", "long_indels",
                                                               "unanchored")


class SwgSeqSet(C.Structure):
    _fields_ = [("offset", C.c_void_p), ("bases", C.c_void_p), ("n_seq", C.c_uint32), ("reserved", C.c_uint32)]


class SwgVariantRequest(C.Structure):
    _fields_ = [("set", C.c_uint32), ("t_genome", C.c_uint32), ("q_genome", C.c_uint32), ("max_indel", C.c_uint32), ("reserved", C.c_uint64),
                ("variant_capacity", C.c_uint64), ("variants", C.c_void_p), ("pool_capacity", C.c_uint64), ("pool", C.c_void_p),
                ("pair_capacity", C.c_uint64), ("pairs", C.c_void_p)]
    _fields_ += [(k, C.c_uint64) for k in ("n_variants", "pool_bytes", "n_pairs", "ops", "cigar_bad", "usable", "no_sequence", "out_of_sequence",
                                           "columns")]


class SwgVcfOptions(C.Structure):
    _fields_ = [("set", C.c_uint32), ("max_indel", C.c_uint32), ("ref_genome", C.c_char_p), ("query_genome", C.c_char_p), ("batch_bytes", C.c_uint64),
                ("reserved", C.c_uint64)]


VCF_COUNTS = ("records", "usable", "bad", "untagged", "variants", "snvs", "n_ins", "n_del", "same", "n_columns", "m_equal", "long_indels", "unanchored",
              "no_sequence", "out_of_sequence", "length_mismatch", "batches")


class SwgVcfCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in VCF_COUNTS]


EQX_FIELDS = ("ops", "cigar_bad", "empty", "usable", "no_sequence", "out_of_sequence", "columns", "out_ops", "text_bytes", "changed", "matches",
              "mismatches", "n_columns", "eq_wrong", "x_wrong", "m_columns")


class SwgEqxRequest(C.Structure):
    _fields_ = [("set", C.c_uint32), ("reserved", C.c_uint32), ("entry_capacity", C.c_uint64), ("entries", C.c_void_p), ("text_capacity", C.c_uint64),
                ("text", C.c_void_p)]
    _fields_ += [(k, C.c_uint64) for k in EQX_FIELDS]


class SwgEqxOptions(C.Structure):
    _fields_ = [("set", C.c_uint32), ("unresolved", C.c_uint32), ("batch_bytes", C.c_uint64), ("reserved", C.c_uint64)]


EQX_COUNTS = ("records", "usable", "bad", "untagged", "no_sequence", "out_of_sequence", "length_mismatch", "changed", "lines", "columns", "matches",
              "mismatches", "eq_wrong", "x_wrong", "m_columns", "batches")


class SwgEqxCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in EQX_COUNTS]


MAF_FIELDS = ("ops", "cigar_bad", "empty", "usable", "no_sequence", "out_of_sequence", "n_blocks", "gap_only", "breakers", "skipped_t", "skipped_q",
              "columns", "aligned", "text_bytes")


class SwgMafRequest(C.Structure):
    _fields_ = [("set", C.c_uint32), ("split_gap", C.c_uint32), ("block_capacity", C.c_uint64), ("blocks", C.c_void_p), ("text_capacity", C.c_uint64),
                ("text", C.c_void_p)]
    _fields_ += [(k, C.c_uint64) for k in MAF_FIELDS]


class SwgMafOptions(C.Structure):
    _fields_ = [("set", C.c_uint32), ("split_gap", C.c_uint32), ("batch_bytes", C.c_uint64), ("reserved", C.c_uint64)]


MAF_COUNTS = ("records", "usable", "bad", "untagged", "no_sequence", "out_of_sequence", "length_mismatch", "blocks", "gap_only", "breakers", "skipped_t",
              "skipped_q", "columns", "aligned", "file_bytes", "batches")


class SwgMafCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in MAF_COUNTS]


class SwgClosureRow(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("region", "seq", "start", "end", "hop", "reserved")]


class SwgClosureSummary(C.Structure):
    _fields_ = [("bases", C.c_uint64)] + [(k, C.c_uint32) for k in ("pieces", "sequences", "hops", "flags")]


class SwgClosureRequest(C.Structure):
    _fields_ = [("set", C.c_uint32), ("axes", C.c_uint32), ("max_hops", C.c_uint32), ("min_len", C.c_uint32), ("capacity", C.c_uint64),
                ("rows", C.c_void_p), ("summary", C.c_void_p), ("n", C.c_uint64), ("projections", C.c_uint64), ("candidates", C.c_uint64 * 2),
                ("hops_run", C.c_uint32), ("reserved", C.c_uint32)]


def load():
    """Loads libsweepga_gpu.so.  Raises (loudly) if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension is not built (run `python -m sweepga_amd.build` or "
            "__graft_entry__.build()).  sweepga_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    lib.swg_abi_version.restype = C.c_int
    lib.swg_create.restype = C.c_int
    lib.swg_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.swg_destroy.restype = None
    lib.swg_destroy.argtypes = [C.c_void_p]
    lib.swg_last_error.restype = C.c_char_p
    lib.swg_last_error.argtypes = [C.c_void_p]
    lib.swg_stream.restype = C.c_void_p
    lib.swg_stream.argtypes = [C.c_void_p]
    lib.swg_synchronize.restype = C.c_int
    lib.swg_synchronize.argtypes = [C.c_void_p]
    for name in ("swg_filter", "swg_filter_device", "swg_filter64", "swg_filter_device64"):  # swg_records64 = same layout
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.POINTER(SwgConfig), C.c_void_p, C.c_void_p,
                      C.POINTER(SwgStats)]
    lib.swg_plane_sweep.restype = C.c_int
    lib.swg_plane_sweep.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_double, C.c_int,
                                    C.c_void_p]
    lib.swg_plane_sweep_scaffolds.restype = C.c_int
    lib.swg_plane_sweep_scaffolds.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                              C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64,
                                              C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.swg_merge_chains.restype = C.c_int
    lib.swg_merge_chains.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.swg_union_find_sets.restype = C.c_int
    lib.swg_union_find_sets.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_uint64)]
    lib.swg_log.restype = C.c_int
    lib.swg_log.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.swg_log_range.restype = C.c_int
    lib.swg_log_range.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.swg_profile_enable.restype = C.c_int
    lib.swg_profile_enable.argtypes = [C.c_void_p, C.c_int]
    lib.swg_profile_reset.restype = C.c_int
    lib.swg_profile_reset.argtypes = [C.c_void_p]
    lib.swg_profile_select.restype = C.c_int
    lib.swg_profile_select.argtypes = [C.c_void_p, C.c_char_p]
    lib.swg_profile_count.restype = C.c_int
    lib.swg_profile_count.argtypes = [C.c_void_p]
    lib.swg_profile_units.restype = C.c_int
    lib.swg_profile_units.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    lib.swg_profile_get.restype = C.c_int
    lib.swg_profile_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_double)]
    lib.swg_paf_open.restype = C.c_int
    lib.swg_paf_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.swg_paf_open_buffer.restype = C.c_int
    lib.swg_paf_open_buffer.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    lib.swg_paf_close.restype = None
    lib.swg_paf_close.argtypes = [C.c_void_p]
    lib.swg_paf_records.restype = C.POINTER(SwgRecords)
    lib.swg_paf_records.argtypes = [C.c_void_p]
    lib.swg_paf_num_lines.restype = C.c_uint64
    lib.swg_paf_num_lines.argtypes = [C.c_void_p]
    lib.swg_paf_ranks.restype = C.c_void_p
    lib.swg_paf_ranks.argtypes = [C.c_void_p]
    lib.swg_paf_num_sequences.restype = C.c_uint32
    lib.swg_paf_num_sequences.argtypes = [C.c_void_p]
    lib.swg_paf_sequence_name.restype = C.c_char_p
    lib.swg_paf_sequence_name.argtypes = [C.c_void_p, C.c_uint32]
    lib.swg_paf_timing.restype = None
    lib.swg_paf_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.swg_paf_text.restype = C.c_int
    lib.swg_paf_text.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.swg_paf_write.restype = C.c_int
    lib.swg_paf_write.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    lib.swg_filter_paf.restype = C.c_int
    lib.swg_filter_paf.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(SwgConfig), C.c_int,
                                   C.POINTER(SwgStats), C.POINTER(C.c_double)]
    lib.swg_paf_last_error.restype = C.c_char_p
    lib.swg_paf_last_error.argtypes = []
    lib.swg_parse_ani_method.restype = C.c_int
    lib.swg_parse_ani_method.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.swg_parse_identity_value.restype = C.c_int
    lib.swg_parse_identity_value.argtypes = [C.c_char_p, C.c_double, C.POINTER(C.c_double)]
    lib.swg_paf_ani_input.restype = C.c_int
    lib.swg_paf_ani_input.argtypes = [C.c_void_p, C.c_int, C.POINTER(SwgAniInput)]
    lib.swg_ani_median.restype = C.c_int
    lib.swg_ani_median.argtypes = [C.c_void_p, C.POINTER(SwgAniInput), C.c_void_p, C.c_int, C.c_double, C.c_int,
                                   C.POINTER(C.c_double)]
    lib.swg_filter_multi.restype = C.c_int
    lib.swg_filter_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(SwgRecords), C.POINTER(SwgConfig), C.c_void_p,
                                     C.c_void_p, C.POINTER(SwgStats)]
    lib.swg_filter_multi64.restype = C.c_int
    lib.swg_filter_multi64.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(SwgRecords), C.POINTER(SwgConfig), C.c_void_p,
                                     C.c_void_p, C.POINTER(SwgStats)]
    lib.swg_memory_info.restype = C.c_int
    lib.swg_memory_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.swg_reserve.restype = C.c_int
    lib.swg_reserve.argtypes = [C.c_void_p, C.c_uint64]
    lib.swg_warmup.restype = C.c_int
    lib.swg_warmup.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int]
    lib.swg_paf_ani_stats.restype = C.c_int
    lib.swg_paf_ani_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.swg_aln_open.restype = C.c_int
    lib.swg_aln_open.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.swg_aln_close.restype = None
    lib.swg_aln_close.argtypes = [C.c_void_p]
    lib.swg_aln_records.restype = C.POINTER(SwgRecords)
    lib.swg_aln_records.argtypes = [C.c_void_p]
    for name in ("swg_paf_seq_offsets", "swg_aln_seq_offsets"):
        f = getattr(lib, name)
        f.restype = C.POINTER(C.c_uint64)
        f.argtypes = [C.c_void_p]
    for name in ("swg_paf_record_offsets", "swg_aln_record_offsets"):
        f = getattr(lib, name)
        f.restype = C.POINTER(C.c_uint64)
        f.argtypes = [C.c_void_p, C.c_int]
    lib.swg_aln_num_sequences.restype = C.c_uint32
    lib.swg_aln_num_sequences.argtypes = [C.c_void_p]
    lib.swg_aln_sequence_name.restype = C.c_char_p
    lib.swg_aln_sequence_name.argtypes = [C.c_void_p, C.c_uint32]
    lib.swg_paf_tree_filter.restype = C.c_int
    lib.swg_paf_tree_filter.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_uint64)]
    lib.swg_set_memory_limit.restype = C.c_int
    lib.swg_set_memory_limit.argtypes = [C.c_void_p, C.c_uint64]
    lib.swg_get_memory_limit.restype = C.c_int
    lib.swg_get_memory_limit.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.swg_free.restype = None
    lib.swg_free.argtypes = [C.c_void_p]
    for name in ("swg_alnstats_records", "swg_alnstats_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(SwgAlnstatsCounts),
                      C.POINTER(SwgAlnstatsCounts)]
    lib.swg_paf_alnstats.restype = C.c_int
    lib.swg_paf_alnstats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    lib.swg_tree_select_pairs.restype = C.c_int
    lib.swg_tree_select_pairs.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_uint64, C.c_uint64, C.c_double, C.c_void_p]
    for name in ("swg_tree_select_records", "swg_tree_select_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_uint64, C.c_uint64,
                      C.c_double, C.c_void_p, C.POINTER(C.c_uint64)]
    for name in ("swg_filter_subset", "swg_filter_subset_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.POINTER(SwgConfig), C.c_void_p, C.c_void_p, C.POINTER(SwgStats)]
    lib.swg_filter_subset_multi.restype = C.c_int
    lib.swg_filter_subset_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(SwgRecords), C.c_void_p, C.POINTER(SwgConfig),
                                            C.c_void_p, C.c_void_p, C.POINTER(SwgStats)]
    lib.swg_paf_tree_select.restype = C.c_int
    lib.swg_paf_tree_select.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_double, C.c_int, C.c_void_p,
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    lib.swg_paf_tree_needs_text.restype = C.c_int
    lib.swg_paf_tree_needs_text.argtypes = [C.c_void_p]
    lib.swg_aln_tree_select.restype = C.c_int
    lib.swg_aln_tree_select.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_double, C.c_void_p, C.POINTER(C.c_uint64)]
    for name in ("swg_paf_num_genomes_two", "swg_aln_num_genomes_two"):
        f = getattr(lib, name)
        f.restype = C.c_uint32
        f.argtypes = [C.c_void_p]
    for name in ("swg_paf_genome_two_prefix", "swg_aln_genome_two_prefix"):
        f = getattr(lib, name)
        f.restype = C.c_char_p
        f.argtypes = [C.c_void_p, C.c_uint32]
    for name in ("swg_breadth_records", "swg_breadth_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(SwgBreadthCounts),
                      C.POINTER(SwgBreadthCounts)]
    for name in ("swg_blocks_records", "swg_blocks_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.POINTER(SwgBlockTable)]
    for name in ("swg_components_records", "swg_components_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.POINTER(SwgComponentParams), C.POINTER(SwgComponentTable)]
    lib.swg_paf_components.restype = C.c_int
    lib.swg_paf_components.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SwgComponentParams), C.c_int, C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_uint64)]
    lib.swg_paf_blocks.restype = C.c_int
    lib.swg_paf_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.swg_paf_breadth.restype = C.c_int
    lib.swg_paf_breadth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_intervals_records", "swg_intervals_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(SwgIntervalRequest)]
    lib.swg_paf_intervals.restype = C.c_int
    lib.swg_paf_intervals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_sharing_records", "swg_sharing_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(SwgSharingRequest)]
    lib.swg_paf_sharing.restype = C.c_int
    lib.swg_paf_sharing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_mosaic_records", "swg_mosaic_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(SwgMosaicRequest)]
    lib.swg_paf_mosaic.restype = C.c_int
    lib.swg_paf_mosaic.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_gaps_records", "swg_gaps_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(SwgGapsRequest)]
    lib.swg_paf_gaps.restype = C.c_int
    lib.swg_paf_gaps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_place_records", "swg_place_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(SwgPlaceRequest)]
    lib.swg_paf_place.restype = C.c_int
    lib.swg_paf_place.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_windows_records", "swg_windows_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(SwgWindowsRequest)]
    lib.swg_paf_windows.restype = C.c_int
    lib.swg_paf_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_dotplot_records", "swg_dotplot_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.POINTER(SwgDotAxes), C.c_void_p, C.POINTER(SwgDotRequest)]
    lib.swg_paf_dotplot.restype = C.c_int
    lib.swg_paf_dotplot.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SwgDotView), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_lift_records", "swg_lift_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SwgLiftRequest)]
    lib.swg_paf_lift.restype = C.c_int
    lib.swg_paf_lift.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_uint64)]
    for name in ("swg_lift_exact_records", "swg_lift_exact_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SwgCigarSet), C.POINTER(SwgLiftExactRequest)]
    for name in ("swg_lift_hit_records", "swg_lift_hit_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                      C.POINTER(C.c_uint64)]
    lib.swg_paf_lift_exact.restype = C.c_int
    lib.swg_paf_lift_exact.argtypes = lib.swg_paf_lift.argtypes
    lib.swg_paf_lift_exact_counts.restype = None
    lib.swg_paf_lift_exact_counts.argtypes = [C.POINTER(C.c_uint64)]
    for name in ("swg_lift_slice_records", "swg_lift_slice_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SwgCigarSet), C.POINTER(SwgLiftSliceRequest)]
    lib.swg_lift_slice_text_tile.restype = C.c_uint32
    lib.swg_lift_slice_text_tile.argtypes = []
    lib.swg_paf_lift_paf_write.restype = C.c_int
    lib.swg_paf_lift_paf_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                           C.c_char_p, C.POINTER(SwgLiftPafCounts)]
    lib.swg_paf_lift_paf_text.restype = C.c_int
    lib.swg_paf_lift_paf_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                          C.POINTER(SwgLiftPafCounts), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_ucsc_chain_records", "swg_ucsc_chain_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.POINTER(SwgCigarSet), C.POINTER(SwgUcscRequest)]
    lib.swg_paf_ucsc_chain_write.restype = C.c_int
    lib.swg_paf_ucsc_chain_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(SwgUcscCounts)]
    lib.swg_paf_ucsc_chain_text.restype = C.c_int
    lib.swg_paf_ucsc_chain_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(SwgUcscCounts),
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_diff_records", "swg_diff_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(SwgCigarSet), C.POINTER(SwgDiffRequest)]
    lib.swg_paf_diffs_write.restype = C.c_int
    lib.swg_paf_diffs_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_char_p, C.c_char_p,
                                        C.POINTER(SwgDiffCounts)]
    lib.swg_paf_diffs_text.restype = C.c_int
    lib.swg_paf_diffs_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(SwgDiffCounts),
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_variant_records", "swg_variant_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(SwgCigarSet), C.POINTER(SwgSeqSet),
                      C.POINTER(SwgVariantRequest)]
    lib.swg_fasta_open.restype, lib.swg_fasta_open.argtypes = C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.swg_fasta_close.restype, lib.swg_fasta_close.argtypes = None, [C.c_void_p]
    lib.swg_fasta_last_error.restype, lib.swg_fasta_last_error.argtypes = C.c_char_p, []
    lib.swg_paf_vcf_write.restype = C.c_int
    lib.swg_paf_vcf_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SwgVcfOptions), C.c_char_p, C.c_char_p, C.POINTER(SwgVcfCounts)]
    lib.swg_paf_vcf_text.restype = C.c_int
    lib.swg_paf_vcf_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SwgVcfOptions), C.POINTER(SwgVcfCounts),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for name in ("swg_eqx_records", "swg_eqx_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.POINTER(SwgCigarSet), C.POINTER(SwgSeqSet), C.POINTER(SwgEqxRequest)]
    lib.swg_paf_eqx_write.restype = C.c_int
    lib.swg_paf_eqx_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SwgEqxOptions), C.c_char_p, C.POINTER(SwgEqxCounts)]
    lib.swg_paf_eqx_text.restype = C.c_int
    lib.swg_paf_eqx_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SwgEqxOptions), C.POINTER(SwgEqxCounts), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_uint64)]
    for name in ("swg_maf_records", "swg_maf_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.POINTER(SwgCigarSet), C.POINTER(SwgSeqSet), C.POINTER(SwgMafRequest)]
    lib.swg_paf_maf_write.restype = C.c_int
    lib.swg_paf_maf_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SwgMafOptions), C.c_char_p, C.POINTER(SwgMafCounts)]
    lib.swg_paf_maf_text.restype = C.c_int
    lib.swg_paf_maf_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SwgMafOptions), C.POINTER(SwgMafCounts), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_uint64)]
    for name in ("swg_divergence_records", "swg_divergence_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(SwgCigarSet),
                      C.POINTER(SwgDivergenceRequest)]
    lib.swg_paf_divergence.restype = C.c_int
    lib.swg_paf_divergence.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_uint64), C.POINTER(SwgDivergenceCounts)]
    for name in ("swg_lift_closure_records", "swg_lift_closure_records_device"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SwgClosureRequest)]
    lib.swg_paf_lift_closure.restype = C.c_int
    lib.swg_paf_lift_closure.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.swg_paf_interval_texts.restype = C.c_int
    lib.swg_paf_interval_texts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.swg_alnstats_last_error.restype = C.c_char_p
    lib.swg_alnstats_last_error.argtypes = []
    _lib = lib
    return lib


class Context:
    """One swg_ctx (one GPU).  Not thread-safe, like the C object it wraps."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.swg_create(int(device), C.byref(h))
        if rc != SWG_OK:
            raise SwgError(rc, (self.lib.swg_last_error(None) or b"").decode())
        self.handle = h
        self.device = device

    def check(self, rc):
        if rc != SWG_OK:
            raise SwgError(rc, (self.lib.swg_last_error(self.handle) or b"").decode())

    def synchronize(self):
        self.check(self.lib.swg_synchronize(self.handle))

    @property
    def stream(self):
        return self.lib.swg_stream(self.handle)

    def profile(self, on=True):
        self.check(self.lib.swg_profile_enable(self.handle, int(bool(on))))

    def profile_reset(self):
        self.check(self.lib.swg_profile_reset(self.handle))

    def profile_select(self, kernel_name=None):
        """HIP events only around launches of this kernel (None: around every launch again)."""
        self.check(self.lib.swg_profile_select(self.handle, kernel_name.encode() if kernel_name else None))

    def profile_table(self):
        """{kernel name: (launches, total_ms)} accumulated since the last reset."""
        n = self.lib.swg_profile_count(self.handle)
        if n < 0:
            self.check(n)
        out = {}
        for i in range(n):
            name = C.c_char_p()
            launches = C.c_uint64()
            ms = C.c_double()
            self.check(self.lib.swg_profile_get(self.handle, i, C.byref(name), C.byref(launches), C.byref(ms)))
            out[name.value.decode()] = (launches.value, ms.value)
        return out

    def profile_units(self):
        """{kernel name: elements worked on, summed over its launches} for kernels that run on sub-problems of the call
        (the radix sort passes); kernels that always run over the whole record set are absent."""
        n = self.lib.swg_profile_count(self.handle)
        if n < 0:
            self.check(n)
        out = {}
        for i in range(n):
            name = C.c_char_p()
            launches = C.c_uint64()
            ms = C.c_double()
            units = C.c_uint64()
            self.check(self.lib.swg_profile_get(self.handle, i, C.byref(name), C.byref(launches), C.byref(ms)))
            self.check(self.lib.swg_profile_units(self.handle, i, C.byref(units)))
            if units.value:
                out[name.value.decode()] = units.value
        return out

    def memory_info(self):
        """(arena capacity, high-water mark of the last call) in bytes."""
        cap, peak = C.c_uint64(), C.c_uint64()
        self.check(self.lib.swg_memory_info(self.handle, C.byref(cap), C.byref(peak)))
        return cap.value, peak.value

    def set_memory_limit(self, nbytes):
        """Device bytes one filter call may hold (scratch arena + staged columns); 0 = no limit (the default).  A call that
        does not fit in one piece -- and every call of 2^31 records or more -- is filtered in ranges of whole genome pairs."""
        self.check(self.lib.swg_set_memory_limit(self.handle, C.c_uint64(int(nbytes))))

    def memory_limit(self):
        v = C.c_uint64()
        self.check(self.lib.swg_get_memory_limit(self.handle, C.byref(v)))
        return v.value

    def reserve(self, arena_bytes):
        self.check(self.lib.swg_reserve(self.handle, int(arena_bytes)))

    def warmup(self, n_records_hint=0, n_seq_hint=0, with_scaffold=True):
        """swg_warmup: device memory for about n_records_hint records and the library's code objects, ahead of the first call
        (meant to run on a thread of its own while the input is read)."""
        self.check(self.lib.swg_warmup(self.handle, C.c_uint64(int(n_records_hint)), C.c_uint32(int(n_seq_hint)),
                                       C.c_int(1 if with_scaffold else 0)))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.swg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=0):
    ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = _default_ctx[device] = Context(device)
    return ctx
