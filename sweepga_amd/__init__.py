"""sweepga_amd: MI355X-native plane-sweep / scaffold filter (drop-in for sweepga's filter path).

The product is libsweepga_gpu.so (hand-written HIP for gfx950, C ABI in include/sweepga_gpu.h);
this package is the thin host-side mirror of the reference's filter interface over that ABI.
"""
from ._lib import Context, SwgError, K_INF, default_context, load  # noqa: F401
from .filter import (ChainStatus, FilterConfig, FilterMode, PafFilter, PlaneSweepMapping, RecordMeta,  # noqa: F401
                     ScoringFunction, SequenceIndex, pack_records, stream_plan, plane_sweep_both, plane_sweep_query,
                     plane_sweep_target, USIZE_MAX, UnionFind, merge_mappings_into_chains, plane_sweep_scaffolds)
from .paf import PafFile  # noqa: F401
from .aln import AlnRecords  # noqa: F401
from .alnstats import AlnStats  # noqa: F401
from .blocks import BLOCK_DTYPE, Blocks, blocks_records, blocks_records_device  # noqa: F401
from .components import (COMPONENT_DTYPE, LINK_DTYPE, Components, components_records,  # noqa: F401
                         components_records_device)
from .breadth import BREADTH_PAIR_DTYPE, Breadth, breadth_records, breadth_records_device  # noqa: F401
from .intervals import INTERVAL_DTYPE, Intervals, intervals_records, intervals_records_device  # noqa: F401
from .sharing import RUN_DTYPE, Sharing, sharing_records, sharing_records_device  # noqa: F401
from .mosaic import ROW_DTYPE, Mosaic, mosaic_records, mosaic_records_device  # noqa: F401
from .gaps import Gaps, GapsResult, gaps_records, gaps_records_device  # noqa: F401  (its ROW_DTYPE / PAIR_DTYPE: sweepga_amd.gaps)
from .place import Place, PlaceResult, place_records, place_records_device  # noqa: F401  (its ROW_DTYPE / PAIR_DTYPE: sweepga_amd.place)
from .windows import Windows, WindowsResult, windows_records, windows_records_device  # noqa: F401  (its ROW_DTYPE / SEQ_DTYPE: sweepga_amd.windows)
from .dotplot import Dotplot, DotplotResult, dotplot_records, dotplot_records_device  # noqa: F401
from .lift import Lift, LiftClosure, LiftClosureResult, LiftResult, lift_closure_records, lift_closure_records_device, lift_records, lift_records_device  # noqa: F401
from .lift import LiftExactResult, lift_exact_records, lift_exact_records_device, lift_hit_records, lift_hit_records_device  # noqa: F401
from .lift import LiftPaf, LiftSliceResult, lift_slice_records, lift_slice_records_device  # noqa: F401  (its SLICE_DTYPE: sweepga_amd.lift)
from .ucsc import UcscChain, UcscResult, ucsc_chain_records, ucsc_chain_records_device  # noqa: F401  (its CHAIN_DTYPE / BLOCK_DTYPE: sweepga_amd.ucsc)
from .diffs import Diffs, DiffsResult, diff_records, diff_records_device  # noqa: F401  (its ROW_DTYPE / PAIR_DTYPE: sweepga_amd.diffs)
from .divergence import Divergence, DivergenceResult, divergence_records, divergence_records_device  # noqa: F401  (its ROW_DTYPE / SEQ_DTYPE: sweepga_amd.divergence)
from .variants import VARIANT_DTYPE, Variants, VariantsResult, variant_records, variant_records_device  # noqa: F401  (its PAIR_DTYPE: sweepga_amd.variants)
from .eqx import EQX_ENTRY_DTYPE, Eqx, EqxResult, eqx_records, eqx_records_device  # noqa: F401
from .maf import MAF_BLOCK_DTYPE, Maf, MafResult, maf_records, maf_records_device  # noqa: F401
from .ani import (AniMethod, AniMethodKind, NSort, calculate_ani_stats, parse_ani_method,  # noqa: F401
                  parse_identity_value)

__version__ = "0.1.0"
