// The texts of swg_paf_gaps: host code only.
#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"

namespace {

void append_i64(std::string& o, long long v, char sep) {
  if (v < 0) o += '-';
  append_u64(o, v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v, sep);
}

}  // namespace

// One line per row: the row's two intervals under the names of its right record, the kind, then what follows from the row --
// size, dq and dt as signed decimals (an inversion: its query length, 0, 0) -- and the two record numbers.
std::string swg_gaps_rows_text(const swg_paf* p, const swg_records* rec, const std::vector<swg_gap_row>& rows) {
  static const char* const KIND[4] = {"EVEN", "INS", "DEL", "INV"};
  std::string o = "#query\tq_start\tq_end\ttarget\tt_start\tt_end\tkind\tsize\tchain\tdq\tdt\tleft\tright\n";
  for (const swg_gap_row& row : rows) {
    const bool inv = row.kind == SWG_GAP_INV;
    const long long q_len = (long long)row.q_hi - (long long)row.q_lo, t_len = (long long)row.t_hi - (long long)row.t_lo;
    const long long dq = inv ? 0 : (row.flags & 1) ? -q_len : q_len, dt = inv ? 0 : (row.flags & 2) ? -t_len : t_len;
    o += swg_paf_sequence_name(p, rec->q_id[row.right]);
    o += '\t';
    append_u64(o, row.q_lo, '\t');
    append_u64(o, row.q_hi, '\t');
    o += swg_paf_sequence_name(p, rec->t_id[row.right]);
    o += '\t';
    append_u64(o, row.t_lo, '\t');
    append_u64(o, row.t_hi, '\t');
    o += KIND[row.kind & 3];
    o += '\t';
    append_i64(o, inv ? q_len : dq - dt, '\t');
    append_u64(o, row.chain, '\t');
    append_i64(o, dq, '\t');
    append_i64(o, dt, '\t');
    append_u64(o, row.left, '\t');
    append_u64(o, row.right, '\n');
  }
  return o;
}

// One line per genome pair, then the non-empty bins of the spectrum ([2][SWG_GAPS_BINS]: INS, DEL) with their inclusive bounds;
// the last bin takes everything from 2^31 up to the largest |size| there is, 2^33 - 2.
std::string swg_gaps_summary_text(const std::vector<std::string>& genome_name, const std::vector<swg_gap_pair>& pairs, const uint64_t* spectrum) {
  std::string o = "#query_genome\ttarget_genome\tlinks\tins\tins_bases\tdel\tdel_bases\tinv\tinv_bases\n";
  for (const swg_gap_pair& g : pairs) {
    o += genome_name[g.q_genome];
    o += '\t';
    o += genome_name[g.t_genome];
    o += '\t';
    append_u64(o, g.links, '\t');
    append_u64(o, g.n_ins, '\t');
    append_u64(o, g.ins_bases, '\t');
    append_u64(o, g.n_del, '\t');
    append_u64(o, g.del_bases, '\t');
    append_u64(o, g.n_inv, '\t');
    append_u64(o, g.inv_bases, '\n');
  }
  for (int kind = 0; kind < 2; ++kind)
    for (int k = 0; k < SWG_GAPS_BINS; ++k) {
      const uint64_t count = spectrum[kind * SWG_GAPS_BINS + k];
      if (!count) continue;
      o += "#spectrum\t";
      o += kind ? "DEL\t" : "INS\t";
      append_u64(o, k ? uint64_t(1) << (k - 1) : 0, '\t');
      append_u64(o, k == SWG_GAPS_BINS - 1 ? (uint64_t(1) << 33) - 2 : k ? (uint64_t(1) << k) - 1 : 0, '\t');
      append_u64(o, count, '\n');
    }
  return o;
}
