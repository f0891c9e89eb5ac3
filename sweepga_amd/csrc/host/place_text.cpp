// The texts of swg_paf_place: host code only.
#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"

namespace {

void append_i64(std::string& o, long long v, char sep) {
  if (v < 0) o += '-';
  append_u64(o, v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v, sep);
}

}  // namespace

// One line per row, in the rows' (layout) order: the placed sequence and its partner under the handle's names with the lengths
// the device call read, then the decision.  end = start + length; both are signed.
std::string swg_place_rows_text(const swg_paf* p, const std::vector<uint32_t>& seq_len, const std::vector<swg_placement>& rows) {
  std::string o =
      "#sequence\tlength\tpartner\tpartner_length\torient\tstart\tend\trank\tbases\tfwd\trev\ttotal\trunner\trecords\tq_lo\tq_hi\tt_lo\tt_hi\n";
  for (const swg_placement& row : rows) {
    const uint32_t length = seq_len[row.seq];
    o += swg_paf_sequence_name(p, row.seq);
    o += '\t';
    append_u64(o, length, '\t');
    o += swg_paf_sequence_name(p, row.partner);
    o += '\t';
    append_u64(o, seq_len[row.partner], '\t');
    o += row.orient ? "-\t" : "+\t";
    append_i64(o, row.start, '\t');
    append_i64(o, row.start + (long long)length, '\t');
    append_u64(o, row.rank, '\t');
    append_u64(o, row.bases, '\t');
    append_u64(o, row.fwd, '\t');
    append_u64(o, row.rev, '\t');
    append_u64(o, row.total_bases, '\t');
    append_u64(o, row.runner_bases, '\t');
    append_u64(o, row.n_records, '\t');
    append_u64(o, row.q_lo, '\t');
    append_u64(o, row.q_hi, '\t');
    append_u64(o, row.t_lo, '\t');
    append_u64(o, row.t_hi, '\n');
  }
  return o;
}

std::string swg_place_summary_text(const std::vector<std::string>& genome_name, const std::vector<swg_place_pair>& pairs) {
  std::string o = "#genome\tpartner_genome\tsequences\treversed\tlength\tbases\ttotal_bases\n";
  for (const swg_place_pair& g : pairs) {
    o += genome_name[g.genome];
    o += '\t';
    o += genome_name[g.partner_genome];
    o += '\t';
    append_u64(o, g.rows, '\t');
    append_u64(o, g.reversed, '\t');
    append_u64(o, g.length, '\t');
    append_u64(o, g.bases, '\t');
    append_u64(o, g.total_bases, '\n');
  }
  return o;
}
