// The texts of swg_paf_windows: host code only.  Integers only; the caller divides.
#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"

// One line per window, (sequence, window) ascending as the rows come: the first three columns are a BED line, then the four
// values of the ALL set and the four of the KEPT set.
std::string swg_windows_rows_text(const swg_paf* p, const std::vector<swg_window_row>& rows) {
  std::string o = "#sequence\tstart\tend\tn_all\tdepth_all\tcovered_all\tmatches_all\tn_kept\tdepth_kept\tcovered_kept\tmatches_kept\n";
  for (const swg_window_row& row : rows) {
    o += swg_paf_sequence_name(p, row.seq);
    o += '\t';
    append_u64(o, row.start, '\t');
    append_u64(o, row.end, '\t');
    for (int set = 0; set < 2; ++set) {
      append_u64(o, row.n[set], '\t');
      append_u64(o, row.depth[set], '\t');
      append_u64(o, row.covered[set], '\t');
      append_u64(o, row.matches[set], set ? '\n' : '\t');
    }
  }
  return o;
}

// One line per listed sequence with the length the device call read; the two sets side by side, quantity by quantity.
std::string swg_windows_summary_text(const swg_paf* p, const std::vector<uint32_t>& seq_len, const std::vector<swg_window_seq>& seqs) {
  std::string o =
      "#sequence\tlength\twindows\tempty_all\tempty_kept\tcovered_all\tcovered_kept\tdepth_all\tdepth_kept\tmatches_all\tmatches_kept\trecords_all\trecords_kept\n";
  for (const swg_window_seq& s : seqs) {
    o += swg_paf_sequence_name(p, s.seq);
    o += '\t';
    append_u64(o, seq_len[s.seq], '\t');
    append_u64(o, s.windows, '\t');
    append_u64(o, s.empty[0], '\t');
    append_u64(o, s.empty[1], '\t');
    append_u64(o, s.covered[0], '\t');
    append_u64(o, s.covered[1], '\t');
    append_u64(o, s.depth[0], '\t');
    append_u64(o, s.depth[1], '\t');
    append_u64(o, s.matches[0], '\t');
    append_u64(o, s.matches[1], '\t');
    append_u64(o, s.records[0], '\t');
    append_u64(o, s.records[1], '\n');
  }
  return o;
}
