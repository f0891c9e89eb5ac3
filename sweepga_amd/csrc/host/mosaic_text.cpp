// The texts of swg_paf_mosaic: host code only.
#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"

// Text 0, BED-like: the row first, then the record that won it -- its other sequence, strand, number, weight and its whole
// interval on the other sequence.  The first three columns with any label make a --lift-regions input.
std::string swg_mosaic_rows_text(const swg_paf* p, const swg_records* rec, const std::vector<swg_mosaic_row>& rows, uint32_t axis, bool by_length) {
  std::string o;
  const uint32_t* other_id = axis ? rec->q_id : rec->t_id;
  const uint32_t *own_start = axis ? rec->t_start : rec->q_start, *own_end = axis ? rec->t_end : rec->q_end;
  const uint32_t *other_start = axis ? rec->q_start : rec->t_start, *other_end = axis ? rec->q_end : rec->t_end;
  for (const swg_mosaic_row& row : rows) {
    const uint32_t r = row.record;
    o += swg_paf_sequence_name(p, row.seq);
    o += '\t';
    append_u64(o, row.start, '\t');
    append_u64(o, row.end, '\t');
    o += swg_paf_sequence_name(p, other_id[r]);
    o += '\t';
    o += rec->strand && rec->strand[r] ? '-' : '+';
    o += '\t';
    append_u64(o, r, '\t');
    append_u64(o, by_length ? own_end[r] - own_start[r] : rec->matches[r], '\t');
    append_u64(o, other_start[r], '\t');
    append_u64(o, other_end[r], '\n');
  }
  return o;
}

std::string swg_mosaic_share_text(const std::vector<std::string>& genome_name, const std::vector<uint64_t>& share, uint64_t bases) {
  std::string o = "genome\tother_genome\tbases\n";
  const size_t G = genome_name.size();
  for (size_t g = 0; g < G && share.size() == G * G; ++g)
    for (size_t h = 0; h < G; ++h) {
      const uint64_t v = share[g * G + h];
      if (!v) continue;
      o += genome_name[g];
      o += '\t';
      o += genome_name[h];
      o += '\t';
      append_u64(o, v, '\n');
    }
  o += "#total\t";
  append_u64(o, bases, '\n');
  return o;
}
