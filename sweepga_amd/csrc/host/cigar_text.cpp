// The two text helpers of swg_paf_lift_exact that need neither a handle nor a device: the finder of a line's
// last cg:Z: tag and the formatter of one exact row.  tests/native/cigar_text_check.cpp builds this file on its own.
#include <cstdint>
#include <cstring>
#include <string>

#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"

// A PAF line's tags are its tab-separated fields behind the twelfth.  A field is THE tag when it begins with `cg:Z:`; the value runs
// to the next tab or to the line's end (a '\r' there is no part of it).  Several: the last one counts, as in the parser's identity
// override.  The bytes `cg:Z:` inside another field's value are no tag.
const char* swg_cigar_tag_find(const char* line, uint64_t len, uint64_t* value_len) {
  *value_len = 0;
  if (len && line[len - 1] == '\n') --len;
  if (len && line[len - 1] == '\r') --len;
  const char* found = nullptr;
  const char* const end = line + len;
  const char* f = line;
  for (int field = 0; f <= end; ++field) {
    const char* tab = f < end ? static_cast<const char*>(std::memchr(f, '\t', (size_t)(end - f))) : nullptr;
    const char* fe = tab ? tab : end;
    if (field >= 12 && fe - f >= 5 && std::memcmp(f, "cg:Z:", 5) == 0) {
      found = f + 5;
      *value_len = (uint64_t)(fe - found);
    }
    if (!tab) break;
    f = tab + 1;
  }
  return found;
}

void swg_lift_exact_row_text(std::string& o, const char* dst_name, const std::string& label, const std::string& src_name, const swg_lift_exact_row& w) {
  o += dst_name;
  o += '\t';
  append_u64(o, w.dst_start, '\t');
  append_u64(o, w.dst_end, '\t');
  o += label;
  o += '\t';
  o += src_name;
  o += '\t';
  append_u64(o, w.src_start, '\t');
  append_u64(o, w.src_end, '\t');
  o += w.flags & SWG_LIFT_MINUS ? "-\t" : "+\t";
  o += w.flags & SWG_LIFT_ON_TARGET ? "t\t" : "q\t";
  append_u64(o, w.record, '\t');
  append_u64(o, w.aligned, '\t');
  append_u64(o, w.matches, '\t');
  o += w.flags & SWG_LIFT_EXACT ? "exact\n" : "interp\n";
}
