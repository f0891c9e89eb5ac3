// FASTA input of `--joblist` (src/main.rs:791-830 names, :963-990 sequences), records numbered across the files in order.
//
// Literal to the reference's line loop (BufRead::lines, then str::trim on sequence lines):
//   - a line is split at '\n'; a "\r\n" ending loses its '\r'; a last line without '\n' still counts;
//   - a line starting with '>' opens a record; its name is the first whitespace-separated token after the '>';
//   - every other line is trimmed and appended to the current record -- lines BEFORE the first header are kept too and end
//     up in front of the first record's sequence (the buffer is only taken at the second header);
//   - whitespace is the ASCII set of char::is_whitespace (\t \n \v \f \r space).  The reference also trims non-ASCII
//     Unicode spaces and refuses input that is not UTF-8; neither is done here.
// Text comes from the same loader as the PAF reader: mmap for plain files, parallel BGZF inflation for .gz / .bgz.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"

struct swg_fasta {
  std::vector<std::string> names;
  std::vector<int> file;
  std::vector<uint64_t> offsets;  // n + 1
  std::vector<uint8_t> bases;
};

namespace {

thread_local std::string g_fasta_error;

int fasta_error(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_fasta_error = buf;
  return code;
}

inline bool ws(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); }

}  // namespace

// One file's text into f (records appended; f->offsets holds record STARTS until swg_fasta_open closes the list).
void swg_fasta_parse_text(const char* p, size_t n, int file_index, swg_fasta* f) {
  const size_t file_start = f->bases.size();
  bool open = false;  // a header of this file has been seen (have_current, main.rs:973)
  size_t pos = 0;
  while (pos < n) {
    const char* nl = static_cast<const char*>(std::memchr(p + pos, '\n', n - pos));
    const size_t end = nl ? (size_t)(nl - p) : n;
    size_t e = end;
    if (nl && e > pos && p[e - 1] == '\r') --e;  // "\r\n"
    if (e > pos && p[pos] == '>') {
      size_t a = pos + 1;
      while (a < e && ws((unsigned char)p[a])) ++a;
      size_t b = a;
      while (b < e && !ws((unsigned char)p[b])) ++b;
      f->names.emplace_back(p + a, b - a);
      f->file.push_back(file_index);
      // the first record of the file keeps the lines before it (cur is not cleared at the first header)
      f->offsets.push_back(open ? f->bases.size() : file_start);
      open = true;
    } else {
      size_t a = pos, b = e;
      while (a < b && ws((unsigned char)p[a])) ++a;
      while (b > a && ws((unsigned char)p[b - 1])) --b;
      f->bases.insert(f->bases.end(), p + a, p + b);
    }
    pos = nl ? end + 1 : n;
  }
  if (!open) f->bases.resize(file_start);  // no record: the buffer is never pushed
}

// detect_file_type (src/main.rs:115-170): the first line that is neither empty nor '#'-led after trimming starts with '>'
bool swg_fasta_text_is_fasta(const char* p, size_t n) {
  size_t pos = 0;
  while (pos < n) {
    const char* nl = static_cast<const char*>(std::memchr(p + pos, '\n', n - pos));
    const size_t end = nl ? (size_t)(nl - p) : n;
    size_t a = pos;
    while (a < end && ws((unsigned char)p[a])) ++a;
    if (a < end && p[a] != '#') return p[a] == '>';
    pos = nl ? end + 1 : n;
  }
  return false;
}

extern "C" int swg_fasta_open(const char* const* paths, int n_paths, int threads, swg_fasta** out) {
  if (!out || n_paths < 0 || (n_paths && !paths)) return fasta_error(SWG_ERR_INVALID, "swg_fasta_open: bad argument");
  *out = nullptr;
  swg_fasta* f = new (std::nothrow) swg_fasta;
  if (!f) return fasta_error(SWG_ERR_OOM, "host allocation failed");
  try {
    for (int i = 0; i < n_paths; ++i) {
      const char* data = nullptr;
      size_t len = 0;
      void* h = nullptr;
      if (!paths[i]) {
        delete f;
        return fasta_error(SWG_ERR_INVALID, "swg_fasta_open: NULL path");
      }
      const int rc = swg_host_text_load(paths[i], threads, &data, &len, &h);
      if (rc != SWG_OK) {
        delete f;
        return fasta_error(rc, "%s", swg_paf_last_error());
      }
      swg_fasta_parse_text(data, len, i, f);
      swg_host_text_release(h);
    }
    f->offsets.push_back(f->bases.size());
  } catch (...) {
    delete f;
    return fasta_error(SWG_ERR_OOM, "out of host memory reading FASTA");
  }
  *out = f;
  return SWG_OK;
}

extern "C" void swg_fasta_close(swg_fasta* f) { delete f; }
extern "C" uint64_t swg_fasta_num_records(const swg_fasta* f) { return f ? f->names.size() : 0; }
extern "C" const char* swg_fasta_name(const swg_fasta* f, uint64_t i) { return f && i < f->names.size() ? f->names[i].c_str() : nullptr; }
extern "C" int swg_fasta_file_index(const swg_fasta* f, uint64_t i) { return f && i < f->file.size() ? f->file[i] : -1; }
extern "C" const uint64_t* swg_fasta_offsets(const swg_fasta* f) { return f ? f->offsets.data() : nullptr; }
extern "C" const uint8_t* swg_fasta_bases(const swg_fasta* f) { return f ? f->bases.data() : nullptr; }
extern "C" const char* swg_fasta_last_error(void) { return g_fasta_error.c_str(); }
