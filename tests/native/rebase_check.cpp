// Runs the host rebasing of sweepga_amd/csrc/host/rebase.h on its own, case after case (host code only, no GPU;
// tests/test_wide_edges_cpu.py writes the cases and checks every output against tests/wide_model.py -- this file holds no
// reference logic, only the order in which a caller of rebase.h uses its functions, as swg_rebase_host does):
//   rebase_check <case list> <directory> <threads>
// The case list is text, one case per line: `<name> n=<records> n_seq=<sequences> n_genome=<genomes>`.  Inputs are raw
// little-endian arrays in <directory>: <name>.q_id, <name>.t_id (u32[n]), <name>.c0 .. <name>.c5 (u64[n]: q_start, q_end, t_start,
// t_end, matches, block_len) and <name>.genome (u32[n_seq], the seq_genome_last table).  One line per case goes to stdout:
//   case <name> answer=<ok|range|invalid> kind=<seq|axis|-> record=<index> field=<0..5|->
// and for an accepted case the outputs go to <directory>: <name>.o0 .. <name>.o5 (u32[n]), <name>.lo (u64[n_seq], kind=seq) or
// <name>.off_q / <name>.off_t (u64[n], kind=axis).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../sweepga_amd/csrc/host/rebase.h"

namespace {

[[noreturn]] void die(const std::string& what) {
  fprintf(stderr, "rebase_check: %s\n", what.c_str());
  exit(2);
}

template <class T>
std::vector<T> read_array(const std::string& path, uint64_t count) {
  std::vector<T> v(count);
  std::ifstream f(path, std::ios::binary);
  if (!f) die("cannot open " + path);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)));
  if ((uint64_t)f.gcount() != count * sizeof(T)) die("short file " + path);
  return v;
}
template <class T>
void write_array(const std::string& path, const std::vector<T>& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  if (!f) die("cannot write " + path);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) die("usage: rebase_check <case list> <directory> <threads>");
  const std::string dir = std::string(argv[2]) + "/";
  const int threads = atoi(argv[3]);
  std::ifstream list(argv[1]);
  if (!list) die(std::string("cannot open ") + argv[1]);
  std::string line;
  while (std::getline(list, line)) {
    std::istringstream ls(line);
    std::string name, kv;
    if (!(ls >> name)) continue;
    std::map<std::string, uint64_t> arg;
    while (ls >> kv) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos) die("bad argument " + kv);
      arg[kv.substr(0, eq)] = strtoull(kv.c_str() + eq + 1, nullptr, 10);
    }
    const uint64_t n = arg["n"];
    const uint32_t n_seq = (uint32_t)arg["n_seq"], n_genome = (uint32_t)arg["n_genome"];
    const std::string base = dir + name;
    const std::vector<uint32_t> q_id = read_array<uint32_t>(base + ".q_id", n), t_id = read_array<uint32_t>(base + ".t_id", n);
    const std::vector<uint32_t> genome = read_array<uint32_t>(base + ".genome", n_seq);
    std::vector<std::vector<uint64_t>> in(6);
    std::vector<std::vector<uint32_t>> out(6);
    const uint64_t* c64[6];
    uint32_t* c32[6];
    for (int f = 0; f < 6; ++f) {
      in[f] = read_array<uint64_t>(base + ".c" + std::to_string(f), n);
      out[f].assign(n, 0xdeadbeefu);
      c64[f] = in[f].data();
      c32[f] = out[f].data();
    }
    std::vector<uint64_t> lo(n_seq, 0), off_q, off_t;
    const char* kind = "seq";
    swg_rebase::Result r = swg_rebase::columns(n, q_id.data(), t_id.data(), c64, n_seq, threads, c32, lo.data());
    if (!r.ok && r.bad_field < 4 && swg_rebase::axis_tables_fit(n_seq, n_genome)) {
      r = swg_rebase::genome_entries(n, q_id.data(), t_id.data(), genome.data(), n_genome);
      if (r.ok) {
        kind = "axis";
        off_q.assign(n, 0);
        off_t.assign(n, 0);
        r = swg_rebase::columns_by_axis(n, q_id.data(), t_id.data(), c64, n_seq, genome.data(), n_genome, threads, c32, off_q.data(),
                                        off_t.data());
      }
    }
    if (r.ok) {
      printf("case %s answer=ok kind=%s record=0 field=-\n", name.c_str(), kind);
      for (int f = 0; f < 6; ++f) write_array(base + ".o" + std::to_string(f), out[f]);
      if (kind[0] == 's') {
        write_array(base + ".lo", lo);
      } else {
        write_array(base + ".off_q", off_q);
        write_array(base + ".off_t", off_t);
      }
    } else if (r.bad_field == 6) {
      printf("case %s answer=invalid kind=- record=%llu field=-\n", name.c_str(), (unsigned long long)r.bad_record);
    } else {
      printf("case %s answer=range kind=- record=%llu field=%d\n", name.c_str(), (unsigned long long)r.bad_record, r.bad_field);
    }
    fflush(stdout);
  }
  return 0;
}
