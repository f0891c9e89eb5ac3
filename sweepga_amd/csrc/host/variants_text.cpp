// swg_paf_vcf_write / swg_paf_vcf_text: the variant calls of an open PAF against FASTA records, as VCF 4.2.
// The handle's sequence names are matched to the FASTA records by exact name, the bases of the sequences the set names go to the
// device once per call, host threads find the last cg:Z: tag of every record of the set, the records go to the device in batches of
// bounded CIGAR text (swg_ucsc_plan_batches; swg_variants.hip builds variants, pool and sums), and after the last batch one stable
// device sort by (target sequence, pos) gives the order of the lines: the VCF is sorted per contig and the same bytes for every
// batch size.  One function body, two sinks.  The formatters and the merge need neither a handle nor a device:
// tests/native/variants_text_check.cpp builds this file on its own.
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"
#include "threads.h"

// ';', '=', ',', '%' and bytes <= 0x20 percent-encoded (an INFO value)
void swg_vcf_escape(std::string& o, const char* s) {
  static const char HEX[] = "0123456789ABCDEF";
  for (; *s; ++s) {
    const unsigned char ch = (unsigned char)*s;
    if (ch <= 0x20 || ch == ';' || ch == '=' || ch == ',' || ch == '%') {
      o += '%';
      o += HEX[ch >> 4];
      o += HEX[ch & 15];
    } else {
      o += (char)ch;
    }
  }
}

// sample: the sample column's name, or NULL for a file without genotypes
void swg_vcf_header_text(std::string& o, const std::vector<std::string>& contig_name, const std::vector<uint64_t>& contig_len, const char* sample) {
  o += "##fileformat=VCFv4.2\n##source=sweepga-gpu\n";
  for (size_t s = 0; s < contig_name.size(); ++s) {
    o += "##contig=<ID=";
    o += contig_name[s];
    o += ",length=";
    append_u64(o, contig_len[s], '>');
    o += '\n';
  }
  o += "##INFO=<ID=QNAME,Number=1,Type=String,Description=\"Query sequence\">\n"
       "##INFO=<ID=QSTART,Number=1,Type=Integer,Description=\"0-based position on the forward strand of the query\">\n"
       "##INFO=<ID=QSTRAND,Number=1,Type=String,Description=\"Strand of the query in the mapping\">\n"
       "##INFO=<ID=REC,Number=1,Type=Integer,Description=\"Record of the input, from 0\">\n";
  if (sample) o += "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n";
  o += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO";
  if (sample) {
    o += "\tFORMAT\t";
    o += sample;
  }
  o += '\n';
}

// one line; alleles: the variant's ref_len + alt_len bytes
void swg_vcf_line_text(std::string& o, const char* t_name, const char* q_name, const swg_variant& v, const uint8_t* alleles, bool genotype) {
  o += t_name;
  o += '\t';
  append_u64(o, (uint64_t)v.pos + 1, '\t');
  o += ".\t";
  o.append(reinterpret_cast<const char*>(alleles), v.ref_len);
  o += '\t';
  o.append(reinterpret_cast<const char*>(alleles) + v.ref_len, v.alt_len);
  o += "\t.\t.\tQNAME=";
  swg_vcf_escape(o, q_name);
  o += ";QSTART=";
  append_u64(o, v.q_pos, ';');
  o += v.kind_flags & SWG_VARIANT_MINUS ? "QSTRAND=-;REC=" : "QSTRAND=+;REC=";
  append_u64(o, v.record, genotype ? '\t' : '\n');
  if (genotype) o += "GT\t1\n";
}

void swg_variants_merge_pairs(std::vector<swg_variant_pair>* total, const swg_variant_pair* add, uint64_t n) {
  auto before = [](const swg_variant_pair& a, const swg_variant_pair& b) { return a.q_genome != b.q_genome ? a.q_genome < b.q_genome : a.t_genome < b.t_genome; };
  std::vector<swg_variant_pair> out;
  out.reserve(total->size() + n);
  size_t i = 0;
  uint64_t j = 0;
  while (i < total->size() || j < n) {
    if (j == n || (i < total->size() && before((*total)[i], add[j]))) {
      out.push_back((*total)[i++]);
    } else if (i == total->size() || before(add[j], (*total)[i])) {
      out.push_back(add[j++]);
    } else {  // the same genome pair: the 24 sums behind the two ids
      swg_variant_pair s = (*total)[i++];
      const uint64_t* v = &add[j++].entries;
      uint64_t* d = &s.entries;
      for (int f = 0; f < 24; ++f) d[f] += v[f];
      out.push_back(s);
    }
  }
  total->swap(out);
}

std::string swg_variants_summary_text(const std::vector<std::string>& genome_name, const std::vector<swg_variant_pair>& pairs) {
  std::string o = "#query_genome\ttarget_genome\tentries\tcompared\tsnvs\tA>C\tA>G\tA>T\tC>A\tC>G\tC>T\tG>A\tG>C\tG>T\tT>A\tT>C\tT>G\tsame\tm_equal\tn_columns\t"
                  "ins\tins_bases\tdel\tdel_bases\tlong_indels\tunanchored\tts\ttv\n";
  for (const swg_variant_pair& g : pairs) {
    o += genome_name[g.q_genome];
    o += '\t';
    o += genome_name[g.t_genome];
    o += '\t';
    const uint64_t* v = &g.entries;
    for (int f = 0; f < 24; ++f) append_u64(o, v[f], '\t');
    const uint64_t ts = g.sub[1] + g.sub[5] + g.sub[6] + g.sub[10];  // A>G, C>T, G>A, T>C
    append_u64(o, ts, '\t');
    append_u64(o, g.snvs - ts, '\n');
  }
  return o;
}

namespace {

int host_threads(uint64_t items) {
  return (int)std::min<uint64_t>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())), items / 4096 + 1);
}

// what needs neither a device nor a file; 0 = fine
int refusal(const char* who, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_vcf_options* opts) {
  if (!opts) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL options", who);
  if (opts->set > 1) return swg_alnstats_error(SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (opts->reserved != 0) return swg_alnstats_error(SWG_ERR_INVALID, "%s: reserved must be 0", who);
  if (opts->set == SWG_IV_KEPT && !status) return swg_alnstats_error(SWG_ERR_INVALID, "%s: the kept set needs a status column", who);
  if (!fasta) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL sequences: the calls need the FASTA records", who);
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "%s: the file has a value >= 2^32, its columns are rebased: variants from 64-bit columns are not supported", who);
  const uint32_t G = swg_paf_num_genomes_two(p);
  for (const char* name : {opts->ref_genome, opts->query_genome}) {
    if (!name) continue;
    bool found = false;
    for (uint32_t g = 0; g < G && !found; ++g) {
      const std::string have = swg_paf_genome_two_prefix(p, g);
      found = have == name || have == std::string(name) + "#";
    }
    if (!found && swg_paf_records(p)->n) return swg_alnstats_error(SWG_ERR_INVALID, "%s: unknown genome '%s'", who, name);
  }
  return SWG_OK;
}

uint32_t genome_of(const swg_paf* p, const char* name) {
  if (!name) return SWG_VARIANTS_ANY;
  const uint32_t G = swg_paf_num_genomes_two(p);
  for (uint32_t g = 0; g < G; ++g) {
    const std::string have = swg_paf_genome_two_prefix(p, g);
    if (have == name || have == std::string(name) + "#") return g;
  }
  return SWG_VARIANTS_ANY;
}

struct bases_guard {  // the device block of the bases lives across the batches
  swg_ctx* ctx;
  uint8_t* d = nullptr;
  ~bases_guard() { swg_variant_bases_free(ctx, d); }
};

// vcf: nullptr = the variants are counted and not built; summary: nullptr = not wanted
int paf_vcf(const char* who, swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_vcf_options* opts, swg_ucsc_sink* vcf,
            std::string* summary, swg_vcf_counts* counts) {
  const int refused = refusal(who, p, status, fasta, opts);
  if (refused != SWG_OK) return refused;
  const swg_records* rec = swg_paf_records(p);
  const uint32_t set = opts->set;
  std::vector<uint32_t> sel;  // the records of the set, ascending
  for (uint64_t i = 0; i < rec->n; ++i)
    if (set == SWG_IV_ALL || status[i] != 0) sel.push_back((uint32_t)i);
  const uint64_t k = sel.size();
  swg_vcf_counts c{};
  c.records = k;
  if (k) {
    if (!ctx) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL context", who);
    const uint32_t n_seq = rec->n_seq, G = rec->n_genome_two;
    const uint32_t want_t = genome_of(p, opts->ref_genome), want_q = genome_of(p, opts->query_genome);
    // the sequences the set names, matched by exact name; one whose PAF length differs from the FASTA's is absent
    std::vector<uint32_t> seq_len;
    const int lens = swg_paf_seq_last_lengths(p, &seq_len);
    if (lens != SWG_OK) return lens;
    std::vector<uint8_t> named(n_seq, 0);
    for (uint64_t j = 0; j < k; ++j) named[rec->q_id[sel[j]]] = named[rec->t_id[sel[j]]] = 1;
    std::unordered_map<std::string, uint64_t> by_name;
    const uint64_t n_fasta = swg_fasta_num_records(fasta);
    const uint64_t* f_off = swg_fasta_offsets(fasta);
    const uint8_t* f_bases = swg_fasta_bases(fasta);
    for (uint64_t i = n_fasta; i-- > 0;) by_name[swg_fasta_name(fasta, i)] = i;  // (of two records with one name the first)
    std::vector<const uint8_t*> src(n_seq, nullptr);
    std::vector<uint64_t> src_len(n_seq, 0), seq_offset(n_seq + 1, 0);
    for (uint32_t s = 0; s < n_seq; ++s) {
      if (!named[s]) continue;
      const auto at = by_name.find(swg_paf_sequence_name(p, s));
      if (at == by_name.end()) continue;
      const uint64_t len = f_off[at->second + 1] - f_off[at->second];
      if (len != seq_len[s]) {
        ++c.length_mismatch;
        continue;
      }
      src[s] = f_bases + f_off[at->second], src_len[s] = len;
    }
    bases_guard bases{ctx};
    int rc = swg_variant_bases_upload(ctx, src.data(), src_len.data(), n_seq, seq_offset.data(), &bases.d);
    if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
    const swg_seq_set seqs{seq_offset.data(), bases.d, n_seq, 0};

    const char* paf_text;
    const uint64_t* rec_off;
    const uint32_t* rec_len;
    swg_paf_lines_view(p, &paf_text, &rec_off, &rec_len);
    std::vector<const char*> at(k);
    std::vector<uint64_t> len(k);
    const int threads = host_threads(k);
    swg_host::run(threads, [&](int t) {
      for (uint64_t j = k * t / threads; j < k * (t + 1) / threads; ++j) at[j] = swg_cigar_tag_find(paf_text + rec_off[sel[j]], rec_len[sel[j]], &len[j]);
    });
    for (uint64_t j = 0; j < k; ++j) {
      c.untagged += at[j] == nullptr;
      if (len[j] >> 32) return swg_alnstats_error(SWG_ERR_RANGE, "%s: the CIGAR of record %llu has 2^32 bytes or more", who, (unsigned long long)sel[j]);
    }
    std::vector<uint64_t> first;
    swg_ucsc_plan_batches(len.data(), k, opts->batch_bytes ? opts->batch_bytes : swg_ucsc_default_batch(ctx), &first);
    std::vector<uint32_t> col[6], local;
    std::vector<uint8_t> strand, usable, is_contig(n_seq, 0);
    std::vector<uint64_t> offset;
    std::string cigar_text;
    std::vector<swg_variant> part_variants, variants;  // a batch's, and all of them with the file's record numbers and offsets
    std::vector<uint8_t> part_pool, pool;
    std::vector<swg_variant_pair> pairs, total;
    const uint32_t* const from[6] = {rec->q_id, rec->t_id, rec->q_start, rec->q_end, rec->t_start, rec->t_end};
    for (size_t b = 0; b + 1 < first.size(); ++b) {
      const uint64_t a = first[b], kb = first[b + 1] - a;
      for (auto& v : col) v.resize(kb);
      strand.resize(kb), local.resize(kb), usable.assign(kb, 0), offset.assign(kb + 1, 0);
      for (uint64_t j = 0; j < kb; ++j) {
        const uint32_t r = sel[a + j];
        for (int f = 0; f < 6; ++f) col[f][j] = from[f][r];
        strand[j] = rec->strand[r], local[j] = (uint32_t)j;
        offset[j + 1] = offset[j] + len[a + j];
      }
      cigar_text.resize(offset[kb]);
      const int bt = host_threads(kb);
      swg_host::run(bt, [&](int t) {
        for (uint64_t j = kb * t / bt; j < kb * (t + 1) / bt; ++j)
          if (at[a + j]) std::memcpy(&cigar_text[offset[j]], at[a + j], len[a + j]);
      });
      swg_records part{};
      part.n = kb, part.n_seq = n_seq;
      part.q_id = col[0].data(), part.t_id = col[1].data(), part.q_start = col[2].data(), part.q_end = col[3].data();
      part.t_start = col[4].data(), part.t_end = col[5].data(), part.strand = strand.data();
      const swg_cigar_set cigars{local.data(), offset.data(), cigar_text.data(), kb};
      pairs.resize((size_t)std::min<uint64_t>((uint64_t)G * G, kb));
      // two device passes per batch by design: the first counts (variants, pool bytes, pairs), the second fills arrays of exactly
      // that size -- no guess relates a CIGAR's bytes to its variants (an M op of two bytes can hold nine), and the device's share
      // of a batch is small beside the host's copy and formatting of what it returns
      swg_variant_request req{};
      req.set = SWG_IV_ALL, req.t_genome = want_t, req.q_genome = want_q, req.max_indel = opts->max_indel;
      req.pair_capacity = pairs.size(), req.pairs = pairs.data();
      rc = swg_variant_run(ctx, &part, 2, rec->seq_genome_two, G, nullptr, &cigars, &seqs, &req, usable.data());
      if (rc == SWG_OK && vcf && req.n_variants) {
        if (part_variants.size() < req.n_variants) part_variants.resize(req.n_variants);
        if (part_pool.size() < req.pool_bytes) part_pool.resize(req.pool_bytes);
        req.variant_capacity = part_variants.size(), req.variants = part_variants.data();
        req.pool_capacity = part_pool.size(), req.pool = part_pool.data();
        rc = swg_variant_run(ctx, &part, 2, rec->seq_genome_two, G, nullptr, &cigars, &seqs, &req, usable.data());
      }
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      for (uint64_t j = 0; j < kb; ++j)
        if (usable[j]) is_contig[col[1][j]] = 1;
      if (vcf && req.n_variants) {
        const uint64_t base = pool.size();
        for (uint64_t i = 0; i < req.n_variants; ++i) {
          swg_variant v = part_variants[i];
          v.record = sel[a + v.record];  // (the call numbered the batch's records: the file's number goes out)
          v.allele_offset += base;
          variants.push_back(v);
        }
        pool.insert(pool.end(), part_pool.begin(), part_pool.begin() + (std::ptrdiff_t)req.pool_bytes);
      }
      swg_variants_merge_pairs(&total, pairs.data(), req.n_pairs);
      c.usable += req.usable, c.bad += req.cigar_bad, c.variants += req.n_variants;
      c.no_sequence += req.no_sequence, c.out_of_sequence += req.out_of_sequence;
      ++c.batches;
    }
    for (const swg_variant_pair& g : total) {
      c.snvs += g.snvs, c.n_ins += g.n_ins, c.n_del += g.n_del, c.same += g.same, c.n_columns += g.n_columns, c.m_equal += g.m_equal;
      c.long_indels += g.long_indels, c.unanchored += g.unanchored;
    }
    if (vcf) {
      // the order of the lines: (target sequence, pos), ties in (record, op, column) order -- one stable sort on the device
      const uint64_t nv = variants.size();
      if (nv >> 32) return swg_alnstats_error(SWG_ERR_RANGE, "%s: 2^32 variants or more in one file", who);
      std::vector<uint64_t> keys(nv);
      std::vector<uint32_t> order(nv);
      for (uint64_t i = 0; i < nv; ++i) keys[i] = (uint64_t)rec->t_id[variants[i].record] << 32 | variants[i].pos;
      int seq_bits = 1;
      while (seq_bits < 32 && (n_seq - 1) >> seq_bits) ++seq_bits;
      rc = swg_variant_order(ctx, keys.data(), nv, 32 + seq_bits, order.data());
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      std::vector<std::string> contig_name;
      std::vector<uint64_t> contig_len;
      for (uint32_t s = 0; s < n_seq; ++s)
        if (is_contig[s]) contig_name.push_back(swg_paf_sequence_name(p, s)), contig_len.push_back(seq_len[s]);
      std::string sample;
      if (opts->query_genome) sample = swg_paf_genome_two_prefix(p, want_q);
      std::string head;
      swg_vcf_header_text(head, contig_name, contig_len, opts->query_genome ? sample.c_str() : nullptr);
      vcf->put(head.data(), head.size());
      const bool genotype = opts->query_genome != nullptr;
      const uint64_t CHUNK = uint64_t(1) << 20;  // lines formatted per round: the text of a round is written before the next is made
      for (uint64_t lo = 0; lo < nv; lo += CHUNK) {
        const uint64_t m = std::min(CHUNK, nv - lo);
        const int rt = host_threads(m);
        std::vector<std::string> text(rt);
        swg_host::run(rt, [&](int t) {
          for (uint64_t i = lo + m * t / rt; i < lo + m * (t + 1) / rt; ++i) {
            const swg_variant& v = variants[order[i]];
            swg_vcf_line_text(text[t], swg_paf_sequence_name(p, rec->t_id[v.record]), swg_paf_sequence_name(p, rec->q_id[v.record]), v,
                              pool.data() + v.allele_offset, genotype);
          }
        });
        for (const std::string& s : text) vcf->put(s.data(), s.size());
      }
      if (vcf->failed) return swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
    }
    if (summary) {
      std::vector<std::string> gname(G);
      for (uint32_t g = 0; g < G; ++g) gname[g] = swg_paf_genome_two_prefix(p, g);
      *summary = swg_variants_summary_text(gname, total);
    }
  }
  if (counts) *counts = c;
  return SWG_OK;
}

}  // namespace

extern "C" int swg_paf_vcf_write(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_vcf_options* opts,
                                 const char* vcf_path, const char* summary_path, swg_vcf_counts* counts) {
  static const char* const who = "swg_paf_vcf_write";
  if (!p || (!vcf_path && !summary_path)) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument, or neither file is asked for", who);
  try {
    // (the refusals come before a file is touched; the checks that need no device are the function body's own first step)
    const int refused = refusal(who, p, status, fasta, opts);
    if (refused != SWG_OK) return refused;
    std::FILE* f = nullptr;
    if (vcf_path && !(f = std::fopen(vcf_path, "wb"))) return swg_alnstats_error(SWG_ERR_INVALID, "%s: cannot open %s: %s", who, vcf_path, std::strerror(errno));
    std::FILE* g = nullptr;
    if (summary_path && !(g = std::fopen(summary_path, "wb"))) {
      const int e = errno;
      if (f) std::fclose(f);
      return swg_alnstats_error(SWG_ERR_INVALID, "%s: cannot open %s: %s", who, summary_path, std::strerror(e));
    }
    swg_ucsc_sink sink;
    sink.file = f;
    std::string summary;
    int rc = paf_vcf(who, ctx, p, status, fasta, opts, f ? &sink : nullptr, g ? &summary : nullptr, counts);
    if (g && rc == SWG_OK && !summary.empty() && std::fwrite(summary.data(), 1, summary.size(), g) != summary.size())
      rc = swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
    if (f && std::fclose(f) != 0 && rc == SWG_OK) rc = swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
    if (g && std::fclose(g) != 0 && rc == SWG_OK) rc = swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
    return rc;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_paf_vcf_text(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_vcf_options* opts,
                                swg_vcf_counts* counts, char** vcf_text, uint64_t* vcf_len, char** summary_text, uint64_t* summary_len) {
  static const char* const who = "swg_paf_vcf_text";
  if (vcf_text) *vcf_text = nullptr;
  if (vcf_len) *vcf_len = 0;
  if (summary_text) *summary_text = nullptr;
  if (summary_len) *summary_len = 0;
  if (!p || (!vcf_text && !summary_text) || (vcf_text && !vcf_len) || (summary_text && !summary_len))
    return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument, or neither text is asked for", who);
  try {
    std::string text[2];
    swg_ucsc_sink sink;
    sink.text = &text[0];
    const int rc = paf_vcf(who, ctx, p, status, fasta, opts, vcf_text ? &sink : nullptr, summary_text ? &text[1] : nullptr, counts);
    if (rc != SWG_OK) return rc;
    const bool wanted[2] = {vcf_text != nullptr, summary_text != nullptr};
    char* out[2] = {nullptr, nullptr};
    uint64_t len[2] = {0, 0};
    const int handed = texts_hand_over(text, wanted, 2, out, len);
    if (handed != SWG_OK) return handed;
    if (vcf_text) *vcf_text = out[0], *vcf_len = len[0];
    if (summary_text) *summary_text = out[1], *summary_len = len[1];
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
