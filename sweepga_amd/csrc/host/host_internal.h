// Shared by the host translation units of libsweepga_gpu.so; not part of the C ABI.
#ifndef SWG_HOST_INTERNAL_H
#define SWG_HOST_INTERNAL_H
#include <cstddef>
#include <cstdint>

// open_paf_input (src/paf.rs:10-30): the whole input as text -- mmap for plain files, parallel BGZF / serial gzip
// inflate for .gz/.bgz (or the gzip magic), "-" = stdin.  *handle owns the bytes until swg_host_text_release.
// Errors: negative code, text in swg_paf_last_error().
int swg_host_text_load(const char* path, int threads, const char** data, size_t* len, void** handle);
void swg_host_text_release(void* handle);

// ---- --joblist (fasta_io.cpp, swg_mash.hip, mash_host.cpp) ----
struct swg_ctx;
struct swg_fasta;
int swg_set_error(swg_ctx* ctx, int code, const char* fmt, ...);
// detect_file_type's FASTA test over text already loaded
bool swg_fasta_text_is_fasta(const char* p, size_t n);
// the sketch of swg_mash_sketch, handed over contig by contig: emit(user, contig, ascending values, count), in contig order
int swg_mash_sketch_each(swg_ctx* ctx, const uint8_t* seq, const uint64_t* offsets, uint64_t n_seq, int k, uint64_t s,
                         void (*emit)(void*, uint64_t, const uint64_t*, uint64_t), void* user, double* timing_ms);
#endif
