// quant_write.hip -- the row section of a quant.sf file (GZipWriter::writeAbundances, src/GZipWriter.cpp:234-245) formatted on the
// device from the columns where they lie: sfgpu_quant_write_text.  Row r is
//     name \t Length \t %g(eff) \t %g(tpm) \t %g(num_reads) \n
// with %g as printf prints a double with six significant digits (gfmt.h: exact, ties to even on the binary value).
// The kernels (cell decode, row sizes and scan, the 4 KB-tile LDS formatter) and the driver are rowtext.h's, which genes.hip
// instantiates for quant.genes.sf as well; this file is the instance whose first numeric column is the integer Length and whose
// row r takes name r.
#include "rowtext.h"

using namespace sfgpu;

extern "C" int sfgpu_quant_write_text(const char* d_names, const uint64_t* d_name_off, const uint32_t* d_length, const double* d_eff,
                                      const double* d_tpm, const double* d_num_reads, uint64_t n_rows, uint64_t chunk_bytes,
                                      sfgpu_text_sink sink, void* user, sfgpu_quant_write_result* out, sfgpu_stream stream) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_quant_write_text: null result");
    memset(out, 0, sizeof(*out));
    if (chunk_bytes == 0) chunk_bytes = rowtext::kDefaultChunk;
    SF_REQUIRE(chunk_bytes >= 16 && chunk_bytes <= rowtext::kMaxChunk, SFGPU_ERR_INVALID,
               "sfgpu_quant_write_text: chunk_bytes must lie in [16, 2^30] (0 = default)");
    if (n_rows == 0) return SFGPU_OK;
    SF_REQUIRE(d_name_off && d_length && d_eff && d_tpm && d_num_reads, SFGPU_ERR_INVALID, "sfgpu_quant_write_text: null column");
    SF_REQUIRE(n_rows < rowtext::kMaxRows, SFGPU_ERR_RANGE, "sfgpu_quant_write_text: n_rows must be below 2^32 - 1");
    const rowtext::Cols cols = {{d_eff, d_tpm, d_num_reads, nullptr}};
    return rowtext::write_rows<false>("sfgpu_quant_write_text", d_names, d_name_off, n_rows, d_length, cols, n_rows, chunk_bytes, sink, user,
                                      out, stream);
}
