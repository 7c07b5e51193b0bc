// aligng_harness.cpp -- csrc/aligngfmt.h alone, as plain C++ (g++ -Wall -Wextra -Werror): the alignment rule in plain loops
// (ag_job_serial: the whole matrix, a list of columns, trimmed and merged) and as a group of lanes runs it (vg_band_group into
// scratch words, ag_walk over them twice: counting, then writing each run to its place), over whole batches.
// tests/test_aligng_cpu.py compares both with hits.align_hits_host.  Built with -DALIGNG_HARNESS_MAIN (and
// -fsanitize=address,undefined) it is a stand-alone program: it reads cases with their expected results from a file
// (tests/aligng_corpus.py: blob) and runs both forms over them; every text is copied to a block of its own size first
// (vf_each_job), and a job's scratch and operations are blocks of exactly their size, so a byte outside any of them is a
// sanitizer report.  agh_write runs the serial writers of csrc/samwfmt.h / csrc/bamwfmt.h (samw_serial, bamw_serial) with an
// alignment handed in, for the comparison with samfile._sam_text(alignments=) and sam_to_bam of it; the per-unit sizes the kernels
// take are cross-checked against the serial pass on the way.
#include "aligngfmt.h"
#include "bamwfmt.h"

#include <cstdio>
#include <cstring>

using namespace sfgpu;

extern "C" {

// the whole pass; lanes = 0: the plain loops, else as the kernel lays it out.  pos, nm: 2 n entries; op_off: 2 n + 1; extra: 6 n
// (clipped, trimmed D, edits per slot); ops: room for cap_ops words.  -> the words needed (nothing but them is reported where they
// exceed cap_ops), or -(1 + the lowest record with tid >= M)
int64_t agh_align(const char* tseq, const uint64_t* tseq_off, const uint32_t* tlen, uint64_t M, const char* seq1, const uint64_t* off1, const char* seq2,
                  const uint64_t* off2, uint32_t n_reads, const sfgpu_hit* hits, const uint32_t* hit_off, uint32_t k, int lanes, int32_t* pos, uint32_t* nm,
                  uint64_t* op_off, uint32_t* ops, uint64_t cap_ops, uint64_t* extra, sfgpu_align_gstats* stats) {
    std::vector<int32_t> p; std::vector<uint32_t> n, o; std::vector<uint64_t> off, x;
    const uint64_t bad = ag_serial_align(tseq, tseq_off, tlen, M, seq1, off1, seq2, off2, n_reads, hits, hit_off, k, lanes != 0, &p, &n, &off, &o, &x, stats);
    if (bad) return -(int64_t)bad;
    if (o.size() > cap_ops) return (int64_t)o.size();
    if (!p.empty()) { memcpy(pos, p.data(), p.size() * 4); memcpy(nm, n.data(), n.size() * 4); memcpy(extra, x.data(), x.size() * 8); }
    if (!o.empty()) memcpy(ops, o.data(), o.size() * 4);
    memcpy(op_off, off.data(), off.size() * 8);
    return (int64_t)o.size();
}

// the arrays of sfgpu_sam_write_text / sfgpu_sam_write_bgzf (host pointers; QNAME r<index>, no qualities).  out[0 .. 8):
// n_bytes, n_lines, n_units, max_unit_bytes, error_kind, error_read, error_record, 1 when the per-unit sizes disagree; bytes !=
// nullptr (room for the n_bytes a first call gave): the text or the records.  -> the error kind
int agh_write(int bam, const void* hits, const uint32_t* hit_off, uint32_t n_reads, int paired, const char* ref, const uint64_t* ref_off, uint32_t n_refs,
              const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2, const int64_t* s2_off, int oriented, const int32_t* aln_pos,
              const uint64_t* aln_op_off, const uint32_t* aln_ops, uint64_t* out, uint8_t* bytes) {
    SamwArgs a = {static_cast<const sfgpu_hit*>(hits), hit_off, n_reads, paired, ref, ref_off, n_refs, nullptr, nullptr, s1, s1_off,
                  paired ? s2 : nullptr, paired ? s2_off : nullptr, 0};
    a.oriented = oriented; a.aln_pos = aln_pos; a.aln_op_off = aln_op_off; a.aln_ops = aln_ops;
    SamwSerial res;
    const int kind = bam ? bamw_serial(a, nullptr, &res) : samw_serial(a, nullptr, &res);
    uint64_t sum = 0, longest = 0, units = 0;
    auto unit = [&](uint64_t len) { sum += len; ++units; if (len > longest) longest = len; };
    for (uint64_t r = 0; !kind && r < a.n_reads; ++r) {
        const uint64_t h0 = a.hit_off[r], h1 = a.hit_off[r + 1];
        if (h0 == h1) unit(bam ? bamw_unit_len(a, r, nullptr, 0) : samw_unit_len(a, r, nullptr, 0));
        for (uint64_t h = h0; h < h1; ++h) {
            const sfgpu_hit copy = a.hits[h];                      // (as the kernels hold it: a copy and the record's index)
            unit(bam ? bamw_unit_len(a, r, &copy, h - h0, h) : samw_unit_len(a, r, &copy, h - h0, h));
        }
    }
    out[0] = res.n_bytes; out[1] = res.n_lines; out[2] = res.n_units; out[3] = res.max_unit_bytes;
    out[4] = (uint64_t)kind; out[5] = res.error_read; out[6] = res.error_record;
    out[7] = !kind && (sum != res.n_bytes || longest != res.max_unit_bytes || units != res.n_units);
    if (kind || !bytes) return kind;
    SamwSerial again;
    const int k2 = bam ? bamw_serial(a, bytes, &again) : samw_serial(a, reinterpret_cast<char*>(bytes), &again);
    if (k2 || again.n_bytes != res.n_bytes) out[7] = 1;
    return k2;
}

}

#ifdef ALIGNG_HARNESS_MAIN
#include "hit_harness.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t n_cases = 0, hd[9];
    while (fread(hd, 8, 9, f) == 9) {
        const uint64_t n_rec = hd[5], n_words = hd[7];
        HarnessBatch b; std::vector<uint64_t> want_off, want_extra, want_stats; std::vector<uint32_t> want_nm, want_ops; std::vector<int32_t> want_pos;
        if (!b.read(f, hd, 6) || !take(f, &want_pos, 2 * n_rec) || !take(f, &want_nm, 2 * n_rec) || !take(f, &want_off, 2 * n_rec + 1) ||
            !take(f, &want_ops, n_words) || !take(f, &want_extra, 6 * n_rec) || !take(f, &want_stats, 6)) { fprintf(stderr, "case %llu: short file\n", (unsigned long long)n_cases); return 2; }
        for (int lanes = 0; lanes < 2; ++lanes) {
            std::vector<int32_t> p; std::vector<uint32_t> n, o; std::vector<uint64_t> off, x; sfgpu_align_gstats st;
            const uint64_t bad = ag_serial_align(b.ts.data(), b.toff.data(), b.tl.data(), b.M, b.s1.data(), b.o1.data(), b.paired ? b.s2.data() : nullptr, b.paired ? b.o2.data() : nullptr,
                                                  (uint32_t)b.n_reads, b.hits.data(), b.hoff.data(), (uint32_t)hd[8], lanes != 0, &p, &n, &off, &o, &x, &st);
            const uint64_t got_stats[6] = {st.jobs, st.jobs_traced, st.unalignable, st.sum_nm, st.words, st.scratch_bytes};
            const bool ok = !bad && p == want_pos && n == want_nm && off == want_off && o == want_ops && x == want_extra && !memcmp(got_stats, want_stats.data(), sizeof got_stats);
            if (!ok) { fprintf(stderr, "case %llu (%s): differs from the statement\n", (unsigned long long)n_cases, lanes ? "lanes" : "serial"); return 1; }
        }
        ++n_cases;
    }
    fclose(f);
    printf("aligng harness ok: %llu cases\n", (unsigned long long)n_cases);
    return 0;
}
#endif
