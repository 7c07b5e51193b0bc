// mdtag_harness.cpp -- csrc/mdfmt.h alone, as plain C++ (g++ -Wall -Wextra -Werror): the NM / MD rule column by column
// (md_slot_serial) and as a group of 16 lanes runs it (md_slot_lanes: 16-byte windows, mismatch masks, the segmented scan, every
// token placed from its lane's offset; counting, then writing), over whole batches.  tests/test_mdtag_cpu.py compares both with
// hits.md_tags_host.  Built with -DMDTAG_HARNESS_MAIN (and -fsanitize=address,undefined) it is a stand-alone program: it reads cases
// with their expected results from a file (tests/mdtag_corpus.py: blob) and runs both forms over them; every text is copied to a
// block of its own size first (vf_each_job) and a slot's MD is a block of exactly its size, so a byte outside any of them is a
// sanitizer report.
#include "mdfmt.h"
#include "bamwfmt.h"

#include <cstdio>
#include <cstring>

using namespace sfgpu;

extern "C" {

// the whole pass; lanes = 0: column by column, else as a group of `lanes` lanes.  nm: 2 n entries; md_off: 2 n + 1; md: room for
// cap_md bytes; stats: 5 words (sfgpu_mdtag_stats).  aln_pos == nullptr: no alignment.  -> the MD bytes needed (nothing but them is
// reported where they exceed cap_md), or -(1 + the lowest record with tid >= M)
int64_t mdh_tags(const char* tseq, const uint64_t* tseq_off, const uint32_t* tlen, uint64_t M, const char* seq1, const uint64_t* off1, const char* seq2,
                 const uint64_t* off2, uint32_t n_reads, const sfgpu_hit* hits, const uint32_t* hit_off, const int32_t* aln_pos, const uint64_t* aln_op_off,
                 const uint32_t* aln_ops, uint32_t lanes, uint32_t* nm, uint64_t* md_off, uint8_t* md, uint64_t cap_md, uint64_t* stats) {
    const VfBatch b{tseq, tseq_off, tlen, M, seq1, off1, seq2, off2, n_reads, hits, hit_off};
    std::vector<uint32_t> n; std::vector<uint64_t> off; std::vector<uint8_t> bytes; sfgpu_mdtag_stats st;
    const uint64_t bad = md_serial(b, aln_pos, aln_op_off, aln_ops, lanes, &n, &off, &bytes, &st);
    if (bad) return -(int64_t)bad;
    if (bytes.size() > cap_md) return (int64_t)bytes.size();
    if (!n.empty()) memcpy(nm, n.data(), n.size() * 4);
    if (!bytes.empty()) memcpy(md, bytes.data(), bytes.size());
    memcpy(md_off, off.data(), off.size() * 8);
    const uint64_t s[5] = {st.slots, st.sum_nm, st.md_bytes, st.max_md_bytes, st.slots_plain};
    memcpy(stats, s, sizeof s);
    return (int64_t)bytes.size();
}

// the serial writers of csrc/samwfmt.h / csrc/bamwfmt.h (samw_serial, bamw_serial) with tags handed in, oriented, for the comparison
// with samfile._sam_text(tags=) and sam_to_bam of it (host pointers; qname_off == nullptr: QNAME r<index>; no qualities).
// out[0 .. 8): n_bytes, n_lines, n_units, max_unit_bytes, error_kind, error_read, error_record, 1 when the per-unit sizes the kernels
// take disagree with the serial pass; bytes != nullptr (room for the n_bytes a first call gave): the text or the records.
// -> the error kind
int mdh_write(int bam, const void* hits, const uint32_t* hit_off, uint32_t n_reads, int paired, const char* ref, const uint64_t* ref_off, uint32_t n_refs,
              const char* qnames, const uint64_t* qname_off, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2, const int64_t* s2_off,
              const int32_t* aln_pos, const uint64_t* aln_op_off, const uint32_t* aln_ops, const uint32_t* tag_nm, const uint64_t* tag_md_off,
              const uint8_t* tag_md, uint64_t* out, uint8_t* bytes) {
    SamwArgs a = {static_cast<const sfgpu_hit*>(hits), hit_off, n_reads, paired, ref, ref_off, n_refs, qnames, qname_off, s1, s1_off,
                  paired ? s2 : nullptr, paired ? s2_off : nullptr, 0};
    a.oriented = 1; a.aln_pos = aln_pos; a.aln_op_off = aln_op_off; a.aln_ops = aln_ops;
    a.tag_nm = tag_nm; a.tag_md_off = tag_md_off; a.tag_md = tag_md;
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

#ifdef MDTAG_HARNESS_MAIN
#include "hit_harness.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t n_cases = 0, hd[10];
    while (fread(hd, 8, 10, f) == 10) {
        const uint64_t n_rec = hd[5], has_aln = hd[7], n_words = hd[8], n_md = hd[9];
        HarnessBatch b; std::vector<int32_t> a_pos; std::vector<uint64_t> a_off, want_off, want_stats; std::vector<uint32_t> a_ops, want_nm; std::vector<uint8_t> want_md;
        if (!b.read(f, hd, 6) || !take(f, &a_pos, has_aln ? 2 * n_rec : 0) || !take(f, &a_off, has_aln ? 2 * n_rec + 1 : 0) || !take(f, &a_ops, n_words) ||
            !take(f, &want_nm, 2 * n_rec) || !take(f, &want_off, 2 * n_rec + 1) || !take(f, &want_md, n_md) || !take(f, &want_stats, 5)) {
            fprintf(stderr, "case %llu: short file\n", (unsigned long long)n_cases); return 2;
        }
        if (has_aln && a_ops.empty()) a_ops.resize(1);
        const VfBatch vb{b.ts.data(), b.toff.data(), b.tl.data(), b.M, b.s1.data(), b.o1.data(), b.paired ? b.s2.data() : nullptr, b.paired ? b.o2.data() : nullptr,
                         (uint32_t)b.n_reads, b.hits.data(), b.hoff.data()};
        for (uint32_t lanes = 0; lanes <= 16; lanes += 16) {
            std::vector<uint32_t> n; std::vector<uint64_t> off; std::vector<uint8_t> bytes; sfgpu_mdtag_stats st;
            const uint64_t bad = md_serial(vb, has_aln ? a_pos.data() : nullptr, has_aln ? a_off.data() : nullptr, has_aln ? a_ops.data() : nullptr, lanes, &n, &off, &bytes, &st);
            const uint64_t got_stats[5] = {st.slots, st.sum_nm, st.md_bytes, st.max_md_bytes, st.slots_plain};
            const bool ok = !bad && n == want_nm && off == want_off && bytes == want_md && !memcmp(got_stats, want_stats.data(), sizeof got_stats);
            if (!ok) { fprintf(stderr, "case %llu (%s): differs from the statement\n", (unsigned long long)n_cases, lanes ? "lanes" : "serial"); return 1; }
        }
        ++n_cases;
    }
    fclose(f);
    printf("mdtag harness ok: %llu cases\n", (unsigned long long)n_cases);
    return 0;
}
#endif
