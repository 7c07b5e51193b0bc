// posterior_harness.cpp -- csrc/postfmt.h alone, as plain C++ (g++ -Wall -Wextra -Werror): the posterior pass as the statement runs it
// (post_serial: 64 accumulators and the whole tree for every read) and as csrc/posterior.hip lays it out (ph_layout: the tree over 4
// leaves for 1 .. 4 records, over 8 and 16 leaves for the lane groups of 8 and 16, strided accumulators and the tree over 64 for the
// rest), over whole batches.  tests/test_posterior_cpu.py compares both with hits.posteriors_host.  The serial writers of
// csrc/samwfmt.h / csrc/bamwfmt.h with posteriors handed in are here too (ph_write).  Built with -DPOSTERIOR_HARNESS_MAIN (and
// -fsanitize=address,undefined) it is a stand-alone program: it reads the corpus's batch with its expected result from a file
// (tests/posterior_corpus.py: blob), every array in a block of exactly its size, and runs both forms over it.
#include "postfmt.h"
#include "bamwfmt.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace sfgpu;

namespace {

// S of one read the way the kernel's width classes take it
double ph_layout_sum(const sfgpu_hit* hits, uint64_t b, uint64_t n, const double* w) {
    auto x = [&](uint64_t i) { return post_weight(w[hits[b + i].tid]); };
    double a[kPostAcc];
    for (int j = 0; j < kPostAcc; ++j) a[j] = 0.0;
    if (n <= 4) return post_sum4(n > 0 ? x(0) : 0.0, n > 1 ? x(1) : 0.0, n > 2 ? x(2) : 0.0, n > 3 ? x(3) : 0.0);
    if (n <= 16) {
        for (uint64_t i = 0; i < n; ++i) a[i] = x(i);
        return n <= 8 ? post_tree<8>(a) : post_tree<16>(a);
    }
    for (int lane = 0; lane < kPostAcc; ++lane)
        for (uint64_t i = (uint64_t)lane; i < n; i += kPostAcc) a[lane] = a[lane] + x(i);
    return post_tree<kPostAcc>(a);
}

int64_t ph_layout(const sfgpu_hit* hits, const uint32_t* hit_off, uint32_t n_reads, const double* w, uint64_t n_refs, double* p, uint32_t* rec, float* f32,
                  sfgpu_posterior_stats* st) {
    for (uint64_t t = 0; t < n_refs; ++t) if (post_weight_bad(w[t])) return (int64_t)(1 + t);
    const uint64_t n_rec = n_reads ? hit_off[n_reads] : 0;
    for (uint64_t h = 0; h < n_rec; ++h) if (hits[h].tid >= n_refs) return -(int64_t)(1 + h);
    *st = sfgpu_posterior_stats{};
    st->reads = n_reads; st->records = n_rec;
    for (uint64_t r = 0; r < n_reads; ++r) {
        const uint64_t b = hit_off[r], n = hit_off[r + 1] - b;
        if (!n) continue;
        st->reads_mapped++;
        if (n >= 2) st->reads_multi++;
        if (n > st->max_records) st->max_records = n;
        const double S = ph_layout_sum(hits, b, n, w);
        if (!(S > 0.0)) st->reads_flat++;
        for (uint64_t i = 0; i < n; ++i) {
            const PostValue v = post_value(post_weight(w[hits[b + i].tid]), S, n);
            p[b + i] = v.p; rec[b + i] = v.rec; f32[b + i] = v.f32;
            if (v.p == 0.0) st->records_zero++;
        }
    }
    return 0;
}

void ph_stats(const sfgpu_posterior_stats& st, uint64_t* out) {
    const uint64_t s[7] = {st.reads, st.reads_mapped, st.reads_multi, st.records, st.reads_flat, st.records_zero, st.max_records};
    memcpy(out, s, sizeof s);
}

}  // namespace

extern "C" {

// the whole pass; layout = 0: the statement's form, else the kernel's.  p, rec, f32: one entry per record; stats: 7 words
// (sfgpu_posterior_stats).  -> 0, 1 + the lowest transcript with a bad weight, or -(1 + the lowest record with tid >= n_refs); on an
// error nothing is written
int64_t ph_posteriors(const sfgpu_hit* hits, const uint32_t* hit_off, uint32_t n_reads, const double* w, uint64_t n_refs, int layout, double* p, uint32_t* rec,
                      float* f32, uint64_t* stats) {
    sfgpu_posterior_stats st;
    const int64_t rc = layout ? ph_layout(hits, hit_off, n_reads, w, n_refs, p, rec, f32, &st) : post_serial(hits, hit_off, n_reads, w, n_refs, p, rec, f32, &st);
    if (!rc) ph_stats(st, stats);
    return rc;
}

// the token of a record through gfmt_len / gfmt_put, as the writers place it: -> its bytes in out (room for kGfmtMaxLen)
int ph_token(uint32_t rec, char* out) {
    const int n = gfmt_len(rec);
    gfmt_put(rec, [&](int i, char ch) { out[n - 1 - i] = ch; });
    return n;
}

// the serial writers of csrc/samwfmt.h / csrc/bamwfmt.h (samw_serial, bamw_serial) with tags and posteriors handed in, for the
// comparison with samfile._sam_text(posteriors=) and sam_to_bam of it (host pointers; qname_off == nullptr: QNAME r<index>).
// out[0 .. 5): n_bytes, n_lines, the error kind, 1 when the per-unit sizes the kernels take disagree with the serial pass, 0;
// bytes != nullptr (room for the n_bytes a first call gave): the text or the records.  -> the error kind
int ph_write(int bam, const void* hits, const uint32_t* hit_off, uint32_t n_reads, int paired, const char* ref, const uint64_t* ref_off, uint32_t n_refs,
             const char* qnames, const uint64_t* qname_off, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2, const int64_t* s2_off,
             const uint8_t* q1, const uint8_t* q2, int oriented, const int32_t* aln_pos, const uint64_t* aln_op_off, const uint32_t* aln_ops,
             const uint32_t* tag_nm, const uint64_t* tag_md_off, const uint8_t* tag_md, const uint32_t* zw_rec, const float* zw_f32, uint64_t* out,
             uint8_t* bytes) {
    SamwArgs a = {static_cast<const sfgpu_hit*>(hits), hit_off, n_reads, paired, ref, ref_off, n_refs, qnames, qname_off, s1, s1_off,
                  paired ? s2 : nullptr, paired ? s2_off : nullptr, 0};
    a.qual1 = q1; a.qual2 = paired ? q2 : nullptr; a.oriented = oriented;
    a.aln_pos = aln_pos; a.aln_op_off = aln_op_off; a.aln_ops = aln_ops;
    a.tag_nm = tag_nm; a.tag_md_off = tag_md_off; a.tag_md = tag_md;
    a.tag_zw_rec = zw_rec; a.tag_zw_f32 = zw_f32;
    SamwSerial res;
    const int kind = bam ? bamw_serial(a, nullptr, &res) : samw_serial(a, nullptr, &res);
    uint64_t sum = 0;
    for (uint64_t r = 0; !kind && r < a.n_reads; ++r) {
        const uint64_t h0 = a.hit_off[r], h1 = a.hit_off[r + 1];
        if (h0 == h1) sum += bam ? bamw_unit_len(a, r, nullptr, 0) : samw_unit_len(a, r, nullptr, 0);
        for (uint64_t h = h0; h < h1; ++h) {
            const sfgpu_hit copy = a.hits[h];                      // (as the kernels hold it: a copy and the record's index)
            sum += bam ? bamw_unit_len(a, r, &copy, h - h0, h) : samw_unit_len(a, r, &copy, h - h0, h);
        }
    }
    out[0] = res.n_bytes; out[1] = res.n_lines; out[2] = (uint64_t)kind; out[3] = !kind && sum != res.n_bytes; out[4] = 0;
    if (kind || !bytes) return kind;
    SamwSerial again;
    const int k2 = bam ? bamw_serial(a, bytes, &again) : samw_serial(a, reinterpret_cast<char*>(bytes), &again);
    if (k2 || again.n_bytes != res.n_bytes) out[3] = 1;
    return k2;
}

}

#ifdef POSTERIOR_HARNESS_MAIN
template <typename T>
static bool take(FILE* f, std::vector<T>* v, uint64_t n) {
    v->resize(n);
    return n == 0 || fread(v->data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s batch.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t hd[3];
    std::vector<sfgpu_hit> hits; std::vector<uint32_t> off, want_rec; std::vector<double> w, want_p; std::vector<float> want_f32; std::vector<uint64_t> want_stats;
    if (fread(hd, 8, 3, f) != 3 || !take(f, &hits, hd[1]) || !take(f, &off, hd[0] + 1) || !take(f, &w, hd[2]) || !take(f, &want_p, hd[1]) || !take(f, &want_rec, hd[1]) ||
        !take(f, &want_f32, hd[1]) || !take(f, &want_stats, 7)) {
        fprintf(stderr, "short file\n"); return 2;
    }
    fclose(f);
    for (int layout = 0; layout < 2; ++layout) {
        std::vector<double> p(hd[1]); std::vector<uint32_t> rec(hd[1]); std::vector<float> f32(hd[1]); uint64_t stats[7];
        const int64_t rc = ph_posteriors(hits.data(), off.data(), (uint32_t)hd[0], w.data(), hd[2], layout, p.data(), rec.data(), f32.data(), stats);
        const bool ok = !rc && !memcmp(p.data(), want_p.data(), 8 * hd[1]) && rec == want_rec && !memcmp(f32.data(), want_f32.data(), 4 * hd[1]) &&
                        !memcmp(stats, want_stats.data(), sizeof stats);
        if (!ok) { fprintf(stderr, "%s: differs from the statement\n", layout ? "the kernel's layout" : "the statement's form"); return 1; }
        char token[kGfmtMaxLen];
        for (uint32_t r : rec) if (ph_token(r, token) < 1) return 1;
    }
    printf("posterior harness ok: %llu reads, %llu records\n", (unsigned long long)hd[0], (unsigned long long)hd[1]);
    return 0;
}
#endif
