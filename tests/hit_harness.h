// hit_harness.h -- what the stand-alone programs of verify_harness.cpp, verifyg_harness.cpp and aligng_harness.cpp share: reading a
// case's arrays from a blob (tests/*_corpus.py: blob).  Every blob begins with a header of 64-bit words -- M, transcript bytes,
// reads, mate 1's bytes, mate 2's bytes, records at words 0 .. 5 -- followed by the batch's arrays ts, toff, tl, s1, o1, s2, o2,
// hits, hoff, then the case's expected results; where `paired` stands in the header differs and is handed in.
#pragma once
#include "verifyfmt.h"

#include <cstdio>

template <typename T>
static bool take(FILE* f, std::vector<T>* v, uint64_t n) {
    v->resize(n);
    return n == 0 || fread(v->data(), sizeof(T), n, f) == n;
}

struct HarnessBatch {
    std::vector<char> ts, s1, s2; std::vector<uint64_t> toff, o1, o2; std::vector<uint32_t> tl, hoff; std::vector<sfgpu_hit> hits;
    uint64_t M = 0, n_reads = 0, n_rec = 0; bool paired = false;
    bool read(FILE* f, const uint64_t* hd, int paired_at) {
        M = hd[0]; n_reads = hd[2]; n_rec = hd[5]; paired = hd[paired_at] != 0;
        return take(f, &ts, hd[1]) && take(f, &toff, M) && take(f, &tl, M) && take(f, &s1, hd[3]) && take(f, &o1, n_reads + 1) && take(f, &s2, hd[4]) &&
               take(f, &o2, paired ? n_reads + 1 : 0) && take(f, &hits, n_rec) && take(f, &hoff, n_reads + 1);
    }
};
