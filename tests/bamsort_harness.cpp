// bamsort_harness.cpp -- csrc/baifmt.h alone, as plain C++ (g++ -Wall -Wextra -Werror): the sorted record stream and the BAI index
// built serially from (records, member sizes) with baifmt.h's functions only.  tests/test_bamsort_cpu.py compares both with
// samfile.write_bam(sort="coordinate") and samfile.build_bai byte for byte.
#include "baifmt.h"

#include <cstring>

using namespace sfgpu;

extern "C" {

const char* bais_hd_line() { return bai_hd_line(); }

// records in write order -> the sorted stream (out has room for n bytes); the number of records, -1 on a broken chain
int64_t bais_sort(const uint8_t* recs, uint64_t n, uint8_t* out) { return bai_serial_sort(recs, n, out); }

// the index of the sorted stream; the bytes it takes (copied to out when cap suffices), -1 on a broken chain, -2 on descending keys
int64_t bais_index(const uint8_t* s, uint64_t n, uint32_t n_ref, const uint32_t* member_sizes, uint64_t n_members, uint64_t first_member,
                   uint8_t* out, uint64_t cap) {
    std::vector<uint8_t> bytes;
    const int64_t rc = bai_serial_index(s, n, n_ref, member_sizes, n_members, first_member, &bytes);
    if (rc >= 0 && (uint64_t)rc <= cap) memcpy(out, bytes.data(), bytes.size());
    return rc;
}

uint64_t bais_key(int32_t ref, int32_t pos) { return bai_key(ref, pos); }
uint32_t bais_reg2bin(uint32_t beg, uint32_t end) { return bamw_reg2bin(beg, end); }

}
