// Host harness for sailfish_amd/csrc/vbmath.h: the header compiled as plain C++ (g++ -ffp-contract=off: vb_x_lean stays free of fma,
// vb_x_fast uses std::fma where the device uses fma), its three host forms over arrays.  Form numbers are sfgpu.h's SFGPU_VB_*.
#include <cstdint>

#include "../sailfish_amd/csrc/vbmath.h"

extern "C" {

// 0: digamma_pos(a)   1: exp(digamma_pos(a) - c) / len   2: vb_x_lean   3: vb_x_fast;   -1 for a form the host does not have
int vb_eval_host(int form, const double* a, const double* c, const double* len, uint64_t n, double* out) {
    if (form < 0 || form > 3) return -1;
    for (uint64_t i = 0; i < n; ++i) {
        if (form == 0) out[i] = sfgpu::digamma_pos(a[i]);
        else if (form == 1) out[i] = std::exp(sfgpu::digamma_pos(a[i]) - c[i]) / len[i];
        else if (form == 2) out[i] = sfgpu::vb_x_lean(a[i], c[i], len[i]);
        else out[i] = sfgpu::vb_x_fast(a[i], c[i], len[i]);
    }
    return 0;
}

}
