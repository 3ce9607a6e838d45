// Test shim: pepper_thesis_amd/csrc/batch_check.hpp behind a C ABI, compiled with the system C++ compiler (no HIP) and called
// through ctypes by tests/test_batch_check_cpu.py.
#include "../pepper_thesis_amd/csrc/batch_check.hpp"

#include <cstring>

extern "C" {
// out = {code, fault, index, n_reads, n_bases, n_cigar, n_cols}; returns the verdict in words
const char* shim_check_batch(const pv_batch_in* in, unsigned reads, int64_t* out) {
    const pv_batch_shape s = pv_check_batch(in, reads);
    const int64_t r[7] = {s.code, s.fault, s.index, s.n_reads, s.n_bases, s.n_cigar, s.n_cols};
    for (int i = 0; i < 7; i++) out[i] = r[i];
    return s.what;
}
unsigned shim_form(int polish) { return polish ? PV_BATCH_POLISH : PV_BATCH_BUILDER; }
// the workspace slots of the arrays a form with `reads` uploads, '\n'-separated; returns their number
int shim_arrays_read(unsigned reads, char* names, int cap) {
    int n = 0;
    names[0] = 0;
    for (const pv_batch_array& a : pv_batch_arrays) {
        if (a.bit && !(reads & a.bit)) continue;
        if ((int)(strlen(names) + strlen(a.slot) + 2) > cap) return -1;
        if (n) strcat(names, "\n");
        strcat(names, a.slot);
        n++;
    }
    return n;
}
}
