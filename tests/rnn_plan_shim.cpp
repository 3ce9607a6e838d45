// Test shim: the plan functions of pepper_thesis_amd/csrc/rnn_plan.hpp behind a C ABI, compiled with the system C++ compiler
// (no HIP) and called through ctypes by tests/test_rnn_plan_cpu.py. Options arrive as ten ints in the order of OPTION_NAMES
// of tests/rnn_forms.py; an output is one row of int64 per batch size.
#include "../pepper_thesis_amd/csrc/rnn_plan.hpp"

static pv_opts opts_of(const int* v) {
    pv_opts o;   // (the defaults of the library for everything not listed)
    o.lstm_split = v[0]; o.lstm_rows = v[1]; o.tail_rows = v[2]; o.head_splits = v[3]; o.shared_device = v[4]; o.gru_rows = v[5];
    o.gru_split = v[6]; o.gru_usplit = v[7]; o.p1_bf16_min_batch = v[8]; o.p1_f32x6_min_batch = v[9];
    return o;
}

extern "C" {
int shim_option_defaults(int* v) {
    const pv_opts o;
    const int d[10] = {o.lstm_split, o.lstm_rows, o.tail_rows, o.head_splits, o.shared_device, o.gru_rows, o.gru_split, o.gru_usplit,
                       o.p1_bf16_min_batch, o.p1_f32x6_min_batch};
    for (int i = 0; i < 10; i++) v[i] = d[i];
    return 10;
}
// rows [chain, lstm, rows, mt, Bp, splits, head_map, tail, tail_rows] for B = lo .. hi
void shim_plan_p1(int dtype, int64_t lo, int64_t hi, int num_cu, const int* v, int64_t* out) {
    const pv_opts o = opts_of(v);
    for (int64_t B = lo; B <= hi; B++, out += 9) {
        const pv_p1_plan p = pv_plan_p1(dtype, B, num_cu, o);
        const int64_t r[9] = {p.chain, p.lstm, p.rows, p.mt, p.Bp, p.splits, p.head_map, p.tail, p.tail_rows};
        for (int i = 0; i < 9; i++) out[i] = r[i];
    }
}
// the chunk size of a call of B windows, B = lo .. hi
void shim_p1_chunk(int dtype, int64_t lo, int64_t hi, const int* v, int64_t* out) {
    const pv_opts o = opts_of(v);
    for (int64_t B = lo; B <= hi; B++) *out++ = pv_p1_chunk(dtype, B, o);
}
// rows [kind, rows, mt, fold_dense, Bp] for B = lo .. hi
void shim_plan_p2(int dtype, int64_t lo, int64_t hi, int num_cu, const int* v, int64_t* out) {
    const pv_opts o = opts_of(v);
    for (int64_t B = lo; B <= hi; B++, out += 5) {
        const pv_p2_plan p = pv_plan_p2(dtype, B, num_cu, o);
        const int64_t r[5] = {p.kind, p.rows, p.mt, p.fold_dense, p.Bp};
        for (int i = 0; i < 5; i++) out[i] = r[i];
    }
}
}
