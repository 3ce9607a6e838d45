// batch_check.hpp — host-only validation of a pv_batch_in that holds HOST pointers, and the list of its arrays. Nothing of
// HIP is included: the header compiles with the system C++ compiler (tests/batch_check_shim.cpp), like rnn_plan.hpp.
// The three entry points that take a host batch (pv_upload_batch, pv_upload_batches per part, pv_polish_summarize_regions)
// call pv_check_batch and word its verdict themselves; their uploads walk pv_batch_arrays.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/pepper_hip.h"

// Arrays a caller may leave out (bits of `reads`): the polisher's kernels read neither the reference bytes, the qualities nor
// the candidate bounds, and pv_upload_batches copies the four large arrays part by part itself. Every other array is always read.
enum : unsigned {
    PV_BA_REF = 1, PV_BA_QUALS = 2, PV_BA_CANDS = 4, PV_BA_BASES = 8, PV_BA_CIGAR = 16,
    PV_BATCH_BUILDER = PV_BA_REF | PV_BA_QUALS | PV_BA_CANDS | PV_BA_BASES | PV_BA_CIGAR,
    PV_BATCH_POLISH = PV_BA_BASES | PV_BA_CIGAR
};

enum pv_batch_fault {
    PV_BF_NONE = 0,
    PV_BF_REGION_COUNT,   // n_regions < 0
    PV_BF_OFFSET_START,   // read_off[0] or ref_off[0] is not 0, or read_off[n_regions] is negative
    PV_BF_REGION_EMPTY,   // region `index`: ref_end - ref_start + 1 < 1
    PV_BF_REF_SHORT,      // region `index`: fewer reference bytes than ref_end - ref_start + 1
    PV_BF_READ_OFF,       // read_off decreases behind region `index`
    PV_BF_BASE_OFF,       // base_off decreases behind read `index`
    PV_BF_CIGAR_OFF       // cigar_off decreases behind read `index`
};

struct pv_batch_shape {
    int code;             // PV_OK or PV_ERR_INVALID
    pv_batch_fault fault; // which check failed
    int64_t index;        // region or read of the fault (-1: none)
    const char* what;     // the fault in words (callers word their own messages around fault and index)
    unsigned reads;       // as given
    int64_t n_reads, n_bases, n_cigar, n_cols;   // the four totals the *_dev entry points take
    int64_t n_regions;
};

// One row per array of pv_batch_in: workspace slot, element size, elements = a count of the shape + `plus`, the field (every
// one a pointer), the `reads` bit (0: always read)
struct pv_batch_array {
    const char* slot;
    size_t elem;
    int64_t pv_batch_shape::*count;
    int plus;
    size_t field;
    unsigned bit;
};
#define PV_BA_ROW(name, elem, count, plus, bit) {"in." #name, elem, &pv_batch_shape::count, plus, offsetof(pv_batch_in, name), bit}
static const pv_batch_array pv_batch_arrays[] = {
    PV_BA_ROW(ref_start, 8, n_regions, 0, 0),
    PV_BA_ROW(ref_end, 8, n_regions, 0, 0),
    PV_BA_ROW(cand_start, 8, n_regions, 0, PV_BA_CANDS),
    PV_BA_ROW(cand_end, 8, n_regions, 0, PV_BA_CANDS),
    PV_BA_ROW(ref_off, 8, n_regions, 1, 0),
    PV_BA_ROW(ref, 1, n_cols, 0, PV_BA_REF),
    PV_BA_ROW(read_off, 8, n_regions, 1, 0),
    PV_BA_ROW(read_pos, 8, n_reads, 0, 0),
    PV_BA_ROW(read_flags, 1, n_reads, 0, 0),
    PV_BA_ROW(read_mapq, 1, n_reads, 0, 0),
    PV_BA_ROW(base_off, 8, n_reads, 1, 0),
    PV_BA_ROW(bases, 1, n_bases, 0, PV_BA_BASES),
    PV_BA_ROW(quals, 1, n_bases, 0, PV_BA_QUALS),
    PV_BA_ROW(cigar_off, 8, n_reads, 1, 0),
    PV_BA_ROW(cigar, 4, n_cigar, 0, PV_BA_CIGAR),
};
#undef PV_BA_ROW

// Checks the offset arrays of a host batch (O(regions + reads)); the first fault in region order, then read order, is
// reported. Only offsets and region bounds are looked at: an array that `reads` leaves out may be null, and so may - as ever -
// one that it names (a builder batch without qualities is not caught here).
static inline pv_batch_shape pv_check_batch(const pv_batch_in* in, unsigned reads) {
    pv_batch_shape s = {PV_OK, PV_BF_NONE, -1, "ok", reads, 0, 0, 0, 0, in->n_regions};
    auto fail = [&](pv_batch_fault f, int64_t index, const char* what) {
        s.code = PV_ERR_INVALID; s.fault = f; s.index = index; s.what = what;
        return s;
    };
    const int G = in->n_regions;
    if (G < 0) return fail(PV_BF_REGION_COUNT, -1, "negative region count");
    if (G == 0) return s;
    const int64_t n_reads = in->read_off[G];
    if (!(in->read_off[0] == 0 && in->ref_off[0] == 0 && n_reads >= 0)) return fail(PV_BF_OFFSET_START, -1, "offset arrays must start at 0");
    for (int g = 0; g < G; g++) {
        const int64_t R = in->ref_end[g] - in->ref_start[g] + 1;
        if (R < 1) return fail(PV_BF_REGION_EMPTY, g, "region of no columns");
        if (in->ref_off[g + 1] - in->ref_off[g] < R) return fail(PV_BF_REF_SHORT, g, "reference shorter than ref_end-ref_start+1");
        if (in->read_off[g + 1] < in->read_off[g]) return fail(PV_BF_READ_OFF, g, "read_off not monotone");
    }
    for (int64_t r = 0; r < n_reads; r++) {
        if (in->base_off[r + 1] < in->base_off[r]) return fail(PV_BF_BASE_OFF, r, "base_off not monotone");
        if (in->cigar_off[r + 1] < in->cigar_off[r]) return fail(PV_BF_CIGAR_OFF, r, "cigar_off not monotone");
    }
    s.n_reads = n_reads;
    s.n_cols = in->ref_off[G];
    s.n_bases = n_reads ? in->base_off[n_reads] : 0;
    s.n_cigar = n_reads ? in->cigar_off[n_reads] : 0;
    return s;
}
