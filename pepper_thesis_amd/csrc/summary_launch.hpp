// summary_launch.hpp — what the summary builders' translation units call in each other. A kernel can only be launched from
// the file that defines it (the library is built without relocatable device code), so each file exports plain host functions.
#pragma once
#include "summary_types.hpp"

namespace pvsum {

// ---- summary_front.hip: the front end shared by the image builders and the polisher -----------------------------------
// Checks the 32-bit index range of the batch (a.n_reads, a.n_cigar, a.n_cols), sets a.n_tiles and claims the workspace of
// the front-end kernels for a.max_pairs pairs: op_ref, op_rd, op_flag, read_region, read_t0, read_t1, tile_cnt, tile_off,
// tile_fill, pairs, diag.
int front_claim(pv_ctx* ctx, SumArgs& a);
void front_init(const SumArgs& a, hipStream_t st);                      // k_init: first launch of a call
void front_check_depth(const SumArgs& a, hipStream_t st);               // k_check_depth (image builders only)
void front_pairs(pv_ctx* ctx, const SumArgs& a, hipStream_t st);        // k_cigar_scan, k_scan_tiles, k_tile_fill
void front_scan_i32(const int32_t* in, int32_t* out, int64_t n, int64_t* total_out, hipStream_t st);   // k_scan_i32, one workgroup

// ---- summary_pileup.hip ----------------------------------------------------------------------------------------------------
void launch_pileup_tiles(const SumArgs& a, bool hp, hipStream_t st);

// ---- summary_builder.hip: the image builders, explicit workspace limits (the *_dev entry points take the heuristics) ------
int summarize_launch(pv_ctx* ctx, const pv_batch_in* in, const pv_params* params, int64_t n_reads, int64_t n_bases,
                     int64_t n_cigar, int64_t n_cols, int64_t max_sites, int64_t max_events, int64_t max_pairs,
                     const pv_batch_out* out, int64_t* d_counts, hipStream_t st, bool hp = false,
                     const int32_t* read_hp = nullptr);
void default_limits(int64_t n_cols, int64_t n_cigar, int64_t n_bases, int64_t n_reads, int64_t capacity, bool hp,
                    int64_t* max_sites, int64_t* max_events, int64_t* max_pairs);

// ---- summary_polish.hip ----------------------------------------------------------------------------------------------------
int polish_launch(pv_ctx* ctx, const pv_batch_in* in, int64_t n_reads, int64_t n_bases, int64_t n_cigar, int64_t n_cols,
                  int64_t max_pairs, int64_t max_ins_rows, int seq_length, int seq_overlap, const pv_polish_out* out,
                  int64_t* d_counts, hipStream_t st);
void polish_limits(int64_t n_cols, int64_t n_bases, int64_t n_reads, int64_t* max_pairs, int64_t* max_ins_rows);

}  // namespace pvsum
