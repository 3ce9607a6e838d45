// rnn_p1.hip — P1 (pepper_variant): the model record, its load, and the forward chains. Host code only: every kernel lives in
// the unit of its family and is reached through a descriptor.
//
// images int8 [B,33,26] -> bi-LSTM(256) -> bi-LSTM(256) -> flatten 16896 ->
//     5 x (Linear 512 + SELU) -> Linear 3 -> softmax        (reference: models/simple_model.py:48-82)
//
// Three chains; which one a launch takes, and in which form, is decided by its plan (rnn_plan.hpp):
//   fp32          k_lstm_layer / k_lstm_split (rnn_lstm.hip) -> k_head_splitk -> k_head_tail (rnn_head.hip): rnn_f32.hpp
//   bf16x3        PV_DTYPE_BF16_INPUT_GEMM: k_rec_bf16 (rnn_rec_bf16.hip) and k_gemm_bf16x3 (rnn_gemm.hip) -> k_tail_bf16 or
//                 k_head_tail: rnn_bf16.hpp
//   split-6       large PV_DTYPE_F32 calls: the same on three-piece operands, k_gemm_bf16x6; a 32-row k_head_tail plan runs
//                 the six-term form of k_tail_bf16
// Weights are packed on the host (rnn_pack_host.hpp) and uploaded once, at load.
#include "pv_common.hpp"
#include "rnn_bf16.hpp"
#include "rnn_f32.hpp"
#include "rnn_pack_host.hpp"

#include <algorithm>
#include <optional>

namespace {

constexpr int T_STEPS = PV_P1_T;
constexpr int F_IN = PV_P1_F;
constexpr int H = PV_P1_H;        // LSTM hidden
constexpr int ROWS = PV_P1_ROWS;  // the 32-row tile every buffer is counted in
constexpr int HEAD_N = PV_HEAD_N;
constexpr int HEAD_K = PV_HEAD_K;
constexpr int HEAD_MAX_SPLITS = PV_HEAD_MAX_SPLITS;   // split-K factor of linear_1 is chosen per launch from {1, 3, 11, 33}

}  // namespace

struct pv_rnn_p1 {
    float* enc_wp[2] = {nullptr, nullptr};  // [0] 32-row tile form, [1] 16-row tile form (mfma_tiles.hpp)
    float* dec_wp[2] = {nullptr, nullptr};
    float* enc_bias = nullptr; float* dec_bias = nullptr;
    float* enc_wps[2] = {nullptr, nullptr};                // unit-split form (k_lstm_split): [0] four parts, [1] two parts
    float* dec_wps[2] = {nullptr, nullptr};
    void* sp_hx = nullptr; int* sp_flags = nullptr;        // its exchange buffer (tagged granules) and counters (fence form)
    int* sp_err = nullptr;                                 // exchange time-outs (device word, read by the host-buffer entry points)
    unsigned* sp_epoch = nullptr;                          // device word: forward calls so far (tags of the exchange derive from it)
    float* w1p = nullptr; float* b1 = nullptr;
    float* wlp[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};  // [tile form][layer]
    float* bl[4] = {nullptr, nullptr, nullptr, nullptr};
    float* wo = nullptr; float* bo = nullptr;
    int dtype = PV_DTYPE_F32;
    // PV_DTYPE_BF16_INPUT_GEMM: bf16 hi/lo splits of the decoder W_ih (both directions, [2048,512]) and linear_1 ([512,16896])
    unsigned char* dec_wih_s = nullptr; float* dec_bias_cat = nullptr;   // split8 rows
    unsigned char* w1_s = nullptr;
    unsigned char* enc_rb = nullptr; unsigned char* dec_rb = nullptr;    // bf16 fragment streams of k_rec_bf16 (encoder: W_ih | W_hh; decoder: W_hh)
    unsigned char* tail_wb = nullptr;                                    // bf16 fragment stream of k_tail_bf16 (linear_2..5)
    // PV_DTYPE_F32, split-6 chain: three-piece fragment streams of k_rec_bf16<X6> and the weights of k_gemm_bf16x6 as three
    // bf16 planes [3][N][K] (split3_host.hpp), made once here
    unsigned char* enc_r6 = nullptr; unsigned char* dec_r6 = nullptr;
    unsigned char* dec_wih_p3 = nullptr;   // decoder W_ih of both directions [3][2048][512] (biases: dec_bias_cat)
    unsigned char* dec_wih_s6 = nullptr;   // ... and as the fragment stream of k_gemm_x6_stream (pack_gemm6_stream), 6.3 MB more
    unsigned char* w1_p3 = nullptr;        // linear_1 [3][512][16896]
    unsigned char* tail_w6 = nullptr;      // three-piece fragment stream of k_tail_bf16<X6> (linear_2..5, pack_tail_x6)
    std::vector<void*> owned;
};

static void p1_free(pv_ctx* ctx) {
    if (!ctx->p1) return;
    for (void* p : ctx->p1->owned) (void)hipFree(p);
    delete ctx->p1;
    ctx->p1 = nullptr;
}

void pv_rnn_free(pv_ctx* ctx) {
    p1_free(ctx);
    pv_rnn_free_p2(ctx);
}

extern "C" int pv_rnn_load_p1(pv_ctx* ctx, const pv_weights_p1* w, int dtype) {
    PV_CHECK(ctx && w, PV_ERR_INVALID, "null argument");
    PV_CHECK(dtype == PV_DTYPE_F32 || dtype == PV_DTYPE_BF16_INPUT_GEMM, PV_ERR_INVALID, "unknown dtype %d", dtype);
    for (int d = 0; d < 2; d++) {
        PV_CHECK(w->encoder[d].w_ih && w->encoder[d].w_hh && w->encoder[d].b_ih && w->encoder[d].b_hh &&
                     w->decoder[d].w_ih && w->decoder[d].w_hh && w->decoder[d].b_ih && w->decoder[d].b_hh,
                 PV_ERR_INVALID, "missing LSTM tensor");
    }
    for (int i = 0; i < 5; i++) PV_CHECK(w->linear_w[i] && w->linear_b[i], PV_ERR_INVALID, "missing linear_%d", i + 1);
    PV_CHECK(w->out_w && w->out_b, PV_ERR_INVALID, "missing output layer");
    PV_HIP(hipSetDevice(ctx->device));
    if (ctx->p1) {
        PV_HIP(hipStreamSynchronize(ctx->stream));
        p1_free(ctx);
    }
    pv_rnn_p1* m = new pv_rnn_p1();
    ctx->p1 = m;
    m->dtype = dtype;
    std::vector<float> wp, bias;
    int rc;
    for (int f = 0; f < 2; f++) {
        pack_lstm(w->encoder, F_IN, 32, f ? 16 : 32, wp, bias);
        if ((rc = pv_dev_upload(wp, &m->enc_wp[f], m->owned))) return rc;
        if (!f && (rc = pv_dev_upload(bias, &m->enc_bias, m->owned))) return rc;
        pack_lstm(w->decoder, 2 * H, 2 * H, f ? 16 : 32, wp, bias);
        if ((rc = pv_dev_upload(wp, &m->dec_wp[f], m->owned))) return rc;
        if (!f && (rc = pv_dev_upload(bias, &m->dec_bias, m->owned))) return rc;
    }
    for (int f = 0; f < 2; f++) {
        pack_lstm_split(w->encoder, F_IN, 32, f ? 2 : 4, wp);
        if ((rc = pv_dev_upload(wp, &m->enc_wps[f], m->owned))) return rc;
        pack_lstm_split(w->decoder, 2 * H, 2 * H, f ? 2 : 4, wp);
        if ((rc = pv_dev_upload(wp, &m->dec_wps[f], m->owned))) return rc;
    }
    // the exchange of the unit-split form: tags start at 0 (no launch ever waits for tag 0)
    if ((rc = pv_dev_zeros(PV_LSTM_HX_BYTES, &m->sp_hx, m->owned)) || (rc = pv_dev_zeros(PV_LSTM_FLAGS_BYTES, &m->sp_flags, m->owned)) ||
        (rc = pv_dev_zeros(64, &m->sp_err, m->owned)) || (rc = pv_dev_zeros(64, &m->sp_epoch, m->owned)))
        return rc;
    pack_linear(w->linear_w[0], HEAD_K, 32, wp);
    if ((rc = pv_dev_upload(wp, &m->w1p, m->owned)) || (rc = pv_dev_upload(w->linear_b[0], HEAD_N, &m->b1, m->owned))) return rc;
    for (int i = 0; i < 4; i++) {
        for (int f = 0; f < 2; f++) {
            pack_linear(w->linear_w[i + 1], HEAD_N, f ? 16 : 32, wp);
            if ((rc = pv_dev_upload(wp, &m->wlp[f][i], m->owned))) return rc;
        }
        if ((rc = pv_dev_upload(w->linear_b[i + 1], HEAD_N, &m->bl[i], m->owned))) return rc;
    }
    if ((rc = pv_dev_upload(w->out_w, 3 * HEAD_N, &m->wo, m->owned)) || (rc = pv_dev_upload(w->out_b, 3, &m->bo, m->owned))) return rc;
    std::vector<float> wcat((size_t)2048 * 512), bcat(2048);   // decoder W_ih of both directions, b_ih + b_hh
    for (int d = 0; d < 2; d++) {
        memcpy(&wcat[(size_t)d * 1024 * 512], w->decoder[d].w_ih, (size_t)1024 * 512 * sizeof(float));
        for (int n = 0; n < 1024; n++) bcat[d * 1024 + n] = w->decoder[d].b_ih[n] + w->decoder[d].b_hh[n];
    }
    if ((rc = pv_dev_upload(bcat, &m->dec_bias_cat, m->owned))) return rc;
    const float* tail_w[4] = {w->linear_w[1], w->linear_w[2], w->linear_w[3], w->linear_w[4]};
    if (dtype == PV_DTYPE_F32) {   // the split-6 chain of large calls: 3.4 + 3.4 + 6.3 MB of fragments, 6 + 51.9 MB of bf16 weight planes, 6.3 MB of
                                   // the decoder W_ih again in k_gemm_x6_stream's order
        if ((rc = pv_pack_rec_x6(w->encoder, F_IN, &m->enc_r6, m->owned))) return rc;
        if ((rc = pv_pack_rec_x6(w->decoder, 0, &m->dec_r6, m->owned))) return rc;
        if ((rc = pv_upload_split3(wcat.data(), 2048, 512, &m->dec_wih_p3, m->owned))) return rc;
        if ((rc = pv_upload_gemm6_stream(wcat.data(), 2048, 512, &m->dec_wih_s6, m->owned))) return rc;
        if ((rc = pv_upload_split3(w->linear_w[0], HEAD_N, HEAD_K, &m->w1_p3, m->owned))) return rc;
        if ((rc = pv_pack_tail_bf16(tail_w, &m->tail_w6, m->owned, 3))) return rc;
        if ((rc = pv_gemm_bf16x3_prepare()) || (rc = pv_rec_bf16_prepare()) || (rc = pv_tail_bf16_prepare())) return rc;
    }
    if (dtype == PV_DTYPE_BF16_INPUT_GEMM) {
        if ((rc = pv_upload_split8(wcat.data(), 2048, 512, &m->dec_wih_s, m->owned))) return rc;
        if ((rc = pv_upload_split8(w->linear_w[0], HEAD_N, HEAD_K, &m->w1_s, m->owned))) return rc;
        if ((rc = pv_pack_rec_bf16(w->encoder, 4, F_IN, &m->enc_rb, nullptr, m->owned))) return rc;
        if ((rc = pv_pack_rec_bf16(w->decoder, 4, 0, &m->dec_rb, nullptr, m->owned))) return rc;
        if ((rc = pv_pack_tail_bf16(tail_w, &m->tail_wb, m->owned))) return rc;
        if ((rc = pv_gemm_bf16x3_prepare()) || (rc = pv_rec_bf16_prepare()) || (rc = pv_tail_bf16_prepare())) return rc;
    }
    if ((rc = pv_lstm_f32_prepare()) || (rc = pv_head_f32_prepare())) return rc;
    return PV_OK;
}

// k_head_tail over the linear_1 slabs part [splits][part_rows][512]
static int launch_tail(pv_ctx* ctx, const pv_p1_plan& pl, const float* part, int64_t part_rows, float* d_probs, int64_t B, hipStream_t st) {
    const pv_rnn_p1* m = ctx->p1;
    pv_head_tail_desc t = {};
    t.rows = pl.tail_rows; t.part = part; t.b1 = m->b1; t.splits = pl.splits; t.part_rows = part_rows;
    t.wo = m->wo; t.bo = m->bo; t.probs = d_probs; t.B = B; t.epoch = m->sp_epoch; t.err = m->sp_err;
    for (int i = 0; i < 4; i++) { t.wp[i] = m->wlp[pl.tail_rows == 16 ? 1 : 0][i]; t.b[i] = m->bl[i]; }
    int rc = pv_head_tail_async(ctx, t, st);
    if (rc) return rc;
    PV_HIP(hipGetLastError());
    return PV_OK;
}

// What tells the two chains on the bf16 MFMA apart (p1_forward_mfma). Rows of the layer outputs are 2 KB in both: split8
// (bf16 hi + lo per element) in the bf16x3 chain, fp32 in the split-6 chain.
struct P1Chain {
    int terms;                                 // of every product: 3 (split8 operands) or 6 (three-piece operands)
    const unsigned char *enc_rec, *dec_rec;    // fragment streams of k_rec_bf16
    const void *dec_wih, *w1;                  // GEMM weights: split8 rows or three bf16 planes
    const char* enc_buf;                       // workspace of the encoder's time-major output
    const char *n_enc, *n_dec_scope, *n_dec_gemm, *n_dec, *n_lin1;   // profile names
};

// Every matrix product of the RNN on the bf16 MFMA, fp32 accumulation, fp32 cell updates: the bf16x3 chain (PV_DTYPE_BF16_INPUT_GEMM,
// 3-term split products) and the split-6 chain (PV_DTYPE_F32, large calls: six terms of three-piece operands, fp32-class: the
// dropped terms are below 2^-24 relative).
//   encoder   k_rec_bf16<LSTM, enc>: byte x-part + h-part per step -> rows, time-major
//   decoder   one GEMM (G = enc . W_ih^T + b, quads) + k_rec_bf16<LSTM, dec> on G -> rows, batch-major (split-6: dec_out itself,
//             fp32 [Bp][T][2H]: the head's operand and the decoder tap)
//   head      linear_1 as a split-K GEMM into slabs [splits][Bp][512] -> k_head_tail or k_tail_bf16 (sum of slabs, linear_2..5,
//             output layer, softmax)
// The split-6 decoder's two launches form ONE profile scope "k_lstm_layer_dec" (the fp32 chain's fused decoder kernel), so
// per-layer figures compare across the two chains; the launches inside carry names outside that prefix.
static int p1_forward_mfma(pv_ctx* ctx, const pv_p1_plan& pl, const int8_t* d_images, int64_t B, float* d_probs, float* enc_out,
                           float* dec_out, float* part, hipStream_t st, bool taps) {
    pv_rnn_p1* m = ctx->p1;
    const bool x6 = pl.chain == PV_CHAIN_X6;
    const P1Chain c = x6 ? P1Chain{6, m->enc_r6, m->dec_r6, m->dec_wih_p3, m->w1_p3, "p1.enc_tm", "k_rec_x6_lstm_enc", "k_lstm_layer_dec",
                                   "k_gemm_bf16x6_dec", "k_rec_x6_lstm_dec", "k_gemm_bf16x6_lin1"}
                         : P1Chain{3, m->enc_rb, m->dec_rb, m->dec_wih_s, m->w1_s, "p1.enc_split", "k_rec_bf16_lstm_enc", nullptr,
                                   "k_gemm_bf16x3_dec", "k_rec_bf16_lstm_dec", "k_gemm_bf16x3_lin1"};
    const int64_t Bp = pl.Bp, M = Bp * T_STEPS;
    const size_t out_bytes = (size_t)M * 2 * H * 4;
    unsigned char *enc = nullptr, *dec = reinterpret_cast<unsigned char*>(dec_out);
    float* G = nullptr;
    int rc;
    if ((rc = pv_get(ctx, c.enc_buf, out_bytes, &enc)) || (!x6 && (rc = pv_get(ctx, "p1.dec_split", out_bytes, &dec))) ||
        (rc = pv_get(ctx, "p1.G", (size_t)M * 2048, &G))) return rc;
    pv_rec_desc re = {};
    re.cell = 4; re.enc = 1; re.wp = c.enc_rec; re.bias = m->enc_bias; re.x = d_images; re.x_row_bytes = PV_WINDOW_BYTES; re.x_t0 = 0;
    re.xf = F_IN; re.x_signed = 1; re.B = B; re.Bp = Bp; re.T = T_STEPS; re.out_tm = enc; re.out_f32 = taps ? enc_out : nullptr;
    re.mt = pl.mt; re.x6 = x6; re.prof_name = c.n_enc;
    if ((rc = pv_rec_bf16_async(ctx, re, st))) return rc;
    {
        std::optional<pv_prof_scope> ps;
        if (c.n_dec_scope) ps.emplace(ctx, c.n_dec_scope, st);
        pv_gemm_desc ga = {};
        ga.A = enc; ga.W = static_cast<const unsigned char*>(c.dec_wih); ga.bias = m->dec_bias_cat; ga.C = G; ga.M = M; ga.N = 2048;
        ga.K = 2 * H; ga.splits = 1; ga.quads = 1; ga.terms = c.terms; ga.prof_name = c.n_dec_gemm;
        ga.W_stream = x6 ? m->dec_wih_s6 : nullptr;
        if ((rc = pv_gemm_bf16x3_async(ctx, ga, st))) return rc;
        pv_rec_desc rd = {};
        rd.cell = 4; rd.enc = 0; rd.G = G; rd.wp = c.dec_rec; rd.B = B; rd.Bp = Bp; rd.T = T_STEPS; rd.out_bm = dec;
        rd.out_f32 = taps && !x6 ? dec_out : nullptr; rd.mt = pl.mt; rd.x6 = x6; rd.prof_name = c.n_dec;
        if ((rc = pv_rec_bf16_async(ctx, rd, st))) return rc;
    }
    pv_gemm_desc gl = {};
    gl.A = dec; gl.W = static_cast<const unsigned char*>(c.w1); gl.bias = nullptr; gl.C = part; gl.M = Bp; gl.N = HEAD_N; gl.K = HEAD_K;
    gl.splits = pl.splits; gl.quads = 0; gl.terms = c.terms; gl.prof_name = c.n_lin1;
    if ((rc = pv_gemm_bf16x3_async(ctx, gl, st))) return rc;
    // a 32-row k_head_tail plan on the split-6 chain is the six-term form of the tail; its 16-row plans (fewer than one 32-row
    // tile per CU) and the bf16x3 chain's small calls keep k_head_tail on the f32 MFMA
    const bool tail6 = x6 && pl.tail == PV_TAIL_HEAD_TAIL && pl.tail_rows == 32;
    if (pl.tail == PV_TAIL_HEAD_TAIL && !tail6) return launch_tail(ctx, pl, part, Bp, d_probs, B, st);
    pv_tail_desc tb = {};
    tb.part = part; tb.b1 = m->b1; tb.splits = pl.splits; tb.part_rows = Bp; tb.wp = tail6 ? m->tail_w6 : m->tail_wb; tb.x6 = tail6;
    for (int i = 0; i < 4; i++) tb.b[i] = m->bl[i];
    tb.wo = m->wo; tb.bo = m->bo; tb.probs = d_probs; tb.B = B; tb.epoch = m->sp_epoch; tb.err = m->sp_err;
    return pv_tail_bf16_async(ctx, tb, st);
}

// The fp32 chain: both LSTM layers in the form the plan names, linear_1 as k_head_splitk, k_head_tail.
static int p1_forward_f32(pv_ctx* ctx, const pv_p1_plan& pl, const int8_t* d_images, int64_t B, float* d_probs, float* enc_out,
                          float* dec_out, float* part, hipStream_t st) {
    pv_rnn_p1* m = ctx->p1;
    const int n_tiles = (int)(pl.Bp / ROWS);   // 32-row tiles: the granularity of every buffer and of the head
    const bool split = pl.lstm == PV_LSTM_SPLIT4 || pl.lstm == PV_LSTM_SPLIT2;
    const int f = pl.lstm == PV_LSTM_SPLIT4 || pl.lstm == PV_LSTM_ROWS32 ? 0 : 1;   // index of the form's packed weights
    int rc;
    pv_lstm_desc e = {};
    e.form = pl.lstm;
    e.x_i8 = d_images; e.wp = split ? m->enc_wps[f] : m->enc_wp[f]; e.bias = m->enc_bias; e.out = enc_out; e.B = B; e.n_tiles = n_tiles;
    e.hx = m->sp_hx; e.flags = m->sp_flags; e.epoch = m->sp_epoch; e.err = m->sp_err;
    if ((rc = pv_lstm_f32_async(ctx, e, st))) return rc;
    pv_lstm_desc d = e;
    d.x_i8 = nullptr; d.x_f32 = enc_out; d.wp = split ? m->dec_wps[f] : m->dec_wp[f]; d.bias = m->dec_bias; d.out = dec_out;
    if ((rc = pv_lstm_f32_async(ctx, d, st))) return rc;
    pv_head_splitk_desc h = {};
    h.dec = dec_out; h.w1p = m->w1p; h.part = part; h.B = B; h.n_tiles = n_tiles; h.splits = pl.splits; h.head_map = pl.head_map;
    if ((rc = pv_head_splitk_async(ctx, h, st))) return rc;
    return launch_tail(ctx, pl, part, B, d_probs, B, st);
}

// one launch of B windows (a whole call, or one chunk of it) in the form rnn_plan.hpp names
static int p1_forward_launch(pv_ctx* ctx, const int8_t* d_images, int64_t B, float* d_probs, float* enc_out,
                             float* dec_out, float* part, hipStream_t st, bool taps = false) {
    const pv_p1_plan pl = pv_plan_p1(ctx->p1->dtype, B, ctx->num_cu, ctx->opt);
    if (pl.chain != PV_CHAIN_F32) return p1_forward_mfma(ctx, pl, d_images, B, d_probs, enc_out, dec_out, part, st, taps);
    return p1_forward_f32(ctx, pl, d_images, B, d_probs, enc_out, dec_out, part, st);
}

static int p1_workspace(pv_ctx* ctx, int64_t B, float** enc, float** dec, float** part) {
    int rc;
    const size_t Bp = (size_t)((B + 2 * ROWS - 1) / (2 * ROWS)) * 2 * ROWS;  // layer kernels store whole tiles (32 rows; 64 in the bf16x3 mode)
    if ((rc = pv_get(ctx, "p1.enc_out", Bp * T_STEPS * 2 * H, enc))) return rc;
    if ((rc = pv_get(ctx, "p1.dec_out", Bp * T_STEPS * 2 * H, dec))) return rc;
    if ((rc = pv_get(ctx, "p1.part", (size_t)HEAD_MAX_SPLITS * Bp * HEAD_N, part))) return rc;
    return PV_OK;
}

// the argument checks of the forward entry points (`has_buffers`: none of the required pointers is null)
static int p1_check_call(const pv_ctx* ctx, bool has_buffers, int64_t B) {
    PV_CHECK(ctx && has_buffers, PV_ERR_INVALID, "null argument");
    PV_CHECK(ctx->p1, PV_ERR_STATE, "pv_rnn_load_p1 has not been called on this context");
    PV_CHECK(B >= 0 && B < (1ll << 24), PV_ERR_INVALID, "batch %lld out of range", (long long)B);
    return PV_OK;
}

extern "C" int pv_rnn_forward_p1_dev(pv_ctx* ctx, const int8_t* d_images, int64_t B, float* d_probs, void* stream) {
    int rc = p1_check_call(ctx, d_images && d_probs, B);
    if (rc || B == 0) return rc;
    PV_HIP(hipSetDevice(ctx->device));
    const int64_t chunk = pv_p1_chunk(ctx->p1->dtype, B, ctx->opt);   // the chains on the bf16 MFMA run large calls as chunks
    float *enc, *dec, *part;
    if ((rc = p1_workspace(ctx, std::min(B, chunk), &enc, &dec, &part))) return rc;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(chunk, B - b0);
        if ((rc = p1_forward_launch(ctx, d_images + b0 * PV_WINDOW_BYTES, nb, d_probs + b0 * 3, enc, dec, part, pv_pick_stream(ctx, stream)))) return rc;
    }
    return PV_OK;
}

extern "C" int pv_rnn_forward_p1_debug(pv_ctx* ctx, const int8_t* images, int64_t B, float* probs, float* enc_out,
                                       float* dec_out) {
    int rc = p1_check_call(ctx, images && probs, B);
    if (rc || B == 0) return rc;
    const int64_t chunk = pv_p1_chunk(ctx->p1->dtype, B, ctx->opt);
    if (B > chunk) {
        // host-buffer form in the bf16x3 mode and the split-6 chain: chunks (the taps are per-window, so chunking does not change them)
        for (int64_t b0 = 0; b0 < B; b0 += chunk) {
            const int64_t nb = std::min(chunk, B - b0);
            const size_t tap = (size_t)b0 * T_STEPS * 2 * H;
            int rcc = pv_rnn_forward_p1_debug(ctx, images + b0 * PV_WINDOW_BYTES, nb, probs + b0 * 3, enc_out ? enc_out + tap : nullptr,
                                              dec_out ? dec_out + tap : nullptr);
            if (rcc) return rcc;
        }
        return PV_OK;
    }
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    float *enc, *dec, *part, *d_probs;
    int8_t* d_img;
    if ((rc = p1_workspace(ctx, B, &enc, &dec, &part))) return rc;
    if ((rc = pv_get(ctx, "p1.images", (size_t)B * PV_WINDOW_BYTES, &d_img))) return rc;
    if ((rc = pv_get(ctx, "p1.probs", (size_t)B * 3, &d_probs))) return rc;
    PV_HIP(hipMemcpyAsync(d_img, images, (size_t)B * PV_WINDOW_BYTES, hipMemcpyHostToDevice, st));
    if ((rc = p1_forward_launch(ctx, d_img, B, d_probs, enc, dec, part, st, enc_out || dec_out))) return rc;
    PV_HIP(hipMemcpyAsync(probs, d_probs, (size_t)B * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    const size_t nb = (size_t)B * T_STEPS * 2 * H * sizeof(float);
    if (enc_out) PV_HIP(hipMemcpyAsync(enc_out, enc, nb, hipMemcpyDeviceToHost, st));
    if (dec_out) PV_HIP(hipMemcpyAsync(dec_out, dec, nb, hipMemcpyDeviceToHost, st));
    int n_timeouts = 0;
    PV_HIP(hipMemcpyAsync(&n_timeouts, ctx->p1->sp_err, sizeof(int), hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    if (n_timeouts) {   // only possible when the launch's workgroups could not all be resident (a GPU shared with other work)
        PV_HIP(hipMemset(ctx->p1->sp_err, 0, sizeof(int)));
        pv_set_error("unit-split LSTM form: %d exchange polls timed out (GPU shared with other work?); the probabilities of this call are NaN. "
                     "Set option shared_device = 1 (or lstm_split = 0) on this context", n_timeouts);
        return PV_ERR_STATE;
    }
    return PV_OK;
}

int pv_p2_take_timeouts(pv_ctx* ctx, int* n);   // rnn_gru.hip

extern "C" int pv_rnn_exchange_timeouts(pv_ctx* ctx) {
    PV_CHECK(ctx, PV_ERR_INVALID, "null argument");
    PV_HIP(hipSetDevice(ctx->device));
    PV_HIP(hipStreamSynchronize(ctx->stream));
    int n1 = 0, n2 = 0;
    if (ctx->p1 && ctx->p1->sp_err) {
        PV_HIP(hipMemcpy(&n1, ctx->p1->sp_err, sizeof(int), hipMemcpyDeviceToHost));
        if (n1) PV_HIP(hipMemset(ctx->p1->sp_err, 0, sizeof(int)));
    }
    int rc = pv_p2_take_timeouts(ctx, &n2);
    if (rc) return rc;
    return n1 + n2;
}

extern "C" int pv_rnn_forward_p1(pv_ctx* ctx, const int8_t* images, int64_t B, float* probs) {
    return pv_rnn_forward_p1_debug(ctx, images, B, probs, nullptr, nullptr);
}
