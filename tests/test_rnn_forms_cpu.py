"""The RNN kernel-form rules restated in tests/rnn_forms.py, pinned on a 256-CU chip with default options: a change of a
threshold in the library has to show up here, in review, as well as in the helper (tests/test_rnn_forms_gpu.py checks on the
GPU that the helper names the forms that run)."""
from collections import Counter

import rnn_forms as rf

# (last size of the old form, first of the new) per chain
SWITCHES_256 = {
    # unit split 4 -> 2 parts, k_head_splitk 33 -> 11 slabs, unit split -> one-workgroup 16 rows, f32 kernels -> split-6,
    # split-6 linear_1 split-K 16 -> 12 -> 11, k_head_tail 16 -> 32 rows, G past 4 GiB, chunks of 16384
    "p1_f32": [(512, 513), (736, 737), (1024, 1025), (2047, 2048), (2560, 2561), (2816, 2817), (8160, 8161), (15872, 15873),
               (16384, 16385)],
    # p1_f32x6_min_batch off: k_lstm_layer 16 -> 32 rows, k_head_tail 16 -> 32 rows
    "p1_f32_native": [(4064, 4065), (8160, 8161)],
    # f32 kernels -> bf16x3, linear_1 split-K 33 -> 22 -> 16 -> 12 -> 11 -> 8 -> 6 (k_head_tail -> k_tail_bf16, 32 -> 64-row
    # tiles between) -> 4 -> 3, G past 4 GiB, -> 2, chunks of 16384
    "p1_bf16x3": [(512, 513), (1280, 1281), (1792, 1793), (2560, 2561), (2816, 2817), (3840, 3841), (4032, 4033), (4096, 4097),
                  (5376, 5377), (7936, 7937), (10752, 10753), (15872, 15873), (16128, 16129), (16384, 16385)],
    # k_gru_us -> direction split -> one workgroup 16 rows -> 32 rows
    "p2_f32": [(1024, 1025), (2048, 2049), (8160, 8161)],
    # k_gru16_bf16 -> k_rec_bf16 32 rows, mt 1 -> 2, p2b.G past 4 GiB
    "p2_bf16x3": [(2048, 2049), (8192, 8193), (13952, 13953)],
}


def test_switches_on_256_cus():
    assert rf.switches(256) == SWITCHES_256


def test_boundaries_are_both_sides_of_every_switch_plus_production_sizes():
    b = rf.boundaries(256)
    assert set(b) == set(SWITCHES_256)
    for chain, sw in SWITCHES_256.items():
        assert b[chain] == sorted({n for pair in sw for n in pair} | set(rf.EXTRA.get(chain, ())))
    assert 16484 in b["p1_f32"] and 16484 in b["p1_bf16x3"] and 2121 in b["p2_bf16x3"]


def test_p1_forms_on_256_cus():
    f = lambda dt, B: rf.p1_launch_form(dt, B, 256)
    assert (f(rf.F32, 512).lstm, f(rf.F32, 513).lstm, f(rf.F32, 1024).lstm, f(rf.F32, 1025).lstm) == ("split4", "split2", "split2", "rows16")
    assert (f(rf.F32, 736).splits, f(rf.F32, 737).splits) == (33, 11)
    assert (f(rf.F32, 2047).chain, f(rf.F32, 2048).chain, f(rf.F32, 2048).splits, f(rf.F32, 2561).splits, f(rf.F32, 2817).splits) == \
        ("f32", "x6", 16, 12, 11)
    assert (f(rf.F32, 8160).tail_rows, f(rf.F32, 8161).tail_rows) == (16, 32)
    assert f(rf.F32, 15872).g_bytes <= rf.GIB4 < f(rf.F32, 15873).g_bytes
    native = {"p1_f32x6_min_batch": 1 << 24}
    assert [rf.p1_launch_form(rf.F32, B, 256, native).rows for B in (4064, 4065)] == [16, 32]
    assert rf.p1_launch_form(rf.F32, 3000, 256, {"lstm_rows": 16}).chain == "f32"   # an explicit tile form keeps the f32 kernels
    assert (f(rf.BF16X3, 512).chain, f(rf.BF16X3, 513).chain) == ("f32", "bf16x3")
    assert [f(rf.BF16X3, B).splits for B in (1280, 1281, 1793, 2561, 2817, 3841, 5377, 7937, 10753, 16129)] == \
        [33, 22, 16, 12, 11, 8, 6, 4, 3, 2]
    assert (f(rf.BF16X3, 4032).tail, f(rf.BF16X3, 4033).tail) == ("k_head_tail", "k_tail_bf16")
    assert (f(rf.BF16X3, 4096).mt, f(rf.BF16X3, 4097).mt) == (1, 2)
    assert f(rf.BF16X3, 15872).g_bytes <= rf.GIB4 < f(rf.BF16X3, 15873).g_bytes
    assert f(rf.BF16X3, 16384).g_bytes > rf.GIB4


def test_p1_chunks_and_names():
    call = rf.p1_call(rf.F32, 16484, 256)
    assert [(b0, nb, f.chain, f.lstm) for b0, nb, f in call] == [(0, 16384, "x6", None), (16384, 100, "f32", "split4")]
    names = sum((f.names for _, _, f in call), Counter())
    assert names == Counter({"k_rec_x6_lstm_enc": 1, "k_lstm_layer_dec": 1, "k_gemm_bf16x6_dec": 1, "k_rec_x6_lstm_dec": 1,
                             "k_gemm_bf16x6_lin1": 1, "k_head_tail": 2, "k_lstm_split_enc": 1, "k_lstm_split_dec": 1,
                             "k_head_splitk": 1})
    assert [(nb, f.chain) for _, nb, f in rf.p1_call(rf.BF16X3, 16484, 256)] == [(16384, "bf16x3"), (100, "f32")]
    assert len(rf.p1_call(rf.F32, 16484, 256, {"p1_f32x6_min_batch": 1 << 24})) == 1   # the f32 kernels do not chunk


def test_p2_forms_on_256_cus():
    f = lambda dt, B, **o: rf.p2_call(dt, B, 256, o)
    assert [(f(rf.F32, B).kind, f(rf.F32, B).rows) for B in (1024, 1025, 2048, 2049, 8160, 8161)] == \
        [("us", 16), ("dsplit", 16), ("dsplit", 16), ("wg", 16), ("wg", 16), ("wg", 32)]
    assert [(f(rf.BF16X3, B).kind, f(rf.BF16X3, B).rows) for B in (2048, 2049, 8192, 8193)] == \
        [("gru16", 16), ("rec", 32), ("rec", 32), ("rec", 64)]
    assert f(rf.BF16X3, 13952).g_bytes <= rf.GIB4 < f(rf.BF16X3, 13953).g_bytes
    assert f(rf.BF16X3, 2121).names == Counter({"k_rec_bf16_gru_enc": 19, "k_gemm_bf16x3_gru_dec": 19, "k_rec_bf16_gru_dec": 19,
                                                "k_p2_combine": 19})
    assert rf.p2_call(rf.BF16X3, 2049, 256, nwin=1).names["k_p2_combine"] == 1
    # options force the fp32 forms names cannot tell apart
    assert (f(rf.F32, 500, gru_split=0).kind, f(rf.F32, 500, gru_usplit=0).kind, f(rf.F32, 100, gru_rows=32).rows) == ("wg", "dsplit", 32)


def test_k_p2_dense_is_unreachable_on_256_cus():
    """the 32-row bf16x3 decoder without dense folding: its forms start at 2049 chunks, folding at 2048 - never on 256 CUs;
    on a smaller chip (here 128 CUs: 32-row forms from 1025 chunks) it runs below 2048 chunks"""
    assert all(rf.p2_call(rf.BF16X3, B, 256).dense == "combine" for B in range(1, 14100))
    assert rf.p2_call(rf.BF16X3, 1500, 128).dense == "dense" and rf.p2_call(rf.BF16X3, 1500, 128).names["k_p2_dense"] == 19


def test_sample_rows_cover_every_tile_position():
    r = rf.sample_rows(1000, [16, 32])
    assert {0, 15, 16, 31, 32, 999}.issubset(r)
    assert 992 in r and 991 in r and 960 in r   # partial last 32-row tile, last full tile
    assert 976 in r                             # last full 16-row tile starts
    assert rf.sample_rows(64, [64]) == [0, 63]
    rows = rf.p1_sample_rows(rf.p1_call(rf.F32, 16484, 256))
    assert {16352, 16383, 16384, 16399, 16400, 16483}.issubset(rows) and max(rows) == 16483
