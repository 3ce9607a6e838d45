"""Test helper (no tests here): the kernel-form selection rules of the RNN library restated in plain Python.

Given (model, dtype, batch size, CU count, options) the functions below say what the library launches: which chain, the tile
rows of the recurrent kernels, the split parts, `mt`, the split-K factor of linear_1, the tail kernel, the chunks a call is
cut into and the profile names (pv_profile_*) the launch must show. They restate, by hand and independently, the plan header the
library's launchers consume, pepper_thesis_amd/csrc/rnn_plan.hpp: pv_p1_chunk (chunking), pv_p1_use_x6, pv_plan_p1 (P1) and
pv_plan_p2 (P2); the profile names are those of the launchers (rnn_lstm.hip, rnn_head.hip, rnn_gemm.hip, rnn_gru.hip, rnn_rec_bf16.hip).
tests/test_rnn_plan_cpu.py holds the two against each other at every batch size, without a GPU.
`boundaries(num_cu)` walks every batch size up to the largest switch and yields the sizes on either side of each change of
form. tests/test_rnn_forms_cpu.py pins what it yields on 256 CUs; tests/test_rnn_forms_gpu.py runs the kernels at those sizes
and checks that the forms named here are the ones that ran."""
from collections import Counter, namedtuple

F32, BF16X3 = "f32", "bf16x3"   # model dtypes (PV_DTYPE_F32, PV_DTYPE_BF16_INPUT_GEMM)

# the library's option defaults (pv_opts, pv_common.hpp) for the options that steer a form
DEFAULTS = {"lstm_split": 1, "lstm_rows": 0, "tail_rows": 0, "head_splits": 0, "shared_device": 0, "gru_rows": 0,
            "gru_split": 1, "gru_usplit": 1, "p1_bf16_min_batch": 513, "p1_f32x6_min_batch": 2048}
OPTION_NAMES = tuple(DEFAULTS)

P1_CHUNK = 16384             # P1_BF16_MAX_BATCH: windows per launch of the bf16x3 chain and of the split-6 chain
P1_ROWS = 32                 # ROWS: the 32-row tile every P1 buffer is counted in
P1_T = 33                    # time steps of a P1 window
SP_MAX_TILES = 64            # 16-row tiles the unit-split exchange buffers are sized for
GEMM_M_TILE = 256            # output rows of one k_gemm_bf16x3 / k_gemm_bf16x6 work item
TAIL_BF16_ROWS = 64          # TL_ROWS of k_tail_bf16
P2_WIN, P2_NWIN = 100, 19    # time steps of a P2 window, windows of a 1000-column chunk
GIB4 = 1 << 32

# the form of one P1 launch (one chunk of a call)
#   chain   "f32" (k_lstm_* + k_head_splitk), "x6" (the split-6 chain of the fp32 mode), "bf16x3"
#   lstm    f32 chain: "split4" / "split2" (k_lstm_split, 4 or 2 parts of the hidden units) or "rows16" / "rows32"
#           (k_lstm_layer); None on the other chains
#   rows    rows of a recurrent tile (16 / 32; 64 = the bf16x3 chain's mt = 2 tiles)
#   mt      32-row tiles per workgroup of k_rec_bf16 (1 or 2; 1 on the x6 chain, None on the f32 chain)
#   splits  split-K factor of linear_1: k_head_splitk's slabs (f32) or the split-K GEMM's (x6, bf16x3)
#   tail    "k_head_tail" or "k_tail_bf16", with tail_rows rows per workgroup
#   g_bytes bytes of the decoder input projections G (x6, bf16x3; 0 on the f32 chain)
P1Form = namedtuple("P1Form", "chain lstm rows mt splits tail tail_rows g_bytes names")
# one P2 call
#   kind    fp32: "us" (k_gru_us, unit split), "dsplit" (k_gru_p2, two workgroups per tile), "wg" (k_gru_p2, one workgroup);
#           bf16x3: "gru16" (k_gru16_bf16) or "rec" (k_rec_bf16)
#   rows    tile rows (16 / 32 / 64)
#   mt      bf16x3 k_rec_bf16 tiles per workgroup (None elsewhere)
#   dense   bf16x3: "combine" (dense1 folded into the decoder, k_p2_combine) or "dense" (k_p2_dense); None for fp32
P2Form = namedtuple("P2Form", "kind rows mt dense g_bytes names")


def _opts(options):
    o = dict(DEFAULTS)
    if options:
        o.update(options)
    return o


def _ceil(a, b):
    return -(-a // b)


def p1_use_x6(dtype, B, o):
    return dtype == F32 and not o["lstm_rows"] and B >= o["p1_f32x6_min_batch"]


def launch_tail(n_tiles32, num_cu, o):
    tr = 32 if n_tiles32 >= num_cu else 16
    return o["tail_rows"] or tr


def _first_div(divs, tiles, num_cu, fallback=33):
    for dv in divs:
        if tiles * dv >= num_cu:
            return dv
    return fallback


def p1_launch_form(dtype, B, num_cu, options=None):
    """the form of ONE p1_forward_launch of B windows (B <= P1_CHUNK where the chain chunks)"""
    o = _opts(options)
    n_tiles = _ceil(B, P1_ROWS)
    if p1_use_x6(dtype, B, o):
        Bp = n_tiles * P1_ROWS
        gs = _first_div((11, 12, 16, 22, 24, 33), _ceil(Bp, 256) * 2, num_cu)
        tr = launch_tail(n_tiles, num_cu, o)
        names = Counter({"k_rec_x6_lstm_enc": 1, "k_lstm_layer_dec": 1, "k_gemm_bf16x6_dec": 1, "k_rec_x6_lstm_dec": 1,
                         "k_gemm_bf16x6_lin1": 1, "k_head_tail": 1})
        return P1Form("x6", None, 32, 1, gs, "k_head_tail", tr, Bp * P1_T * 2048 * 4, names)
    if dtype == BF16X3 and B >= o["p1_bf16_min_batch"]:
        mt = 2 if n_tiles * 2 > num_cu else 1
        Bp = _ceil(B, 32 * mt) * 32 * mt
        gs = _first_div((1, 2, 3, 4, 6, 8, 11, 12, 16, 22, 24, 33), _ceil(Bp, 256) * 2, num_cu)
        names = Counter({"k_rec_bf16_lstm_enc": 1, "k_gemm_bf16x3_dec": 1, "k_rec_bf16_lstm_dec": 1, "k_gemm_bf16x3_lin1": 1})
        if _ceil(B, 64) < num_cu // 4:
            tail, tr = "k_head_tail", launch_tail(n_tiles, num_cu, o)
        else:
            tail, tr = "k_tail_bf16", TAIL_BF16_ROWS
        names[tail] += 1
        return P1Form("bf16x3", None, 32 * mt, mt, gs, tail, tr, Bp * P1_T * 2048 * 4, names)
    # the fp32 kernels (the fp32 mode, and small calls of the bf16x3 mode)
    tr = 32 if n_tiles * 2 >= num_cu else 16
    if o["lstm_rows"]:
        tr = o["lstm_rows"]
    n_t16 = n_tiles * 2
    sp_ns = 4 if n_t16 * 2 * 4 <= num_cu else 2
    split = n_t16 <= SP_MAX_TILES and n_t16 * 2 * sp_ns <= num_cu
    if not o["lstm_split"] or o["lstm_rows"] or o["shared_device"]:
        split = False
    splits = o["head_splits"] or (11 if n_tiles * 11 >= num_cu else 33)
    ttr = launch_tail(n_tiles, num_cu, o)
    if split:
        lstm, rows = "split%d" % sp_ns, 16
        names = Counter({"k_lstm_split_enc": 1, "k_lstm_split_dec": 1})
    else:
        lstm, rows = "rows%d" % tr, tr
        names = Counter({"k_lstm_layer_enc": 1, "k_lstm_layer_dec": 1})
    names.update({"k_head_splitk": 1, "k_head_tail": 1})
    return P1Form("f32", lstm, rows, None, splits, "k_head_tail", ttr, 0, names)


def p1_chunks(dtype, B, options=None):
    """[(first window, windows)] of the launches a call of B windows is cut into (pv_rnn_forward_p1_dev)"""
    o = _opts(options)
    chunk = P1_CHUNK if (dtype == BF16X3 or p1_use_x6(dtype, B, o)) else B
    return [(b0, min(chunk, B - b0)) for b0 in range(0, B, chunk)]


def p1_call(dtype, B, num_cu, options=None):
    """[(first window, windows, P1Form)] of a call of B windows"""
    return [(b0, nb, p1_launch_form(dtype, nb, num_cu, options)) for b0, nb in p1_chunks(dtype, B, options)]


def p2_call(dtype, B, num_cu, options=None, nwin=P2_NWIN):
    """the P2Form of a call of B chunks (nwin = 1: the single-window operator, pv_rnn_forward_p2_window)"""
    o = _opts(options)
    if dtype == BF16X3:
        mt = 2 if _ceil(B, 32) * 2 > 2 * num_cu else 1
        tr16 = _ceil(B, 16) * 2 <= num_cu
        rows = 16 if tr16 else 32 * mt
        Bp = _ceil(B, rows) * rows
        # dense1 folded into the decoder in the 16-row form always, in the 32-row forms from 2048 chunks on. The 32-row forms
        # start where the 16-row form's (tile, direction) workgroups no longer fit the chip: 2049 chunks on 256 CUs, where
        # folding already holds - k_p2_dense cannot run there (it can on a chip of fewer than 256 CUs)
        fold = True if tr16 else B >= 2048
        kind = "gru16" if tr16 else "rec"
        pre = "k_gru16_bf16_" if tr16 else "k_rec_bf16_gru_"
        dense = "combine" if fold else "dense"
        names = Counter({pre + "enc": nwin, "k_gemm_bf16x3_gru_dec": nwin, pre + "dec": nwin, "k_p2_" + dense: nwin})
        return P2Form(kind, rows, None if tr16 else mt, dense, P2_WIN * Bp * 6 * 128 * 4, names)
    tr = 32 if _ceil(B, 32) >= num_cu else 16
    if o["gru_rows"]:
        tr = o["gru_rows"]
    n_tiles = _ceil(B, tr)
    split = tr == 16 and 2 * n_tiles <= num_cu and o["gru_split"] and not o["shared_device"]
    usplit = tr == 16 and 4 * n_tiles <= num_cu and o["gru_usplit"] and o["gru_split"] and not o["shared_device"]
    if usplit:
        return P2Form("us", 16, None, None, 0, Counter({"k_gru_us": 1}))
    return P2Form("dsplit" if split else "wg", tr, None, None, 0, Counter({"k_gru_p2": 1}))


# options that force a P2 fp32 form wherever the library can run it (names cannot tell k_gru_p2's three forms apart)
P2_FORCE = {("dsplit", 16): {"gru_usplit": 0, "gru_rows": 16}, ("wg", 16): {"gru_split": 0, "gru_rows": 16},
            ("wg", 32): {"gru_rows": 32}}


def p1_tiles(form):
    """the row granularities a P1 launch's kernels tile the batch in: each is a place where a tile edge can go wrong"""
    t = {form.rows, form.tail_rows, P1_ROWS}
    if form.chain != "f32":
        t.add(GEMM_M_TILE)
    return sorted(t)


def p2_tiles(form):
    return sorted({form.rows, 16, 32} if form.kind in ("us", "dsplit") else {form.rows})


def sample_rows(B, tiles, b0=0):
    """rows spread over a launch of B rows starting at b0: row 0, both sides of the first tile edge, a tile edge in the middle,
    the first and last rows of the last full tile, the first row of a partial last tile, row B - 1"""
    r = {0, B - 1}
    for T in tiles:
        full = B // T
        r.update((T - 1, T))
        if full >= 2:
            mid = full // 2 * T
            r.update((mid - 1, mid, (full - 1) * T, full * T - 1))
        if full * T < B:
            r.add(full * T)
    return sorted(b0 + i for i in r if 0 <= i < B)


def p1_sample_rows(call):
    return sorted({i for b0, nb, f in call for i in sample_rows(nb, p1_tiles(f), b0)})


def _scan(form_of, lo, hi):
    """[(last size of the old form, first of the new)] over batch sizes lo..hi"""
    out, prev = [], form_of(lo)
    for B in range(lo + 1, hi + 1):
        cur = form_of(B)
        if cur != prev:
            out.append((B - 1, B))
        prev = cur
    return out


def switches(num_cu, options=None):
    """{chain: [(N - 1, N), ...]}: every change of form, N the first size of the new form"""
    o = _opts(options)
    hi1 = P1_CHUNK + 100   # past the first chunk boundary: the remainder's form is the same for all of 1 .. 100 windows

    def p1(dtype, opt):
        def key(B):
            call = p1_call(dtype, B, num_cu, opt)
            return (len(call),) + tuple((f.chain, f.lstm, f.rows, f.mt, f.splits, f.tail, f.tail_rows, f.g_bytes > GIB4)
                                        for _, _, f in call)
        return key

    def p2(dtype):
        def key(B):
            f = p2_call(dtype, B, num_cu, o)
            return (f.kind, f.rows, f.mt, f.dense, f.g_bytes > GIB4)
        return key

    native = dict(o, p1_f32x6_min_batch=1 << 24)
    hi2 = 14100            # past the size where p2b.G outgrows 4 GiB
    return {
        "p1_f32": _scan(p1(F32, o), 1, hi1),
        # the fp32 kernels beyond the split-6 threshold: where the default fp32 chain no longer runs them
        "p1_f32_native": [s for s in _scan(p1(F32, native), 1, hi1) if s[1] > o["p1_f32x6_min_batch"]],
        "p1_bf16x3": _scan(p1(BF16X3, o), 1, hi1),
        "p2_f32": _scan(p2(F32), 1, hi2),
        "p2_bf16x3": _scan(p2(BF16X3), 1, hi2),
    }


# production sizes that sit near a switch without being one
EXTRA = {"p1_f32": (P1_CHUNK + 100,), "p1_bf16x3": (P1_CHUNK + 100,), "p2_bf16x3": (2121,)}


def boundaries(num_cu, options=None):
    """{chain: sorted batch sizes}: N - 1 and N on either side of every switch, plus EXTRA"""
    out = {}
    for chain, sw in switches(num_cu, options).items():
        s = {b for pair in sw for b in pair}
        s.update(EXTRA.get(chain, ()))
        out[chain] = sorted(s)
    return out
