"""GPU: the split-6 LSTM layers (k_rec_bf16<4, ., 1, true>) on v_mfma_f32_16x16x32_bf16. The fragment maps of that shape differ
from the 32x32x16 form's in every index - A rows (lane & 15 of two 16-row tiles), k-groups (lane >> 4 of a k-step of 32), the
weight slots (k-step, gate, column half) and the accumulators [row tile][gate][column half] - so the shapes here are chosen for
what a wrong map would break. The split-6 chain is forced (p1_f32x6_min_batch = 1), T is the model's 33.

1. B = 32 and B = 64 (one and two full tiles), EVERY row: probabilities and both layer taps against the float64 oracle under
   tests/rnn_budget.py's budget (FACTOR) and under the suite's absolute bars (1e-4, 2e-5), at both gains. A swapped row tile,
   column half or k-group moves whole rows or columns of a tap by O(0.1).
2. B = 17 (one tile whose rows 17-31 replicate row 16): rows 0-16 within the same budget. The entry point hands back B rows, so
   the tile's other rows are looked at through a B = 32 call whose windows 17-31 ARE window 16: the kernel computes on the same
   tile contents, all 32 rows of both taps are finite, rows 17-31 equal row 16 bit for bit, and the B = 17 call equals that call's
   rows 0-16 bit for bit.
3. Structured weights: W_hh of both layers is zero except one 16 x 32 block (16 units of one gate, one column half of one wave,
   one k-step of 32 inputs), the biases are the synthetic model's; B = 32. The block runs through all 4 gates x 2 halves x 8
   k-steps of wave 3 and, in wave 6 (the other priority half of the workgroup), through the first and last k-step of every
   (gate, half): 80 weight loads at 0.17 s each, as five cases of 16. Both taps must meet the float64 oracle
   (oracle/rnn_oracle.py's bilstm: the layers without the head) within the same budget and bar: a slot whose fragment met
   another accumulator, or other A columns, than it was packed for changes 16 columns of the tap by O(0.1).
4. The launches are the six of the split-6 chain (X6_NAMES of tests/test_rec_x6_phased_gpu.py)."""
from collections import Counter

import numpy as np
import pytest

import rnn_budget as bud
from oracle import rnn_oracle
from pepper_thesis_amd import _ffi, runtime, synth
from test_rec_x6_phased_gpu import X6_NAMES

pytestmark = pytest.mark.gpu
TOL, TOL_TAPS = 1e-4, 2e-5
H = 256
N = 64


@pytest.fixture(scope="module")
def x64():
    return synth.synth_windows(4264, N)


@pytest.fixture(scope="module")
def restated(x64):
    return {g: bud.restated_p1(g, x64) for g in bud.GAINS}


@pytest.fixture
def ctx6():
    ctx = runtime.Context(0)
    keep = ctx.get_option("p1_f32x6_min_batch")
    ctx.set_option("p1_f32x6_min_batch", 1)
    yield ctx
    ctx.set_option("p1_f32x6_min_batch", keep)
    ctx.close()


def forward(ctx, x):
    """(probs, enc, dec) of one profiled call; the launches must be the split-6 chain's"""
    ctx.profile_begin()
    out = ctx.forward_p1(x, taps=True)
    names = Counter({k: n for k, (_, n) in ctx.profile_end().items()})
    assert names == X6_NAMES, names
    return out


def within_budget(got, ref, plain, rows, what):
    """every output is measured and printed before the first failure is raised"""
    fails = []
    for k, (name, bar) in enumerate((("probs", TOL), ("enc", TOL_TAPS), ("dec", TOL_TAPS))):
        if got[k] is None:
            continue
        tag = "%s %s" % (what, name)
        try:
            bud.budget(got[k], ref[k], plain[k], bud.FACTOR, tag, rows)
            err = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
            assert err <= bar, "%s: %.3g from float64 (bar %g)" % (tag, err, bar)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B", [32, 64])
@pytest.mark.parametrize("g", bud.GAINS)
def test_every_row_of_full_tiles_within_budget(g, B, ctx6, x64, restated):
    ctx6.load_p1(bud.weights_p1(g), _ffi.PV_DTYPE_F32)
    got = forward(ctx6, x64[:B])
    assert np.abs(got[0].sum(1) - 1).max() < 1e-5
    rows = list(range(B))
    within_budget(got, restated[g](rows, "f64"), restated[g](rows, "f32"), rows, "P1 split-6 16x16x32 g=%d B=%d" % (g, B))


@pytest.mark.parametrize("g", bud.GAINS)
def test_partial_tile_and_its_replica_rows(g, ctx6, x64, restated):
    B = 17
    ctx6.load_p1(bud.weights_p1(g), _ffi.PV_DTYPE_F32)
    got = forward(ctx6, x64[:B])
    rows = list(range(B))
    within_budget(got, restated[g](rows, "f64"), restated[g](rows, "f32"), rows, "P1 split-6 16x16x32 g=%d B=%d" % (g, B))
    xr = x64[:32].copy()
    xr[B:] = xr[B - 1]                        # the tile as the kernels see it at B = 17
    full = forward(ctx6, xr)
    for name, a, b in zip(("probs", "enc", "dec"), got, full):
        assert np.isfinite(b).all(), name
        assert np.array_equal(a.view(np.uint32), b[:B].view(np.uint32)), name
        assert np.array_equal(b[B:].view(np.uint32), np.broadcast_to(b[B - 1], b[B:].shape).view(np.uint32)), name


def block_weights(base, wave, gate, half, ks):
    """`base` with W_hh of both layers and directions zero except rows gate * 256 + 32 wave + 16 half + [0, 16), columns
    32 ks + [0, 32): N(0, 0.5), another draw per tensor"""
    rng = np.random.default_rng(1000 * wave + 100 * gate + 10 * half + ks)
    w = dict(base)
    for layer in ("encoder", "decoder"):
        for sfx in ("", "_reverse"):
            m = np.zeros((4 * H, H), np.float32)
            r0 = gate * H + 32 * wave + 16 * half
            m[r0:r0 + 16, 32 * ks:32 * ks + 32] = rng.normal(0.0, 0.5, (16, 32)).astype(np.float32)
            w[layer + ".weight_hh_l0" + sfx] = m
    return w


def layers(w, x, dtype):
    wd = {k: np.asarray(v, dtype=dtype) for k, v in w.items() if k.startswith(("encoder.", "decoder."))}
    enc = rnn_oracle.bilstm(np.asarray(x).astype(dtype), wd, "encoder")
    return enc, rnn_oracle.bilstm(enc, wd, "decoder")


WAVE, WAVE2 = 3, 6
BLOCK_SETS = {"gate%d" % gate: [(WAVE, gate, half, ks) for half in range(2) for ks in range(8)] for gate in range(4)}
BLOCK_SETS["wave%d" % WAVE2] = [(WAVE2, gate, half, ks) for gate in range(4) for half in range(2) for ks in (0, 7)]


@pytest.mark.parametrize("which", sorted(BLOCK_SETS))
def test_one_block_of_w_hh_through_every_slot(which, ctx6, x64):
    base = synth.make_weights_p1(5, 2.0)
    x = x64[:32]
    rows = list(range(32))
    fails = []
    for wave, gate, half, ks in BLOCK_SETS[which]:
        w = block_weights(base, wave, gate, half, ks)
        ctx6.load_p1(w, _ffi.PV_DTYPE_F32)
        _, enc, dec = forward(ctx6, x)
        ref, plain = layers(w, x, np.float64), layers(w, x, np.float32)
        what = "block wave %d gate %d half %d k-step %d" % (wave, gate, half, ks)
        try:
            within_budget((None, enc, dec), (None,) + ref, (None,) + plain, rows, what)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "%d of %d blocks:\n%s" % (len(fails), len(BLOCK_SETS[which]), "\n".join(fails[:8]))


def test_launch_names_are_the_split6_chain(ctx6, x64):
    ctx6.load_p1(synth.make_weights_p1(5, 2.0), _ffi.PV_DTYPE_F32)
    ctx6.profile_begin()
    ctx6.forward_p1(x64[:32])
    names = Counter({k: n for k, (_, n) in ctx6.profile_end().items()})
    assert names == X6_NAMES, names
