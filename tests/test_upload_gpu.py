"""GPU: the two ways a host batch reaches the device-resident builders - pv_upload_batch (one batch) and pv_upload_batches
(the same regions in parts, one of them empty) - give what the host-buffer forms give, for the 26-plane and the haplotag
builder; and the polisher's host form equals its device form on the same batch."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
from pepper_thesis_amd import _ffi, synth
from pepper_thesis_amd.batch import PRESETS, hp_params, pack_regions
from pepper_thesis_amd.device import DeviceBatch, DeviceOut, DevicePolishOut

pytestmark = pytest.mark.gpu

P = PRESETS["ont_r9_guppy5_sup"]
P_HP = hp_params(P)
CAP = 512
PART_SIZES = (2, 0, 2)


def _regions():
    """four regions of 300 columns at depth ~8 with a planted site every ~40 columns; the second has no reads"""
    regs = [synth.synth_region(31 + g, region_len=300, depth=8, read_len=150, site_every=40, ref_start=50_000 + 1000 * g, safe=20)
            for g in range(4)]
    regs[1].reads = []
    return cases.tag_reads(regs, 7)


@pytest.fixture(scope="module")
def batches():
    regs = _regions()
    parts, g = [], 0
    for n in PART_SIZES:
        parts.append(pack_regions(regs[g:g + n]))
        g += n
    merged = pack_regions(regs)
    assert [p.n_regions for p in parts] == list(PART_SIZES) and merged.n_regions == 4
    assert merged.read_off[2] == merged.read_off[1] and merged.n_reads > 0
    return merged, parts


def _upload_parts(ctx, parts):
    """Context.upload_batches without its filter: the part of no regions reaches pv_upload_batches too"""
    cins = [b.as_c() for b in parts]
    arr = (C.POINTER(_ffi.pv_batch_in) * len(cins))(*[C.pointer(c) for c in cins])
    dev = _ffi.pv_batch_in()
    totals = (C.c_int64 * 4)()
    _ffi.check(ctx.lib.pv_upload_batches(ctx.handle, len(cins), arr, C.byref(dev), totals, None))
    return dev, [int(v) for v in totals], (cins, arr)


def _dev_out(hp):
    shape = (CAP, _ffi.PV_HP_WINDOW_ROWS, _ffi.PV_HP_FEATURES) if hp else (CAP, _ffi.PV_WINDOW_ROWS, _ffi.PV_FEATURES)
    return DeviceOut(CAP, 16 * CAP, images=torch.zeros(shape, dtype=torch.int8, device="cuda:0"))


def _run_uploaded(ctx, uploaded, hp, read_hp):
    dev, (n_reads, n_bases, n_cigar, n_ref), _keep = uploaded
    dout = _dev_out(hp)
    if hp:
        cp = P_HP.as_c()
        d_hp = torch.from_numpy(read_hp).to("cuda:0")
        _ffi.check(ctx.lib.pv_summarize_regions_hp_dev(ctx.handle, C.byref(dev), d_hp.data_ptr(), C.byref(cp), n_reads, n_bases,
                                                       n_cigar, n_ref, C.byref(dout.c), dout.counts.data_ptr(), None))
    else:
        ctx.summarize_uploaded(uploaded, P, dout)
    ctx.synchronize()
    assert dout.status() == 0
    return dout


def _assert_same(dout, exp, what):
    n = dout.n_out()
    assert n == len(exp) > 0, what
    for f in ("images", "region", "position", "depth", "cand_freq"):
        np.testing.assert_array_equal(getattr(dout, f)[:n].cpu().numpy(), getattr(exp, f), err_msg="%s: %s" % (what, f))
    off = dout.cand_off[:n + 1].cpu().numpy()
    raw = dout.cand_str[:int(off[-1])].cpu().numpy().tobytes().decode("latin-1")
    assert [raw[off[i]:off[i + 1]] for i in range(n)] == exp.candidates, what


@pytest.mark.parametrize("hp", [False, True], ids=["26-plane", "haplotag"])
def test_uploaded_batches_give_what_the_host_form_gives(hip_ctx, batches, hp):
    merged, parts = batches
    exp = hip_ctx.summarize_hp(merged, P_HP) if hp else hip_ctx.summarize(merged, P)
    assert len(exp) > 0 and set(np.unique(exp.region)) == {0, 2, 3}   # every region with reads gives windows, the empty one none
    totals = [merged.n_reads, merged.n_bases, merged.n_cigar, int(merged.ref.shape[0])]
    one = hip_ctx.upload_batch(merged)
    assert one[1] == totals
    _assert_same(_run_uploaded(hip_ctx, one, hp, merged.read_hp), exp, "pv_upload_batch")
    hip_ctx.synchronize()   # the previous upload's copies are done before the next one
    three = _upload_parts(hip_ctx, parts)
    assert three[1] == totals and three[0].n_regions == 4
    _assert_same(_run_uploaded(hip_ctx, three, hp, merged.read_hp), exp, "pv_upload_batches")


def test_polisher_host_form_equals_device_form(hip_ctx, batches):
    merged, _ = batches
    L, O = 100, 10
    exp = hip_ctx.polish_summarize(merged, L, O)
    n = exp.images.shape[0]
    assert n >= 4 * 3   # 300 columns and more rows per region, chunks of 100 rows stepping by 90
    dout = DevicePolishOut(n + 8, L, O)
    hip_ctx.polish_summarize_dev(DeviceBatch(merged), dout)
    hip_ctx.synchronize()
    assert dout.status() == 0 and dout.n_chunks() == n
    for f in ("images", "position", "index", "region", "chunk_id"):
        np.testing.assert_array_equal(getattr(dout, f)[:n].cpu().numpy(), getattr(exp, f), err_msg=f)
