"""Diagnostic: phase cycle sums of k_rec_bf16 and the clock it ran at (needs a -DPV_REC_STAMPS variant, e.g.
PEPPER_HIP_LIB=variants/libpepper_hip_recstamps.so; with -DPV_REC_X6_MFMA32 as well: the split-6 form on 32x32x16).

  rec_stamps.py          the bf16x3 forms of P1 and P2
  rec_stamps.py x6       the split-6 LSTM form (fp32 P1 at 8192 windows): phase sums, and the held clock = s_memtime ticks per
                         s_memrealtime tick x 100 MHz around the step loops, after two seconds of back-to-back calls
  rec_stamps.py tail     the six-term tail of the split-6 chain (k_tail_bf16<X6>) at 8192 windows: phase sums of a launch"""
import sys, os, time, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from pepper_thesis_amd import runtime, synth, _ffi
lib = _ffi.load()
lib.pv_debug_rec_stamps.argtypes = [C.POINTER(C.c_ulonglong)]
lib.pv_debug_rec_clock.argtypes = [C.POINTER(C.c_ulonglong)]
def stamps():
    o = (C.c_ulonglong * 5)()
    lib.pv_debug_rec_stamps(o)
    return [int(v) for v in o]
def clock_ghz():
    """read BEFORE stamps(), which resets"""
    o = (C.c_ulonglong * 2)()
    lib.pv_debug_rec_clock(o)
    return 0.1 * o[0] / max(int(o[1]), 1)
names = ["x issue", "mfma", "cell", "init", "barrier"]
def show(tag, nwaves, steps):
    ghz = clock_ghz()
    v = stamps(); tot = sum(v)
    print(tag, "cycles per step and wave:", {n: round(x / nwaves / steps) for n, x in zip(names, v)}, "total", round(tot / nwaves / steps),
          "clock %.3f GHz" % ghz, flush=True)
dev = "cuda:0"
ctx = runtime.Context(0)
if sys.argv[1:] == ["x6"]:
    B, CALLS = 8192, 20
    ctx.load_p1(synth.make_weights_p1(5, 2.0), _ffi.PV_DTYPE_F32)
    x = torch.from_numpy(synth.synth_windows(10, B)).to(dev); p = torch.zeros((B, 3), dtype=torch.float32, device=dev)
    t0 = time.time()
    while time.time() - t0 < 2.0:
        for _ in range(16): ctx.forward_p1_dev(x.data_ptr(), B, p.data_ptr())
        ctx.synchronize()
    stamps()
    for _ in range(CALLS): ctx.forward_p1_dev(x.data_ptr(), B, p.data_ptr())
    ctx.synchronize()
    show("P1 split-6 B=%d enc+dec (2 launches)" % B, 8, 66 * CALLS)
    sys.exit(0)
if sys.argv[1:] == ["tail"]:
    # the six-term tail of the split-6 chain (k_tail_bf16<X6>, 32-row k_head_tail plans): cycles per launch and wave of workgroup 0
    B, CALLS = 8192, 20
    lib.pv_debug_tail_stamps.argtypes = [C.POINTER(C.c_ulonglong)]
    ctx.load_p1(synth.make_weights_p1(5, 2.0), _ffi.PV_DTYPE_F32)
    x = torch.from_numpy(synth.synth_windows(10, B)).to(dev); p = torch.zeros((B, 3), dtype=torch.float32, device=dev)
    for _ in range(4): ctx.forward_p1_dev(x.data_ptr(), B, p.data_ptr())
    o = (C.c_ulonglong * 5)()
    lib.pv_debug_tail_stamps(o)
    for _ in range(CALLS): ctx.forward_p1_dev(x.data_ptr(), B, p.data_ptr())
    lib.pv_debug_tail_stamps(o)
    v = [int(t) for t in o]
    print("tail x6 B=%d cycles per launch and wave:" % B,
          dict(zip(["slab sum", "rings", "ring wait", "write-back", "output"], [round(t / 8 / CALLS) for t in v])), "total", round(sum(v) / 8 / CALLS), flush=True)
    sys.exit(0)
ctx.load_p1(synth.make_weights_p1(5, 2.0), _ffi.PV_DTYPE_BF16_INPUT_GEMM)
for B in (2048, 8192):
    x = torch.from_numpy(synth.synth_windows(10, B)).to(dev); p = torch.zeros((B, 3), dtype=torch.float32, device=dev)
    ctx.forward_p1_dev(x.data_ptr(), B, p.data_ptr()); ctx.synchronize(); stamps()
    ctx.forward_p1_dev(x.data_ptr(), B, p.data_ptr()); ctx.synchronize()
    show("P1 B=%d enc+dec (2 launches)" % B, 8, 66)
ctx.load_p2(synth.make_weights_p2(17, 2.0), _ffi.PV_DTYPE_BF16_INPUT_GEMM)
for B in (64, 4096):
    y = torch.from_numpy(synth.synth_p2_images(20, B)).to(dev); l = torch.zeros((B, 1000), dtype=torch.uint8, device=dev); a = torch.zeros((B, 1000, 5), dtype=torch.float32, device=dev)
    ctx.forward_p2_dev(y.data_ptr(), B, l.data_ptr(), a.data_ptr()); ctx.synchronize(); stamps()
    ctx.forward_p2_dev(y.data_ptr(), B, l.data_ptr(), a.data_ptr()); ctx.synchronize()
    show("P2 B=%d enc+dec (38 launches)" % B, 4, 3800)
