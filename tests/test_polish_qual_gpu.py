"""GPU: the polisher's per-base quality: pv_polish_row_qual[_dev] and pv_polish_stitch_qual[_dev] against the host checker
(tests/qual_ref.py) byte for byte, `polish --qualities` and the three steps with --qualities end to end on a small BAM, and
the two kernels as a captured graph. Nothing here has a tolerance: the rule counts literal float32 thresholds."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import qual_ref as qr
from pepper_thesis_amd import _ffi, cli, pepper, polish, polish_steps, synth
from pepper_thesis_amd.batch import Read, Region, pack_regions
from pepper_thesis_amd.device import DevicePolishOut

pytestmark = pytest.mark.gpu
L, O = 1000, 50
KEY_ROWS = {1.0: (0, 49, 950, 999), 2.0: (50, 949, 63, 64)}     # the count boundaries and a wave boundary
MORE_ROWS = {1.0: range(1, 17), 2.0: list(range(100, 114)) + [255, 256]}   # every case once more; 255/256: a block boundary


# ---- row kernel -------------------------------------------------------------------------------------------------------

def _row_inputs(B, seed):
    """synthetic labels 0..4 and acc in [0, 2], with qr.threshold_rows() at the key rows of every chunk (a different case per
    chunk) and all of them on further rows -> (labels, acc)"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 5, (B, L)).astype(np.uint8)
    acc = (rng.random((B, L, 5), dtype=np.float32) * np.float32(2.0)).astype(np.float32)
    # a good share of confident rows, as P2 gives them: acc close to the count
    near = rng.random((B, L)) < 0.5
    acc[near] = np.float32(2.0) - (np.float32(10.0) ** -(rng.random((int(near.sum()), 5), dtype=np.float32) * 9)).astype(np.float32)
    cases = qr.threshold_rows()
    for cnt in (1.0, 2.0):
        mine = [c for c in cases if c[2] == cnt]
        for b in range(B):
            for i, r in enumerate(KEY_ROWS[cnt]):
                lb, v, _, _ = mine[(4 * (b + seed) + i) % len(mine)]
                labels[b, r], acc[b, r, lb] = lb, v
            for r, (lb, v, _, _) in zip(MORE_ROWS[cnt], mine):
                labels[b, r], acc[b, r, lb] = lb, v
    return labels, acc


def _dev_row_qual(ctx, labels, acc, shift=0):
    """the device-resident form on uploaded copies -> (qual, counts); shift: floats by which acc is moved off its 16-byte
    alignment (the kernel then stages with 4-byte loads)"""
    B = labels.shape[0]
    lab = torch.from_numpy(labels).cuda()
    buf = torch.zeros(acc.size + 4, dtype=torch.float32, device="cuda")
    a = buf[shift:shift + acc.size]
    a.copy_(torch.from_numpy(acc.ravel()))
    assert a.data_ptr() % 16 == 4 * shift
    qual = torch.full((B, L), 0xEE, dtype=torch.uint8, device="cuda")
    counts = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.polish_row_qual_dev(lab.data_ptr(), a.data_ptr(), B, qual.data_ptr(), counts.data_ptr(), L, O)
    ctx.synchronize()
    return qual.cpu().numpy(), counts.cpu().numpy().tolist()


@pytest.mark.parametrize("B", [1, 3])
def test_row_qual_equals_checker(hip_ctx, B):
    labels, acc = _row_inputs(B, seed=B)
    want = qr.row_qual(labels, acc, O)
    cases = {(c[2], c[0], c[1].tobytes()): c[3] for c in qr.threshold_rows()}
    for b in range(B):                                   # the planted rows hold what the hand-worked cases say
        for cnt in (1.0, 2.0):
            for r in list(KEY_ROWS[cnt]) + list(MORE_ROWS[cnt]):
                assert want[b, r] == cases[(cnt, int(labels[b, r]), acc[b, r, labels[b, r]].tobytes())], (b, r)
    assert len(np.unique(want)) > 40 and want.max() == 93 and want.min() == 0
    got = hip_ctx.polish_row_qual(labels, acc, O)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    for shift in (0, 1):
        dq, c = _dev_row_qual(hip_ctx, labels, acc, shift)
        assert c == [B * L, 0, -1, 0] and np.array_equal(dq, want), shift


def test_row_qual_label_255_is_an_error(hip_ctx):
    labels, acc = _row_inputs(3, seed=7)
    labels[1, 700] = 255
    labels[2, 3] = 9
    want = qr.row_qual(labels, acc, O)
    assert want[1, 700] == 0 and want[2, 3] == 0
    counts = (C.c_int64 * 4)()
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.polish_row_qual(labels, acc, O, counts=counts)
    assert e.value.code == _ffi.PV_ERR_STATE and "chunk 1, row 700" in str(e.value)
    assert list(counts) == [3 * L, _ffi.PV_ERR_STATE, 1, 700]
    dq, c = _dev_row_qual(hip_ctx, labels, acc)
    assert c == [3 * L, _ffi.PV_ERR_STATE, 1, 700] and np.array_equal(dq, want)


# ---- stitch with the plane ----------------------------------------------------------------------------------------------

def _stitch_case(ctx, seed=5):
    """regions of 13 chunks (a 12000-base insert: the 9/10 overlap), 1 chunk and 2 chunks, the last two with region_start > 0
    (their first 200 columns are dropped), random labels with label-0 runs on both sides of every overlap, row qualities that
    differ between the two chunks on every shared column"""
    rng = np.random.default_rng(seed)
    ins = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 12_000))
    regs = [Region(0, 299, b"A" * 300, [Read.make(10, "5M12000I60M", b"C" * 5 + ins + b"G" * 60), Read.make(0, "250M", "A" * 250)]),
            synth.synth_region(300, region_len=400, depth=8, read_len=300, site_every=50, ref_start=5000),
            synth.synth_region(301, region_len=1200, depth=8, read_len=500, site_every=50, ref_start=8000)]
    b = pack_regions(regs)
    out = ctx.polish_summarize(b)
    per_region = [int((out.region == g).sum()) for g in range(3)]
    assert per_region[0] >= 11 and per_region[1] == 1 and per_region[2] == 2, per_region
    for g in range(3):
        assert (out.position[out.region == g][-1] < 0).any()     # padding rows in a region's last chunk
    assert ((out.position[out.region == 2] >= 0) & (out.position[out.region == 2] <= 8200)).any()   # the dropped buffer
    n = len(out.chunk_id)
    labels = rng.integers(0, 5, (n, L)).astype(np.uint8)
    rq = rng.integers(0, 94, (n, L)).astype(np.uint8)
    for k in range(1, n):
        if out.region[k] == out.region[k - 1]:
            assert np.array_equal(out.position[k, :O], out.position[k - 1, L - O:]) and np.array_equal(out.index[k, :O], out.index[k - 1, L - O:])
            labels[k - 1, L - O - 10:L - O + 15] = 0             # a label-0 run into the overlap from the left chunk
            labels[k, O - 20:O + 10] = 0                         # and one out of it in the right chunk
            same = rq[k, :O] == rq[k - 1, L - O:]
            rq[k, :O][same] = (rq[k, :O][same] + 1) % 94
            assert (rq[k, :O] != rq[k - 1, L - O:]).all()
    return b, out, labels, rq


def _expected(b, out, labels, rq):
    spans = list(zip(b.ref_start.tolist(), b.ref_end.tolist()))
    regs = qr.regions_with_qual(out.position, out.index, out.region, out.chunk_id, labels, rq, spans)
    per = [qr.create_consensus_qual([r]) for r in regs]
    return [s.encode() for s, _ in per], [q for _, q in per]


def _dev_stitch_qual(ctx, out, labels, rq, region_start, capacity=None):
    n = len(out.chunk_id)
    do = DevicePolishOut(max(n, 1))
    for name in ("position", "index", "region", "chunk_id"):
        getattr(do, name)[:n].copy_(torch.from_numpy(getattr(out, name)))
    lab, drq = torch.from_numpy(labels).cuda(), torch.from_numpy(rq).cuda()
    rs = torch.from_numpy(np.asarray(region_start, np.int64)).cuda()
    cap = n * L if capacity is None else capacity
    seq = torch.full((max(cap, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    qual = torch.full((max(cap, 1),), 0xDD, dtype=torch.uint8, device="cuda")
    roff = torch.full((len(region_start) + 1,), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.polish_stitch_qual_dev(do, n, lab.data_ptr(), drq.data_ptr(), rs.data_ptr(), len(region_start), roff.data_ptr(),
                               seq.data_ptr(), qual.data_ptr(), cap, counts.data_ptr())
    ctx.synchronize()
    return roff.cpu().numpy(), seq.cpu().numpy(), qual.cpu().numpy(), counts.cpu().numpy().tolist()


def test_stitch_qual_equals_checker(hip_ctx):
    b, out, labels, rq = _stitch_case(hip_ctx)
    exp_seq, exp_q = _expected(b, out, labels, rq)
    exp_off = np.concatenate([[0], np.cumsum([len(s) for s in exp_seq])])
    total = int(exp_off[-1])
    roff0, seq0 = hip_ctx.polish_stitch(out, labels, b.ref_start)            # the stitch as it was
    assert seq0 == b"".join(exp_seq) and total > 10_000
    roff, seq, qual = hip_ctx.polish_stitch_qual(out, labels, rq, b.ref_start)
    assert np.array_equal(roff, roff0) and np.array_equal(roff, exp_off)
    assert seq == seq0 and qual == b"".join(exp_q)
    droff, dseq, dqual, c = _dev_stitch_qual(hip_ctx, out, labels, rq, b.ref_start)
    assert c == [total, 0, -1, 0] and np.array_equal(droff, exp_off)
    assert dseq[:total].tobytes() == seq0 and dqual[:total].tobytes() == qual
    assert (dseq[total:] == 0xEE).all() and (dqual[total:] == 0xDD).all()
    # chunk 9 beats chunk 10 on their shared columns: the bytes there are chunk 9's
    k9, k10 = (int(np.flatnonzero((out.region == 0) & (out.chunk_id == c_))[0]) for c_ in (9, 10))
    labels[k9, L - O:], labels[k10, :O] = 1, 4
    rq[k9, L - O:], rq[k10, :O] = 90, 5
    _, seq2, qual2 = hip_ctx.polish_stitch_qual(out, labels, rq, b.ref_start)
    exp_seq2, exp_q2 = _expected(b, out, labels, rq)
    assert seq2 == b"".join(exp_seq2) and qual2 == b"".join(exp_q2)
    assert bytes([90] * O) in qual2 and bytes([5] * O) not in qual2 and seq2 == hip_ctx.polish_stitch(out, labels, b.ref_start)[1]


def test_stitch_qual_capacity_and_poisoned_label(hip_ctx):
    b, out, labels, rq = _stitch_case(hip_ctx, seed=6)
    exp_seq, exp_q = _expected(b, out, labels, rq)
    exp_off = np.concatenate([[0], np.cumsum([len(s) for s in exp_seq])])
    total = int(exp_off[-1])
    droff, dseq, dqual, c = _dev_stitch_qual(hip_ctx, out, labels, rq, b.ref_start, capacity=total - 1)
    assert c[:2] == [total, _ffi.PV_ERR_CAPACITY] and np.array_equal(droff, exp_off)      # nothing written but region_off
    assert (dseq == 0xEE).all() and (dqual == 0xDD).all()
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.polish_stitch_qual(out, labels, rq, b.ref_start, seq_capacity=total - 1)
    assert e.value.code == _ffi.PV_ERR_CAPACITY and ("need %d bases" % total) in str(e.value)
    _, dseq, dqual, c = _dev_stitch_qual(hip_ctx, out, labels, rq, b.ref_start, capacity=total)
    assert c[:2] == [total, 0] and dseq.tobytes() == b"".join(exp_seq) and dqual.tobytes() == b"".join(exp_q)
    k = len(out.chunk_id) - 2
    assert out.region[k] == 2 and out.position[k, 700] > 8200
    labels[k, 700] = 255                                     # a kept column of a middle chunk
    _, dseq, dqual, c = _dev_stitch_qual(hip_ctx, out, labels, rq, b.ref_start)
    assert c[1:3] == [_ffi.PV_ERR_STATE, k] and (dseq == 0xEE).all() and (dqual == 0xDD).all()
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.polish_stitch_qual(out, labels, rq, b.ref_start)
    assert e.value.code == _ffi.PV_ERR_STATE


# ---- graph capture ------------------------------------------------------------------------------------------------------

def test_graph_of_row_qual_plus_stitch_qual(hip_ctx):
    """the two kernels of --qualities captured as one graph; replays on refilled labels and acc equal the eager calls"""
    b, out, _, _ = _stitch_case(hip_ctx, seed=8)
    n = len(out.chunk_id)
    do = DevicePolishOut(n)
    for name in ("position", "index", "region", "chunk_id"):
        getattr(do, name)[:n].copy_(torch.from_numpy(getattr(out, name)))
    rs = torch.from_numpy(b.ref_start.astype(np.int64)).cuda()
    fills = []
    for s in range(3):
        rng = np.random.default_rng(80 + s)
        lab = rng.integers(0, 5, (n, L)).astype(np.uint8)
        acc = (rng.random((n, L, 5), dtype=np.float32) * np.float32(2.0)).astype(np.float32)
        acc[:, ::3] = np.float32(2.0) - np.float32(10.0) ** -(rng.random((n, len(range(0, L, 3)), 5), dtype=np.float32) * 9)
        fills.append((lab, acc))
    lab_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    acc_d = torch.zeros((n, L, 5), dtype=torch.float32, device="cuda")
    rq_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    seq = torch.zeros(n * L, dtype=torch.uint8, device="cuda")
    qual = torch.zeros(n * L, dtype=torch.uint8, device="cuda")
    roff = torch.zeros(4, dtype=torch.int64, device="cuda")
    c_row = torch.zeros(4, dtype=torch.int64, device="cuda")
    c_st = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = hip_ctx.stream

    def pair():
        hip_ctx.polish_row_qual_dev(lab_d.data_ptr(), acc_d.data_ptr(), n, rq_d.data_ptr(), c_row.data_ptr(), L, O, stream=st)
        hip_ctx.polish_stitch_qual_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), 3, roff.data_ptr(), seq.data_ptr(),
                                       qual.data_ptr(), n * L, c_st.data_ptr(), stream=st)

    def state():
        t = int(c_st[0].item())
        return (rq_d.cpu().numpy().copy(), seq[:t].cpu().numpy().tobytes(), qual[:t].cpu().numpy().tobytes(), roff.cpu().numpy().copy(),
                c_row.cpu().numpy().tolist(), c_st.cpu().numpy().tolist())

    eager = []
    for lab, acc in fills:
        lab_d.copy_(torch.from_numpy(lab)); acc_d.copy_(torch.from_numpy(acc))
        torch.cuda.synchronize()
        pair()
        hip_ctx.synchronize()
        eager.append(state())
        want_rq = qr.row_qual(lab, acc, O)
        _, want_q = _expected(b, out, lab, want_rq)
        assert np.array_equal(eager[-1][0], want_rq) and eager[-1][2] == b"".join(want_q) and eager[-1][5][1] == 0
    assert eager[0][2] != eager[1][2]
    with hip_ctx.graph_capture(st) as g:
        pair()
    for k in (1, 0, 2, 2):
        lab_d.copy_(torch.from_numpy(fills[k][0])); acc_d.copy_(torch.from_numpy(fills[k][1]))
        for t in (rq_d, seq, qual, roff, c_row, c_st):
            t.zero_()
        torch.cuda.synchronize()
        g.launch()
        hip_ctx.synchronize()
        got = state()
        assert np.array_equal(got[0], eager[k][0]) and np.array_equal(got[3], eager[k][3]), k
        assert got[1:3] == eager[k][1:3] and got[4:] == eager[k][4:], k
    g.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """three contigs (ctg1 without reads), 60 reads of ~1.5 kb per contig with reads, seeded P2 weights"""
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    tmp = tmp_path_factory.mktemp("qual")
    rng = np.random.default_rng(21)
    contigs = [("ctg2", "".join(rng.choice(list("ACGT"), size=9_500))), ("ctg10", "".join(rng.choice(list("ACGT"), size=6_200))),
               ("ctg1", "".join(rng.choice(list("ACGT"), size=3_000)))]
    bw.write_fasta(str(tmp / "ref.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs[:2]):
        recs += bw.random_records(rng, 60, len(seq), tid=tid, mean_len=1500)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "reads.bam"), [(n, len(s)) for n, s in contigs], recs)
    np.savez(str(tmp / "model.npz"), **synth.make_weights_p2(31, 3.0))
    return tmp


class _RecordingChain(polish._DeviceChain):
    """polish's device chain, reading back what every launch's quality kernels were given"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.launches = []

    def _labels_and_stitch(self, db, n, n_regions):
        res = super()._labels_and_stitch(db, n, n_regions)
        if n and self.qualities:
            d = self.dout
            self.launches.append(dict(position=d.position[:n].cpu().numpy(), index=d.index[:n].cpu().numpy(),
                                      region=d.region[:n].cpu().numpy(), chunk_id=d.chunk_id[:n].cpu().numpy(),
                                      labels=self.labels[:n].cpu().numpy(), acc=self.acc[:n].cpu().numpy(),
                                      row_qual=self.row_qual[:n].cpu().numpy(),
                                      ref_start=db.t["ref_start"][:n_regions].cpu().numpy(),
                                      ref_end=db.t["ref_end"][:n_regions].cpu().numpy()))
        return res


def _fastq_records(path):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    recs = [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]
    assert all(lines[i][:1] == b"@" and lines[i + 2] == b"+" for i in range(0, len(lines) - 1, 4))
    return recs


def _check_fastq_against_launches(recs, launches):
    """the FASTQ's qualities are the checker's, from the labels and acc the device held: the region pieces in run order are the
    contigs' strings in FASTQ order (regions ascending inside a contig, contigs in natural order)"""
    want_seq, want_q = b"", b""
    for la in launches:
        rq = qr.row_qual(la["labels"], la["acc"], O)
        assert np.array_equal(la["row_qual"], rq)
        spans = list(zip(la["ref_start"].tolist(), la["ref_end"].tolist()))
        for reg in qr.regions_with_qual(la["position"], la["index"], la["region"], la["chunk_id"], la["labels"], rq, spans):
            s, q = qr.create_consensus_qual([reg])
            want_seq, want_q = want_seq + s.encode(), want_q + q
    assert b"".join(r[1] for r in recs) == want_seq
    got_q = bytes(v - 33 for v in b"".join(r[2] for r in recs))
    assert got_q == want_q
    assert len(set(got_q)) > 1                               # a constant plane could not show a byte out of place


def _recording_opener(hip_ctx, chains):
    def open_chain(device, shared, state_dict, dtype, qualities=False):
        hip_ctx.load_p2(state_dict, dtype)
        chains.append(_RecordingChain(hip_ctx, qualities=qualities))
        return chains[-1]
    return open_chain


def test_polish_qualities_with_realign_and_gpu_decode(inputs, hip_ctx, opts):
    """the flag beside --realign and --gpu_decode: the same FASTA as without it, and the checker's FASTQ"""
    t = inputs
    opts(shared_device=1)
    chains = []
    base = ["-b", str(t / "reads.bam"), "-f", str(t / "ref.fa"), "-m", str(t / "model.npz"), "-t", "3", "--realign", "--gpu_decode"]
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / "plain_rd")]), open_chain=_recording_opener(hip_ctx, chains)) == 0
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / "qual_rd"), "--qualities"]),
                      open_chain=_recording_opener(hip_ctx, chains)) == 0
    fasta = open(str(t / "qual_rd" / "_pepper_polished.fa"), "rb").read()
    assert fasta == open(str(t / "plain_rd" / "_pepper_polished.fa"), "rb").read() and fasta.startswith(b">ctg2\n")
    recs = _fastq_records(str(t / "qual_rd" / "_pepper_polished.fq"))
    assert [r[1] for r in recs] == fasta.split(b"\n")[1:-1:2]
    _check_fastq_against_launches(recs, chains[1].launches)


@pytest.mark.parametrize("bf16", [False, True])
def test_polish_qualities_end_to_end(inputs, hip_ctx, opts, monkeypatch, bf16):
    t = inputs
    tag = "b" if bf16 else "f"
    monkeypatch.setenv("PV_SHARED_DEVICE", "1")
    opts(shared_device=1)            # what PV_SHARED_DEVICE=1 sets on a new context: a chunk's result does not depend on its launch
    chains = []

    open_chain = _recording_opener(hip_ctx, chains)
    base = ["-b", str(t / "reads.bam"), "-f", str(t / "ref.fa"), "-m", str(t / "model.npz"), "-t", "3", "-bs", "16"] + (["--bf16"] if bf16 else [])
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / ("plain_" + tag))]), open_chain=open_chain) == 0
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / ("qual_" + tag)), "--qualities"]), open_chain=open_chain) == 0
    assert [c.qualities for c in chains] == [False, True]
    assert os.listdir(str(t / ("plain_" + tag))) == ["_pepper_polished.fa"]
    assert sorted(os.listdir(str(t / ("qual_" + tag)))) == ["_pepper_polished.fa", "_pepper_polished.fq"]
    fasta = open(str(t / ("qual_" + tag) / "_pepper_polished.fa"), "rb").read()
    assert fasta == open(str(t / ("plain_" + tag) / "_pepper_polished.fa"), "rb").read()       # the flag does not touch the FASTA
    fa = fasta.split(b"\n")
    recs = _fastq_records(str(t / ("qual_" + tag) / "_pepper_polished.fq"))
    assert [r[0] for r in recs] == [l[1:] for l in fa[0:-1:2]] == [b"ctg2", b"ctg10"]
    assert [r[1] for r in recs] == fa[1:-1:2]
    assert all(len(r[1]) == len(r[2]) and min(r[2]) >= 33 and max(r[2]) <= 126 for r in recs)
    assert len(chains[1].launches) > 1                       # -bs 16: 8 regions per launch
    _check_fastq_against_launches(recs, chains[1].launches)

    # the three steps with --qualities: the same FASTA and FASTQ bytes
    img, pred, out = (str(t / ("%s_%s" % (k, tag))) for k in ("img", "pred", "out"))
    ap = pepper.parser()
    args = ap.parse_args(["make_images", "-b", str(t / "reads.bam"), "-f", str(t / "ref.fa"), "-o", img, "-t", "2"])
    assert polish_steps.make_images_run(args, polish_steps._ImageChain(polish._DeviceChain(hip_ctx))) == 0

    def open_caller(device, shared, state_dict, dtype):
        hip_ctx.load_p2(state_dict, dtype)
        return polish._DeviceChain(hip_ctx)
    args = ap.parse_args(["call_consensus", "-i", img, "-m", str(t / "model.npz"), "-o", pred, "-bs", "512", "--qualities"]
                         + (["--bf16"] if bf16 else []))
    assert polish_steps.call_consensus_run(args, open_caller) == 0
    assert polish_steps.stitch_run(ap.parse_args(["stitch", "-i", pred, "-o", out + "/p", "--qualities"]), hip_ctx) == 0
    assert open(out + "/p_pepper_polished.fa", "rb").read() == fasta
    assert open(out + "/p_pepper_polished.fq", "rb").read() == open(str(t / ("qual_" + tag) / "_pepper_polished.fq"), "rb").read()
    # every row of every chunk has its quality in the file, label-0 rows included
    from pepper_thesis_amd.hdf5io import PolishPredictionStore
    with PolishPredictionStore(os.path.join(pred, "pepper_prediction_0.hdf")) as s:
        c = s.contigs()[0]
        reg = s.regions(c)[0]
        ph = s.read_phred(c, reg, "0")
        lab = s.read_chunk(c, reg, "0")["bases"]
        assert ph.shape == (L,) and ph.dtype == np.uint8 and ph.max() <= 93 and (lab == 0).any()
    # without the flag the stitch of these files writes the FASTA alone
    assert polish_steps.stitch_run(ap.parse_args(["stitch", "-i", pred, "-o", out + "/n"]), hip_ctx) == 0
    assert open(out + "/n_pepper_polished.fa", "rb").read() == fasta and not os.path.exists(out + "/n_pepper_polished.fq")
