"""GPU: `polish -hp` end to end. The oracle is the project's own single-haplotype path on a pre-split file: haplotype h's files
must be, byte for byte, those of a plain `polish` on a BAM that holds only the untagged reads and those tagged HP:h. No trained
weights are needed: both sides run the same seeded network."""
import os

import numpy as np
import pytest

from pepper_thesis_amd import bamio, cli, polish, synth

pytestmark = pytest.mark.gpu
ALL_FLAGS = ["--realign", "--gpu_decode", "--qualities", "--edits", "--min_depth", "3", "--min_qual", "20"]


def _write(bw, path, refs, recs, keep):
    bw.write_bam(path, refs, [r for r in recs if r.get("hp") in keep])


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """two contigs of a few kb, each region under reads of both haplotypes, untagged reads and a few tagged HP:3 (in neither
    split file); the two split files; an untagged copy; a file whose second contig holds HP:2 reads only"""
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    tmp = tmp_path_factory.mktemp("hp")
    rng = np.random.default_rng(47)
    contigs = [("ctgA", "".join(rng.choice(list("ACGTacgt"), size=3_200))), ("ctgB", "".join(rng.choice(list("ACGTacgt"), size=2_100)))]
    bw.write_fasta(str(tmp / "ref.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs):
        mine = bw.random_records(rng, 90, len(seq), tid=tid, mean_len=900)
        for k, r in enumerate(mine):
            r["hp"] = (None, 1, 2, 1, 2, None, 2, 1, 3)[k % 9]
        recs += mine
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    refs = [(n, len(s)) for n, s in contigs]
    _write(bw, str(tmp / "tagged.bam"), refs, recs, (None, 1, 2, 3))
    _write(bw, str(tmp / "split1.bam"), refs, recs, (None, 1))
    _write(bw, str(tmp / "split2.bam"), refs, recs, (None, 2))
    bw.write_bam(str(tmp / "untagged.bam"), refs, [dict(r, hp=None) for r in recs])
    bw.write_bam(str(tmp / "b_is_hp2.bam"), refs, [dict(r, hp=2) if r["tid"] == 1 else r for r in recs])
    # every region holds reads of both haplotypes (so the split files cut the same launches) and far fewer than the 1500 at
    # which the reader samples
    fa = bamio.FastaHandler(str(tmp / "ref.fa"))
    for name in ("split1.bam", "split2.bam"):
        bm = bamio.BamHandler(str(tmp / name))
        work, _ = polish.polish_work(fa, bm, None)
        assert len(work) == 7
        for w in work:
            tags = [rd.hp_tag for rd in bm.get_reads(w.contig, w.start, w.end, False, 0, 0)]
            assert 3 <= tags.count(int(name[5])) and 3 <= len(tags) < 200 and set(tags) == {0, int(name[5])}, (name, w)
    # dense gain 100: qualities from 3 to 93 under the seeded weights, so that --min_qual 20 takes some edits back and keeps some
    np.savez(str(tmp / "model.npz"), **synth.make_weights_p2(37, 100.0))
    return tmp


def _polish(inputs, hip_ctx, bam, name, flags, bs=8):
    out_dir = str(inputs / name)
    argv = ["-b", str(inputs / bam), "-f", str(inputs / "ref.fa"), "-m", str(inputs / "model.npz"), "-t", "3", "-bs", str(bs), "-o",
            out_dir]

    def open_chain(device, shared, state_dict, dtype, **k):
        hip_ctx.load_p2(state_dict, dtype)
        return polish._DeviceChain(hip_ctx, **k)
    assert polish.run(cli.polish_parser().parse_args(argv + flags), open_chain=open_chain) == 0
    out = {}
    for f in sorted(os.listdir(out_dir)):
        if not f.endswith(".tbi"):
            out[f] = bamio.bgzf_read_all(os.path.join(out_dir, f)) if f.endswith(".vcf.gz") else open(os.path.join(out_dir, f), "rb").read()
    return out


def _fasta(data: bytes):
    lines = data.decode().split("\n")
    return dict(zip((l[1:] for l in lines[0:-1:2]), lines[1:-1:2]))


@pytest.mark.parametrize("flags", [[], ALL_FLAGS], ids=["plain", "all_flags"])
def test_each_haplotype_equals_plain_polish_of_its_split_file(inputs, hip_ctx, opts, flags):
    opts(shared_device=1)
    tag = "all" if flags else "plain"
    got = _polish(inputs, hip_ctx, "tagged.bam", "hp_" + tag, ["-hp"] + flags)
    kinds = [".edits.vcf.gz", ".fa", ".fq"] if flags else [".fa"]
    assert list(got) == ["_pepper_polished_hp%d%s" % (h, x) for h in (1, 2) for x in kinds]
    for h in (1, 2):
        want = _polish(inputs, hip_ctx, "split%d.bam" % h, "split%d_%s" % (h, tag), flags)
        assert list(want) == ["_pepper_polished" + x for x in kinds]
        assert got["_pepper_polished_hp%d.fa" % h] == want["_pepper_polished.fa"], h
        assert set(_fasta(want["_pepper_polished.fa"])) == {"ctgA", "ctgB"}
        if flags:
            assert got["_pepper_polished_hp%d.fq" % h] == want["_pepper_polished.fq"], h
            mine = got["_pepper_polished_hp%d.edits.vcf.gz" % h].decode().split("\n")
            assert mine.count("##pepper_haplotype=%d" % h) == 1
            mine.remove("##pepper_haplotype=%d" % h)
            theirs = want["_pepper_polished.edits.vcf.gz"].decode().split("\n")
            assert mine == theirs and sum(bool(l) and not l.startswith("#") for l in theirs) >= 5, h
    # the haplotypes differ: the reads of the two files are different reads
    assert got["_pepper_polished_hp1.fa"] != got["_pepper_polished_hp2.fa"]


def test_a_region_without_reads_of_a_haplotype_is_absent_from_its_fasta(inputs, hip_ctx, opts):
    """-bs 16: all seven regions are one launch, so haplotype 1's pass runs ctgB's three emptied regions through the chain beside
    ctgA's four and drops their pieces; -bs 8: ctgB's regions are a launch of their own, which haplotype 1 skips"""
    opts(shared_device=1)
    for bs in (16, 8):
        got = _polish(inputs, hip_ctx, "b_is_hp2.bam", "hp_empty_%d" % bs, ["-hp"], bs=bs)
        one, two = _fasta(got["_pepper_polished_hp1.fa"]), _fasta(got["_pepper_polished_hp2.fa"])
        assert set(one) == {"ctgA"} and set(two) == {"ctgA", "ctgB"}
        assert 1_900 < len(two["ctgB"]) < 2_300 and 2_900 < len(one["ctgA"]) < 3_500
    filled = _polish(inputs, hip_ctx, "b_is_hp2.bam", "hp_empty_depth", ["-hp", "--min_depth", "1"], bs=16)
    draft = bamio.FastaHandler(str(inputs / "ref.fa")).get_reference_sequence("ctgB", 0, 2_100).upper()
    assert _fasta(filled["_pepper_polished_hp1.fa"])["ctgB"] == draft


def test_untagged_file_gives_the_plain_fasta_twice(inputs, hip_ctx, opts, capfd):
    opts(shared_device=1)
    plain = _polish(inputs, hip_ctx, "untagged.bam", "untagged_plain", [])
    assert list(plain) == ["_pepper_polished.fa"]                       # without the flag: no _hp file appears
    got = _polish(inputs, hip_ctx, "untagged.bam", "untagged_hp", ["-hp"])
    assert list(got) == ["_pepper_polished_hp1.fa", "_pepper_polished_hp2.fa"]
    assert got["_pepper_polished_hp1.fa"] == plain["_pepper_polished.fa"] == got["_pepper_polished_hp2.fa"]
    assert "no read carries an HP tag" in capfd.readouterr().err
    # the device read path keeps the tags on the device and selects (everything) twice: the same files
    dec = _polish(inputs, hip_ctx, "untagged.bam", "untagged_hp_dec", ["-hp", "--gpu_decode"])
    assert dec == got


def test_the_builders_host_fallback_gets_the_selected_batch(hip_ctx, opts, monkeypatch):
    """polish_cases.pair_overflow(): the device builder reports PV_ERR_LIMIT and the chain builds on the host instead. With
    use_hp the host form must get the reads of the haplotype, not all of them: each haplotype's result is the plain chain's
    on the checker's selection of the batch."""
    import polish_cases as pc
    import select_ref as sel
    from pepper_thesis_amd import polish_summary
    from pepper_thesis_amd.batch import pack_regions
    opts(shared_device=1)
    hip_ctx.load_p2(synth.make_weights_p2(37, 100.0))
    b = pack_regions(pc.pair_overflow())
    b.read_hp = np.array([1 + k % 2 if k < 10 else 0 for k in range(b.n_reads)], np.int32)   # the ten long deletions, dealt in turn
    calls, real = [], polish_summary.polish_summarize

    def spy(ctx, batch, *a, **k):
        calls.append(batch.n_reads)
        return real(ctx, batch, *a, **k)
    monkeypatch.setattr(polish_summary, "polish_summarize", spy)
    got = polish._DeviceChain(hip_ctx, use_hp=True).run(b)
    assert calls == [b.n_reads - 5, b.n_reads - 5]                      # the host form ran, once per haplotype, on its reads
    assert got.tags == (b.n_reads, b.n_reads - 10, 5, 5, 0) and [h.tolist() for h in got.has_reads] == [[True], [True]]
    for h in (1, 2):
        want = polish._DeviceChain(hip_ctx).run(sel.select(b, h)[0])
        assert got.results[h - 1].region_off.tolist() == want.region_off.tolist() and got.results[h - 1].bases == want.bases, h
        assert len(want.bases) > 20_000
