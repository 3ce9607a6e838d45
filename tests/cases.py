"""Hand-built and seeded regions shared by the golden-fixture generator and the parity tests.

The edge cases are the ones SURVEY.md section 8(c) lists for the image builder; each names the
reference behaviour (region_summary.cpp line) it exercises.
"""
import numpy as np

from pepper_thesis_amd import synth
from pepper_thesis_amd.batch import PRESETS, Params, Read, Region, pack_regions


def _flip(seq: bytes, i: int, b: str) -> bytes:
    s = bytearray(seq)
    s[i] = ord(b)
    return bytes(s)


def kat1_snp():
    """SURVEY Appendix D KAT-1"""
    ref = ("ACGT" * 19).encode()
    reads = [Read.make(0, "76M", _flip(ref, 40, "T") if i < 3 else ref, 20, is_reverse=(i % 2 == 1)) for i in range(6)]
    return Region(0, 75, ref, reads)


def kat23_indel():
    """SURVEY Appendix D KAT-2 / KAT-3"""
    ref = ("ACGTTGCA" * 10).encode()
    reads = []
    for i in range(8):
        if i < 4:
            seq, cg = ref[:31] + ref[33:], "31M2D47M"
        elif i < 7:
            seq, cg = ref[:51] + b"GG" + ref[51:], "51M2I29M"
        else:
            seq, cg = ref, "80M"
        reads.append(Read.make(1000, cg, seq, 20, is_reverse=(i % 2 == 1)))
    return Region(1000, 1079, ref, reads)


def kat4_clamp():
    """SURVEY KAT-4: depth>125 (clip before the frequency test, :682-689), clamp of planes 11-24 only
    (:648-653) and int8 wrap of the unclamped planes (DataStore.py:68)."""
    ref = ("ACGT" * 20).encode()
    reads = [Read.make(0, "80M", _flip(ref, 40, "G") if i < 60 else ref, 20) for i in range(300)]
    return Region(0, 79, ref, reads)


def multiallelic():
    """three SNP alleles + an insert + a delete on one site; set<string> order (:670)"""
    ref = ("GATTACAGATTACAGGCCTTAA" * 5).encode()
    reads = []
    p = 50
    for i in range(24):
        rv = i % 3 == 0
        if i < 5:
            reads.append(Read.make(200, "110M", _flip(ref, p, "C" if ref[p:p + 1] != b"C" else "A"), 30, rv))
        elif i < 9:
            reads.append(Read.make(200, "110M", _flip(ref, p, "T" if ref[p:p + 1] != b"T" else "G"), 30, rv))
        elif i < 12:
            reads.append(Read.make(200, "110M", _flip(ref, p, "N"), 30, rv))
        elif i < 16:
            reads.append(Read.make(200, "51M3I59M", ref[:51] + b"TTT" + ref[51:], 30, rv))
        elif i < 19:
            reads.append(Read.make(200, "51M1I59M", ref[:51] + b"T" + ref[51:], 30, rv))
        elif i < 22:
            reads.append(Read.make(200, "51M4D55M", ref[:51] + ref[55:], 30, rv))
        else:
            reads.append(Read.make(200, "110M", ref, 30, rv))
    return Region(200, 309, ref, reads)


def softclip_refskip():
    """S inside the read, N (REF_SKIP falls through to SOFT_CLIP: read_index += len, :556-561),
    P, H, = and X ops, unknown op 9"""
    ref = ("ACGTACGTTTGACCA" * 8).encode()
    reads = []
    for i in range(10):
        rv = i % 2 == 0
        if i < 3:
            # 5S kept inside the read, then aligned
            reads.append(Read.make(500, "20M5S30M", ref[:20] + b"GGGGG" + ref[20:50], 25, rv))
        elif i < 6:
            # REF_SKIP of 10: reference jumps 10, AND 10 read bases are skipped (fall-through)
            reads.append(Read.make(500, "20M10N40M", ref[:20] + b"A" * 10 + ref[30:70], 25, rv))
        elif i < 8:
            reads.append(Read.make(500, "10=1X9=2H3P20M", ref[:10] + b"N" + ref[11:20] + b"CCC" + ref[20:40], 25, rv))
        else:
            cg = np.asarray([(30 << 4) | 0, (4 << 4) | 9, (30 << 4) | 0], dtype=np.uint32)
            reads.append(Read.make(500, cg, ref[:60], 25, rv))
    # a few mismatching reads so that sites exist
    for i in range(4):
        reads.append(Read.make(500, "120M", _flip(_flip(ref, 25, "T"), 60, "G"), 25, i % 2 == 0))
    return Region(500, 619, ref, reads)


def edges_and_clipping():
    """reads starting before the region (:361-365), ending after it (break only at op boundaries,
    :355), delete running past the region end (substr truncation, :500), delete longer than the
    window (rows stop at 31, :885), candidates in the first/last 16 columns (zero rows, :835),
    mapq==0 read (:619), low-quality bases and the insert anchor coverage rule (:452-454)."""
    ref = ("TTGACCAGTAGGCATCA" * 6).encode()  # 102
    R = len(ref)
    reads = []
    long_ref = b"ACGTA" * 4 + ref + b"GGCAT" * 4
    for i in range(8):
        rv = i % 2 == 1
        # starts 20 before the region and ends 20 after it
        seq = _flip(long_ref, 20 + 3, "A" if ref[3:4] != b"A" else "C")
        seq = _flip(seq, 20 + R - 2, "A" if ref[R - 2:R - 1] != b"A" else "C")
        reads.append(Read.make(3000 - 20, "%dM" % len(long_ref), seq, 22, rv))
    for i in range(5):
        # 40-base deletion anchored at column 30 (longer than the 16 rows right of the centre)
        reads.append(Read.make(3000, "31M40D%dM" % (R - 71), ref[:31] + ref[71:], 22, i % 2 == 0))
    for i in range(4):
        # deletion that runs past the region end: anchor at R-3, length 10
        reads.append(Read.make(3000, "%dM10D5M" % (R - 2), ref[:R - 2] + b"ACGTA", 22, i % 2 == 0))
    for i in range(4):
        # 70-base deletion: key longer than 61 -> counted on plane 13/24 but never an allele (:511)
        reads.append(Read.make(3000 + 10, "5M70D10M", ref[10:15] + ref[85:95], 22, i % 2 == 0))
    for i in range(3):
        # insert of 60 bases: 1+61 = 62 > 61 -> rejected; insert of 59 -> accepted (:461)
        reads.append(Read.make(3000, "20M60I20M", ref[:20] + b"A" * 60 + ref[20:40], 22, False))
        reads.append(Read.make(3000, "20M59I20M", ref[:20] + b"C" * 59 + ref[20:40], 22, True))
    # mapq 0 read carrying a private SNP: must be ignored
    reads.append(Read.make(3000, "%dM" % R, _flip(ref, 50, "A" if ref[50:51] != b"A" else "C"), 22, False, mapq=0))
    reads.append(Read.make(3000, "%dM" % R, _flip(ref, 50, "A" if ref[50:51] != b"A" else "C"), 22, True, mapq=0))
    # insert whose anchor base has quality 0 (< min_snp_baseq) but whose mean quality passes
    for i in range(4):
        q = np.full(45, 22, np.uint8)
        q[19] = 0
        reads.append(Read.make(3000 + 40, "20M5I20M", ref[40:60] + b"GATTA" + ref[60:80], q, i % 2 == 0))
    # low-quality insert (rejected by the quality rule) and low-quality mismatches (not counted)
    for i in range(3):
        q = np.full(44, 22, np.uint8)
        q[20:24] = 0
        q[19] = 0
        reads.append(Read.make(3000 + 40, "20M4I20M", ref[40:60] + b"TTTT" + ref[60:80], q, i % 2 == 0))
    return Region(3000, 3000 + R - 1, ref, reads, 3000, 3000 + R - 1)


def nonacgt_reference():
    """reference N/lower-case columns: get_feature_index returns -1 (:201-229); SNP alleles still
    counted (:394-421). Candidates ON such a column are UB in the reference, so the
    candidate range excludes them; neighbours still copy those rows."""
    ref = bytearray(("CATGGTACCA" * 9).encode())
    ref[44] = ord("N")
    ref[45] = ord("N")
    ref = bytes(ref)
    reads = []
    for i in range(12):
        seq = ref.replace(b"N", b"A")
        if i < 6:
            seq = _flip(seq, 40, "T" if ref[40:41] != b"T" else "G")
            seq = _flip(seq, 48, "T" if ref[48:49] != b"T" else "G")
        reads.append(Read.make(7000, "90M", seq, 15, i % 2 == 0))
    for i in range(4):
        reads.append(Read.make(7000, "44M3D43M", ref[:44].replace(b"N", b"A") + ref[47:], 15, i % 2 == 0))
    return Region(7000, 7089, ref, reads, 7000, 7043)


def deep_wrap():
    """>128 same-strand reads: unclamped planes 4, 8-10 drop below -128 and wrap in int8 (Q18);
    plane 25 (*REV) is NOT clamped while 14 (*FRW) is (:648)."""
    ref = ("ACGGT" * 16).encode()
    reads = []
    for i in range(150):
        reads.append(Read.make(100, "80M", _flip(ref, 30, "T") if i % 3 == 0 else ref, 30, False))
    for i in range(140):
        # reverse reads with a 1-base deletion at column 50 -> plane 25 (*REV) = -140 unclamped... and 24 clamped
        reads.append(Read.make(100, "50M1D29M", ref[:50] + ref[51:], 30, True))
    return Region(100, 179, ref, reads)


def empty_and_tiny():
    """a region with no reads, a region whose reads are all mapq 0, a 1-column region"""
    ref = b"ACGTACGTAC"
    r0 = Region(10, 19, ref, [])
    r1 = Region(10, 19, ref, [Read.make(10, "10M", b"ACGTTCGTAC", 20, False, mapq=0) for _ in range(5)])
    r2 = Region(14, 14, b"T", [Read.make(12, "5M", b"GTCCG", 20, i % 2 == 0) for i in range(4)])
    return [r0, r1, r2]


EDGE_CASES = {
    "kat1_snp": lambda: [kat1_snp()],
    "kat23_indel": lambda: [kat23_indel()],
    "kat4_clamp": lambda: [kat4_clamp()],
    "multiallelic": lambda: [multiallelic()],
    "softclip_refskip": lambda: [softclip_refskip()],
    "edges_and_clipping": lambda: [edges_and_clipping()],
    "nonacgt_reference": lambda: [nonacgt_reference()],
    "deep_wrap": lambda: [deep_wrap()],
    "empty_and_tiny": empty_and_tiny,
}


def edge_batch(name):
    return pack_regions(EDGE_CASES[name]())


def all_edges_batch():
    regs = []
    for name in EDGE_CASES:
        regs.extend(EDGE_CASES[name]())
    return pack_regions(regs)


# seeded random regions committed as golden fixtures: (seed, kwargs, preset)
GOLDEN_RANDOM = [
    (11, dict(region_len=2000, depth=25, read_len=700, site_every=60), "ont_r9_guppy5_sup"),
    (12, dict(region_len=2000, depth=25, read_len=700, site_every=60, n_rate=0.002), "ont_r9_guppy4_hac"),
    (13, dict(region_len=1500, depth=30, read_len=1500, site_every=80, mismatch=0.002, ins_rate=0.002, del_rate=0.002), "hifi"),
    (14, dict(region_len=1500, depth=20, read_len=400, site_every=50), "ont_r10_q20"),
    (15, dict(region_len=1200, depth=35, read_len=600, site_every=40, mismatch=0.08, ins_rate=0.05, del_rate=0.05), "clr"),
    (16, dict(region_len=1800, depth=150, read_len=900, site_every=70), "ont_r9_guppy5_sup"),
]


def random_batch(seed, kw):
    return pack_regions([synth.synth_region(seed, **kw)])


# ---- haplotag-aware builder (region_summary_hp.cpp): the same regions with an HP tag on every read -------------------
# tags 0 (untagged), 1, 2 and the values a real BAM never carries but the reference still has a defined answer for (3, -1)
HP_TAG_CHOICES = (0, 0, 1, 2, 1, 2, 3, -1)


def tag_reads(regions, seed, choices=HP_TAG_CHOICES):
    rng = np.random.default_rng(seed)
    for r in regions:
        for rd in r.reads:
            rd.hp_tag = int(rng.choice(choices))
    return regions


def hp_edge_batch(name, seed=5):
    return pack_regions(tag_reads(EDGE_CASES[name](), seed))


def hp_all_edges_batch(seed=5):
    regs = []
    for name in EDGE_CASES:
        regs.extend(EDGE_CASES[name]())
    return pack_regions(tag_reads(regs, seed))


def hp_known_answer():
    """hand-checkable: 8 reads over ACGTACGTAC...; column 40 (ref 'A') carries a T in three reads (one per tag 0, 1, 2)"""
    ref = (b"ACGT" * 30)[:100]
    reads = []
    for i, (hp, rev, alt) in enumerate([(0, False, True), (1, False, True), (2, True, True), (0, True, False),
                                        (1, False, False), (2, False, False), (1, True, False), (2, True, False)]):
        seq = _flip(ref, 40, "T") if alt else ref
        reads.append(Read.make(0, "100M", seq, 30, rev, hp_tag=hp))
    return Region(0, 99, ref, reads)


def hp_random_batch(seed, kw):
    return pack_regions(tag_reads([synth.synth_region(seed, **kw)], seed))


# ---- deep shapes of the haplotag-aware builder: shared by the GPU limit tests and the oracle-vs-reference pins -----------
def _acgt(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n).astype(np.uint8)


def mutated(ref, rng, rate):
    """ref with about `rate` of its bases moved one step along A -> C -> G -> T -> A"""
    seq = ref.copy()
    flip = rng.random(len(seq)) < rate
    seq[flip] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), seq[flip]) + 1) % 4]
    return seq


def hp_depth_5000():
    """MAX_READS_IN_REGION = 5000 reads over 700 columns, every haplotag"""
    reg = synth.synth_region(77, region_len=700, depth=5000, read_len=600, site_every=40)
    return tag_reads([reg], 77)[0]


# the reads of hp_many_reads that carry a one-base deletion at column 65 (anchor 64): (hp_tag, is_reverse)
HP_MANY_DEL_READS = ((0, False), (1, False), (2, False), (3, True), (-1, False), (1, True))


def hp_many_reads(n, tags=None, all_forward=False):
    """n reads over the same 120 columns; one in three carries a SNP at column 60; the reads listed in HP_MANY_DEL_READS
    (the first six) delete column 65. tags: None = HP_TAG_CHOICES at random, else a function of the read index"""
    rng = np.random.default_rng(12)
    R = 120
    ref = _acgt(rng, R)
    alt = ref.copy()
    alt[60] = ord("A") if ref[60] != ord("A") else ord("C")
    tag_rng = np.random.default_rng(13)
    reads = []
    for i in range(n):
        seq = alt if i % 3 == 0 else ref
        if i < len(HP_MANY_DEL_READS):
            hp, rev = HP_MANY_DEL_READS[i]
            reads.append(Read.make(1000, "65M1D54M", np.concatenate([seq[:65], seq[66:]]).tobytes(), 20, rev, hp_tag=hp))
            continue
        hp = int(tag_rng.choice(HP_TAG_CHOICES)) if tags is None else tags(i)
        reads.append(Read.make(1000, "%dM" % R, seq.tobytes(), 20, False if all_forward else bool(i & 1), hp_tag=hp))
    return Region(1000, 1000 + R - 1, ref.tobytes(), reads, 1000, 1000 + R - 1)


def hp_every_column_a_site(R=40_000):
    """six reads that each differ from the reference on about half of the R columns: nearly every column is a site"""
    rng = np.random.default_rng(9)
    ref = _acgt(rng, R)
    reads = []
    for i in range(6):
        seq = ref.copy()
        flip = rng.random(R) < 0.5
        seq[flip] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), seq[flip]) + 1) % 4]
        reads.append(Read.make(0, "%dM" % R, seq.tobytes(), 20, i % 2 == 0, hp_tag=HP_TAG_CHOICES[i]))
    return Region(0, R - 1, ref.tobytes(), reads)


def hp_many_alleles(n_distinct):
    """one insertion site (anchor column 14) with n_distinct distinct alleles: n_distinct - 1 six-base inserts seen once
    each, and a three-base insert seen 200 times (so that the site emits a candidate)"""
    ref = b"ACGTACGTACGTACGTACGTACGTACGTAC"
    reads = []
    for i in range(n_distinct - 1):
        ins = "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(6))
        reads.append(Read.make(0, "15M6I15M", ref[:15] + ins.encode() + ref[15:], 30, i % 2 == 0, hp_tag=HP_TAG_CHOICES[i % 8]))
    for i in range(200):
        reads.append(Read.make(0, "15M3I15M", ref[:15] + b"GTT" + ref[15:], 30, i % 2 == 1, hp_tag=HP_TAG_CHOICES[(i + 3) % 8]))
    return Region(0, 29, ref, reads)


def hp_long_indels():
    """a 3000-base insertion, a deletion longer than the region remainder, a reference buffer longer than the region"""
    rng = np.random.default_rng(4)
    ref = bytes(_acgt(rng, 400))
    reads = []
    for i in range(8):
        ins = bytes(_acgt(rng, 3000))
        reads.append(Read.make(100, "50M3000I50M", ref[100:150] + ins + ref[150:200], 12 + i, i % 2 == 0))
    for i in range(6):
        reads.append(Read.make(100, "120M500D10M", ref[100:220] + b"ACGTACGTAC", 20, i % 2 == 0))
    for i in range(6):   # SNPs at columns 152 and 215, next to the two long indels, so that windows cover them
        seq = _flip(_flip(ref, 152, "T" if ref[152:153] != b"T" else "G"), 215, "T" if ref[215:216] != b"T" else "G")
        reads.append(Read.make(90, "200M", seq[90:290], 20, i % 2 == 1))
    return tag_reads([Region(100, 299, ref[100:], reads)], 4)[0]   # 300 reference bytes for a 200-column region


# one overlay case: (candidate type 1 SNP / 2 INS / 3 DEL, reads of the candidate allele in the big group, big group)
# groups: 0 forward set 1, 1 forward set 2, 2 reverse set 1, 3 reverse set 2 (the byte order of the packed counts)
HP_OVERLAY_COUNTS = (124, 125, 126, 255, 256, 300)
HP_OVERLAY_CASES = tuple((t, n, (3 * t + k) % 4) for t in (1, 2, 3) for k, n in enumerate(HP_OVERLAY_COUNTS))


def _hp_allele_read(t, ref, col, rev, hp):
    """a 60-base read over ref carrying candidate type t at column col (SNP at col, insert / delete anchored on col)"""
    if t == 1:
        return Read.make(0, "60M", _flip(ref, col, "T" if ref[col:col + 1] != b"T" else "G"), 30, rev, hp_tag=hp)
    if t == 2:
        return Read.make(0, "%dM2I%dM" % (col + 1, 59 - col), ref[:col + 1] + b"GA" + ref[col + 1:60], 30, rev, hp_tag=hp)
    return Read.make(0, "%dM2D%dM" % (col + 1, 57 - col), ref[:col + 1] + ref[col + 3:60], 30, rev, hp_tag=hp)


def hp_overlay_region(t, n, big, seed=0):
    """column 30 carries one candidate of type t. Group `big` gets n observations of it: n - 2 from reads tagged with its
    set and 2 untagged (which join the other set on the same strand as well). The other groups get 3, 5 and 7 more from
    tagged reads; 2 forward reads tagged 3 and 2 reverse reads tagged -1 carry it too (they join no group's allele
    counts); 20 reads match. Returns (region, the four expected group counts before the clamp)."""
    rng = np.random.default_rng(100 + seed)
    ref = bytes(_acgt(rng, 60))
    col = 30
    reads, counts = [], [0, 0, 0, 0]

    def add(rev, hp):
        reads.append(_hp_allele_read(t, ref, col, rev, hp))
        for s in (1, 2):
            if hp == 0 or hp == s:
                counts[(2 if rev else 0) + (s - 1)] += 1
    rev_b, set_b = big >= 2, 1 + (big & 1)
    for i in range(n - 2):
        add(rev_b, set_b)
    add(rev_b, 0)
    add(rev_b, 0)
    small = iter((3, 5, 7))
    for g in range(4):
        if g != big:
            for i in range(next(small)):
                add(g >= 2, 1 + (g & 1))
    for rev, hp in ((False, 3), (False, 3), (True, -1), (True, -1)):
        add(rev, hp)
    for i in range(20):
        reads.append(Read.make(0, "60M", ref, 30, i % 2 == 0, hp_tag=HP_TAG_CHOICES[i % 8]))
    return Region(0, 59, ref, reads), counts


def hp_overlay_batch_regions():
    """every HP_OVERLAY_CASES region, 1000 columns apart; -> (regions, expected group counts per region)"""
    regs, counts = [], []
    for k, (t, n, big) in enumerate(HP_OVERLAY_CASES):
        r, c = hp_overlay_region(t, n, big, k)
        off = 1000 * k
        regs.append(Region(off, off + 59, r.ref, [Read.make(off + x.pos, x.cigar, x.bases, x.quals, x.is_reverse, x.mapq, x.hp_tag)
                                                  for x in r.reads]))
        counts.append(c)
    return regs, counts


def hp_failing_inserts():
    """anchor column 30: 200 reads insert 'GT' with inserted bases of quality 0 (they fail the bar; the anchor, quality 30,
    passes, so each takes its anchor's coverage back), 40 reads insert 'CA' at quality 30, 30 reads match.
    Coverage at the anchor: 270 - 200 = 70."""
    rng = np.random.default_rng(31)
    ref = bytes(_acgt(rng, 60))
    reads = []
    for i in range(270):
        hp = HP_TAG_CHOICES[i % 8]
        if i < 200:
            q = np.full(62, 30, np.uint8)
            q[31:33] = 0
            reads.append(Read.make(0, "31M2I29M", ref[:31] + b"GT" + ref[31:], q, i % 2 == 0, hp_tag=hp))
        elif i < 240:
            reads.append(Read.make(0, "31M2I29M", ref[:31] + b"CA" + ref[31:], 30, i % 2 == 1, hp_tag=hp))
        else:
            reads.append(Read.make(0, "60M", ref, 30, i % 2 == 0, hp_tag=hp))
    return Region(0, 59, ref, reads)


# depths of the allele-table switch: k_site_rank sends a site to the large-table launch when nev + 4 > UM_SMALL (96)
SWITCH_DEPTHS = tuple(range(88, 98))


def switch_regions(kind):
    """one region per SWITCH_DEPTHS entry d, 2000 columns apart. kind 'snp' (haplotag form): d reads over 80 columns that all
    mismatch at column 40 (two thirds T / one third G, every tag); kind 'ins' (26-plane form): d reads that all insert 'AC'
    after column 40"""
    regs = []
    for k, d in enumerate(SWITCH_DEPTHS):
        rng = np.random.default_rng(200 + k)
        ref = bytearray(_acgt(rng, 80))
        ref[40] = ord("A")
        ref = bytes(ref)
        off = 2000 * k
        reads = []
        for i in range(d):
            if kind == "snp":
                reads.append(Read.make(off, "80M", _flip(ref, 40, "T" if i % 3 else "G"), 30, i % 2 == 0,
                                       hp_tag=HP_TAG_CHOICES[(i + k) % 8]))
            else:
                reads.append(Read.make(off, "41M2I39M", ref[:41] + b"AC" + ref[41:], 30, i % 2 == 0))
        regs.append(Region(off, off + 79, ref, reads))
    return regs
