"""The rule of the BAM record decode (csrc/bam_decode.hip, csrc/pv_io.cpp), restated plainly for the tests: the record walk
of one interval, the flag / MAPQ filter, the aux walk, the long-CIGAR placeholder and, through bam_writer.clip_read, the clip.
Pure Python on the record dicts of bam_writer; nothing is imported from the package and nothing is in closed form: the clip
is clip_read's walk, base by base."""
import struct

import bam_writer as bw

OK, BAD_BLOCK, BAD_RECORD, CIGAR_LONGER, BLOCK_SIZE, PAST_PLAN, SEEK, BAD_TABLE = range(8)

_FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_ELEM = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_HP = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<i"}   # (an I above 2^31 - 1 wraps: the field is an int32)


def aux_walk(aux):
    """pv_io.cpp aux_next over a record's aux bytes -> (words of the first CG:B,I field or None, value of the last HP field of
    an integer type or 0); the walk stops at the first field that does not fit or has an unknown type or sub-type"""
    cg, hp, s, end = None, 0, 0, len(aux)
    while s < end:
        if end - s < 3:
            break
        tag, ty = aux[s:s + 2], chr(aux[s + 2])
        s += 3
        if ty in _FIXED:
            vb = _FIXED[ty]
        elif ty in "ZH":
            e = s
            while e < end and aux[e] != 0:
                e += 1
            if e >= end:
                break
            vb = e - s + 1
        elif ty == "B":
            if end - s < 5:
                break
            es = _ELEM.get(chr(aux[s]))
            if es is None:
                break
            vb = 5 + struct.unpack_from("<I", aux, s + 1)[0] * es
        else:
            break
        if end - s < vb:
            break
        if tag == b"HP" and ty in _HP:
            hp = struct.unpack_from(_HP[ty], aux, s)[0]
        if cg is None and tag == b"CG" and ty == "B" and aux[s] == ord("I"):
            n = struct.unpack_from("<I", aux, s + 1)[0]
            cg = list(struct.unpack_from("<%dI" % n, aux, s + 5))
        s += vb
    return cg, hp


def cigar_in_use(rec, cg):
    """the record's own CIGAR, or the CG tag's behind the <l_seq>S<rlen>N placeholder (htslib bam_tag2cigar)"""
    own = bw.record_cigar(rec)
    if len(own) >= 1 and rec["tid"] >= 0 and rec["pos"] >= 0 and cg is not None and own[0] == (4, len(rec["seq"])):
        return [(w & 0xF, w >> 4) for w in cg]
    return own


def decode_record(rec, rs, re, include_supp=False, min_mapq=0):
    """one listed record -> (status, read or None); read = dict(pos, rev, mapq, hp, seq, qual, cigar words)"""
    fl = rec["flag"]
    if fl & (0x200 | 0x400 | 0x100 | 0x4) or (not include_supp and fl & 0x800) or rec["mapq"] < min_mapq:
        return OK, None
    cg, hp = aux_walk(bw.record_aux(rec))
    used = dict(rec, cigar=cigar_in_use(rec, cg))
    try:
        c = bw.clip_read(used, rs, re)
    except IndexError:            # a kept base past l_seq: the reader's "CIGAR longer than SEQ"
        return CIGAR_LONGER, None
    if c is None:
        return OK, None
    return OK, dict(pos=c[0], rev=1 if fl & 0x10 else 0, mapq=rec["mapq"], hp=hp, seq=c[2].encode(), qual=bytes(c[3]),
                    cigar=[(ln << 4) | op for op, ln in c[4]])


def decode_interval(chunks, tid, rs, re, include_supp=False, min_mapq=0):
    """chunks: the records under every chunk of the interval, in file order -> dict(n_rec, reads, n_bases, n_cigar, status,
    offender (index among the listed records of the first record with an error, or None), done (the walk met its end: a
    larger tid, or pos >= re), listed (the listed records))"""
    listed, done = [], False
    for recs in chunks:
        for rec in recs:
            if rec["tid"] != tid:
                if rec["tid"] > tid:
                    done = True
                    break
                continue
            if rec["pos"] >= re:
                done = True
                break
            listed.append(rec)
        if done:
            break
    reads, status, offender = [], OK, None
    for i, rec in enumerate(listed):
        st, rd = decode_record(rec, rs, re, include_supp, min_mapq)
        if st != OK and offender is None:
            status, offender = st, i
        if rd is not None:
            rd["listed"] = i
            reads.append(rd)
    return dict(n_rec=len(listed), reads=reads, n_bases=sum(len(r["seq"]) for r in reads), n_cigar=sum(len(r["cigar"]) for r in reads),
                status=status, offender=offender, done=done, listed=listed)
