"""Generates tests/golden/realign_golden.npz from the REFERENCE's own striped Smith-Waterman.

Run in the build container only (needs /root/reference): `python tests/golden/make_realign_golden.py`.
It compiles the reference's ssw.c and a small driver that includes its ssw_cpp.cpp into a temporary directory (nothing
is written into the repository but the .npz), runs the read loop of ReadAligner::align_reads_to_reference
(simple_aligner.cpp:66-107) with Aligner(4, 6, 8, 2), the default Filter and maskLen 0 on the cases of
tests/realign_cases.py, and stores INPUTS and EXPECTED OUTPUTS as arrays (data only).

The cases at the realigner's limits (realign_cases.FIXTURE_CASES, listed under "limit_names") store OUTPUTS only, plus a
SHA-1 of their inputs: tests/test_polish_realign_cpu.py rebuilds the inputs from the seeds and checks the digest. Where
oracle/_ref/libref_polish.so is built (oracle/Makefile), the reference's whole ReadAligner is run on them as well and must
give the same positions and CIGARs.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import realign_cases  # noqa: E402

REF = "/root/reference/pepper/modules/src/local_reassembly"

# reads "n_cases" then per case: start n_reads wlen <wlen bytes as ints>, per read: pos qlen <qlen bytes as ints>
# writes per read: state score ref_begin ref_end query_begin query_end new_pos n_ops op... (CigarOperationFromChar codes)
DRIVER = r'''
#include "%s/ssw_cpp.cpp"
#include <cstdio>
#include <sstream>
using namespace StripedSmithWaterman;
static int op_code(char c) { return (c == '=' || c == 'X') ? 0 : c == 'S' ? 4 : c == 'D' ? 2 : c == 'I' ? 1 : -1; }
int main() {
    Aligner aligner(4, 6, 8, 2);
    Filter filter;
    long long n_cases; if (scanf("%%lld", &n_cases) != 1) return 1;
    for (long long c = 0; c < n_cases; c++) {
        long long start, n_reads, wlen; (void)!scanf("%%lld %%lld %%lld", &start, &n_reads, &wlen);
        std::string win((size_t)wlen, '\0');
        for (long long k = 0; k < wlen; k++) { int v; (void)!scanf("%%d", &v); win[k] = (char)v; }
        for (long long r = 0; r < n_reads; r++) {
            long long pos, qlen; (void)!scanf("%%lld %%lld", &pos, &qlen);
            std::string q((size_t)qlen, '\0');
            for (long long k = 0; k < qlen; k++) { int v; (void)!scanf("%%d", &v); q[k] = (char)v; }
            if (pos < start) { printf("2 0 0 0 0 0 %%lld 0\n", pos); continue; }
            std::string sub = win.substr((size_t)(pos - start));
            if (sub.empty() || q.empty()) { printf("0 0 0 0 0 0 %%lld 0\n", pos); continue; }
            aligner.SetReferenceSequence(sub.c_str(), (int)sub.length());
            Alignment al;
            aligner.Align_cpp(q.c_str(), filter, &al, 0);
            if (al.sw_score > 1) {
                std::istringstream parser(al.cigar_string);
                std::vector<std::pair<int, int>> ops; int len; char ch;
                while (parser >> len >> ch) ops.push_back(std::make_pair(op_code(ch), len));
                printf("1 %%d %%d %%d %%d %%d %%lld %%zu", (int)al.sw_score, al.ref_begin, al.ref_end, al.query_begin,
                       al.query_end, pos + al.ref_begin, ops.size());
                for (auto& o : ops) printf(" %%u", ((unsigned)o.second << 4) | (unsigned)o.first);
                printf("\n");
            } else {
                printf("0 %%d 0 0 0 0 %%lld 0\n", (int)al.sw_score, pos);
            }
        }
    }
    return 0;
}
''' % REF


def all_cases():
    out = [(name, s, e, w, reads) for name, s, e, w, reads in realign_cases.edge_regions()]
    for seed in range(6):
        s, e, w, reads = realign_cases.random_region(100 + seed, start=1000 * seed, n_reads=24, long_ins=0.001 * (seed % 3))
        out.append(("random%d" % seed, s, e, w, reads))
    s, e, w, reads = realign_cases.random_region(200, start=9000, n_reads=20, contig_len=9000 + 1210)
    out.append(("random_contig_end", s, e, w, reads))
    s, e, w, reads = realign_cases.random_region(201, start=300, n_reads=20, alphabet=b"NacgtUuRYN")
    out.append(("random_alphabet", s, e, w, reads))
    return out


def limit_cases():
    """one single-read case per realign_cases.FIXTURE_CASES entry, named as realign_cases.fixture_case names it"""
    out = []
    for group, region, read in realign_cases.FIXTURE_CASES:
        name, start, win, rd = realign_cases.fixture_case(group, region, read)
        out.append((name, start, start + len(win) - 20, win, [rd]))
    return out


def check_against_read_aligner(cases, blob):
    """the same cases through the reference's ReadAligner (oracle/_ref/libref_polish.so), where it is built"""
    from oracle import oracle
    from pepper_thesis_amd import realign
    from pepper_thesis_amd.batch import pack_regions
    if not oracle.have_reference_polish():
        print("oracle/_ref/libref_polish.so not built: ReadAligner cross-check skipped")
        return
    for name, s, e, w, reads in cases:
        b = pack_regions([realign_cases.as_region(s, e, w, reads)])
        woff, win = realign.pack_windows([w])
        state, pos, _, coff, cig = oracle.reference_polish_realign(b, woff, win)
        assert state.tolist() == [oracle.REF_KEPT] * len(reads), name
        assert pos.tolist() == blob[name + "/record"][:, 6].tolist(), name
        assert np.array_equal(coff, blob[name + "/cigar_off"]) and np.array_equal(cig, blob[name + "/cigar"]), name
        print("%-34s ReadAligner gives the same position and cigar" % name)


def main():
    limits = limit_cases()
    cases = all_cases() + limits
    limit_names = set(c[0] for c in limits)
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.cpp")
        with open(drv, "w") as fh:
            fh.write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.check_call(["gcc", "-O2", "-c", os.path.join(REF, "ssw.c"), "-o", os.path.join(tmp, "ssw.o")])
        subprocess.check_call(["g++", "-O2", "-std=c++11", drv, os.path.join(tmp, "ssw.o"), "-o", exe])
        lines = ["%d" % len(cases)]
        for _, s, _, w, reads in cases:
            lines.append("%d %d %d %s" % (s, len(reads), len(w), " ".join(str(b) for b in w)))
            for rd in reads:
                lines.append("%d %d %s" % (rd.pos, len(rd.bases), " ".join(str(b) for b in rd.bases)))
        res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    blob, names, k = {}, [], 0
    for name, s, e, w, reads in cases:
        recs, cig, cig_off = [], [], [0]
        for _ in reads:
            v = [int(t) for t in res[k].split()]
            k += 1
            recs.append(v[:7])
            cig.extend(v[8:8 + v[7]])
            cig_off.append(len(cig))
        if name in limit_names:
            blob[name + "/input_sha1"] = realign_cases.input_digest(s, w, reads)
        else:
            names.append(name)
            blob[name + "/start"] = np.int64(s)
            blob[name + "/end"] = np.int64(e)
            blob[name + "/window"] = np.frombuffer(w, np.uint8)
            blob[name + "/read_pos"] = np.asarray([r.pos for r in reads], np.int64)
            blob[name + "/base_off"] = np.cumsum([0] + [len(r.bases) for r in reads]).astype(np.int64)
            blob[name + "/bases"] = np.frombuffer(b"".join(r.bases for r in reads), np.uint8)
            blob[name + "/in_cigar_off"] = np.cumsum([0] + [len(r.cigar) for r in reads]).astype(np.int64)
            blob[name + "/in_cigar"] = np.concatenate([r.cigar for r in reads]).astype(np.uint32)
        blob[name + "/record"] = np.asarray(recs, np.int64)   # state score ref_begin ref_end query_begin query_end new_pos
        blob[name + "/cigar_off"] = np.asarray(cig_off, np.int64)
        blob[name + "/cigar"] = np.asarray(cig, np.uint32)
        st = np.asarray(recs)[:, 0]
        print("%-34s reads=%3d realigned=%3d dropped=%d max_score=%d" % (name, len(reads), (st == 1).sum(), (st == 2).sum(),
                                                                        np.asarray(recs)[:, 1].max()))
    blob["names"] = np.asarray(names, dtype="S")
    blob["limit_names"] = np.asarray([c[0] for c in limits], dtype="S")
    check_against_read_aligner(limits, blob)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "realign_golden.npz"), **blob)


if __name__ == "__main__":
    main()
