/* Host checker of the polisher's read realignment: a plain scalar restatement of the rules in
 * pepper_thesis_amd/csrc/polish_realign.hip (the reference's ReadAligner over striped Smith-Waterman, match 4, mismatch 6,
 * gap open 8, gap extend 2). Built by tests/realign_ref.py with the system C compiler and called through ctypes.
 *
 * rl_align(window, wlen, query, qlen, res, cigar, cap) aligns one query against one window (already cut at the read's pos):
 *   res = {score, ref_begin, ref_end, query_begin, query_end}; returns the number of output CIGAR words (BAM packing, with
 *   '='/'X' as op 7/8 so that the caller sees the runs) or 0 when score <= 1 (nothing past res[0] is filled), -1 when cap is
 *   too small, -2 on a traceback that leaves the band (never seen; reported, not guessed).
 * rl_last_band() is the band width at which that call's banded pass reached the score (0 when none ran). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { MATCH = 4, MISMATCH = 6, GAP_O = 8, GAP_E = 2 };

static int code(uint8_t b) {
    switch (b) {
        case 'A': case 'a': case 'U': case 'u': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}

static int score(int a, int b) { return (a == b && a < 4) ? MATCH : -MISMATCH; }

static int last_band = 0;   /* banded()'s final band width of the latest rl_align (0: no banded pass ran) */
int rl_last_band(void) { return last_band; }

/* local affine DP over ref columns (outer) and query rows (inner).
 * forward: best = max, first column holding it, smallest row in that column.
 * reverse (term > 0): stop at the first column whose max equals term; row = smallest row with H == term there. */
static void sw_pass(const int* r, int rlen, const int* q, int qlen, int term, int* best, int* bcol, int* brow) {
    int* H = (int*)calloc((size_t)qlen + 1, sizeof(int));
    int* E = (int*)calloc((size_t)qlen + 1, sizeof(int));
    *best = 0; *bcol = -1; *brow = qlen - 1;
    for (int c = 0; c < rlen; c++) {
        int hd = 0, f = 0, colmax = 0, colrow = -1;
        for (int i = 0; i < qlen; i++) {
            int e = E[i] - GAP_E, t = H[i] - GAP_O;
            if (t > e) e = t;
            if (e < 0) e = 0;
            int h = hd + score(q[i], r[c]);
            if (h < e) h = e;
            if (h < f) h = f;
            if (h < 0) h = 0;
            hd = H[i];
            H[i] = h; E[i] = e;
            int nf = f - GAP_E; t = h - GAP_O;
            f = nf > t ? nf : t;
            if (f < 0) f = 0;
            if (h > colmax) { colmax = h; colrow = i; }
        }
        if (term > 0) {
            if (colmax == term) { *best = term; *bcol = c; *brow = colrow; break; }
        } else if (colmax > *best) {
            *best = colmax; *bcol = c; *brow = colrow;
        }
    }
    free(H); free(E);
}

/* ssw.c banded_sw, index for index: returns the number of ops written to c (reversed order fixed), or -2 */
static int banded(const int* ref, const int* read, int refLen, int readLen, int sc, uint32_t* out, int cap) {
    int w = abs(refLen - readLen) + 1, mx = 0;
    const int width_max = refLen + 2;
    int *h_b = NULL, *e_b = NULL, *h_c = NULL;
    uint8_t* dir = NULL;
    int bw = 0;
    for (;;) {
        const int width = 2 * w + 3;
        const int asz = width < width_max ? width : width_max;
        h_b = (int*)realloc(h_b, sizeof(int) * (size_t)asz);
        e_b = (int*)realloc(e_b, sizeof(int) * (size_t)asz);
        h_c = (int*)realloc(h_c, sizeof(int) * (size_t)asz);
        bw = 2 * w + 1 < refLen ? 2 * w + 1 : refLen;
        dir = (uint8_t*)realloc(dir, (size_t)bw * (size_t)readLen);
        memset(h_b, 0, sizeof(int) * (size_t)asz);
        memset(e_b, 0, sizeof(int) * (size_t)asz);
        memset(h_c, 0, sizeof(int) * (size_t)asz);
        for (int i = 0; i < readLen; i++) {
            int beg = i - w > 0 ? i - w : 0, end = i + w < refLen - 1 ? i + w : refLen - 1;
            int edge = end + 1 < width - 1 ? end + 1 : width - 1;
            int x = beg, xp = i - 1 - w > 0 ? i - 1 - w : 0, u = 0, f = 0;
            h_b[0] = e_b[0] = h_b[edge] = e_b[edge] = h_c[0] = 0;
            uint8_t* dl = dir + (size_t)i * (size_t)bw;
            for (int j = beg; j <= end; j++) {
                u = j - x + 1;
                int e = j - xp + 1, b = u - 1, d = j - xp;
                int t1 = i == 0 ? -GAP_O : h_b[e] - GAP_O;
                int t2 = i == 0 ? -GAP_E : e_b[e] - GAP_E;
                e_b[u] = t1 > t2 ? t1 : t2;
                int de = t1 > t2 ? 3 : 2;
                t1 = h_c[b] - GAP_O;
                t2 = f - GAP_E;
                f = t1 > t2 ? t1 : t2;
                int df = t1 > t2 ? 5 : 4;
                int e1 = e_b[u] > 0 ? e_b[u] : 0, f1 = f > 0 ? f : 0;
                t1 = e1 > f1 ? e1 : f1;
                t2 = h_b[d] + score(ref[j], read[i]);
                h_c[u] = t1 > t2 ? t1 : t2;
                if (h_c[u] > mx) mx = h_c[u];
                int dh = t1 <= t2 ? 1 : (e1 > f1 ? de : df);
                dl[j - x] = (uint8_t)(dh | (de == 3 ? 8 : 0) | (df == 5 ? 16 : 0));
            }
            for (int j = 1; j <= u; j++) h_b[j] = h_c[j];
        }
        if (mx >= sc) break;
        w *= 2;
    }
    last_band = w;
    /* traceback from the last cell; ops are collected in reverse */
    int n = 0, i = readLen - 1, j = refLen - 1, e = 0, state = 2;
    char op = 'M', prev = 'M';
    int rc = 0;
    uint32_t* tmp = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)readLen + (size_t)refLen + 4));
    while (i > 0) {
        int x = i - w > 0 ? i - w : 0;
        if (j - x < 0 || j - x >= bw) { rc = -2; break; }
        int v = dir[(size_t)i * (size_t)bw + (size_t)(j - x)], code3 = state == 2 ? (v & 7) : state == 0 ? ((v & 8) ? 3 : 2) : ((v & 16) ? 5 : 4);
        switch (code3) {
            case 1: --i; --j; state = 2; op = 'M'; break;
            case 2: --i; state = 0; op = 'I'; break;
            case 3: --i; state = 2; op = 'I'; break;
            case 4: --j; state = 1; op = 'D'; break;
            case 5: --j; state = 2; op = 'D'; break;
            default: rc = -2; break;
        }
        if (rc) break;
        if (op == prev) ++e;
        else { tmp[n++] = ((uint32_t)e << 4) | (uint32_t)(prev == 'M' ? 0 : prev == 'I' ? 1 : 2); prev = op; e = 1; }
    }
    if (!rc) {
        if (op == 'M') tmp[n++] = ((uint32_t)(e + 1) << 4) | 0u;
        else { tmp[n++] = ((uint32_t)e << 4) | (uint32_t)(op == 'I' ? 1 : 2); tmp[n++] = (1u << 4) | 0u; }
        if (n > cap) rc = -1;
        else for (int k = 0; k < n; k++) out[k] = tmp[n - 1 - k];
    }
    free(tmp); free(h_b); free(e_b); free(h_c); free(dir);
    return rc ? rc : n;
}

int rl_align(const uint8_t* win, int wlen, const uint8_t* query, int qlen, int32_t* res, uint32_t* cigar, int cap) {
    memset(res, 0, 5 * sizeof(int32_t));
    last_band = 0;
    if (wlen <= 0 || qlen <= 0) return 0;
    int* r = (int*)malloc(sizeof(int) * (size_t)wlen);
    int* q = (int*)malloc(sizeof(int) * (size_t)qlen);
    for (int k = 0; k < wlen; k++) r[k] = code(win[k]);
    for (int k = 0; k < qlen; k++) q[k] = code(query[k]);
    int sc, re, qe;
    sw_pass(r, wlen, q, qlen, 0, &sc, &re, &qe);
    res[0] = sc;
    int n = 0;
    if (sc > 1) {
        int* rr = (int*)malloc(sizeof(int) * (size_t)(re + 1));
        int* qr = (int*)malloc(sizeof(int) * (size_t)(qe + 1));
        for (int k = 0; k <= re; k++) rr[k] = r[re - k];
        for (int k = 0; k <= qe; k++) qr[k] = q[qe - k];
        int s2, c2, r2;
        sw_pass(rr, re + 1, qr, qe + 1, sc, &s2, &c2, &r2);
        const int rb = re - c2, qb = qe - r2;
        res[1] = rb; res[2] = re; res[3] = qb; res[4] = qe;
        uint32_t* raw = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)qlen + (size_t)wlen + 4));
        int nr = banded(r + rb, q + qb, re - rb + 1, qe - qb + 1, sc, raw, qlen + wlen + 4);
        if (nr < 0) n = nr;
        else {
            /* soft clips + M split into '=' / 'X' runs by translated code */
            if (qb > 0) { if (n >= cap) n = -1; else cigar[n++] = ((uint32_t)qb << 4) | 4u; }
            int ri = rb, qi = qb, run = 0, run_op = -1;
            for (int k = 0; k < nr && n >= 0; k++) {
                int op = (int)(raw[k] & 15), len = (int)(raw[k] >> 4);
                if (op == 0) {
                    for (int t = 0; t < len; t++, ri++, qi++) {
                        int o = r[ri] == q[qi] ? 7 : 8;
                        if (o != run_op && run > 0) {
                            if (n >= cap) { n = -1; break; }
                            cigar[n++] = ((uint32_t)run << 4) | (uint32_t)run_op; run = 0;
                        }
                        run_op = o; run++;
                    }
                } else {
                    if (run > 0) {
                        if (n >= cap) { n = -1; break; }
                        cigar[n++] = ((uint32_t)run << 4) | (uint32_t)run_op; run = 0;
                    }
                    if (n >= cap) { n = -1; break; }
                    cigar[n++] = raw[k];
                    if (op == 1) qi += len; else ri += len;
                }
            }
            if (n >= 0 && run > 0) { if (n >= cap) n = -1; else cigar[n++] = ((uint32_t)run << 4) | (uint32_t)run_op; }
            const int tail = qlen - qe - 1;
            if (n >= 0 && tail > 0) { if (n >= cap) n = -1; else cigar[n++] = ((uint32_t)tail << 4) | 4u; }
        }
        free(raw); free(rr); free(qr);
    }
    free(r); free(q);
    return n;
}
