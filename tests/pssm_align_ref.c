/* pssm_align_ref.c — scalar full-matrix reference of sw_align_hits_pssm (include/cudasw4_amd_pssm.h, DESIGN.md "Hit
 * alignment of PSSM queries").  TEST INFRASTRUCTURE ONLY: compiled on demand by tests/pssm_align_ref.py.
 *
 * The four steps of align_ref.c with two differences: the substitution score of query position i against subject letter
 * c is p[21 * i + c] (p: qlen x 21, row-major), and an aligned pair at position i is '=' when the subject code is below
 * 20 and equals cons[i], else 'X'.  cons == NULL: position i has the lowest code c < 20 with the largest p[21 * i + c].
 *   1. S = max H; end (qe, se) = the cell with H == S of smallest se, then smallest qe.
 *   2. G(i, j) = global score of rows i..qe x s[j..se]; start (qs, ss) = the cell with G == S of largest ss, then largest qs.
 *   3. global DP of rows qs..qe x s[ss..se], traced back from (qe, se) in state H: H prefers diag, E, F; E and F prefer
 *      open over extend.
 *   4. CIGAR words len << 4 | op: '=' 7, 'X' 8, 'I' 1 (query position, gap), 'D' 2 (subject residue, gap).
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG (-1000000000)

enum { R_SCORE, R_STATUS, R_QB, R_QE, R_SB, R_SE, R_COLS, R_IDS, R_MIS, R_GOPENS, R_GCOLS, R_NCIGAR, R_FIELDS };
enum { ST_OK = 0, ST_EMPTY = 1, ST_NO_TRACE = 2 };
enum { OP_I = 1, OP_D = 2, OP_EQ = 7, OP_X = 8 };

static int32_t max2(int32_t a, int32_t b) { return a > b ? a : b; }

/* phase 1: S and the end cell */
static int32_t local_end(const int8_t* p, int32_t qlen, const int8_t* s, int32_t slen, int32_t gop,
                         int32_t gex, int32_t* qe, int32_t* se) {
    int32_t* H = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(slen + 1));
    int32_t* F = H + slen + 1;
    for (int32_t j = 0; j <= slen; j++) { H[j] = 0; F[j] = NEG; }
    int32_t best = 0, bi = -1, bj = -1;
    for (int32_t i = 0; i < qlen; i++) {
        int32_t diag = 0, left = 0, E = NEG;
        for (int32_t j = 1; j <= slen; j++) {
            const int32_t up = H[j];
            E = max2(E + gex, left + gop);
            F[j] = max2(F[j] + gex, up + gop);
            int32_t h = max2(max2(diag + p[21 * i + s[j - 1]], E), max2(F[j], 0));
            H[j] = h;
            diag = up;
            left = h;
            if (h > best || (h == best && h > 0 && (j - 1 < bj || (j - 1 == bj && i < bi)))) { best = h; bi = i; bj = j - 1; }
        }
    }
    free(H);
    *qe = bi;
    *se = bj;
    return best;
}

/* phase 2: the start cell, from one global pass over the reversed prefixes: rows qe..0 x s[se..0] */
static int32_t global_start(const int8_t* p, int32_t qe, const int8_t* s, int32_t se, int32_t gop,
                            int32_t gex, int32_t* qs, int32_t* ss) {
    const int32_t rows = qe + 1, cols = se + 1;
    int32_t* H = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(cols + 1));
    int32_t* F = H + cols + 1;
    H[0] = 0;
    F[0] = NEG;
    for (int32_t j = 1; j <= cols; j++) { H[j] = gop + (j - 1) * gex; F[j] = NEG; }
    int32_t best = NEG, bi = -1, bj = -1;
    for (int32_t i = 1; i <= rows; i++) {
        const int8_t* row = p + 21 * (qe - (i - 1));
        int32_t diag = H[0], E = NEG;
        H[0] = gop + (i - 1) * gex;
        int32_t left = H[0];
        for (int32_t j = 1; j <= cols; j++) {
            const int32_t up = H[j];
            E = max2(E + gex, left + gop);
            F[j] = max2(F[j] + gex, up + gop);
            const int32_t h = max2(max2(diag + row[s[se - (j - 1)]], E), F[j]);
            H[j] = h;
            diag = up;
            left = h;
            /* reversed coordinates: largest ss == smallest j, largest qs == smallest i */
            if (h > best || (h == best && (j < bj || (j == bj && i < bi)))) { best = h; bi = i; bj = j; }
        }
    }
    free(H);
    *qs = qe - (bi - 1);
    *ss = se - (bj - 1);
    return best;
}

static int32_t consensus(const int8_t* p, const int8_t* cons, int32_t i) {
    if (cons) return cons[i];
    int32_t best = 0;
    for (int32_t c = 1; c < 20; c++)
        if (p[21 * i + c] > p[21 * i + best]) best = c;
    return best;
}

/* phase 3 + 4: global DP of the rectangle with direction nibbles, traceback, CIGAR */
static int trace(const int8_t* p, const int8_t* cons, int32_t qs, int32_t qe, const int8_t* s, int32_t ss, int32_t se,
                 int32_t gop, int32_t gex, int32_t* out, uint32_t* cigar, int32_t cap) {
    const int32_t rows = qe - qs + 1, cols = se - ss + 1;
    uint8_t* dir = (uint8_t*)malloc((size_t)rows * (size_t)cols);
    int32_t* H = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(cols + 1));
    int32_t* F = H + cols + 1;
    if (!dir || !H) { free(dir); free(H); return -1; }
    H[0] = 0;
    F[0] = NEG;
    for (int32_t j = 1; j <= cols; j++) { H[j] = gop + (j - 1) * gex; F[j] = NEG; }
    for (int32_t i = 1; i <= rows; i++) {
        const int8_t* row = p + 21 * (qs + i - 1);
        int32_t diag = H[0], E = NEG;
        H[0] = gop + (i - 1) * gex;
        int32_t left = H[0];
        for (int32_t j = 1; j <= cols; j++) {
            const int32_t up = H[j];
            const int e_ext = E + gex > left + gop, f_ext = F[j] + gex > up + gop;
            E = max2(E + gex, left + gop);
            F[j] = max2(F[j] + gex, up + gop);
            const int32_t dm = diag + row[s[ss + j - 1]];
            const int32_t h = max2(max2(dm, E), F[j]);
            const int src = h == dm ? 0 : (h == E ? 1 : 2);
            dir[(size_t)(i - 1) * cols + (j - 1)] = (uint8_t)(src | e_ext << 2 | f_ext << 3);
            H[j] = h;
            diag = up;
            left = h;
        }
    }
    free(H);
    /* walk back, runs collected last-first */
    int32_t i = rows, j = cols, state = 0, nruns = 0, run_op = 0, run_len = 0;
    int32_t ids = 0, mis = 0, opens = 0, gcols = 0;
    uint32_t* runs = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(rows + cols + 1));
#define EMIT(op)                                                                    \
    do {                                                                            \
        if ((op) != run_op && run_len) { runs[nruns++] = (uint32_t)run_len << 4 | (uint32_t)run_op; run_len = 0; } \
        if ((op) != run_op && ((op) == OP_I || (op) == OP_D)) opens++;              \
        run_op = (op);                                                              \
        run_len++;                                                                  \
    } while (0)
    while (i > 0 && j > 0) {
        const uint8_t d = dir[(size_t)(i - 1) * cols + (j - 1)];
        if (state == 0) {
            if ((d & 3) == 0) {
                const int32_t a = consensus(p, cons, qs + i - 1), b = s[ss + j - 1];
                if (b >= 0 && b < 20 && a == b) { EMIT(OP_EQ); ids++; } else { EMIT(OP_X); mis++; }
                i--;
                j--;
            } else {
                state = d & 3;
            }
        } else if (state == 1) {
            EMIT(OP_D);
            gcols++;
            state = (d >> 2 & 1) ? 1 : 0;
            j--;
        } else {
            EMIT(OP_I);
            gcols++;
            state = (d >> 3 & 1) ? 2 : 0;
            i--;
        }
    }
    while (i > 0) { EMIT(OP_I); gcols++; i--; }
    while (j > 0) { EMIT(OP_D); gcols++; j--; }
    if (run_len) runs[nruns++] = (uint32_t)run_len << 4 | (uint32_t)run_op;
#undef EMIT
    free(dir);
    out[R_IDS] = ids;
    out[R_MIS] = mis;
    out[R_GOPENS] = opens;
    out[R_GCOLS] = gcols;
    out[R_COLS] = ids + mis + gcols;
    out[R_NCIGAR] = nruns;
    const int fits = nruns <= cap;
    if (fits)
        for (int32_t k = 0; k < nruns; k++) cigar[k] = runs[nruns - 1 - k];
    free(runs);
    return fits ? 0 : 1;
}

/* out: R_FIELDS int32 (see the enum); cigar: room for cap words.  Returns 0, or -1 when memory ran out. */
int par_align(const int8_t* p, const int8_t* cons, int32_t qlen, const int8_t* s, int32_t slen, int32_t gop, int32_t gex,
              int coords_only, int32_t* out, uint32_t* cigar, int32_t cap) {
    for (int k = 0; k < R_FIELDS; k++) out[k] = 0;   /* counts stay 0 without a CIGAR */
    out[R_QB] = out[R_QE] = out[R_SB] = out[R_SE] = -1;
    int32_t qe = -1, se = -1, qs = -1, ss = -1;
    const int32_t S = (qlen > 0 && slen > 0) ? local_end(p, qlen, s, slen, gop, gex, &qe, &se) : 0;
    out[R_SCORE] = S;
    if (S == 0) { out[R_STATUS] = ST_EMPTY; return 0; }
    const int32_t G = global_start(p, qe, s, se, gop, gex, &qs, &ss);
    if (G != S) return -1;
    out[R_QB] = qs;
    out[R_QE] = qe + 1;
    out[R_SB] = ss;
    out[R_SE] = se + 1;
    out[R_STATUS] = ST_OK;
    if (coords_only) return 0;
    const int rc = trace(p, cons, qs, qe, s, ss, se, gop, gex, out, cigar, cap);
    if (rc < 0) return -1;
    if (rc > 0) {
        out[R_STATUS] = ST_NO_TRACE;
        for (int k = R_COLS; k < R_FIELDS; k++) out[k] = 0;
    }
    return 0;
}
