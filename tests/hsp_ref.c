/* hsp_ref.c — scalar full-matrix reference of sw_align_hsps / sw_align_hsps_pssm (include/cudasw4_amd_hsps.h, DESIGN.md
 * "Several alignments per hit").  TEST INFRASTRUCTURE ONLY: compiled on demand by tests/hsp_ref.py.
 *
 * Alignment k of a pair is what the four steps of align_ref.c / pssm_align_ref.c give when the substitution score of every
 * cell that is an aligned pair ('=' / 'X' column) of alignments 0 .. k-1 is minus infinity in all three passes: the
 * diagonal move into such a cell does not exist; E and F run through it.
 *   score of cell (i, j): letters  m[21 * q[i] + s[j]]        (m: rows x 21, one row per query code)
 *                         PSSM     pssm[21 * i + min(s[j], 20)]
 *   1. S = max H of the local recurrence; end = the cell with H == S of smallest column, then smallest row.
 *   2. global recurrence over the reversed prefixes from the end; start = the cell with G == S of largest column, then
 *      largest row.
 *   3. global recurrence over the rectangle, traced back from its far corner in state H: H prefers diag, E, F; E and F
 *      prefer open over extend.  A vetoed diagonal never equals H.
 *   4. CIGAR words len << 4 | op; '=': letters the same standard residue, PSSM subject code < 20 equal to the consensus
 *      code (the caller's, or the lowest code < 20 with the largest score of the row).
 * Slots: 0 as sw_align_hits (expected score, trace budget, CIGAR cap, max_subject_len); k >= 1: S_k < min_score -> EMPTY from
 * there on; behind EMPTY: EMPTY; behind NO_TRACE / SCORE_MISMATCH / BAD_LENGTH: NOT_COMPUTED.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG (-1000000000)

enum { R_SCORE, R_STATUS, R_QB, R_QE, R_SB, R_SE, R_COLS, R_IDS, R_MIS, R_GOPENS, R_GCOLS, R_NCIGAR, R_FIELDS };
enum { ST_OK = 0, ST_EMPTY = 1, ST_NO_TRACE = 2, ST_SCORE_MISMATCH = 3, ST_BAD_LENGTH = 4, ST_NOT_COMPUTED = 5 };
enum { OP_I = 1, OP_D = 2, OP_EQ = 7, OP_X = 8 };

typedef struct {
    const int8_t* q;      /* letters: query codes; PSSM: consensus codes or NULL */
    const int8_t* m;      /* letters: the table; NULL: PSSM form */
    const int8_t* pssm;   /* PSSM form: qlen x 21 */
    const int8_t* s;
    int32_t qlen, slen, gop, gex;
    const uint8_t* used;  /* qlen x slen: 1 = an aligned pair of an earlier alignment */
} pair_t;

static int32_t max2(int32_t a, int32_t b) { return a > b ? a : b; }

/* diag + substitution score, NEG for a used cell (NEG is below every H, E and F a pass can hold next to a real path) */
static int32_t diag_move(const pair_t* p, int32_t diag, int32_t i, int32_t j) {
    if (p->used[(size_t)i * p->slen + j]) return NEG;
    const int32_t c = p->s[j] > 20 ? 20 : p->s[j];
    return diag + (p->m ? p->m[21 * p->q[i] + p->s[j]] : p->pssm[21 * i + c]);
}

static int identical(const pair_t* p, int32_t i, int32_t j) {
    const int32_t b = p->s[j];
    if (p->m) return p->q[i] == b && b < 20;
    if (b >= 20) return 0;
    if (p->q) return p->q[i] == b;
    int32_t best = 0;
    for (int32_t c = 1; c < 20; c++)
        if (p->pssm[21 * i + c] > p->pssm[21 * i + best]) best = c;
    return best == b;
}

/* phase 1: S and the end cell */
static int32_t local_end(const pair_t* p, int32_t* qe, int32_t* se) {
    const int32_t slen = p->slen;
    int32_t* H = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(slen + 1));
    int32_t* F = H + slen + 1;
    for (int32_t j = 0; j <= slen; j++) { H[j] = 0; F[j] = NEG; }
    int32_t best = 0, bi = -1, bj = -1;
    for (int32_t i = 0; i < p->qlen; i++) {
        int32_t diag = 0, left = 0, E = NEG;
        for (int32_t j = 1; j <= slen; j++) {
            const int32_t up = H[j];
            E = max2(E + p->gex, left + p->gop);
            F[j] = max2(F[j] + p->gex, up + p->gop);
            const int32_t h = max2(max2(diag_move(p, diag, i, j - 1), E), max2(F[j], 0));
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

/* phase 2: the start cell, from one global pass over the reversed prefixes q[qe..0] x s[se..0] */
static int32_t global_start(const pair_t* p, int32_t qe, int32_t se, int32_t* qs, int32_t* ss) {
    const int32_t rows = qe + 1, cols = se + 1;
    int32_t* H = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(cols + 1));
    int32_t* F = H + cols + 1;
    H[0] = 0;
    F[0] = NEG;
    for (int32_t j = 1; j <= cols; j++) { H[j] = p->gop + (j - 1) * p->gex; F[j] = NEG; }
    int32_t best = NEG, bi = -1, bj = -1;
    for (int32_t i = 1; i <= rows; i++) {
        int32_t diag = H[0], E = NEG;
        H[0] = p->gop + (i - 1) * p->gex;
        int32_t left = H[0];
        for (int32_t j = 1; j <= cols; j++) {
            const int32_t up = H[j];
            E = max2(E + p->gex, left + p->gop);
            F[j] = max2(F[j] + p->gex, up + p->gop);
            const int32_t h = max2(max2(diag_move(p, diag, qe - (i - 1), se - (j - 1)), E), F[j]);
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

/* phase 3 + 4: global DP of the rectangle with direction nibbles, traceback, CIGAR; the aligned pairs go to `mark` */
static int trace(const pair_t* p, int32_t qs, int32_t qe, int32_t ss, int32_t se, int32_t* out, uint32_t* cigar, int32_t cap,
                 uint8_t* mark) {
    const int32_t rows = qe - qs + 1, cols = se - ss + 1, gop = p->gop, gex = p->gex;
    uint8_t* dir = (uint8_t*)malloc((size_t)rows * (size_t)cols);
    int32_t* H = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(cols + 1));
    int32_t* F = H + cols + 1;
    if (!dir || !H) { free(dir); free(H); return -1; }
    H[0] = 0;
    F[0] = NEG;
    for (int32_t j = 1; j <= cols; j++) { H[j] = gop + (j - 1) * gex; F[j] = NEG; }
    for (int32_t i = 1; i <= rows; i++) {
        int32_t diag = H[0], E = NEG;
        H[0] = gop + (i - 1) * gex;
        int32_t left = H[0];
        for (int32_t j = 1; j <= cols; j++) {
            const int32_t up = H[j];
            const int e_ext = E + gex > left + gop, f_ext = F[j] + gex > up + gop;
            E = max2(E + gex, left + gop);
            F[j] = max2(F[j] + gex, up + gop);
            const int32_t dm = diag_move(p, diag, qs + i - 1, ss + j - 1);
            const int32_t h = max2(max2(dm, E), F[j]);
            const int src = (h == dm && dm != NEG) ? 0 : (h == E ? 1 : 2);
            dir[(size_t)(i - 1) * cols + (j - 1)] = (uint8_t)(src | e_ext << 2 | f_ext << 3);
            H[j] = h;
            diag = up;
            left = h;
        }
    }
    free(H);
    int32_t i = rows, j = cols, state = 0, nruns = 0, run_op = 0, run_len = 0;
    int32_t ids = 0, mis = 0, opens = 0, gcols = 0, npairs = 0;
    uint32_t* runs = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(rows + cols + 1));
    int32_t* pairs = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(rows + 1));
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
                if (identical(p, qs + i - 1, ss + j - 1)) { EMIT(OP_EQ); ids++; } else { EMIT(OP_X); mis++; }
                pairs[2 * npairs] = qs + i - 1;
                pairs[2 * npairs + 1] = ss + j - 1;
                npairs++;
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
    const int fits = nruns <= cap;
    if (fits) {
        out[R_IDS] = ids;
        out[R_MIS] = mis;
        out[R_GOPENS] = opens;
        out[R_GCOLS] = gcols;
        out[R_COLS] = ids + mis + gcols;
        out[R_NCIGAR] = nruns;
        for (int32_t k = 0; k < nruns; k++) cigar[k] = runs[nruns - 1 - k];
        for (int32_t k = 0; k < npairs; k++) mark[(size_t)pairs[2 * k] * p->slen + pairs[2 * k + 1]] = 1;
    }
    free(runs);
    free(pairs);
    return fits ? 0 : 1;
}

static void blank(int32_t* out, int status) {
    for (int k = 0; k < R_FIELDS; k++) out[k] = 0;
    out[R_QB] = out[R_QE] = out[R_SB] = out[R_SE] = -1;
    out[R_STATUS] = status;
}

/* q: letters: the query; PSSM form (m == NULL): the consensus or NULL.  expected: < 0 = none.  trace_bytes: < 0 = no limit.
 * caps: max_hsps CIGAR slot sizes in words; cigar: the slots one behind the other.  out: max_hsps x R_FIELDS.
 * Returns 0, or -1 when memory ran out or the reference contradicts itself. */
int hsr_align(const int8_t* q, const int8_t* m, const int8_t* pssm, int32_t qlen, const int8_t* s, int32_t slen, int32_t gop,
              int32_t gex, int32_t max_hsps, int32_t min_score, int32_t max_subject_len, int32_t expected, int64_t trace_bytes,
              const int32_t* caps, int32_t* out, uint32_t* cigar) {
    uint8_t* used = (uint8_t*)calloc((size_t)(qlen > 0 ? qlen : 1) * (size_t)(slen > 0 ? slen : 1), 1);
    if (!used) return -1;
    const pair_t p = {q, m, pssm, s, qlen, slen, gop, gex, used};
    int rc = 0, fill = -1;   /* fill: the status of every slot from k on, once nothing more is computed */
    for (int32_t k = 0; k < max_hsps; k++, out += R_FIELDS, cigar += caps[k - 1]) {
        if (fill >= 0) { blank(out, fill); continue; }
        blank(out, ST_OK);
        if (slen > max_subject_len) { out[R_STATUS] = ST_BAD_LENGTH; fill = ST_NOT_COMPUTED; continue; }
        int32_t qe = -1, se = -1, qs = -1, ss = -1;
        int32_t S = (qlen > 0 && slen > 0) ? local_end(&p, &qe, &se) : 0;
        if (k > 0 && S < min_score) S = 0;
        out[R_SCORE] = S;
        const int mismatch = k == 0 && expected >= 0 && expected != S;
        if (S == 0) {
            out[R_STATUS] = mismatch ? ST_SCORE_MISMATCH : ST_EMPTY;
            fill = mismatch ? ST_NOT_COMPUTED : ST_EMPTY;
            continue;
        }
        if (global_start(&p, qe, se, &qs, &ss) != S) { rc = -1; break; }
        out[R_QB] = qs;
        out[R_QE] = qe + 1;
        out[R_SB] = ss;
        out[R_SE] = se + 1;
        if (mismatch) { out[R_STATUS] = ST_SCORE_MISMATCH; fill = ST_NOT_COMPUTED; continue; }
        const int64_t need = (int64_t)((qe - qs + 1 + 511) / 512) * (se - ss + 1 + 63) * 256;
        int t = 1;
        if (trace_bytes < 0 || need <= trace_bytes) {
            t = trace(&p, qs, qe, ss, se, out, cigar, caps[k], used);
            if (t < 0) { rc = -1; break; }
        }
        if (t > 0) { out[R_STATUS] = ST_NO_TRACE; fill = ST_NOT_COMPUTED; }
    }
    free(used);
    return rc;
}
