/* pssm_ref.c — scalar reference of profile search: local alignment with affine gaps of a position-specific scoring matrix
 * against a subject, written from the recurrence in DESIGN.md (section "Profile search"):
 *
 *   E(i,j) = max(E(i,j-1) + gex, H(i,j-1) + gop)        a run of subject residues against a gap
 *   F(i,j) = max(F(i-1,j) + gex, H(i-1,j) + gop)        a run of query positions against a gap
 *   H(i,j) = max(0, H(i-1,j-1) + pssm[i][s_j], E(i,j), F(i,j)),   score = max H
 *
 * (the first gap column costs gop, every further one gex — the convention of the scan kernels and of the oracle).
 * pssm: qlen x 21 int8, row = query position, column = dbdata subject code 0..20; subject codes outside 0..20 count as 20.
 * Test infrastructure: tests/test_pssm_cpu.py pins it to the project's oracle (swo_score) through pssm.from_sequence. */
#include <stdint.h>
#include <stdlib.h>

#define PR_NEG (-(1 << 29))

static int32_t max2(int32_t a, int32_t b) { return a > b ? a : b; }

int32_t pr_score(const int8_t* pssm, int32_t qlen, const int8_t* subject, int32_t slen, int gop, int gex) {
    if (qlen <= 0 || slen <= 0) return 0;
    /* column by column: H and F of the previous column, one entry per query position */
    int32_t* H = (int32_t*)malloc(sizeof(int32_t) * (size_t)(qlen + 1));
    int32_t* E = (int32_t*)malloc(sizeof(int32_t) * (size_t)(qlen + 1));
    if (!H || !E) { free(H); free(E); return -1; }
    for (int32_t i = 0; i <= qlen; i++) { H[i] = 0; E[i] = PR_NEG; }
    int32_t best = 0;
    for (int32_t j = 0; j < slen; j++) {
        int c = subject[j];
        if (c < 0 || c > 20) c = 20;
        int32_t diag = 0;      /* H(i-1, j-1) */
        int32_t f = PR_NEG;    /* F(i, j): vertical, inside this column */
        int32_t up = 0;        /* H(i-1, j) */
        for (int32_t i = 1; i <= qlen; i++) {
            const int32_t left = H[i];                       /* H(i, j-1) */
            const int32_t e = max2(E[i] + gex, left + gop);  /* E(i, j) */
            f = max2(f + gex, up + gop);
            int32_t h = diag + (int32_t)pssm[(size_t)(i - 1) * 21 + c];
            h = max2(max2(h, 0), max2(e, f));
            diag = left;
            H[i] = h;
            E[i] = e;
            up = h;
            if (h > best) best = h;
        }
    }
    free(H);
    free(E);
    return best;
}

/* every subject of a dbdata-layout DB: chars + (offsets[i] - offsets[0]), lengths[i] residues */
void pr_scan(const int8_t* pssm, int32_t qlen, const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int64_t n,
             int gop, int gex, int32_t* out) {
    for (int64_t i = 0; i < n; i++) out[i] = pr_score(pssm, qlen, chars + (offsets[i] - offsets[0]), lengths[i], gop, gex);
}
