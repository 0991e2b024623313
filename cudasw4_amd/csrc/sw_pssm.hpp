// sw_pssm.hpp — the device form of a position-specific scoring matrix (sw_set_query_pssm, include/cudasw4_amd_pssm.h).
//
// A PSSM query replaces "query letter -> row of the substitution table" by "query position -> its own row of 21 scores".
// The scan kernels never see the difference: they read the per-query profile tile, and the profile builder
// (sw_dp_kernel.hpp: sw_build_profile_kernel) takes its scores from the staged PSSM instead of matrix[letter].  The row
// pipeline (sw_rows_pipeline.hpp) has no tile: a stage walks the query row by row and needs row i's 21 scores, one per
// lane, when it gets there.  Both read ONE staged form, laid out for the pipeline:
//
//     tile t = rows 16 t .. 16 t + 15,   byte ((t * 32 + letter) * 16 + (row & 15)) = score(row, letter)
//
// i.e. the 16 rows of a tile are transposed, so that lane `letter` of a stage fetches its scores for a whole batch of rows
// (8: half a tile row) with one aligned 8-byte load, batches ahead of their use.
// Letters 21..31 are padding of the 32-lane tile row (never selected), rows from qlen on — up to the end of the tile
// behind the query's last one — score kPssmPadScore against every letter: they are the padding rows of the last stripe.
#pragma once
#include <cstddef>
#include <cstdint>

namespace swk {

constexpr int kPssmTileRows = 16;
constexpr int kPssmTileLetters = 32;
constexpr int kPssmTileBytes = kPssmTileRows * kPssmTileLetters;
constexpr int kPssmPadScore = -1;   // any negative score neutralises padding (sw_set_matrix asks the same of a table)

// staged rows for a query of qlen positions: whole tiles, and one more (the padding row qlen always exists; a prefetch
// of the batch behind the last one stays inside the buffer)
__host__ __device__ constexpr int64_t pssm_staged_rows(int64_t qlen) {
    return ((qlen + kPssmTileRows - 1) / kPssmTileRows + 1) * kPssmTileRows;
}
__host__ __device__ constexpr size_t pssm_index(int64_t row, int letter) {
    return ((size_t)(row / kPssmTileRows) * kPssmTileLetters + (size_t)letter) * kPssmTileRows + (size_t)(row % kPssmTileRows);
}

}  // namespace swk
