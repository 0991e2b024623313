// pssm_query.hpp — position-specific scoring matrices as queries of the host driver: the NCBI ASCII reader of `align --pssm`
// and the submit that installs a PSSM through sw_set_query_pssm (include/cudasw4_amd_pssm.h).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "search_driver.hpp"

namespace swh {

constexpr int kPssmColumns = 21;        // dbdata subject codes 0..20
constexpr int8_t kPssmOtherScore = -1;  // column 20 of every row read from an ASCII file (the format has 20 columns)

struct PssmQuery {
    std::string name;            // base name of the file it was read from
    std::string consensus;       // the residue column of the file
    std::vector<int8_t> scores;  // length() x kPssmColumns, row-major
    int32_t length() const { return int32_t(scores.size() / size_t(kPssmColumns)); }
};

// An NCBI ASCII PSSM (psiblast -out_ascii_pssm): a header line with the 20 column letters A R N D C Q E G H I L K M F P S T W Y V
// (this project's code order 0..19; repeated when the percentage block follows), then one line per position — index
// (consecutive from 1), consensus residue, 20 integer scores, optionally 20 percentages and two information columns, which
// are ignored.  Reading stops at the first line behind the positions that is not a position line (the Lambda / K footer).
// Throws std::runtime_error("<file>:<line>: <what>") for a missing header, a wrong number of columns, a score outside
// int8 or non-consecutive indices.  No GPU involved.
PssmQuery read_ascii_pssm(const std::string& path);

// The writer of that format (align --outPssm): the 20 standard columns of `pssm` (length x kPssmColumns; column 20 is not
// part of the format) under the header, one line per position with its consensus residue; the layout of the Python
// module's pssm.write_ascii, which read_ascii_pssm and pssm.read_ascii read back.  No GPU involved.
void write_ascii_pssm(const std::string& path, const int8_t* pssm, int32_t length, const std::string& consensus);

// SearchDriver::submit for a PSSM (pssm: length x kPssmColumns int8, column 20 negative in every row; copied):
// collect() returns its results like a letter query's, and a letter query may be in flight beside it.
void submit_pssm(SearchDriver& driver, const int8_t* pssm, int32_t length);

}  // namespace swh
