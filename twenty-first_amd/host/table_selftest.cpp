// table_selftest.cpp -- table_columns_to_rows / table_rows_to_columns / table_gather_rows of the C++ mirror (twenty_first.hpp) on
// small tables against loops on the host.  One PASS line per case.
// Exit code 0 = all passed; 77 = no GPU (skipped); anything else = failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "twenty_first.hpp"

using namespace twenty_first;
using B = BFieldElement;
using X = XFieldElement;

#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static B b(uint64_t v) { return B::new_(v); }
static B make(B*, uint64_t v) { return b(v); }
static X make(X*, uint64_t v) { return X{{b(v), b(v + 1000000), b(v + 2000000)}}; }

// element (i, j) of table t, in either layout
template <class FF>
static FF at(uint64_t t, uint64_t i, uint64_t j) { return make((FF*)nullptr, (t * 1000 + i) * 1000 + j); }

template <class FF>
static int run(const char* field, size_t n_rows, size_t n_cols, size_t batch) {
    std::vector<FF> cols(batch * n_rows * n_cols), rows(batch * n_rows * n_cols);
    for (size_t t = 0; t < batch; ++t)
        for (size_t i = 0; i < n_rows; ++i)
            for (size_t j = 0; j < n_cols; ++j) {
                cols[(t * n_cols + j) * n_rows + i] = at<FF>(t, i, j);
                rows[(t * n_rows + i) * n_cols + j] = at<FF>(t, i, j);
            }
    EXPECT(table_columns_to_rows(cols, n_rows, n_cols, batch) == rows);
    EXPECT(table_rows_to_columns(rows, n_rows, n_cols, batch) == cols);
    EXPECT(table_rows_to_columns(table_columns_to_rows(cols, n_rows, n_cols, batch), n_rows, n_cols, batch) == cols);
    std::printf("PASS %s transposes, %zu tables of %zu x %zu\n", field, batch, n_rows, n_cols);
    std::vector<uint32_t> idx;
    for (size_t q = 0; q < 70; ++q) idx.push_back((uint32_t)((q * 37 + 5) % n_rows));
    idx.push_back(idx[3]);  // a repeat
    std::vector<FF> want(batch * idx.size() * n_cols);
    for (size_t t = 0; t < batch; ++t)
        for (size_t q = 0; q < idx.size(); ++q)
            for (size_t j = 0; j < n_cols; ++j) want[(t * idx.size() + q) * n_cols + j] = at<FF>(t, idx[q], j);
    EXPECT(table_gather_rows(cols, TF_TABLE_COLUMN_MAJOR, n_rows, n_cols, idx, batch) == want);
    EXPECT(table_gather_rows(rows, TF_TABLE_ROW_MAJOR, n_rows, n_cols, idx, batch) == want);
    std::printf("PASS %s gather_rows from both layouts, %zu rows of %zu elements per table\n", field, idx.size(), n_cols);
    return 0;
}

int main() {
    if (tf_device_count() == 0) {
        std::printf("no GPU: skipped\n");
        return 77;
    }
    if (run<B>("BFieldElement", 130, 67, 2)) return 1;   // two tiles and a ragged edge of the 64 x 64 tile, either way
    if (run<X>("XFieldElement", 65, 35, 2)) return 1;    // the same for the 32 x 32 tile
    if (run<B>("BFieldElement", 1, 200, 1)) return 1;    // one row, beyond the 16 words of gather_elements
    if (run<X>("XFieldElement", 7, 1, 3)) return 1;
    // an index == n_rows is an error of the call (code 17)
    int code = 0;
    try {
        (void)table_gather_rows(std::vector<B>(12), TF_TABLE_ROW_MAJOR, 4, 3, std::vector<uint32_t>{0, 4, 1});
    } catch (const BackendError& e) {
        code = e.code;
    }
    EXPECT(code == TF_ERR_INVALID_ARGUMENT);
    std::printf("PASS gather_rows reports an index beyond the table (code 17)\n");
    // empty tables
    EXPECT(table_columns_to_rows(std::vector<B>{}, 0, 5).empty() && table_gather_rows(std::vector<X>(2), TF_TABLE_COLUMN_MAJOR, 2, 1, {}).empty());
    std::printf("PASS empty tables and empty index lists\n");
    return 0;
}
