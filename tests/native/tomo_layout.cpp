// rt_tomo.h as a program of its own (tests/test_tomo_ref.py builds it plain and with -fsanitize=address,undefined): the sliced
// layout of a compiled tomography matrix.  stdin: the number of blocks, then per block its row count and its rows' lengths.
// For every block it fills exactly-sized base and value arrays through tomo_slot / tomo_value -- a slot written twice or an
// index outside the arrays ends the program with status 1 (or under the sanitizer) -- and prints
//     block <first> <rows> <segments> <padded> off <off[0]> ... <off[slices]>
//     row <global row> <slot of segment 0, or -1> <value index of segment 0, q = 3, or -1>
// then "rows <total>".  A block's rows are numbered from the rows of the blocks before it, as rtmi_tomo_append numbers them.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../raytracing_amd/csrc/rt_tomo.h"

int main() {
    long nblocks = 0;
    if (std::scanf("%ld", &nblocks) != 1 || nblocks < 0) return 2;
    std::vector<std::vector<int32_t>> lens((size_t)nblocks);
    std::vector<int64_t> first((size_t)nblocks);
    int64_t total = 0;
    for (long b = 0; b < nblocks; b++) {
        long rows = 0;
        if (std::scanf("%ld", &rows) != 1 || rows < 0) return 2;
        lens[(size_t)b].resize((size_t)rows);
        for (long r = 0; r < rows; r++) {
            int v = 0;
            if (std::scanf("%d", &v) != 1 || v < 0) return 2;
            lens[(size_t)b][(size_t)r] = v;
        }
        first[(size_t)b] = total;
        total += rows;
    }
    for (long b = 0; b < nblocks; b++) {
        const std::vector<int32_t>& len = lens[(size_t)b];
        const int64_t rows = (int64_t)len.size(), ns = rt::tomo_slices(rows);
        std::vector<int64_t> off((size_t)ns + 1);
        const int64_t segments = rt::tomo_offsets(len.data(), rows, off.data());
        const int64_t padded = off[(size_t)ns];
        std::vector<int32_t> base((size_t)padded, -1);
        std::vector<double> val((size_t)padded * 4, -1.0);
        int64_t written = 0;
        for (int64_t r = 0; r < rows; r++) {
            const int64_t o = off[(size_t)(r >> 6)];
            const int lane = (int)(r & 63);
            for (int32_t k = 0; k < len[(size_t)r]; k++) {
                int32_t& s = base.at((size_t)rt::tomo_slot(o, k, lane));
                if (s != -1) return 1;
                s = (int32_t)r;
                for (int q = 0; q < 4; q++) {
                    double& v = val.at((size_t)rt::tomo_value(o, k, q, lane));
                    if (v != -1.0) return 1;
                    v = (double)(4 * k + q);
                }
                written++;
            }
        }
        if (written != segments) return 1;
        std::printf("block %lld %lld %lld %lld off", (long long)first[(size_t)b], (long long)rows, (long long)segments, (long long)padded);
        for (int64_t v : off) std::printf(" %lld", (long long)v);
        std::printf("\n");
        for (int64_t r = 0; r < rows; r++) {
            const int64_t o = off[(size_t)(r >> 6)], g = first[(size_t)b] + r;
            const bool any = len[(size_t)r] > 0;
            std::printf("row %lld %lld %lld\n", (long long)g, any ? (long long)rt::tomo_slot(o, 0, (int)(r & 63)) : -1LL,
                        any ? (long long)rt::tomo_value(o, 0, 3, (int)(r & 63)) : -1LL);
        }
    }
    std::printf("rows %lld\n", (long long)total);
    return 0;
}
