// rt_tomo.h -- the storage layout of a compiled tomography matrix (tomo.hip, rtmi_tomo_*), as arithmetic:
// host and device, no HIP in it, so that a host program can include it (tests/native/tomo_layout.cpp).
//
// A handle holds blocks, one per append.  A block's rows are cut into slices of 64 (a wave: one lane per row); a slice is as wide as
// its longest row, and its k-th segments lie side by side:
//     slot(row r, segment k)      = off[r / 64] + 64 k + r % 64           base[slot]: the segment's first column
//     value(row r, segment k, q)  = 4 off[r / 64] + 64 (4 k + q) + r % 64   val[...]: its four weights p[q]
// off[s] = 64 times the widths of the slices before s, off[slices] the block's padded segment count.  A wave's load of the k-th
// base, or of the k-th p[q], of its 64 rows is one contiguous 256- or 512-byte access.  Slots past a row's own length are padding:
// base 0, values +0.0, never read by the products (each lane stops at its row's length).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RT_TOMO_HD __host__ __device__
#else
#define RT_TOMO_HD
#endif

namespace rt {

constexpr int kTomoSlice = 64;

RT_TOMO_HD inline int64_t tomo_slices(int64_t rows) { return (rows + kTomoSlice - 1) / kTomoSlice; }
// off: the slice's offset off[r / 64]
RT_TOMO_HD inline int64_t tomo_slot(int64_t off, int64_t k, int lane) { return off + kTomoSlice * k + lane; }
RT_TOMO_HD inline int64_t tomo_value(int64_t off, int64_t k, int q, int lane) { return 4 * off + kTomoSlice * (4 * k + q) + lane; }

// off [slices + 1] from the rows' lengths len [rows]; returns the segments (the sum of len).  off[slices] is the padded count.
inline int64_t tomo_offsets(const int32_t* len, int64_t rows, int64_t* off) {
    const int64_t ns = tomo_slices(rows);
    int64_t total = 0, at = 0;
    for (int64_t s = 0; s < ns; s++) {
        off[s] = at;
        int32_t width = 0;
        const int64_t r1 = (s + 1) * kTomoSlice < rows ? (s + 1) * kTomoSlice : rows;
        for (int64_t r = s * kTomoSlice; r < r1; r++) {
            width = len[r] > width ? len[r] : width;
            total += len[r];
        }
        at += (int64_t)kTomoSlice * width;
    }
    off[ns] = at;
    return total;
}

}  // namespace rt
