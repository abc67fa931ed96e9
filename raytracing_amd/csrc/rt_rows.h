// rt_rows.h -- a batch's record as a kernel reads it: s_ray [rec_rows][6][R] of the batch's dtype, istep [R] and perm [R] or NULL
// (rtmi_device_view).  Plain loads and index arithmetic; how a kernel walks its rows is the kernel's own.  Anonymous namespace,
// as with rt_crossing.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rtmi.h"

namespace {

// the columns of a row
enum : int { COL_X, COL_Y, COL_PX, COL_PY, COL_T, COL_TH };

template <typename T> struct Rows {
    const T* s_ray;
    const int32_t* istep;         // [R] last written row
    const int32_t* perm;          // [R] or NULL: slot k holds the caller's ray perm[k]
    long R, rec_rows;
    // row i of slot k: p[COL_* * R] is a column of it, p + pitch() the next row
    __device__ __forceinline__ const T* row(long i, long k) const { return s_ray + (size_t)i * pitch() + k; }
    __device__ __forceinline__ size_t pitch() const { return (size_t)6 * R; }
    // the last row the ray wrote, and the last one the record holds of it
    __device__ __forceinline__ long last(long k) const { return istep[k]; }
    __device__ __forceinline__ long last_recorded(long k) const { return last(k) < rec_rows - 1 ? last(k) : rec_rows - 1; }
    __device__ __forceinline__ long caller(long k) const { return perm ? (long)perm[k] : k; }
};

template <typename T> Rows<T> rows_of(const rtmi_device_view& v) { return Rows<T>{(const T*)v.s_ray, v.istep, v.perm, (long)v.R, (long)v.rec_rows}; }

}  // namespace
