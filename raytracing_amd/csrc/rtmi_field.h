// rtmi_field.h -- the field handle, shared by the unit that builds it (field.hip) and the unit whose kernels look it up (rtmi.hip).
// Every other unit sees a field through rtmi_internal_field_poly (rtmi_internal.h).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "rtmi_host.h"

struct rtmi_field {
    int device = 0;
    int dtype = RTMI_F64;
    int qx = 0, qy = 0;
    double ax = 0, hx = 0, bx = 0, ay = 0, hy = 0, by = 0;
    // fp64 build products (kept for rtmi_field_read and as the source of the packed arrays)
    double *dZ = nullptr, *dCdy = nullptr, *dCdx = nullptr;
    // packed, dtype-typed arrays the trace kernels gather from
    void *zn = nullptr, *g = nullptr;
    void* poly = nullptr;        // [(qy-1)*(qx-1)][rt::kPolyStride] of dtype: one polynomial per cell (rt_polytab.h)
    void* poly_base = nullptr;   // the allocation: the flat-cell map ([flat_pad] of dtype, rt::FieldDev::flat), then the table
    long flat_pad = 0;           // elements from the map's start to the table's
    long flat_cells = 0;         // cells the map marks flat
    double gmax = 0;             // the largest gradient-spline coefficient of the grid in magnitude (k_absmax)
    long steep_cells = 0;        // fp64 fields: cells whose map entry carries a steepness (k_polytab); with neither kind the kernels never look at the map
    int layered = 0;             // 1: the samples do not depend on x and the fast-form step kernels look the field up by its row alone (rtmi.h, rtmi_field_layered);
                                 // the row table then sits in the map's region, rt::kLayerStride * (row + 1) elements in front of poly
    double* rdiv = nullptr;      // [qx][24] then [qy][24]: reciprocals of the knot differences fpbspl divides by, knots, differences (rt_exact.h, AxisTab)
    hipStream_t stream = nullptr;
};

// A field's device memory is only valid on the device it was built on; callers that switch devices
// (rtmi_set_device, torch.cuda.set_device) get RTMI_ERR_ARG instead of a cross-device access.
static hipError_t check_device_impl(const rtmi_field* f, const char* who, int* rc) {
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev != f->device) {
        *rc = rtmi_internal_fail(RTMI_ERR_ARG, (std::string(who) + ": the field lives on device " + std::to_string(f->device) +
                                                " but the current device is " + std::to_string(dev)).c_str());
    }
    return hipSuccess;
}
#define DEVICE_TRY(f, who)                                  \
    do {                                                    \
        int rc_ = RTMI_OK;                                  \
        HIP_TRY(check_device_impl((f), (who), &rc_));       \
        if (rc_) return rc_;                                \
    } while (0)
