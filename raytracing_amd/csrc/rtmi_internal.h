// rtmi_internal.h -- hooks between the translation units of librtmi.so (not part of the C ABI, hidden visibility).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/rtmi.h"

// sets rtmi_last_error() and returns `code`
int rtmi_internal_fail(int code, const char* msg);
// RTMI_ERR_ARG, reported under `who`, unless the calling thread's current device is the field's.
int rtmi_internal_on_device(const char* who, const rtmi_field* f);
// what 0: d_ray [3][R] (rtmi_read_d_ray's content), 1: final [9][R] (rtmi_read_final's), fp64, the caller's ray order, written to
// dst -- DEVICE memory on the batch's device -- by a kernel enqueued on `stream` (a hipStream_t) after the batch's own stream
// has been synchronised.  For shard.hip's device-to-device read-back.
int rtmi_internal_pack_device(rtmi_batch* b, int what, double* dst, void* stream);
// Relaunch: theta0 [R] (DEVICE, fp64) become the batch's launch angles -- the stored launch conditions that the re-trace of
// critical rays restarts from, not only the ray state -- and the batch is reset (trajectory arrays cleared).  max_size [R]
// (DEVICE, may be NULL) sets per-ray max_size as rtmi_batch_set_per_ray does, with the batch's own DELTA_S; values below 2 are
// allowed here (1: the ray takes no step).  Not on a batch with sort_rays (RTMI_ERR_STATE).  For twopoint.hip's refinement.
int rtmi_internal_relaunch(rtmi_batch* b, const double* theta0, const int32_t* max_size);
// The field's per-cell polynomial table (rt_polytab.h) as the fast-form step kernels see it (rt::FieldDev), widened to fp64: for
// paraxial.hip, which evaluates the same polynomials and their derivatives.  flat: 0, or the distance (in elements) from the
// flat-cell map to poly (rt::FieldDev::flat).  The calling thread's current device must be the field's (RTMI_ERR_ARG).
struct rtmi_internal_poly {
    const void* poly;
    long flat;
    int dtype, ncx, ncy;
    double ax, bx, inv_hx, ay, by, inv_hy;
};
int rtmi_internal_field_poly(const rtmi_field* f, rtmi_internal_poly* out);
// A batch's field and parameters; *rows_from_state = 1 when rtmi_batch_set_state / restore_state gave any ray a state at a row
// other than 0 since the last create / reset (its rows before that row are not a trajectory from its launch point).
int rtmi_internal_batch_info(rtmi_batch* b, const rtmi_field** f, rtmi_params* p, int* rows_from_state);
// A batch's ray count, host-side (no device work): for argument checks that come before any.
int rtmi_internal_batch_rays(rtmi_batch* b, int64_t* R);
// paraxial.hip: J = n0 Q2 and the caustic count after every recorded row, written to DEVICE buffers [rec_rows][R] (slot order)
// by rtmi_paraxial's kernel; with rtmi_paraxial's checks, reported under `who`, the public entry's name.  For ttgrid.hip's
// amplitude columns.
int rtmi_internal_paraxial_rows(const char* who, rtmi_batch* b, double* row_J, int32_t* row_kmah);
// paraxial.hip: Q1 P1 Q2 P2 and n after every recorded row, written to a DEVICE buffer [rec_rows][5][R] (slot order; rows past a
// ray's last row are left as they were) by rtmi_paraxial's kernel; with rtmi_paraxial's checks.  A ray that runs past rec_rows
// gets its recorded rows.  For beams.hip.
int rtmi_internal_paraxial_tube(const char* who, rtmi_batch* b, double* row_tube);
// A batch's launch angles theta0 [R] in the caller's ray order, copied to a host buffer.
int rtmi_internal_batch_theta0(rtmi_batch* b, double* theta0);
// kirchhoff.hip: max |x_i| over the finite values of n doubles on the device (0 when there is none): k_absmax_finite and an 8-byte
// read-back.  red: a device word for the result (a handle's); cus: the device's compute units.  For every unit that scales a
// fixed-point sum by an order-independent maximum.
int rtmi_internal_absmax_finite(const char* who, unsigned long long* red, int cus, const double* d_x, size_t n, double* out);
