// rtmi_locator.h -- the locator handle as its two units see it: locate.hip creates and destroys it and searches it with picks
// (DESIGN.md section 29), stack.hip searches it with traces (section 30).  After rtmi_host.h.
#pragma once
#include "rtmi_host.h"

struct rtmi_locator {
    rtmi_locator_params lp{};
    int device = -1, cus = 0;
    size_t nn = 0;
    double* T = nullptr;          // device [P][ny][nx]
    ~rtmi_locator() {
        if (T) (void)hipFree(T);
    }
};

namespace {

#define RTMI_ALLOC(expr)                                                                                          \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) {                                                                                   \
            (void)hipGetLastError();                                                                              \
            return rtmi_internal_fail(RTMI_ERR_ALLOC, (std::string(who) + ": " + #expr + ": " + hipGetErrorString(e_)).c_str()); \
        }                                                                                                         \
    } while (0)

// the calling thread's current device is the handle's
int check_device(const rtmi_locator* loc, const char* who) {
    int dev = -1;
    RTMI_HIP(hipGetDevice(&dev));
    RTMI_ARG(dev == loc->device, "the calling thread's current device is not the handle's");
    return RTMI_OK;
}

}  // namespace
