// shim_common.h -- what every satellite library's extern "C" glue (*_shim.hip, one per library) says the same way: the
// library's thread-local error text, how a refusal and a failed runtime call are recorded, the answer of
// rtlws_*_supported, the head of a plan's open, and which stream a call runs on.  Everything has internal linkage: a library has one shim, so it has one error slot of its own, and a
// refusal in one library does not touch another's *_last_error().
#ifndef RTLWS_SHIM_COMMON_H
#define RTLWS_SHIM_COMMON_H

#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "rtlws_hip.h"

namespace {

thread_local std::string g_err;

// "<function>: <why>"; returns rc
[[maybe_unused]] int fail(const char* fn, const char* why, int rc)
{
    g_err = std::string(fn) + ": " + why;
    return rc;
}

// "<function>: <what>: <the runtime's text>"; returns -3
[[maybe_unused]] int fail_hip(const char* fn, const char* what, hipError_t e)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s: %s", fn, what, hipGetErrorString(e));
    g_err = buf;
    return -3;
}

// rtlws_*_supported: `why` is the verdict of the library's rules; 1, or 0 with "<lib>: <why>" recorded
[[maybe_unused]] int supported(const char* lib, const char* why)
{
    g_err.clear();
    if (why) fail(lib, why, 0);
    return why ? 0 : 1;
}

// what a run answers to a null plan, beside the null engine's text below: the open that would have made it failed
[[maybe_unused]] const char* const NULL_PLAN = "null plan (no usable HIP device: there is no CPU path)";

// The head of an rtlws_*_open (pfb_plan.h, ddc_plan.h): `why`, the verdict of the library's own rules, or else the null
// engine is refused; then the engine's device is made current.  That device, or -1 with the text recorded
[[maybe_unused]] int open_device(const char* fn, const char* why, rtlws_engine* e)
{
    if (!why && !e) why = "null engine (no usable HIP device: there is no CPU path)";
    if (why) return fail(fn, why, -1);
    const int device = rtlws_engine_device(e);
    const hipError_t err = hipSetDevice(device);
    if (err != hipSuccess) return (void)fail_hip(fn, "hipSetDevice", err), -1;
    return device;
}

// include/rtlws_hip.h "Streams": RTLWS_STREAM_DEFAULT is HIP's default stream, null the engine's own, else the caller's
[[maybe_unused]] hipStream_t stream_of(rtlws_engine* e, void* stream)
{
    return stream == RTLWS_STREAM_DEFAULT ? hipStreamLegacy
           : stream                       ? reinterpret_cast<hipStream_t>(stream)
                                          : reinterpret_cast<hipStream_t>(rtlws_engine_stream(e));
}

}  // namespace
#endif
