// shim_common.h -- what every satellite library's extern "C" glue (*_shim.hip, one per library) says the same way: the
// library's thread-local error text, how a refusal and a failed runtime call are recorded, and which stream a call
// runs on.  Everything has internal linkage: a library has one shim, so it has one error slot of its own, and a
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

// include/rtlws_hip.h "Streams": RTLWS_STREAM_DEFAULT is HIP's default stream, null the engine's own, else the caller's
[[maybe_unused]] hipStream_t stream_of(rtlws_engine* e, void* stream)
{
    return stream == RTLWS_STREAM_DEFAULT ? hipStreamLegacy
           : stream                       ? reinterpret_cast<hipStream_t>(stream)
                                          : reinterpret_cast<hipStream_t>(rtlws_engine_stream(e));
}

}  // namespace
#endif
