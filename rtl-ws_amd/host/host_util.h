/* host_util.h -- what the host files share about a descriptor: the size of a frame and of a row,
 * which batch entry point it takes, and the clock the timings are read from.  Private to host/. */
#ifndef RTLWS_HOST_UTIL_H
#define RTLWS_HOST_UTIL_H

#include <stddef.h>
#include <time.h>
#include "rtlws_hip.h"

/* bytes of one input frame: n_fft samples (cic_r raw samples each when a CIC stage precedes the transform) */
static inline size_t rtlws_frame_bytes(const rtlws_spectra_desc* d)
{
    const size_t r = d->cic_r > 1 ? (size_t)d->cic_r : 1u;
    const size_t per = d->input == RTLWS_IN_CS32 ? 8u : d->input == RTLWS_IN_RF32 ? 4u : 2u * r;
    return per * (size_t)d->n_fft;
}

/* bytes of one output row: payload bytes, f64 rows (f64 arithmetic without RTLWS_FLAG_ROWS_F32),
 * f32 rows otherwise */
static inline size_t rtlws_row_bytes(const rtlws_spectra_desc* d, int f64)
{
    const size_t e = d->output == RTLWS_OUT_PAYLOAD_U8 ? 1u
                     : (f64 && !(d->flags & RTLWS_FLAG_ROWS_F32)) ? 8u : 4u;
    return e * (size_t)d->n_fft;
}

/* one launch: the f32 fused kernel, or the reference's arithmetic (src/spectrum.c:54-60,21,28) */
static inline int rtlws_launch_desc(rtlws_engine* e, const rtlws_spectra_desc* d, int f64, const void* in,
                                    long frames, void* out, void* stream)
{
    return f64 ? rtlws_spectra_batch_f64(e, d, in, frames, out, stream)
               : rtlws_spectra_batch(e, d, in, frames, out, stream);
}

static inline double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

#endif
