/* spectrum_gpu.c -- spectrum.h (drop-in boundary #1) over the HIP shim.
 *
 * Replaces reference src/spectrum.c:37-107.  The device does conversion,
 * DFT, |X|^2 and the fft-shift for one frame IN DOUBLE, as the reference does
 * (rtlws_spectra_batch_f64 with one frame, K = 1: src/spectrum.c:54-58 converts
 * to double, :21 is an f64 FFTW plan, :28 accumulates doubles); this file moves
 * the frame across PCIe and performs the read-modify-write into the caller's
 * host f64 buffer, including the order-dependent DC-slot rule of reference
 * src/spectrum.c:25-33, because that buffer belongs to the caller and lives in
 * host memory.  One frame per call is launch- and PCIe-bound whatever the
 * arithmetic costs, so nothing is gained by computing it in f32; the f32 fused
 * kernel is the batch API's (rtlws_hip.h).
 *
 * Frames above 8192 points (powers of two up to 2^20) go through rtlws_long.h's plans instead, one per input
 * kind, opened on first use for one frame, K = 1, power sums.  That needs librtlws_long.so, which only the product
 * build links: it compiles this file with -DRTLWS_LONG_FRAMES (rtl-ws_amd/Makefile).  Without the switch -- a host
 * program built against a shim that lacks the library -- this file refers to none of its symbols and refuses those
 * sizes as it always did.
 *
 * Every other length above 8192 points, up to 2^19, can go through rtlws_anylen.h's plans (Bluestein, librtlws_anylen.so)
 * in the same way -- behind -DRTLWS_ANYLEN_FRAMES, which the product build sets too, and ONLY in a process whose
 * environment sets RTLWS_ANY_LENGTH to a non-zero number, read on every spectrum_alloc.  It is an opt-in because the
 * refusal of those sizes is pinned by a test of the drop-in (tests/test_long_gpu.py::test_dropin_long_frames);
 * serving them by default is the one-line change of any_length_opted_in() returning 1.
 */
#include "spectrum.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "host_ctx.h"
#include "rtlws_hip.h"
#ifdef RTLWS_LONG_FRAMES
#include "rtlws_long.h"
#endif
#ifdef RTLWS_ANYLEN_FRAMES
#include "rtlws_anylen.h"
#endif

#define SHORT_MAX 8192    /* rtlws_spectra_batch_f64's largest frame */

struct spectrum {
    int N;
    rtlws_engine* eng;
    void* h_in;       /* pinned, N * 8 bytes: large enough for cmplx_s32 */
    double* h_out;    /* pinned, N doubles */
#ifdef RTLWS_LONG_FRAMES
    rtlws_long_plan* plan[3];    /* N > SHORT_MAX: by enum rtlws_input, opened on first use */
#endif
#ifdef RTLWS_ANYLEN_FRAMES
    int anylen;                  /* N > SHORT_MAX and not a power of two: rtlws_anylen.h's plans instead */
    rtlws_anylen_plan* aplan[3];
#endif
};

/* whether frames of N > SHORT_MAX points are served (powers of two up to 2^20, product build only) */
static int long_size_ok(int N)
{
#ifdef RTLWS_LONG_FRAMES
    rtlws_spectra_desc d;
    memset(&d, 0, sizeof d);
    d.n_fft = N;
    d.k_avg = 1;
    return rtlws_long_supported(&d);
#else
    (void)N;
    return 0;
#endif
}

/* whether frames of N > SHORT_MAX points that rtlws_long.h refuses are served: up to 2^19, product build, opted in */
#ifdef RTLWS_ANYLEN_FRAMES
static int any_length_opted_in(void)
{
    const char* v = getenv("RTLWS_ANY_LENGTH");    /* every call: a process may set it between two handles */
    return v && atoi(v) != 0;
}
#endif

static int anylen_size_ok(int N)
{
#ifdef RTLWS_ANYLEN_FRAMES
    rtlws_spectra_desc d;
    memset(&d, 0, sizeof d);
    d.n_fft = N;
    d.k_avg = 1;
    return any_length_opted_in() && rtlws_anylen_supported(&d);
#else
    (void)N;
    return 0;
#endif
}

/* one frame from h_in to h_out on the engine's stream; 0 or the failing call's code (its text: *why) */
static int run_frame(struct spectrum* s, const rtlws_spectra_desc* d, const char** why)
{
    int rc;
#ifdef RTLWS_ANYLEN_FRAMES
    if (s->anylen) {
        rtlws_anylen_plan** p = &s->aplan[d->input];
        *why = NULL;
        if (!*p) *p = rtlws_anylen_open(s->eng, d, 1);
        rc = *p ? rtlws_anylen_run(*p, s->h_in, 1, s->h_out, NULL) : -3;
        if (rc) *why = rtlws_anylen_last_error();
        if (!rc && (rc = rtlws_stream_sync(s->eng, NULL)) != 0) *why = rtlws_last_error();
        return rc;
    }
#endif
#ifdef RTLWS_LONG_FRAMES
    if (s->N > SHORT_MAX) {
        rtlws_long_plan** p = &s->plan[d->input];
        *why = NULL;
        if (!*p) *p = rtlws_long_open(s->eng, d, 1);
        rc = *p ? rtlws_long_run(*p, s->h_in, 1, s->h_out, NULL) : -3;
        if (rc) *why = rtlws_long_last_error();
        if (!rc && (rc = rtlws_stream_sync(s->eng, NULL)) != 0) *why = rtlws_last_error();
        return rc;
    }
#endif
    rc = rtlws_spectra_batch_f64(s->eng, d, s->h_in, 1, s->h_out, NULL);
    if (!rc) rc = rtlws_stream_sync(s->eng, NULL);
    *why = rtlws_last_error();
    return rc;
}

struct spectrum* spectrum_alloc(int N)
{
    struct spectrum* s;
    rtlws_spectra_desc probe;
    int anylen = 0;
    memset(&probe, 0, sizeof probe);
    probe.n_fft = N;
    probe.k_avg = 1;
    if (N > SHORT_MAX ? !(long_size_ok(N) || (anylen = anylen_size_ok(N)) != 0) : rtlws_spectra_kernel_kind(&probe) == 0) {
        fprintf(stderr, "rtlws: spectrum_alloc(%d): size not supported by the device engine\n", N);
        return NULL;
    }
    s = (struct spectrum*)calloc(1, sizeof(*s));
    if (!s) return NULL;
    s->N = N;
#ifdef RTLWS_ANYLEN_FRAMES
    s->anylen = anylen;
#else
    (void)anylen;
#endif
    s->eng = rtlws_engine_create(rtlws_host_device());
    if (!s->eng) {
        fprintf(stderr, "rtlws: spectrum_alloc: %s\n", rtlws_last_error());
        free(s);
        return NULL;
    }
    s->h_in = rtlws_pinned_alloc((size_t)N * sizeof(cmplx_s32));
    s->h_out = (double*)rtlws_pinned_alloc((size_t)N * sizeof(double));
    if (!s->h_in || !s->h_out) {
        fprintf(stderr, "rtlws: spectrum_alloc: %s\n", rtlws_last_error());
        spectrum_free(s);
        return NULL;
    }
    return s;
}

/* One frame through the device, then the reference's accumulation loop. */
static int add_frame(struct spectrum* s, const void* src, size_t sample_bytes, int input_kind,
                     double* power_spectrum, int len)
{
    rtlws_spectra_desc d;
    const int N = s->N;
    const int offset = N / 2;
    const char* why;
    int i;

    if (len != N) return -1;                      /* reference src/spectrum.c:51-52 */

    memset(&d, 0, sizeof d);
    d.n_fft = N;
    d.k_avg = 1;
    d.input = input_kind;
    d.window = RTLWS_WIN_RECT;
    d.output = RTLWS_OUT_POWER_SUM;

    memcpy(s->h_in, src, (size_t)N * sample_bytes);
    /* One frame per call: the kernel reads the frame from, and stores the row into, the pinned
     * (device-mapped) staging buffers itself -- one launch and one synchronisation per call
     * instead of two copies around them. */
    if (run_frame(s, &d, &why)) {
        fprintf(stderr, "rtlws: spectrum_add: device failure: %s\n", why);
        return -3;
    }

    /* h_out[i] already is |X[(i + N/2) % N]|^2.  Walk the slots in increasing
     * order so the slot showing bin 0 picks up its left neighbour's updated
     * value (reference src/spectrum.c:25-33). */
    for (i = 0; i < len; i++) {
        if ((offset + i) % len > 0)
            power_spectrum[i] += s->h_out[i];
        else
            power_spectrum[i] += power_spectrum[i - 1];
    }
    return 0;
}

int spectrum_add_cmplx_u8(struct spectrum* s, const cmplx_u8* src, double* power_spectrum, int len)
{
    return add_frame(s, src, sizeof(cmplx_u8), RTLWS_IN_CU8, power_spectrum, len);
}

int spectrum_add_cmplx_s32(struct spectrum* s, const cmplx_s32* src, double* power_spectrum, int len)
{
    return add_frame(s, src, sizeof(cmplx_s32), RTLWS_IN_CS32, power_spectrum, len);
}

int spectrum_add_real_f32(struct spectrum* s, const float* src, double* power_spectrum, int len)
{
    return add_frame(s, src, sizeof(float), RTLWS_IN_RF32, power_spectrum, len);
}

void spectrum_free(struct spectrum* s)
{
    if (!s) return;
#ifdef RTLWS_LONG_FRAMES
    for (int k = 0; k < 3; k++) rtlws_long_close(s->plan[k]);
#endif
#ifdef RTLWS_ANYLEN_FRAMES
    for (int k = 0; k < 3; k++) rtlws_anylen_close(s->aplan[k]);
#endif
    rtlws_pinned_free(s->h_in);
    rtlws_pinned_free(s->h_out);
    rtlws_engine_destroy(s->eng);
    free(s);
}
