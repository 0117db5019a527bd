/* audio_gpu.c -- audio_main.h over the HIP shim (replaces reference
 * src/audio_main.c:1-161).  Per decimator block: H2D, ONE launch of the fused
 * chain (rtlws_fm.h: demodulator and both half-bands), D2H of len/4 floats; the
 * phase carry and the two 10-sample delay lines are the chain's 21-float state,
 * two buffers on the device, swapped each call.
 */
#include "audio_main.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "host_ctx.h"
#include "resample.h"
#include "rtlws_fm.h"
#include "rtlws_hip.h"

#define AUDIO_BUFFER_POOL 50          /* reference src/audio_main.c:11 */
#define STATE_STRIDE 24               /* floats between the two states (RTLWS_FM_STATE_FLOATS = 21, padded) */

static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;
static rtlws_engine* g_eng = NULL;
static int g_len = 0;                 /* block length the device buffers are sized for */
static void* g_d_iq = NULL;
static float* g_d_audio = NULL;       /* len/4 samples                */
static float* g_d_state = NULL;       /* two states: in / out, swapped each call; independent of the block length */
static int g_state_idx = 0;
static cmplx_s32* g_h_iq = NULL;      /* pinned */
static float* g_h_audio = NULL;       /* pinned */

/* FIFO of finished audio buffers */
static float* g_pool[AUDIO_BUFFER_POOL];
static int g_q_head = 0, g_q_count = 0, g_audio_len = 0, g_read_pos = 0;

static void free_device(void)
{
    if (!g_eng) return;
    rtlws_dev_free(g_eng, g_d_iq); g_d_iq = NULL;
    rtlws_dev_free(g_eng, g_d_audio); g_d_audio = NULL;
    rtlws_pinned_free(g_h_iq); g_h_iq = NULL;
    rtlws_pinned_free(g_h_audio); g_h_audio = NULL;
}

void audio_init(void)
{
    pthread_mutex_lock(&g_mu);
    if (!g_eng) {
        g_eng = rtlws_engine_create(rtlws_host_device());
        if (!g_eng) {                 /* no CPU path; inert audio side, failure recorded (rtlws_host.h) */
            rtlws_host_fail("audio_init", rtlws_last_error());
        } else {
            /* zeroed state is the reference's start (src/audio_main.c:77-79) */
            g_d_state = (float*)rtlws_dev_alloc(g_eng, 2 * STATE_STRIDE * sizeof(float));
            const char* why = NULL;
            if (!g_d_state || rtlws_memset_dev(g_eng, g_d_state, 0, 2 * STATE_STRIDE * sizeof(float), NULL) ||
                rtlws_stream_sync(g_eng, NULL))
                why = rtlws_last_error();
            else if (rtlws_fm_prepare(g_eng))
                why = rtlws_fm_last_error();
            if (why) {
                rtlws_host_fail("audio_init", why);
                rtlws_dev_free(g_eng, g_d_state);
                g_d_state = NULL;
                rtlws_engine_destroy(g_eng);
                g_eng = NULL;
            }
            g_len = 0;
            g_state_idx = 0;
        }
    }
    /* a second audio_init without audio_close only restarts the queue: the phase
     * carry, the delay lines and the block length are function statics in the
     * reference (src/audio_main.c:76-79) and survive there, so they survive here */
    g_q_head = g_q_count = g_read_pos = 0;
    pthread_mutex_unlock(&g_mu);
}

int audio_new_audio_available(void)
{
    int r;
    pthread_mutex_lock(&g_mu);
    r = g_q_count > 0;
    pthread_mutex_unlock(&g_mu);
    return r;
}

int audio_get_audio_payload(char* buf, int buf_len)
{
    int want = buf_len / (int)sizeof(float), copied = 0;
    pthread_mutex_lock(&g_mu);
    while (want > 0 && g_q_count > 0) {
        const float* src = g_pool[g_q_head];
        int n = g_audio_len - g_read_pos;
        if (n > want) n = want;
        memcpy(buf + (size_t)copied * sizeof(float), src + g_read_pos, (size_t)n * sizeof(float));
        copied += n;
        want -= n;
        g_read_pos += n;
        if (g_read_pos >= g_audio_len) {          /* buffer drained: back to the pool */
            g_q_head = (g_q_head + 1) % AUDIO_BUFFER_POOL;
            g_q_count--;
            g_read_pos = 0;
        }
    }
    pthread_mutex_unlock(&g_mu);
    return copied * (int)sizeof(float);
}

static int resize_for(int len)
{
    int i;
    free_device();
    g_len = len;
    g_d_iq = rtlws_dev_alloc(g_eng, (size_t)len * sizeof(cmplx_s32));
    g_d_audio = (float*)rtlws_dev_alloc(g_eng, (size_t)(len / 4 + 1) * sizeof(float));
    g_h_iq = (cmplx_s32*)rtlws_pinned_alloc((size_t)len * sizeof(cmplx_s32));
    g_h_audio = (float*)rtlws_pinned_alloc((size_t)(len / 4 + 1) * sizeof(float));
    if (!g_d_iq || !g_d_audio || !g_h_iq || !g_h_audio) return -3;
    /* reference src/audio_main.c:82-104: a new block length restarts the queue
     * (delay lines and phase carry are function statics there and survive: g_d_state is not touched) */
    g_audio_len = (len / 2) / 2;
    for (i = 0; i < AUDIO_BUFFER_POOL; i++) {
        free(g_pool[i]);
        g_pool[i] = (float*)calloc((size_t)(g_audio_len > 0 ? g_audio_len : 1), sizeof(float));
    }
    g_q_head = g_q_count = g_read_pos = 0;
    return 0;
}

void audio_fm_demodulator(const cmplx_s32* signal, int len)
{
    const int quarter = (len / 2) / 2;
    int rc = 0, have_buf;
    if (len <= 0) return;
    pthread_mutex_lock(&g_mu);
    if (!g_eng) {                     /* before audio_init, or audio_init found no device: nothing is queued */
        pthread_mutex_unlock(&g_mu);
        rtlws_host_fail("audio_fm_demodulator", "no engine (audio_init not called, or no usable HIP device)");
        return;
    }
    if (g_len != len) rc = resize_for(len);
    /* reference src/audio_main.c:137-142: the second half-band runs -- and its delay
     * line advances -- only when a pool buffer is free to take its output; a
     * block that meets an exhausted pool leaves delay line 2 untouched */
    have_buf = g_q_count < AUDIO_BUFFER_POOL;
    if (!rc) {
        const float* st_in = g_d_state + g_state_idx * STATE_STRIDE;
        float* st_out = g_d_state + (1 - g_state_idx) * STATE_STRIDE;
        const char* why = NULL;
        memcpy(g_h_iq, signal, (size_t)len * sizeof(cmplx_s32));
        if (rtlws_copy_h2d(g_eng, g_d_iq, g_h_iq, (size_t)len * sizeof(cmplx_s32), NULL))
            rc = -3;
        /* :110-142 in one launch; have_buf == 0 leaves delay line 2 as it is */
        else if ((rc = rtlws_fm_audio_blocks(g_eng, g_d_iq, len, 1, st_in, st_out, have_buf, g_d_audio, NULL)) != 0)
            why = rtlws_fm_last_error();
        else if ((have_buf && rtlws_copy_d2h(g_eng, g_h_audio, g_d_audio, (size_t)quarter * sizeof(float), NULL)) ||
                 rtlws_stream_sync(g_eng, NULL))
            rc = -3;
        else
            g_state_idx = 1 - g_state_idx;
        if (why) {
            pthread_mutex_unlock(&g_mu);
            rtlws_host_fail("audio_fm_demodulator", why);
            return;
        }
    }
    if (rc) {                         /* void signature: the block yields no audio, the failure is recorded */
        pthread_mutex_unlock(&g_mu);
        rtlws_host_fail("audio_fm_demodulator", rtlws_last_error());
        return;
    }
    if (have_buf && quarter > 0) {
        float* dst = g_pool[(g_q_head + g_q_count) % AUDIO_BUFFER_POOL];
        memcpy(dst, g_h_audio, (size_t)quarter * sizeof(float));
        g_q_count++;
    }
    pthread_mutex_unlock(&g_mu);
}

void audio_close(void)
{
    int i;
    pthread_mutex_lock(&g_mu);
    free_device();
    if (g_eng) {
        rtlws_dev_free(g_eng, g_d_state);
        g_d_state = NULL;
        rtlws_engine_destroy(g_eng);
        g_eng = NULL;
    }
    for (i = 0; i < AUDIO_BUFFER_POOL; i++) { free(g_pool[i]); g_pool[i] = NULL; }
    g_len = 0;
    g_q_head = g_q_count = g_read_pos = 0;
    pthread_mutex_unlock(&g_mu);
}
