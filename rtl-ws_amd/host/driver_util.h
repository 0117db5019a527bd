/* driver_util.h -- what the two drivers (multi_stream_main.c, multi_batch_main.c) share: the synthetic
 * IQ, the --precision / --output names and the topology fields of a --plan-only line. */
#ifndef RTLWS_DRIVER_UTIL_H
#define RTLWS_DRIVER_UTIL_H

#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rtlws_hip.h"
#include "rtlws_topo.h"

/* tone (cycles_per_sample) + xorshift noise, quantised like an RTL2832U sample */
static void synth_iq(unsigned char* buf, long samples, unsigned seed, double cycles_per_sample)
{
    unsigned x = seed;
    long i;
    for (i = 0; i < samples; i++) {
        const double ph = 2.0 * 3.14159265358979 * cycles_per_sample * (double)i;
        double re, im;
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        re = 0.6 * cos(ph) + ((double)(x & 0xffff) / 65536.0 - 0.5) * 0.2;
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        im = 0.6 * sin(ph) + ((double)(x & 0xffff) / 65536.0 - 0.5) * 0.2;
        buf[2 * i] = (unsigned char)fmin(255.0, fmax(0.0, floor(re * 128.0 + 128.5)));
        buf[2 * i + 1] = (unsigned char)fmin(255.0, fmax(0.0, floor(im * 128.0 + 128.5)));
    }
}

/* --precision: f64 arithmetic or not, and RTLWS_FLAG_ROWS_F32 or 0.  -1 and the usage line for any other name. */
static int parse_precision(const char* name, int* f64, int* row_flags)
{
    if (!strcmp(name, "f32")) { *f64 = 0; *row_flags = 0; }
    else if (!strcmp(name, "f64")) { *f64 = 1; *row_flags = 0; }
    else if (!strcmp(name, "f64c_f32o")) { *f64 = 1; *row_flags = RTLWS_FLAG_ROWS_F32; }
    else { fprintf(stderr, "--precision f32|f64|f64c_f32o\n"); return -1; }
    return 0;
}

/* --output: the RTLWS_OUT_* of a name.  -1 and the usage line for any other name. */
static int parse_output(const char* name, int* output)
{
    if (!strcmp(name, "f32")) *output = RTLWS_OUT_POWER_SUM;
    else if (!strcmp(name, "db")) *output = RTLWS_OUT_MEAN_DB;
    else if (!strcmp(name, "payload")) *output = RTLWS_OUT_PAYLOAD_U8;
    else { fprintf(stderr, "--output f32|db|payload\n"); return -1; }
    return 0;
}

/* the i-th comma-separated entry of --bus-ids, copied into one[n]; "" when the list is too short */
static const char* nth_bus_id(const char* bus_ids, int i, char* one, size_t n_one)
{
    const char* p = bus_ids;
    size_t n;
    while (i > 0 && (p = strchr(p, ',')) != NULL) { ++p; --i; }
    n = p ? strcspn(p, ",") : 0;
    if (!p || n == 0 || n >= n_one) return "";
    memcpy(one, p, n);
    one[n] = 0;
    return one;
}

/* --plan-only: the topology fields of device `dev` as JSON members.  With bus_ids the devices are named
 * by it and no GPU is asked; sysfs_root as in rtlws_topo_describe. */
static void print_device_topology(int dev, const char* bus_ids, const char* sysfs_root)
{
    rtlws_topo_info t;
    char one[32];
    const char* bus = bus_ids ? nth_bus_id(bus_ids, dev, one, sizeof one) : NULL;
    if (rtlws_topo_describe(bus ? -1 : dev, bus, sysfs_root, &t) != 0) { memset(&t, 0, sizeof t); t.numa_node = -1; }
    printf("\"bus_id\": \"%s\", \"numa_node\": %d, \"cpus\": %d, \"cpulist\": \"%s\"",
           t.bus_id, t.numa_node, t.ncpus, t.cpulist);
}

#endif
