#!/usr/bin/env python3
"""Coherent dedispersion on device-resident channel streams (include/rtlws_cdd.h): the time of rtlws_cdd_run at a
256-channel workload of N = 2^12 .. 2^14 points a segment and at N = 2^9, as voltages and as power rows of 16 samples in
both layouts.

    python tools/cdd_bench.py [--out FILE]     device events around the launches only, one process, three alternating
                                               rounds over the forms of one N; the lines go to FILE (default
                                               profiles/cdd.txt) and to stdout

The workload: 256 channels of 2^19 complex f32 samples each (1 GiB), lead = trail = N / 16 (hop = 7 N / 8), random unit-phase
tables.  A run's algorithmic bytes: every segment reads its 8 N bytes once and writes 8 hop bytes (voltages) or 4 hop / 16
(power rows); the channel's table (8 N bytes a segment, the same for every segment of a channel) is not counted.  The HBM
peak is taken, not measured, as 8.0 TB/s (the guide's chip table; a float4 copy reaches 6.29 TB/s there)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
NCHAN, SAMPLES, KSUM = 256, 1 << 19, 16
LOG2NS = (12, 13, 14, 9)
FORMS = (("voltages", 0, "channel"), ("power, time-major", KSUM, "time"), ("power, channel-major", KSUM, "channel"))


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "cdd.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]

    import torch
    import rtlws
    import rtlws.cdd as cdd
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    H = rtlws.hip_lib()
    stream = rtlws.torch_stream_handle()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()

    def timed(fns, steps):
        times = {name: [] for name in fns}
        for _ in range(3):
            for name, fn in fns.items():
                fn(0), fn(1)
                H.rtlws_event_record(e0, eng.h, stream)
                for i in range(steps):
                    fn(i)
                H.rtlws_event_record(e1, eng.h, stream)
                torch.cuda.synchronize()
                times[name].append(1e3 * H.rtlws_event_elapsed_ms(e0, e1) / steps)
        return times

    say("complex f32 streams on the device; device events around the launches only, three alternating rounds, two sets of streams and of "
        "outputs in turn; the HBM peak taken, not measured, as %.1f TB/s" % (HBM_PEAK / 1e12))
    say("workload: %d channels x %d samples, lead = trail = N / 16, ksum %d for the power rows, random unit-phase tables" % (NCHAN, SAMPLES, KSUM))
    streams = [torch.randn((NCHAN, SAMPLES, 2), dtype=torch.float32, device=dev) for _ in range(2)]
    rng = np.random.default_rng(1)
    for log2n in LOG2NS:
        n = 1 << log2n
        lead = trail = n // 16
        hop = n - lead - trail
        nseg = (SAMPLES - n) // hop + 1
        tables = np.exp(2j * np.pi * rng.random((NCHAN, n))).astype(np.complex64)
        rc, blocks, threads, lds = cdd.geometry(log2n, lead, trail, NCHAN, 0, nseg)
        assert rc == 0
        outs = [torch.empty((NCHAN, nseg * hop, 2), dtype=torch.float32, device=dev) for _ in range(2)]
        plans, fns = [], {}
        for name, ksum, layout in FORMS:
            plan = cdd.CddPlan(eng, log2n, lead, trail, NCHAN, ksum, tables)
            plans.append(plan)
            stride = NCHAN if layout == "time" else plan.outputs(nseg)

            def run(i, plan=plan, stride=stride, layout=layout):
                plan.run(streams[i % 2].data_ptr(), SAMPLES, nseg, outs[i % 2].data_ptr(), stride, layout, stream=stream)
            fns[name] = run
        times = timed(fns, 5)
        say("N = 2^%d: %d segments a channel of hop %d, %d workgroups of %d threads, LDS %d B" % (log2n, nseg, hop, blocks, threads, lds))
        for name, ksum, layout in FORMS:
            t = times[name]
            nbytes = float(NCHAN) * nseg * (8 * n + (4 * hop // ksum if ksum else 8 * hop))
            say("    %-22s %9.1f .. %9.1f us/run  %7.1f MB of algorithmic bytes = %.3f .. %.3f of the HBM peak  (%s)"
                % (name, min(t), max(t), nbytes / 1e6, nbytes / (max(t) * 1e-6) / HBM_PEAK, nbytes / (min(t) * 1e-6) / HBM_PEAK,
                   " ".join("%.1f" % x for x in t)))
        for plan in plans:
            plan.close()
        del outs
    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
