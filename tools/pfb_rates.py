#!/usr/bin/env python3
"""The polyphase channelizer on a device-resident capture: one launch of rtlws_pfb_run (include/rtlws_pfb.h) per
shape and layout, against the two kernels it stands next to on the same box -- the down-converter bank at R = 32,
C = 32 (the same 32 channel centres, the block sum as the only filter) and the f32 spectrum batch at N = 1024 (the
same transform without branch filters, power rows out).

    python tools/pfb_rates.py [--samples LOG2] [--out FILE]      2^27 cmplx_u8, hop M, (M, T) = (16,8) (32,1) (32,8)
                                                                 (64,8) (1024,1) (1024,8), both layouts, device
                                                                 events, one process, three alternating rounds

Every round times `steps` launches between two events; consecutive launches read and write different buffer sets
(three captures, two outputs), so no launch finds its input or its output lines in a cache.  Before a shape is timed
its two layouts are compared on the device, value for value.  Algorithmic bytes are 2 + 8 M / D per input sample.
The lines go to FILE (default profiles/pfb_rates.txt) and to stdout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
STEPS = 20
SHAPES = ((4, 8), (5, 1), (5, 8), (6, 8), (10, 1), (10, 8))


def main():
    args = sys.argv[1:]
    log2, out_path = 27, os.path.join(ROOT, "profiles", "pfb_rates.txt")
    while args and args[0] in ("--samples", "--out"):
        if args[0] == "--samples":
            log2 = int(args[1])
        else:
            out_path = args[1]
        args = args[2:]

    import torch
    import rtlws
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    H = rtlws.hip_lib()
    stream = rtlws.torch_stream_handle()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nsamples = 1 << log2
    srcs = [torch.randint(0, 256, (nsamples, 2), dtype=torch.uint8, device=dev) for _ in range(3)]
    outs = [torch.empty(nsamples, dtype=torch.complex64, device=dev) for _ in range(2)]
    say("%d cmplx_u8 samples on the device, hop M, algorithmic bytes = 2 + 8 M / D = 10 per input sample, HBM peak %.1f TB/s, "
        "%d launches per round, three alternating rounds, buffer sets rotate" % (nsamples, HBM_PEAK / 1e12, STEPS))
    e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()

    def timed(fns):
        """{name: fn(i)} -> {name: [us per launch of each of three alternating rounds]}"""
        times = {name: [] for name in fns}
        for _ in range(3):
            for name, fn in fns.items():
                fn(0), fn(1)
                H.rtlws_event_record(e0, eng.h, stream)
                for i in range(STEPS):
                    fn(i)
                H.rtlws_event_record(e1, eng.h, stream)
                torch.cuda.synchronize()
                times[name].append(1e3 * H.rtlws_event_elapsed_ms(e0, e1) / STEPS)
        return times

    def line(tag, t, byts):
        say("%-34s %8.1f .. %8.1f us/launch  %6.0f .. %6.0f GB/s algorithmic = %.2f .. %.2f of the peak  (%s)"
            % (tag, min(t), max(t), byts / max(t) / 1e3, byts / min(t) / 1e3, byts / max(t) * 1e6 / HBM_PEAK,
               byts / min(t) * 1e6 / HBM_PEAK, " ".join("%.1f" % x for x in t)))

    med = {}
    for k, T in SHAPES:
        M = 1 << k
        n = (nsamples - T * M) // M + 1                       # frames the capture holds at hop M
        plan = rtlws.PfbPlan.open(eng, k, rtlws.pfb_design(k, T) if T > 1 else np.ones(M, np.int16))

        def run(i, layout):
            plan.run(srcs[i % 3].data_ptr(), n, outs[i % 2].data_ptr(), hop=M, layout=layout, stream=stream)

        # the values first: the two layouts of one input
        few = min(n, 4099)
        plan.run(srcs[0].data_ptr(), few, outs[0].data_ptr(), hop=M, layout="time", stream=stream)
        plan.run(srcs[0].data_ptr(), few, outs[1].data_ptr(), hop=M, layout="channel", stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(outs[0][:few * M].view(few, M), outs[1][:few * M].view(M, few).T), "the layouts differ"

        times = timed({"time": lambda i: run(i, "time"), "channel": lambda i: run(i, "channel")})
        byts = 2 * rtlws.pfb_samples_needed(k, T, M, n) + 8 * n * M
        for layout in ("time", "channel"):
            line("M=%-4d T=%-2d pfb %s-major" % (M, T, layout), times[layout], byts)
            med[(M, T, layout)] = float(np.median(times[layout]))
        plan.close()

    # the bank's 32 channel centres: R = 32, C = 32 against M = 32
    n = nsamples // 32
    words = [((c * 2048 + 32768) % 65536) - 32768 for c in range(32)]
    bank = rtlws.DdcPlan.open(eng)
    t = timed({"ddc": lambda i: bank.run(32, srcs[i % 3].data_ptr(), n, words, outs[i % 2].data_ptr(), stream=stream)})["ddc"]
    line("R=32 C=32 ddc bank", t, n * (2 * 32 + 8 * 32))
    bank.close()
    for T in (1, 8):
        for layout in ("channel", "time"):
            say("M=32 T=%d pfb %s-major / ddc bank R=32 C=32 = %.2f (medians)" % (T, layout, med[(32, T, layout)] / float(np.median(t))))

    # the f32 spectrum batch at N = 1024: the same transform, power rows (4 bytes per bin) out
    n = nsamples // 1024
    desc = rtlws.make_desc(1024, 1, "cu8", "rect", "power_sum", 0, 0, 0)
    u = timed({"spectra": lambda i: eng.spectra_batch(desc, srcs[i % 3].data_ptr(), n, outs[i % 2].data_ptr(), stream=stream)})["spectra"]
    line("N=1024 f32 spectra batch", u, n * 1024 * (2 + 4))
    say("M=1024 T=1 pfb time-major / f32 spectra batch N=1024 = %.2f (medians; the channelizer writes 8 bytes per bin, the "
        "spectrum 4)" % (med[(1024, 1, "time")] / float(np.median(u))))

    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
