#!/usr/bin/env python3
"""The polyphase spectrometer on a device-resident capture: one launch of rtlws_pfbspec_run (include/rtlws_pfbspec.h)
per shape, K and output kind, against rtlws_pfb_run time-major at the same shape in the same process (the same
arithmetic, 8 bytes per input sample more to write) and the f32 spectrum batch at N = 1024 (the same transform
without branch filters).

    python tools/pfbspec_rates.py [--samples LOG2] [--out FILE]    2^27 cmplx_u8, hop M, (M, T) = (32,8) (64,8)
                                                                   (1024,1) (1024,8), K = 1, 16, 256, raw sums and
                                                                   payload bytes, device events, one process, three
                                                                   alternating rounds

The method is tools/pfb_rates.py's: every round times `steps` launches between two events; consecutive launches read
and write different buffer sets (three captures, two outputs).  Before a shape is timed, its K = 1 rows are compared
on the device with the squared samples of the channelizer.  Algorithmic bytes per input sample are 2 + 4 M / (K D) for
f32 rows and 2 + M / (K D) for byte rows.  The lines go to FILE (default profiles/pfbspec_rates.txt) and to stdout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
STEPS = 20
SHAPES = ((5, 8), (6, 8), (10, 1), (10, 8))
K_AVGS = (1, 16, 256)


def main():
    args = sys.argv[1:]
    log2, out_path = 27, os.path.join(ROOT, "profiles", "pfbspec_rates.txt")
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
    say("%d cmplx_u8 samples on the device, hop M, algorithmic bytes per input sample = 2 + 4 M / (K D) (f32 rows), "
        "2 + M / (K D) (byte rows), 10 (channelizer), HBM peak %.1f TB/s, %d launches per round, three alternating rounds, "
        "buffer sets rotate" % (nsamples, HBM_PEAK / 1e12, STEPS))
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
        say("%-38s %8.1f .. %8.1f us/launch  %6.0f .. %6.0f GB/s algorithmic = %.2f .. %.2f of the peak  (%s)"
            % (tag, min(t), max(t), byts / max(t) / 1e3, byts / min(t) / 1e3, byts / max(t) * 1e6 / HBM_PEAK,
               byts / min(t) * 1e6 / HBM_PEAK, " ".join("%.1f" % x for x in t)))

    med = {}
    for k, T in SHAPES:
        M = 1 << k
        n = (nsamples - T * M) // M + 1                       # frames the capture holds at hop M
        taps = rtlws.pfb_design(k, T) if T > 1 else np.ones(M, np.int16)
        bank = rtlws.PfbPlan.open(eng, k, taps)
        spec = rtlws.PfbSpecPlan.open(eng, k, taps)

        # the values first: K = 1 against the channelizer's samples, squared on the device without contraction
        few = min(n, 4099)
        bank.run(srcs[0].data_ptr(), few, outs[0].data_ptr(), hop=M, layout="time", stream=stream)
        spec.run(srcs[0].data_ptr(), few, 1, outs[1].data_ptr(), hop=M, stream=stream)
        torch.cuda.synchronize()
        y = torch.view_as_real(outs[0][:few * M])
        sq = y * y
        assert torch.equal(sq[:, 0] + sq[:, 1], outs[1].view(torch.float32)[:few * M]), "K = 1 is not the channelizer squared"

        fns = {"pfb": lambda i: bank.run(srcs[i % 3].data_ptr(), n, outs[i % 2].data_ptr(), hop=M, layout="time", stream=stream)}
        for K in K_AVGS:
            for output in ("power", "payload"):
                fns[(K, output)] = (lambda i, K=K, output=output:
                                    spec.run(srcs[i % 3].data_ptr(), n // K, K, outs[i % 2].data_ptr(), hop=M, output=output,
                                             scale=1e-12, stream=stream))
        times = timed(fns)
        line("M=%-4d T=%-2d pfb time-major" % (M, T), times["pfb"], 2 * rtlws.pfb_samples_needed(k, T, M, n) + 8 * n * M)
        med[(M, T, "pfb")] = float(np.median(times["pfb"]))
        for K in K_AVGS:
            for output in ("power", "payload"):
                ns = n // K
                byts = 2 * rtlws.pfbspec_samples_needed(k, T, M, K, ns) + (4 if output == "power" else 1) * ns * M
                line("M=%-4d T=%-2d pfbspec K=%-3d %s" % (M, T, K, output), times[(K, output)], byts)
                med[(M, T, K, output)] = float(np.median(times[(K, output)]))
        for K in K_AVGS:
            say("M=%d T=%d pfbspec K=%d / pfb time-major = %.2f (raw sums), %.2f (payload bytes) (medians)"
                % (M, T, K, med[(M, T, K, "power")] / med[(M, T, "pfb")], med[(M, T, K, "payload")] / med[(M, T, "pfb")]))
        bank.close()
        spec.close()

    # the f32 spectrum batch at N = 1024: the same transform without branch filters, power rows out
    n = nsamples // 1024
    desc = rtlws.make_desc(1024, 1, "cu8", "rect", "power_sum", 0, 0, 0)
    u = timed({"spectra": lambda i: eng.spectra_batch(desc, srcs[i % 3].data_ptr(), n, outs[i % 2].data_ptr(), stream=stream)})["spectra"]
    line("N=1024 f32 spectra batch K=1", u, n * 1024 * (2 + 4))
    um = float(np.median(u))
    say("M=1024 T=1: pfbspec K=16 raw sums / f32 spectra batch N=1024 = %.2f, pfb time-major / f32 spectra batch = %.2f (medians)"
        % (med[(1024, 1, 16, "power")] / um, med[(1024, 1, "pfb")] / um))

    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
