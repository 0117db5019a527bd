#!/usr/bin/env python3
"""The polyphase spectrometer with spectral-kurtosis excision on a device-resident capture: one launch of
rtlws_pfbsk_run (include/rtlws_pfbsk.h) per shape and (K, L), against rtlws_pfbspec_run at the same (M, T) and
k_avg = K L in the same process: the same frames into the same number of rows, without the second sum, the decision
and the walk over the sub-integrations.

    python tools/pfbsk_rates.py [--samples LOG2] [--out FILE]    2^27 cmplx_u8, hop M, (M, T) = (32,8) (64,8) (1024,1)
                                                                 (1024,8), (K, L) = (16,16) (64,16) (256,4), clean f32
                                                                 rows with their counts, with and without the S1 and
                                                                 S2 rows, device events, one process, three
                                                                 alternating rounds

The method is tools/pfbspec_rates.py's: every round times `steps` launches between two events; consecutive launches
read and write different buffer sets (three captures, two outputs).  Before a shape is timed, its L = 1 rows under open
bounds are compared on the device with the spectrometer's, and the S1 rows of a run with its rows of the short spectra.
The bounds are those of estimator thresholds 0.5 and 1.6 (rtlws_pfbsk_bounds), the scale rtlws_pfbsk_power_scale's.
Algorithmic bytes per input sample are 2 + 8 M / (K L D) for a clean f32 row with its counts, and 8 M / (K D) more with
the S1 and S2 rows.  The lines go to FILE (default profiles/pfbsk_rates.txt) and to stdout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
STEPS = 20
SHAPES = ((5, 8), (6, 8), (10, 1), (10, 8))
SUBS = ((16, 16), (64, 16), (256, 4))                 # (K, L)


def main():
    args = sys.argv[1:]
    log2, out_path = 27, os.path.join(ROOT, "profiles", "pfbsk_rates.txt")
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
    outs = [torch.empty(nsamples, dtype=torch.float32, device=dev) for _ in range(2)]        # clean rows, or the spectrometer's
    cnts = [torch.empty(nsamples // 16, dtype=torch.int32, device=dev) for _ in range(2)]
    sub1 = [torch.empty(nsamples // 16, dtype=torch.float32, device=dev) for _ in range(2)]   # K >= 16: M / (K D) <= 1 / 16
    sub2 = [torch.empty(nsamples // 16, dtype=torch.float32, device=dev) for _ in range(2)]
    say("%d cmplx_u8 samples on the device, hop M, random bytes, bounds of estimator thresholds 0.5 and 1.6, algorithmic bytes "
        "per input sample = 2 + 8 M / (K L D) (clean f32 rows and counts; 8 M / (K D) more with the S1 and S2 rows), "
        "2 + 4 M / (K L D) (spectrometer), HBM peak %.1f TB/s, %d launches per round, three alternating rounds, buffer sets rotate"
        % (nsamples, HBM_PEAK / 1e12, STEPS))
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
        say("%-44s %8.1f .. %8.1f us/launch  %6.0f .. %6.0f GB/s algorithmic = %.2f .. %.2f of the peak  (%s)"
            % (tag, min(t), max(t), byts / max(t) / 1e3, byts / min(t) / 1e3, byts / max(t) * 1e6 / HBM_PEAK,
               byts / min(t) * 1e6 / HBM_PEAK, " ".join("%.1f" % x for x in t)))

    for k, T in SHAPES:
        M = 1 << k
        n = (nsamples - T * M) // M + 1                       # frames the capture holds at hop M
        taps = rtlws.pfb_design(k, T) if T > 1 else np.ones(M, np.int16)
        spec = rtlws.PfbSpecPlan.open(eng, k, taps)
        sk = rtlws.PfbSkPlan.open(eng, k, taps)
        pscale = rtlws.pfbsk_power_scale(k, taps)

        # the values first: L = 1 under open bounds is the spectrometer; the S1 rows of a run are its short rows
        K, L = SUBS[0]
        few = min(n // (K * L), 67)
        spec.run(srcs[0].data_ptr(), few * L, K, outs[0].data_ptr(), hop=M, stream=stream)
        sk.run(srcs[0].data_ptr(), few * L, K, 1, pscale, outs[1].data_ptr(), hop=M, stream=stream)
        lo, hi = rtlws.pfbsk_bounds(K, 0.5, 1.6)
        sk.run(srcs[0].data_ptr(), few, K, L, pscale, sub2[1].data_ptr(), lo, hi, cnts[0].data_ptr(), sub1[0].data_ptr(),
               sub2[0].data_ptr(), hop=M, stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(outs[0][:few * L * M], outs[1][:few * L * M]), "L = 1 under open bounds is not the spectrometer"
        assert torch.equal(outs[0][:few * L * M], sub1[0][:few * L * M]), "the S1 rows are not the spectrometer's"
        kept = cnts[0][:few * M]
        assert int(kept.min()) >= 0 and int(kept.max()) <= L

        fns = {}
        for K, L in SUBS:
            lo, hi = rtlws.pfbsk_bounds(K, 0.5, 1.6)
            rows = n // (K * L)
            fns[("spec", K * L)] = (lambda i, K=K, L=L, rows=rows:
                                    spec.run(srcs[i % 3].data_ptr(), rows, K * L, outs[i % 2].data_ptr(), hop=M, stream=stream))
            fns[("sk", K, L)] = (lambda i, K=K, L=L, rows=rows, lo=lo, hi=hi:
                                 sk.run(srcs[i % 3].data_ptr(), rows, K, L, pscale, outs[i % 2].data_ptr(), lo, hi,
                                        cnts[i % 2].data_ptr(), hop=M, stream=stream))
            fns[("sk+rows", K, L)] = (lambda i, K=K, L=L, rows=rows, lo=lo, hi=hi:
                                      sk.run(srcs[i % 3].data_ptr(), rows, K, L, pscale, outs[i % 2].data_ptr(), lo, hi,
                                             cnts[i % 2].data_ptr(), sub1[i % 2].data_ptr(), sub2[i % 2].data_ptr(), hop=M,
                                             stream=stream))
        times = timed(fns)
        for K, L in SUBS:
            rows = n // (K * L)
            read = 2 * rtlws.pfbsk_samples_needed(k, T, M, K, L, rows)
            line("M=%-4d T=%-2d pfbspec K=%d, %d rows" % (M, T, K * L, rows), times[("spec", K * L)], read + 4 * rows * M)
            line("M=%-4d T=%-2d pfbsk K=%d L=%d" % (M, T, K, L), times[("sk", K, L)], read + 8 * rows * M)
            line("M=%-4d T=%-2d pfbsk K=%d L=%d + S1, S2 rows" % (M, T, K, L), times[("sk+rows", K, L)], read + 8 * rows * M * (1 + L))
            ms = float(np.median(times[("spec", K * L)]))
            say("M=%d T=%d pfbsk K=%d L=%d / pfbspec K=%d = %.2f, %.2f with the S1 and S2 rows (medians)"
                % (M, T, K, L, K * L, float(np.median(times[("sk", K, L)])) / ms, float(np.median(times[("sk+rows", K, L)])) / ms))
        spec.close()
        sk.close()

    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
