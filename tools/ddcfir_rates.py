#!/usr/bin/env python3
"""The filtered down-converter bank on a device-resident capture: one launch of rtlws_ddcfir_run
(include/rtlws_ddcfir.h) against one launch of rtlws_ddc_run (include/rtlws_ddc.h) at the same R and C on the same
input, alternating in one process -- what the channel filter costs over the unfiltered bank.

    python tools/ddcfir_rates.py [--samples LOG2] [--out FILE]    2^26 cmplx_u8, (R, L) = (12, 12) (12, 96) (8, 64)
                                                                   (10, 80), C = 1 8 32, device events, one process,
                                                                   three alternating rounds per shape

The method is tools/ddc_rates.py's: every round times `steps` launches between two events; consecutive launches read
and write different buffer sets (three captures, two or three outputs), so no launch finds its input or its output
lines in a cache.  Before anything is timed the filtered bank with L = R taps of 16384 and out_shift 14 is compared
with the unfiltered bank on the device, integer for integer.  The taps are rtlws_ddcfir_design's.  The lines go to
FILE (default profiles/ddcfir_rates.txt) and to stdout.

Stated before the first run: the filter multiplies the matrix work by L / min(R, 16 ceil(R / 16))
and re-reads every byte L / R times from the caches, and its operands come from LDS where the R = 8, 10, 12 kernels
of the unfiltered bank hold theirs in registers.  Expected: L = R within 0.8 .. 2 of the unfiltered bank at every C;
L = 8 R at C = 1 within 1 .. 4 (the capture's bytes still dominate); L = 8 R at C = 32 between 4 and 16 (the matrix
pipe decides: eight times the unfiltered bank's multiplications)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

STEPS = 10
SHAPES = ((12, 12), (12, 96), (8, 64), (10, 80))
EXPECTED = {"L = R": (0.8, 2.0), "L = 8 R, C = 1": (1.0, 4.0), "L = 8 R, C = 8": (1.0, 16.0), "L = 8 R, C = 32": (4.0, 16.0)}


def main():
    args = sys.argv[1:]
    log2, out_path = 26, os.path.join(ROOT, "profiles", "ddcfir_rates.txt")
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
    ddc_plan = rtlws.DdcPlan.open(eng)
    stream = rtlws.torch_stream_handle()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    srcs = [torch.randint(0, 256, (1 << log2, 2), dtype=torch.uint8, device=dev) for _ in range(3)]
    say("%d cmplx_u8 samples on the device, %d launches per round, three alternating rounds (ddcfir, ddc), buffer sets "
        "rotate; ratio = ddcfir / ddc at the same R, C and dec_len" % (1 << log2, STEPS))
    say("expected before the run: " + "; ".join("%s: %.1f .. %.1f" % (k, lo, hi) for k, (lo, hi) in EXPECTED.items()))
    e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()
    rng = np.random.default_rng(1)
    verdicts = {}
    for R, L in SHAPES:
        n = ((1 << log2) - L) // R + 1
        assert rtlws.ddcfir_samples_needed(R, L, n) <= 1 << log2
        plan = rtlws.DdcFirPlan.open(eng, R, rtlws.ddcfir_design(R, L))
        box = rtlws.DdcFirPlan.open(eng, R, np.full(R, 16384, np.int16))
        for C in (1, 8, 32):
            words = [12345] + [int(k) for k in rng.integers(-32768, 32768, C - 1)]
            nsets = 2 if n * C * 8 >= (1 << 30) else 3
            outs = [torch.empty((C, n, 2), dtype=torch.int32, device=dev) for _ in range(nsets)]

            # the integers first: the boxcar at out_shift 14 is the unfiltered bank
            box.run(srcs[0].data_ptr(), n, words, outs[0].data_ptr(), out_shift=14, stream=stream)
            ddc_plan.run(R, srcs[0].data_ptr(), n, words, outs[1].data_ptr(), stream=stream)
            torch.cuda.synchronize()
            assert torch.equal(outs[0], outs[1]), "the boxcar and rtlws_ddc_run differ"

            def fir(i):
                plan.run(srcs[i % 3].data_ptr(), n, words, outs[i % nsets].data_ptr(), out_shift=14, stream=stream)

            def ddc(i):
                ddc_plan.run(R, srcs[i % 3].data_ptr(), n, words, outs[i % nsets].data_ptr(), stream=stream)

            times = {"fir": [], "ddc": []}
            for _ in range(3):
                for name, fn in (("fir", fir), ("ddc", ddc)):
                    fn(0), fn(1)
                    H.rtlws_event_record(e0, eng.h, stream)
                    for i in range(STEPS):
                        fn(i)
                    H.rtlws_event_record(e1, eng.h, stream)
                    torch.cuda.synchronize()
                    times[name].append(1e3 * H.rtlws_event_elapsed_ms(e0, e1) / STEPS)
            t, u = times["fir"], times["ddc"]
            ratios = [a / b for a, b in zip(t, u)]
            macs = 8.0 * L * C * n                           # int8 multiplications of the two operands, re and im
            say("R=%-2d L=%-3d C=%-2d ddcfir %8.1f .. %8.1f us/launch (%s)  %5.1f .. %5.1f Tmac/s   ddc %8.1f .. %8.1f us (%s)   "
                "ratio %.2f .. %.2f (per round: %s)"
                % (R, L, C, min(t), max(t), " ".join("%.1f" % x for x in t), macs / max(t) / 1e6, macs / min(t) / 1e6,
                   min(u), max(u), " ".join("%.1f" % x for x in u), min(ratios), max(ratios), " ".join("%.2f" % x for x in ratios)))
            key = "L = R" if L == R else "L = 8 R, C = %d" % C
            lo, hi = EXPECTED[key]
            verdicts.setdefault(key, []).append(lo <= min(ratios) and max(ratios) <= hi)
            del outs
            torch.cuda.empty_cache()
        plan.close()
        box.close()
    for key, oks in verdicts.items():
        say("expectation %s in %.1f .. %.1f: %s" % (key, EXPECTED[key][0], EXPECTED[key][1], "confirmed" if all(oks) else "refuted"))
    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    ddc_plan.close()
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
