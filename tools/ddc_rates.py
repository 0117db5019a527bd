#!/usr/bin/env python3
"""The down-converter bank on a device-resident capture: one launch of rtlws_ddc_run (include/rtlws_ddc.h) for C
channels against rtlws_cic_block_sums on the same input -- the existing kernel with the same bytes at C = 1, and,
C times over, the floor of any approach that takes one pass per channel.

    python tools/ddc_rates.py [--samples LOG2] [--out FILE] [R ...]    2^27 cmplx_u8, R = 8 10 12, C = 1 8 32,
                                                                       device events, one process, three
                                                                       alternating rounds per (R, C)

Every round times `steps` launches between two events; consecutive launches read and write different buffer sets
(three captures, two or three outputs), so no launch finds its input or its output lines in a cache.  Before
anything is timed the bank's k = 0 channel is compared with rtlws_cic_block_sums on the device, integer for
integer.  The lines go to FILE (default profiles/ddc_rates.txt) and to stdout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
STEPS = 30


def main():
    args = sys.argv[1:]
    log2, out_path = 27, os.path.join(ROOT, "profiles", "ddc_rates.txt")
    while args and args[0] in ("--samples", "--out"):
        if args[0] == "--samples":
            log2 = int(args[1])
        else:
            out_path = args[1]
        args = args[2:]
    factors = [int(a) for a in args] or [8, 10, 12]

    import torch
    import rtlws
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    H = rtlws.hip_lib()
    plan = rtlws.DdcPlan.open(eng)
    stream = rtlws.torch_stream_handle()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    srcs = [torch.randint(0, 256, (1 << log2, 2), dtype=torch.uint8, device=dev) for _ in range(3)]
    say("%d cmplx_u8 samples on the device, algorithmic bytes = (2 R + 8 C) per decimated sample, HBM peak %.1f TB/s, "
        "%d launches per round, three alternating rounds (ddc, cic), buffer sets rotate" % (1 << log2, HBM_PEAK / 1e12, STEPS))
    e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()
    rng = np.random.default_rng(1)
    for R in factors:
        n = (1 << log2) // R
        for C in (1, 8, 32):
            words = [12345] + [int(k) for k in rng.integers(-32768, 32768, C - 1)]
            nsets = 2 if n * C * 8 >= (1 << 30) else 3
            outs = [torch.empty((C, n, 2), dtype=torch.int32, device=dev) for _ in range(nsets)]
            cics = [torch.empty((min(C, 8), n, 2), dtype=torch.int32, device=dev) for _ in range(2)]
            ncic = min(C, 8)                             # C CIC launches stand for C channels (timed up to C = 8)

            # the integers first: channel 0 at k = 0 is the CIC
            plan.run(R, srcs[0].data_ptr(), n, [0] + words[1:], outs[0].data_ptr(), stream=stream)
            eng.cic_block_sums(R, srcs[0].data_ptr(), n, cics[0].data_ptr(), stream=stream)
            torch.cuda.synchronize()
            assert torch.equal(outs[0][0], cics[0][0]), "the k = 0 channel and rtlws_cic_block_sums differ"

            def ddc(i):
                plan.run(R, srcs[i % 3].data_ptr(), n, words, outs[i % nsets].data_ptr(), stream=stream)

            def cic(i):
                for c in range(ncic):
                    eng.cic_block_sums(R, srcs[i % 3].data_ptr(), n, cics[i % 2][c].data_ptr(), stream=stream)

            times = {"ddc": [], "cic": []}
            for _ in range(3):
                for name, fn in (("ddc", ddc), ("cic", cic)):
                    fn(0), fn(1)
                    H.rtlws_event_record(e0, eng.h, stream)
                    for i in range(STEPS):
                        fn(i)
                    H.rtlws_event_record(e1, eng.h, stream)
                    torch.cuda.synchronize()
                    times[name].append(1e3 * H.rtlws_event_elapsed_ms(e0, e1) / STEPS)
            byts = n * (2 * R + 8 * C)
            t, u = times["ddc"], times["cic"]
            say("R=%-2d C=%-2d ddc  %8.1f .. %8.1f us/launch  %6.0f .. %6.0f GB/s algorithmic = %.2f .. %.2f of the peak  (%s)"
                % (R, C, min(t), max(t), byts / max(t) / 1e3, byts / min(t) / 1e3, byts / max(t) * 1e6 / HBM_PEAK,
                   byts / min(t) * 1e6 / HBM_PEAK, " ".join("%.1f" % x for x in t)))
            say("R=%-2d C=%-2d %d x cic %6.1f .. %8.1f us  (%s);  one cic launch %.1f us = %.2f of the peak at (2 R + 8) bytes"
                % (R, C, ncic, min(u), max(u), " ".join("%.1f" % x for x in u), float(np.median(u)) / ncic,
                   n * (2 * R + 8) / (float(np.median(u)) / ncic) * 1e6 / HBM_PEAK))
            if C == 1:
                say("R=%-2d C=1  ddc / cic = %.2f (medians); ranges overlap: %s"
                    % (R, float(np.median(t) / np.median(u)), not (max(t) < min(u) or max(u) < min(t))))
            else:
                say("R=%-2d C=%-2d one ddc launch / %d cic launches = %.2f (medians); ddc range wholly below: %s"
                    % (R, C, ncic, float(np.median(t) / np.median(u)), max(t) < min(u)))
            del outs, cics
            torch.cuda.empty_cache()
    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    plan.close()
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
