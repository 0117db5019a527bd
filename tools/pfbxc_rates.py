#!/usr/bin/env python3
"""The polyphase cross-correlator on device-resident captures: one launch of rtlws_pfbxc_run (include/rtlws_pfbxc.h)
per shape, K and A = 2 and 4, against what a caller runs today in the same process: A launches of rtlws_pfbspec_run
(raw sums: the powers alone) and A launches of rtlws_pfb_run time-major (the samples a multiply-and-sum kernel of the
caller's would then read).

    python tools/pfbxc_rates.py [--samples LOG2] [--out FILE]    2^27 cmplx_u8 per capture, hop M, (M, T) = (32,8)
                                                                 (64,8) (1024,1), K = 1, 16, 256, device events, one
                                                                 process, three alternating rounds

The method is tools/pfbspec_rates.py's: every round times `steps` launches (or groups of A launches) between two
events; consecutive launches read and write different buffer sets (six captures, of which launch i takes i, i + 1, ..,
and two sets of outputs).  Before a shape is timed, its K = 1 rows are compared on the device with the spectrometer's
rows and with the channelizer's samples multiplied.  Algorithmic bytes per input sample per capture are
2 + (4 A + 8 NX) M / (A K D).  The lines go to FILE (default profiles/pfbxc_rates.txt) and to stdout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
STEPS = 20
SHAPES = ((5, 8), (6, 8), (10, 1))
K_AVGS = (1, 16, 256)
INPUTS = (2, 4)
NSRC = 6


def main():
    args = sys.argv[1:]
    log2, out_path = 27, os.path.join(ROOT, "profiles", "pfbxc_rates.txt")
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
    amax = max(INPUTS)
    nxmax = amax * (amax - 1) // 2
    srcs = [torch.randint(0, 256, (nsamples, 2), dtype=torch.uint8, device=dev) for _ in range(NSRC)]
    autos = [torch.empty(amax * nsamples, dtype=torch.float32, device=dev) for _ in range(2)]
    cross = [torch.empty(nxmax * nsamples, dtype=torch.complex64, device=dev) for _ in range(2)]
    say("%d cmplx_u8 samples per capture on the device, hop M, algorithmic bytes per input sample per capture = "
        "2 + (4 A + 8 NX) M / (A K D) (cross-correlator), 2 + 4 M / (K D) (spectrometer), 10 (channelizer), HBM peak %.1f TB/s, "
        "%d launches (or groups of A launches) per round, three alternating rounds, buffer sets rotate"
        % (nsamples, HBM_PEAK / 1e12, STEPS))
    e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()

    def timed(fns):
        """{name: fn(i)} -> {name: [us per call of fn of each of three alternating rounds]}"""
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
        say("%-44s %8.1f .. %8.1f us  %6.0f .. %6.0f GB/s algorithmic = %.2f .. %.2f of the peak  (%s)"
            % (tag, min(t), max(t), byts / max(t) / 1e3, byts / min(t) / 1e3, byts / max(t) * 1e6 / HBM_PEAK,
               byts / min(t) * 1e6 / HBM_PEAK, " ".join("%.1f" % x for x in t)))

    med, rng = {}, {}
    for k, T in SHAPES:
        M = 1 << k
        n = (nsamples - T * M) // M + 1                       # frames a capture holds at hop M
        taps = rtlws.pfb_design(k, T) if T > 1 else np.ones(M, np.int16)
        bank = rtlws.PfbPlan.open(eng, k, taps)
        spec = rtlws.PfbSpecPlan.open(eng, k, taps)
        xc = {A: rtlws.PfbXcPlan.open(eng, k, taps, A) for A in INPUTS}

        # the values first, K = 1, A = 2: the powers against the spectrometer's rows, the cross-spectrum against the
        # channelizer's samples multiplied on the device without contraction (one torch kernel per operation)
        few = min(n, 4099)
        xc[2].run([srcs[0].data_ptr(), srcs[1].data_ptr()], few, 1, autos[0].data_ptr(), cross[0].data_ptr(), hop=M, stream=stream)
        ys = []
        for a in range(2):
            bank.run(srcs[a].data_ptr(), few, cross[1].data_ptr(), hop=M, layout="time", stream=stream)
            spec.run(srcs[a].data_ptr(), few, 1, autos[1].data_ptr(), hop=M, stream=stream)
            torch.cuda.synchronize()
            ys.append(torch.view_as_real(cross[1][:few * M]).clone())
            got = autos[0][:2 * few * M].view(few, 2, M)[:, a]
            assert torch.equal(got, autos[1][:few * M].view(few, M)), "K = 1: the powers are not the spectrometer's"
        re = ys[0][:, 0] * ys[1][:, 0]
        re = re + ys[0][:, 1] * ys[1][:, 1]
        im = ys[0][:, 1] * ys[1][:, 0]
        im = im - ys[0][:, 0] * ys[1][:, 1]
        got = torch.view_as_real(cross[0][:few * M])
        assert torch.equal(got[:, 0], re) and torch.equal(got[:, 1], im), "K = 1: the cross-spectrum is not the channelizer's samples multiplied"
        del ys, re, im, got

        def pfb_group(A):
            def fn(i):
                for a in range(A):
                    bank.run(srcs[(i + a) % NSRC].data_ptr(), n, cross[i % 2][a * nsamples:].data_ptr(), hop=M, layout="time", stream=stream)
            return fn

        def spec_group(A, K):
            def fn(i):
                for a in range(A):
                    spec.run(srcs[(i + a) % NSRC].data_ptr(), n // K, K, autos[i % 2][a * nsamples:].data_ptr(), hop=M, stream=stream)
            return fn

        def xc_one(A, K):
            def fn(i):
                xc[A].run([srcs[(i + a) % NSRC].data_ptr() for a in range(A)], n // K, K, autos[i % 2].data_ptr(),
                          cross[i % 2].data_ptr(), hop=M, stream=stream)
            return fn

        fns = {}
        for A in INPUTS:
            fns[("pfb", A)] = pfb_group(A)
            for K in K_AVGS:
                fns[("spec", A, K)] = spec_group(A, K)
                fns[("xc", A, K)] = xc_one(A, K)
        times = timed(fns)
        for A in INPUTS:
            NX = A * (A - 1) // 2
            name = (M, T, "pfb", A)
            med[name], rng[name] = float(np.median(times[("pfb", A)])), (min(times[("pfb", A)]), max(times[("pfb", A)]))
            line("M=%-4d T=%-2d %d x pfb time-major" % (M, T, A), times[("pfb", A)], A * (2 * rtlws.pfb_samples_needed(k, T, M, n) + 8 * n * M))
            for K in K_AVGS:
                ns = n // K
                need = rtlws.pfbxc_samples_needed(k, T, M, K, ns)
                for kind, byts in (("spec", A * (2 * need + 4 * ns * M)), ("xc", A * 2 * need + (4 * A + 8 * NX) * ns * M)):
                    name = (M, T, kind, A, K)
                    t = times[(kind, A, K)]
                    med[name], rng[name] = float(np.median(t)), (min(t), max(t))
                    line("M=%-4d T=%-2d K=%-3d %s" % (M, T, K, "%d x pfbspec raw sums" % A if kind == "spec" else "pfbxc A=%d" % A), t, byts)
        for K in K_AVGS:
            say("M=%d T=%d K=%d: pfbxc A=2 / 2 x pfb time-major = %.2f, pfbxc A=2 / 2 x pfbspec = %.2f, pfbxc A=4 / 4 x pfbspec = %.2f, "
                "per capture pfbxc A=4 / pfbxc A=2 = %.2f (medians)"
                % (M, T, K, med[(M, T, "xc", 2, K)] / med[(M, T, "pfb", 2)], med[(M, T, "xc", 2, K)] / med[(M, T, "spec", 2, K)],
                   med[(M, T, "xc", 4, K)] / med[(M, T, "spec", 4, K)], med[(M, T, "xc", 4, K)] / 4 / (med[(M, T, "xc", 2, K)] / 2)))
        bank.close()
        spec.close()
        for p in xc.values():
            p.close()

    # the two expectations of DESIGN.md 4.16, written down before anything was measured
    for (k, T) in SHAPES:
        M = 1 << k
        for K in K_AVGS:
            x, p, s = (M, T, "xc", 2, K), (M, T, "pfb", 2), (M, T, "spec", 2, K)
            if K >= 16:
                verdict = "confirmed" if rng[x][1] < rng[p][0] else "refuted" if rng[x][0] > rng[p][1] else "ranges overlap"
                say("expectation 1, M=%d T=%d K=%d: pfbxc A=2 %.1f .. %.1f us < 2 x pfb %.1f .. %.1f us: %s (medians %.2f)"
                    % (M, T, K, rng[x][0], rng[x][1], rng[p][0], rng[p][1], verdict, med[x] / med[p]))
            verdict = "confirmed" if rng[x][1] <= 1.5 * rng[s][0] else "refuted" if rng[x][0] > 1.5 * rng[s][1] else "ranges overlap"
            say("expectation 2, M=%d T=%d K=%d: pfbxc A=2 %.1f .. %.1f us <= 1.5 x (2 x pfbspec %.1f .. %.1f us): %s (medians %.2f)"
                % (M, T, K, rng[x][0], rng[x][1], rng[s][0], rng[s][1], verdict, med[x] / med[s]))

    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
