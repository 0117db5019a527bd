#!/usr/bin/env python3
"""The polyphase beamformer on device-resident captures: one launch of rtlws_pfbbf_run or rtlws_pfbbf_power
(include/rtlws_pfbbf.h) per shape, against what a caller runs today in the same process: A launches of rtlws_pfb_run
time-major (the samples a combine pass of the caller's would then read) for the voltages, and one launch of
rtlws_pfbxc_run over the same A captures for the powers.

    python tools/pfbbf_rates.py [--samples LOG2] [--out FILE]    2^26 cmplx_u8 per capture, hop M, (M, T) = (32,8)
                                                                 (64,8) (1024,1), A = 4, B = 1 and 4, K = 16 and 256,
                                                                 device events, one process, three alternating rounds

The method is tools/pfbxc_rates.py's: every round times `steps` launches (or groups of A launches) between two events;
consecutive launches read and write different buffer sets (six captures, of which launch i takes i, i + 1, .., and two
sets of outputs).  Before a shape is timed, a one-capture beam's values are compared on the device with the
channelizer's samples and the spectrometer's rows.  Algorithmic bytes per launch are 2 A S + 8 B n M (voltages) and
2 A S + 4 B (n / K) M (powers), S the samples of a capture.  The lines go to FILE (default profiles/pfbbf_rates.txt) and
to stdout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
STEPS = 20
SHAPES = ((5, 8), (6, 8), (10, 1))
K_AVGS = (16, 256)
A = 4
BEAMS = (1, 4)
NSRC = 6


def main():
    args = sys.argv[1:]
    log2, out_path = 26, os.path.join(ROOT, "profiles", "pfbbf_rates.txt")
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
    bmax = max(BEAMS)
    srcs = [torch.randint(0, 256, (nsamples, 2), dtype=torch.uint8, device=dev) for _ in range(NSRC)]
    volts = [torch.empty(max(A, bmax) * nsamples, dtype=torch.complex64, device=dev) for _ in range(2)]
    rows = [torch.empty(A * nsamples, dtype=torch.float32, device=dev) for _ in range(2)]
    cross = [torch.empty(A * (A - 1) // 2 * (nsamples // min(K_AVGS)), dtype=torch.complex64, device=dev) for _ in range(2)]
    say("%d cmplx_u8 samples per capture on the device, hop M, A = %d captures, algorithmic bytes per launch = 2 A S + 8 B n M "
        "(beam voltages), 2 A S + 4 B (n / K) M (beam powers), 10 S per channelizer launch, HBM peak %.1f TB/s, "
        "%d launches (or groups of A launches) per round, three alternating rounds, buffer sets rotate"
        % (nsamples, A, HBM_PEAK / 1e12, STEPS))
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
        xc = rtlws.PfbXcPlan.open(eng, k, taps, A)
        bf = {B: rtlws.PfbBfPlan.open(eng, k, taps, A, B) for B in BEAMS}
        g = torch.Generator(device="cpu").manual_seed(k)
        w = {B: torch.view_as_real(torch.polar(2.0 * torch.rand((B, A, M), generator=g), 6.2831853 * torch.rand((B, A, M), generator=g))).to(dev)
             for B in BEAMS}
        hot = torch.zeros((1, A, M, 2), dtype=torch.float32, device=dev)
        hot[0, 1, :, 0] = 1.0

        # the values first: the beam that passes capture 1 alone against the channelizer's samples (by value) and the
        # spectrometer's rows (bit for bit, K = 16)
        few = min(n, 4099) // 16 * 16
        ptrs = [srcs[a].data_ptr() for a in range(A)]
        bf[1].run(ptrs, hot.data_ptr(), few, volts[0].data_ptr(), hop=M, layout="time", stream=stream)
        bank.run(srcs[1].data_ptr(), few, volts[1].data_ptr(), hop=M, layout="time", stream=stream)
        bf[1].power(ptrs, hot.data_ptr(), few // 16, 16, rows[0].data_ptr(), hop=M, stream=stream)
        spec.run(srcs[1].data_ptr(), few // 16, 16, rows[1].data_ptr(), hop=M, stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(volts[0][:few * M]), torch.view_as_real(volts[1][:few * M])), "the one-capture beam is not the channelizer's output"
        assert torch.equal(rows[0][:few // 16 * M], rows[1][:few // 16 * M]), "the one-capture beam's powers are not the spectrometer's"

        def pfb_group(i):
            for a in range(A):
                bank.run(srcs[(i + a) % NSRC].data_ptr(), n, volts[i % 2][a * nsamples:].data_ptr(), hop=M, layout="time", stream=stream)

        def bf_volts(B):
            def fn(i):
                bf[B].run([srcs[(i + a) % NSRC].data_ptr() for a in range(A)], w[B].data_ptr(), n, volts[i % 2].data_ptr(), hop=M,
                          layout="time", stream=stream)
            return fn

        def bf_power(B, K):
            def fn(i):
                bf[B].power([srcs[(i + a) % NSRC].data_ptr() for a in range(A)], w[B].data_ptr(), n // K, K, rows[i % 2].data_ptr(), hop=M,
                            stream=stream)
            return fn

        def xc_one(K):
            def fn(i):
                xc.run([srcs[(i + a) % NSRC].data_ptr() for a in range(A)], n // K, K, rows[i % 2].data_ptr(), cross[i % 2].data_ptr(),
                       hop=M, stream=stream)
            return fn

        fns = {("pfb",): pfb_group}
        for B in BEAMS:
            fns[("bfv", B)] = bf_volts(B)
        for K in K_AVGS:
            fns[("xc", K)] = xc_one(K)
            for B in BEAMS:
                fns[("bfp", B, K)] = bf_power(B, K)
        times = timed(fns)
        S = rtlws.pfb_samples_needed(k, T, M, n)

        def keep(name, tag, byts):
            t = times[name]
            med[(M, T) + name], rng[(M, T) + name] = float(np.median(t)), (min(t), max(t))
            line("M=%-4d T=%-2d %s" % (M, T, tag), t, byts)

        keep(("pfb",), "%d x pfb time-major" % A, A * (2 * S + 8 * n * M))
        for B in BEAMS:
            keep(("bfv", B), "pfbbf voltages A=%d B=%d" % (A, B), 2 * A * S + 8 * B * n * M)
        for K in K_AVGS:
            ns = n // K
            keep(("xc", K), "K=%-3d pfbxc A=%d" % (K, A), 2 * A * S + (4 * A + 8 * A * (A - 1) // 2) * ns * M)
            for B in BEAMS:
                keep(("bfp", B, K), "K=%-3d pfbbf powers A=%d B=%d" % (K, A, B), 2 * A * S + 4 * B * ns * M)
        say("M=%d T=%d: pfbbf voltages B=1 / %d x pfb = %.2f, B=4 / %d x pfb = %.2f; pfbbf powers B=1 / pfbxc = %s, B=4 / pfbxc = %s (medians)"
            % (M, T, A, med[(M, T, "bfv", 1)] / med[(M, T, "pfb")], A, med[(M, T, "bfv", 4)] / med[(M, T, "pfb")],
               ", ".join("%.2f (K=%d)" % (med[(M, T, "bfp", 1, K)] / med[(M, T, "xc", K)], K) for K in K_AVGS),
               ", ".join("%.2f (K=%d)" % (med[(M, T, "bfp", 4, K)] / med[(M, T, "xc", K)], K) for K in K_AVGS)))
        bank.close()
        spec.close()
        xc.close()
        for p in bf.values():
            p.close()

    # the two expectations of DESIGN.md 4.17, written down before anything was measured
    def verdict(x, y):
        return "confirmed" if rng[x][1] < rng[y][0] else "refuted" if rng[x][0] > rng[y][1] else "ranges overlap"

    for (k, T) in SHAPES:
        M = 1 << k
        x, p = (M, T, "bfv", 1), (M, T, "pfb")
        say("expectation 1, M=%d T=%d: pfbbf voltages A=4 B=1 %.1f .. %.1f us < 4 x pfb %.1f .. %.1f us: %s (medians %.2f)"
            % (M, T, rng[x][0], rng[x][1], rng[p][0], rng[p][1], verdict(x, p), med[x] / med[p]))
        for K in K_AVGS:
            x, c = (M, T, "bfp", 1, K), (M, T, "xc", K)
            say("expectation 2, M=%d T=%d K=%d: pfbbf powers A=4 B=1 %.1f .. %.1f us < pfbxc A=4 %.1f .. %.1f us: %s (medians %.2f)"
                % (M, T, K, rng[x][0], rng[x][1], rng[c][0], rng[c][1], verdict(x, c), med[x] / med[c]))

    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
