#!/usr/bin/env python3
"""Acceleration search on the device: rtlws_accel_search (include/rtlws_accel.h) per shape against the composition it
replaces -- a materialised copy of every series per acceleration (a torch gather, its indices computed outside the
timing), then rtlws_periodlong_run over the copies -- and rtlws_accel_resample alone against that gather alone; beside
them rtlws_periodlong_run over as many plain trials with no resampling at all, the floor the fused run is to be read
against (it carries no condition: how well the accelerations of a trial share the caches is what is being measured).

    python tools/accel_rates.py [--out FILE]    4 trials x 16 accelerations x 2^18, 1 x 16 x 2^20 and 1 x 8 x 2^22
                                                samples, nsamp = N; levels 5, norm 64, seg 256, klo 8, the optional rows
                                                NULL; device events, one process, three alternating rounds

The method is tools/periodlong_rates.py's: every round times `steps` runs between two events; consecutive runs read and
write different buffers (two sets of series, of copies and of outputs).  The coefficients are spread evenly over -2^40 ..
2^40.  Before a shape is timed the fused run's peaks and bins are compared bit for bit with the composition's, and the
gather's copies with rtlws_accel_resample's.  Per shape: microseconds per run, min .. max of the rounds, and whether the
ranges overlap.  The lines go to FILE (default profiles/accel_rates.txt) and to stdout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEVELS, NORM, SEG, KLO = 5, 64, 256, 8
SHAPES = ((4, 16, 18), (1, 16, 20), (1, 8, 22))         # trials, accelerations, log2n
STEPS = 10


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "accel_rates.txt")
    if args and args[0] == "--out":
        out_path = args[1]

    import torch
    import accel_ref
    import rtlws
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    H = rtlws.hip_lib()
    stream = rtlws.torch_stream_handle()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("f32 series on the device; rtlws_accel_search against a torch gather (indices computed beforehand) followed by "
        "rtlws_periodlong_run over the copies, rtlws_accel_resample against that gather, and rtlws_periodlong_run over as many plain "
        "trials; one process, device events, %d runs per round, three alternating rounds, two sets of series, copies and outputs in "
        "turn; nsamp = N, levels %d, norm %d, seg %d, klo %d, the optional rows NULL; coefficients evenly over -2^40 .. 2^40"
        % (STEPS, LEVELS, NORM, SEG, KLO))
    e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()

    def timed(fns):
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

    for ntrials, naccel, log2n in SHAPES:
        n, m = 1 << log2n, 1 << (log2n - 1)
        nsamp, nseg, nv = n, m // SEG, ntrials * naccel
        coefs = [int(c) for c in np.rint(np.linspace(-1.0, 1.0, naccel) * (1 << 40)).astype(np.int64)]
        acc = rtlws.AccelPlan(eng, log2n, LEVELS, NORM, SEG, KLO, coefs, max_trials=nv)
        per = rtlws.PeriodLongPlan(eng, log2n, LEVELS, NORM, SEG, KLO, max_trials=nv)
        assert acc.workspace_bytes() == per.workspace_bytes()                                 # one group each
        index = torch.from_numpy(np.stack([accel_ref.index(c, nsamp) for c in coefs])).to(dev)
        series = [10.0 + torch.randn((ntrials, nsamp), dtype=torch.float32, device=dev) for _ in range(2)]
        plain = [10.0 + torch.randn((nv, nsamp), dtype=torch.float32, device=dev) for _ in range(2)]
        copies = [torch.empty((ntrials, naccel, nsamp), dtype=torch.float32, device=dev) for _ in range(2)]
        bests = [torch.empty(nv * LEVELS * nseg, dtype=torch.float32, device=dev) for _ in range(3)]
        ats = [torch.empty(nv * LEVELS * nseg, dtype=torch.int32, device=dev) for _ in range(3)]

        def fused(i, o=None):
            o = i % 2 if o is None else o
            acc.search(series[i % 2].data_ptr(), nsamp, ntrials, nsamp, bests[o].data_ptr(), ats[o].data_ptr(), stream=stream)

        def gather(i):
            torch.index_select(series[i % 2], 1, index.view(-1), out=copies[i % 2].view(ntrials, naccel * nsamp))

        def long_run(src, i, o=None):
            o = i % 2 if o is None else o
            per.run(src.data_ptr(), nsamp, nv, nsamp, bests[o].data_ptr(), ats[o].data_ptr(), stream=stream)

        def composed(i, o=None):
            gather(i)
            long_run(copies[i % 2], i, o)

        def resample(i):
            acc.resample(series[i % 2].data_ptr(), nsamp, ntrials, nsamp, 0, naccel, copies[i % 2].data_ptr(), nsamp, stream=stream)

        # the two forms give the same bits before either is timed
        gather(0)
        torch.cuda.synchronize()
        gathered = copies[0].clone()
        resample(0)
        torch.cuda.synchronize()
        assert torch.equal(gathered.view(torch.int32), copies[0].view(torch.int32)), "the gather and rtlws_accel_resample differ"
        fused(0, 2)
        torch.cuda.synchronize()
        b, a = bests[2].clone(), ats[2].clone()
        composed(0, 2)
        torch.cuda.synchronize()
        assert torch.equal(b.view(torch.int32), bests[2].view(torch.int32)) and torch.equal(a, ats[2]), "the fused run and the composition differ"
        del gathered, b, a

        times = timed({"fused": fused, "composed": composed, "resample": resample, "gather": gather, "plain": lambda i: long_run(plain[i % 2], i)})
        tf, tc, tr, tg, tp = (times[k] for k in ("fused", "composed", "resample", "gather", "plain"))
        verdict = lambda fast, slow: "do not overlap" if min(slow) > max(fast) else "OVERLAP: the product is not faster"
        say("%d trials x %d accelerations x 2^%d samples (%d virtual trials):" % (ntrials, naccel, log2n, nv))
        say("    rtlws_accel_search                     %10.1f .. %10.1f us/run  (%s)" % (min(tf), max(tf), " ".join("%.1f" % x for x in tf)))
        say("    gather + rtlws_periodlong_run          %10.1f .. %10.1f us/run  = %.2f times the fused run's median; the ranges %s  (%s)"
            % (min(tc), max(tc), float(np.median(tc)) / float(np.median(tf)), verdict(tf, tc), " ".join("%.1f" % x for x in tc)))
        say("    rtlws_accel_resample alone             %10.1f .. %10.1f us/run  (%s)" % (min(tr), max(tr), " ".join("%.1f" % x for x in tr)))
        say("    the gather alone                       %10.1f .. %10.1f us/run  = %.2f times the resampling's median; the ranges %s  (%s)"
            % (min(tg), max(tg), float(np.median(tg)) / float(np.median(tr)), verdict(tr, tg), " ".join("%.1f" % x for x in tg)))
        say("    rtlws_periodlong_run, %3d plain trials  %10.1f .. %10.1f us/run  = %.2f of the fused run's median (no condition)  (%s)"
            % (nv, min(tp), max(tp), float(np.median(tp)) / float(np.median(tf)), " ".join("%.1f" % x for x in tp)))
        acc.close()
        per.close()
        del series, plain, copies, bests, ats, index
        torch.cuda.empty_cache()

    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
