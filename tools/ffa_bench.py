#!/usr/bin/env python3
"""The fast folding search on device-resident series (include/rtlws_ffa.h): the time of rtlws_ffa_run at one workload
shape, the time of each of its passes, and the time of the only other route to the same profiles, rtlws_fold_run over the
table of periods p + s / (m - 1) (include/rtlws_fold.h), at the shape both can run.

    python tools/ffa_bench.py [--out FILE]     both measurements with device events around the launches only, one
                                               process, three alternating rounds; the lines go to FILE (default
                                               profiles/ffa_passes.txt) and to stdout
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/ffa_bench.py --profile-run
                                               the workload shape alone, a few runs: the passes are launches of
                                               ffa_pass<false> (every pass but the last) and ffa_pass<true> (the last), so the
                                               kernel statistics give the time of each
    python tools/ffa_bench.py --passes FALSE_US TRUE_US [--out FILE]
                                               as the first form, with the two kernels' mean times of such a trace added
                                               to the lines as the passes' times and their fractions of the HBM peak

The workload: 64 trials, base periods 256 .. 319 samples, L = 10 (1024 periods a base period), 8 widths, segments of the
last pass's workgroup rows, no profiles stored.  A pass's algorithmic bytes: every pass reads the m p f32 of each (trial,
base period) pair once and every pass but the last writes them once; the peaks are 8 bytes per (pair, segment, width).
The HBM peak is taken, not measured, as 8.0 TB/s (the guide's chip table; a float4 copy reaches 6.29 TB/s there).
The comparison: p = 256 bins, L = 10, 4 trials of 2^18 samples; rtlws_fold_run with steps rtlws_fold_step(p + s / 1023), one
sub-integration.  The two fold differently (nearest-bin phase against shifted rows), so only the times are compared."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
P0, NPER, L, WIDTHS, NTRIALS = 256, 64, 10, (1, 2, 3, 4, 6, 8, 12, 16), 64
CMP_P, CMP_L, CMP_TRIALS = 256, 10, 4


def pass_bytes(p0, nper, L, ntrials, passes, nseg, nwidths):
    """algorithmic bytes of each pass over all pairs"""
    cells = ntrials * sum((p0 + i) << L for i in range(nper)) * 4
    peaks = ntrials * nper * nseg * nwidths * 8
    return [2 * cells] * (passes - 1) + [cells + peaks]


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "ffa_passes.txt")
    profile_run = "--profile-run" in args
    kernel_us = None
    if "--passes" in args:
        k = args.index("--passes")
        kernel_us = (float(args[k + 1]), float(args[k + 2]))
    if "--out" in args:
        out_path = args[args.index("--out") + 1]

    import torch
    import rtlws
    import rtlws.ffa as ffa
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
                for i in range(steps[name]):
                    fn(i)
                H.rtlws_event_record(e1, eng.h, stream)
                torch.cuda.synchronize()
                times[name].append(1e3 * H.rtlws_event_elapsed_ms(e0, e1) / steps[name])
        return times

    # ---- the workload shape ----
    rc, passes, stages, blocks, threads, lds, merge, ws, pairs = ffa.geometry(P0, NPER, L, WIDTHS, 1, max_trials=NTRIALS)
    assert rc == 0
    seg = 1 << stages[passes - 1]
    rc, passes, stages, blocks, threads, lds, merge, ws, pairs = ffa.geometry(P0, NPER, L, WIDTHS, seg, max_trials=NTRIALS)
    assert rc == 0 and merge == 0
    m, p_max = 1 << L, P0 + NPER - 1
    need, nseg = m * p_max, m // seg
    series = [torch.randn((NTRIALS, need), dtype=torch.float32, device=dev) for _ in range(2)]
    npeaks = NTRIALS * NPER * nseg * len(WIDTHS)
    peaks = [torch.empty(npeaks, dtype=torch.float32, device=dev) for _ in range(2)]
    ats = [torch.empty(npeaks, dtype=torch.int32, device=dev) for _ in range(2)]
    plan = ffa.FfaPlan(eng, P0, NPER, L, WIDTHS, seg, max_trials=NTRIALS)

    def search(i):
        plan.run(series[i % 2].data_ptr(), need, NTRIALS, peaks[i % 2].data_ptr(), ats[i % 2].data_ptr(), None, 0, stream=stream)

    if profile_run:
        for i in range(6):
            search(i)
        torch.cuda.synchronize()
        plan.close()
        eng.close()
        return

    groups = -(-NTRIALS * NPER // pairs)
    nbytes = pass_bytes(P0, NPER, L, NTRIALS, passes, nseg, len(WIDTHS))
    say("f32 series on the device; device events around the launches only, three alternating rounds, two sets of series and of outputs in "
        "turn; the HBM peak taken, not measured, as %.1f TB/s" % (HBM_PEAK / 1e12))
    say("workload: %d trials, base periods %d .. %d, L = %d, widths %s, seg %d, no profiles: %d passes of %s stages, %s workgroups a pair of %d "
        "threads, LDS %s B, %d pairs in flight of %d (%d groups, %d launches a run), workspace %.1f MiB"
        % (NTRIALS, P0, p_max, L, WIDTHS, seg, passes, stages[:passes], blocks[:passes], threads, lds[:passes], pairs, NTRIALS * NPER, groups,
           groups * passes, ws / 2.0 ** 20))
    t = timed({"run": search}, {"run": 5})["run"]
    total = float(sum(nbytes))
    say("    rtlws_ffa_run     %10.1f .. %10.1f us/run  %.1f MB of algorithmic bytes = %.3f .. %.3f of the HBM peak  (%s)"
        % (min(t), max(t), total / 1e6, total / (max(t) * 1e-6) / HBM_PEAK, total / (min(t) * 1e-6) / HBM_PEAK, " ".join("%.1f" % x for x in t)))
    if kernel_us is not None:
        # a trace's mean time of one launch: a group's pairs; the passes before the last share one kernel
        for name, us, b, count in (("every pass but the last (ffa_pass<false>)", kernel_us[0], nbytes[0], passes - 1), ("the last pass (ffa_pass<true>)", kernel_us[1], nbytes[-1], 1)):
            if count:
                per_run = us * groups
                say("    %-44s %8.1f us a launch (kernel trace, mean), %8.1f us a run  %.1f MB = %.3f of the HBM peak"
                    % (name, us, per_run, b / 1e6, b / (per_run * 1e-6) / HBM_PEAK))
    plan.close()
    del series, peaks, ats

    # ---- the shape both libraries run: one base period of 256 bins, 1024 periods ----
    cm = 1 << CMP_L
    nsamp = CMP_P * cm
    cseries = [torch.randn((CMP_TRIALS, nsamp), dtype=torch.float32, device=dev) for _ in range(2)]
    steps_h = np.array([rtlws.fold_step(ffa.period(CMP_P, s, CMP_L)) for s in range(cm)], np.uint64)
    fold = rtlws.FoldPlan.open(eng, steps_h, np.zeros(cm, np.uint64), CMP_P, nsamp)
    assert fold.subints(nsamp) == 1
    profs = [torch.empty(CMP_TRIALS * cm * CMP_P, dtype=torch.float32, device=dev) for _ in range(2)]
    fplan = ffa.FfaPlan(eng, CMP_P, 1, CMP_L, (1,), cm, max_trials=CMP_TRIALS)
    cpk = [torch.empty(CMP_TRIALS, dtype=torch.float32, device=dev) for _ in range(2)]
    cat = [torch.empty(CMP_TRIALS, dtype=torch.int32, device=dev) for _ in range(2)]

    def by_fold(i):
        fold.run(cseries[i % 2].data_ptr(), nsamp, CMP_TRIALS, nsamp, profs[i % 2].data_ptr(), None, stream=stream)

    def by_ffa(i):
        fplan.run(cseries[i % 2].data_ptr(), nsamp, CMP_TRIALS, cpk[i % 2].data_ptr(), cat[i % 2].data_ptr(), profs[i % 2].data_ptr(), CMP_P, stream=stream)

    times = timed({"fold": by_fold, "ffa": by_ffa}, {"fold": 3, "ffa": 10})
    tf, ta = times["fold"], times["ffa"]
    say("comparison: %d trials x %d samples, %d bins, the %d periods %d + s / %d, every profile stored" % (CMP_TRIALS, nsamp, CMP_P, cm, CMP_P, cm - 1))
    say("    rtlws_fold_run    %10.1f .. %10.1f us/launch  (%s)" % (min(tf), max(tf), " ".join("%.1f" % x for x in tf)))
    say("    rtlws_ffa_run     %10.1f .. %10.1f us/run     (%s)  = %.1f times faster by the medians; the ranges %s"
        % (min(ta), max(ta), " ".join("%.1f" % x for x in ta), float(np.median(tf)) / float(np.median(ta)),
           "do not overlap" if min(tf) > max(ta) or max(tf) < min(ta) else "overlap"))
    fold.close()
    fplan.close()
    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
