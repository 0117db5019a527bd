#!/usr/bin/env python3
"""Subband dedispersion on device-resident rows: rtlws_subdedisp_run (include/rtlws_subdedisp.h, two launches) against
rtlws_dedisp_run of the full table (include/rtlws_dedisp.h, the brute-force product it is meant to undercut) in the same
process.

    python tools/subdedisp_rates.py [--out FILE] [--stages DIR]
        tools/dedisp_rates.py's sweep: M = 1024 and 64, 256 trials of DM 0, 0.5, .. (408 MHz centre, 2.4 MHz, 0.8533 ms
        rows), 8192 and 65 536 rows; (nsub, per_nominal) = (M / 16, 16), (M / 32, 8), (M / 8, 32); device events, 20
        launches on rotating buffers, three alternating rounds
    rocprofv3 --kernel-trace -d DIR --output-format csv -- python tools/subdedisp_rates.py --profile-run
        the same configurations in the same order, 2 + 20 runs each and nothing else: the kernel trace from which --stages
        DIR takes the time of either stage (the events see only their sum)

Per shape: microseconds per launch of the brute force, min .. max of the rounds; per configuration the same of the two
launches together, each stage's mean from the trace (where --stages is given), the ratio of the medians to the brute
force beside the ratio of additions (A M + T B) / (T M), smear_rows, and the largest difference between the two outputs
relative to the standard deviation of the brute-force series of that trial.  The lines go to FILE (default
profiles/subdedisp_rates.txt) and to stdout."""
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

SWEEP = (408e6, 2.4e6, 0.8533e-3)               # centre, bandwidth, seconds per row
TRIALS, DM0, DM_STEP = 256, 0.0, 0.5
SHAPES = [(m, nrows) for m in (1024, 64) for nrows in (8192, 65536)]
WARM, STEPS = 2, 20


def configs(m):
    return [(m // 16, 16), (m // 32, 8), (m // 8, 32)]


def stage_times(d):
    """[(stage 1 us, stage 2 us)] per configuration in the order of --profile-run, the first WARM runs of each dropped"""
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "subdedisp_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = 2 * (WARM + STEPS)
    ncfg = sum(len(configs(m)) for m, _ in SHAPES)
    assert len(rows) == per * ncfg, "the trace holds %d launches of the library, %d expected" % (len(rows), per * ncfg)
    out = []
    for c in range(ncfg):
        mine = rows[c * per + 2 * WARM:(c + 1) * per]
        assert all("subband_kernel" in r["Kernel_Name"] for r in mine[0::2]) and all("trial_kernel" in r["Kernel_Name"] for r in mine[1::2])
        dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine]
        out.append((float(np.mean(dur[0::2])), float(np.mean(dur[1::2]))))
    return out


def main():
    args = sys.argv[1:]
    out_path, stages, profile_run = os.path.join(ROOT, "profiles", "subdedisp_rates.txt"), None, "--profile-run" in args
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    if "--stages" in args:
        stages = stage_times(args[args.index("--stages") + 1])

    import torch
    import rtlws
    import rtlws.subdedisp as sd
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    H = rtlws.hip_lib()
    stream = rtlws.torch_stream_handle()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("f32 rows on the device; rtlws_subdedisp_run (two launches) against rtlws_dedisp_run of the full table in one process; device "
        "events, %d launches on two sets of rows, outputs and workspaces in turn, three alternating rounds; %s"
        % (STEPS, "each stage's time: the mean of those launches in a rocprofv3 --kernel-trace run of the same configurations (no counters were taken)"
           if stages else "the stages were not timed apart (no kernel trace was given), and no counters were taken"))
    e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()

    def timed(fns):
        times = {name: [] for name in fns}
        for _ in range(3):
            for name, fn in fns.items():
                for i in range(WARM):
                    fn(i)
                H.rtlws_event_record(e0, eng.h, stream)
                for i in range(STEPS):
                    fn(i)
                H.rtlws_event_record(e1, eng.h, stream)
                torch.cuda.synchronize()
                times[name].append(1e3 * H.rtlws_event_elapsed_ms(e0, e1) / STEPS)
        return times

    done = 0
    for m, nrows in SHAPES:
        full = rtlws.dedisp_delays(m, 1, *SWEEP, TRIALS, DM0, DM_STEP)
        tables = [sd.delays(m, b, 1, *SWEEP, TRIALS, DM0, DM_STEP, per) for b, per in configs(m)]
        nout = nrows - max([int(full.max())] + [int(d1.max()) + int(d2.max()) for _, d1, d2, _ in tables])
        torch.manual_seed(m + nrows)
        rows = [torch.rand((nrows, m), dtype=torch.float32, device=dev) for _ in range(2)]
        outs = [torch.empty((TRIALS, nout), dtype=torch.float32, device=dev) for _ in range(3)]
        brute = rtlws.DedispPlan.open(eng, full)
        assert brute.rows_needed(nout) <= nrows
        plans = [sd.SubdedispPlan(eng, first, d1, d2) for first, d1, d2, _ in tables]
        assert all(p.rows_needed(nout) <= nrows for p in plans)
        works = [torch.empty(max(p.work_floats(nout) for p in plans), dtype=torch.float32, device=dev) for _ in range(2)]

        def run_brute(i, out=None):
            brute.run(rows[i % 2].data_ptr(), nout, (outs[i % 2] if out is None else out).data_ptr(), stream=stream)

        def runner(p):
            return lambda i, out=None: p.run(rows[i % 2].data_ptr(), nout, works[i % 2].data_ptr(), (outs[i % 2] if out is None else out).data_ptr(), stream=stream)

        if profile_run:
            for p in plans:
                for i in range(WARM + STEPS):
                    runner(p)(i)
                torch.cuda.synchronize()
        else:
            fns = {"brute": run_brute}
            fns.update({k: runner(p) for k, p in enumerate(plans)})
            times = timed(fns)
            tb = times["brute"]
            adds = TRIALS * nout * m
            say("M=%-4d %d trials DM 0..127.5 %6d rows, %d outputs a trial" % (m, TRIALS, nrows, nout))
            say("    rtlws_dedisp_run (brute force, %d trials a workgroup)   %9.1f .. %9.1f us/launch  %6.2f T additions/s  (%s)"
                % (rtlws.dedisp_geometry(full, None, nout)[5], min(tb), max(tb), adds / float(np.median(tb)) / 1e6, " ".join("%.1f" % x for x in tb)))
            run_brute(0, outs[2])
            torch.cuda.synchronize()
            sigma = outs[2].std(dim=1, keepdim=True)
            for k, ((b, per), (first, d1, d2, smear), p) in enumerate(zip(configs(m), tables, plans)):
                A = len(first) - 1
                g = sd.geometry(first, d1, d2, None, nout)
                runner(p)(0, outs[1])                                      # the rows the brute force above read
                torch.cuda.synchronize()
                off = float(((outs[1] - outs[2]).abs() / sigma).max())
                ts = times[k]
                split = "stage 1 %8.1f us, stage 2 %8.1f us" % stages[done + k] if stages else "stages not timed apart"
                say("    nsub %4d (C = %2d), %2d trials a nominal (A = %3d): %9.1f .. %9.1f us/run  (%s)  %s; %d nominals and %d trials a workgroup, %s B LDS"
                    % (b, m // b, per, A, min(ts), max(ts), " ".join("%.1f" % x for x in ts), split, g[5], g[6], "/".join(str(x) for x in g[3])))
                say("        time %.3f of the brute force's, additions (A M + T B) / (T M) = %.3f; smear_rows %.3f; largest difference %.3f of the brute-force series' standard deviation"
                    % (float(np.median(ts)) / float(np.median(tb)), (A * m + TRIALS * b) / (TRIALS * m), smear, off))
        done += len(plans)
        brute.close()
        for p in plans:
            p.close()
        del rows, outs, works

    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    if not profile_run:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
